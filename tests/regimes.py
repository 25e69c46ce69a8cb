"""Trained-like parameter regimes for the parity tests (tests/test_trained_regimes_gpu.py; DESIGN.md "Trained-like regimes").

oracle.cnn_gru_oracle.init_params — and nn's default initialisers — leave a model near initialisation: pre-activations of order 1,
BatchNorm gamma positive, logits of order 1.  apply() moves a copy of such a parameter set to where training takes it, one
aspect at a time, on any param_specs layout (two layers of 64 units, one layer of 32, with or without the gate's tensors).
Every regime MIXES saturated and ordinary units: with every unit of a layer saturated, fp32's quantisation of 1 - z alone puts
the fp32 oracle 6e-3 of the largest gradient away from the fp64 one, and a comparison says nothing.
The stage-2 regimes (bn1_always_on, conv2_offcentre, conv_rows: conv2 channels far off centre, convolution rows without spread), their
activity conditions and their frozen case tables are at the end of this file's constants and helpers; they run in
tests/test_stage2_regimes_host.py and tests/test_stage2_regimes_gpu.py (DESIGN.md "Stage-2 regimes")."""
import numpy as np

# constants added to the rows of ONE gate of gru.bias_ih_* (gate order r, z, n), one draw per unit
GATE_BIAS = {
    # z: at 20 z == 1 in fp32, at 12 1 - z = 6e-6, at +-100 exp overflows (the kernels rely on rcp(inf) = 0)
    "z_sat": (1, (100.0, 20.0, 12.0, 6.0, 0.0, -6.0, -12.0, -100.0)),
    "r_sat": (0, (100.0, 20.0, 8.0, 0.0, -8.0, -20.0, -100.0)),
    "n_sat": (2, (50.0, 9.0, 4.0, 0.0, -4.0, -9.0, -50.0)),
}
INPUT_DRIVEN_UNITS, INPUT_DRIVEN_FACTORS = 16, (3.0, 4.0, 3.0)      # rows r, z, n of the chosen units of gru.weight_ih_*
BN_GAMMA, BN_BETA = (-1.5, -0.3, 0.0, 0.7, 2.0), (-2.0, -0.5, 0.0, 0.5, 2.0)
HEAD_SAT = {"classifier.3.weight": 400.0, "classifier.0.weight": 4.0}
# Stage-2 regimes (tests/test_stage2_regimes_host.py, tests/test_stage2_regimes_gpu.py; DESIGN.md "Stage-2 regimes"): BatchNorm-1's (gamma,
# beta) drawn per channel — a small gamma under a positive beta is an "always on" channel, which feeds conv2 a nearly constant positive
# input —, the first ONE_SIGNED output rows of conv2 made one-signed, and rows of both convolutions zeroed / scaled.
BN1_ON = {"bn1_always_on": ((1.0, 0.25, 0.1, 0.05), (0.0, 1.0, 2.0, 3.0)), "conv2_offcentre": ((0.1, 0.05, 0.02), (2.0, 3.0, 4.0))}
ONE_SIGNED = 8
ROW_SCALES = (0.0, 1e-3, 1e3)           # conv_rows: one output row of cnn_encoder.0.weight and of cnn_encoder.4.weight each
STAGE2_REGIMES = tuple(BN1_ON) + ("conv_rows",)
REGIMES = tuple(GATE_BIAS) + ("input_driven", "bn_affine", "head_sat") + STAGE2_REGIMES


def apply(params_np, name, rs):
    """A copy of `params_np` ({state_dict key: array}) in regime `name`; `rs` (np.random.RandomState) draws what the regime
    leaves open.  Buffers and tensors the regime does not name are copied unchanged."""
    if name not in REGIMES:
        raise KeyError(name)
    out = {k: np.array(v, copy=True) for k, v in params_np.items()}
    f32 = lambda a, like: np.asarray(a).astype(like.dtype)
    if name in GATE_BIAS:
        gate, values = GATE_BIAS[name]
        for k in sorted(k for k in out if k.startswith("gru.bias_ih_")):        # every layer and direction present
            H = out[k].shape[0] // 3
            out[k][gate * H:(gate + 1) * H] += f32(rs.choice(values, size=H), out[k])
    elif name == "input_driven":
        for k in sorted(k for k in out if k.startswith("gru.weight_ih_")):
            H = out[k].shape[0] // 3
            units = rs.choice(H, size=min(INPUT_DRIVEN_UNITS, H), replace=False)
            for gate, factor in enumerate(INPUT_DRIVEN_FACTORS):
                out[k][gate * H + units] *= np.asarray(factor, dtype=out[k].dtype)
    elif name == "bn_affine":
        for idx in (1, 5):
            w, b = f"cnn_encoder.{idx}.weight", f"cnn_encoder.{idx}.bias"
            CH = out[w].shape[0]
            gamma, beta = rs.choice(BN_GAMMA, size=CH), rs.choice(BN_BETA, size=CH)
            neg, dead_pos, dead_neg = rs.permutation(CH)[:3]                   # guaranteed: gamma < 0; (0, beta > 0); (0, beta < 0)
            gamma[neg] = rs.choice([g for g in BN_GAMMA if g < 0])
            gamma[dead_pos], beta[dead_pos] = 0.0, rs.choice([v for v in BN_BETA if v > 0])
            gamma[dead_neg], beta[dead_neg] = 0.0, rs.choice([v for v in BN_BETA if v < 0])
            out[w], out[b] = f32(gamma, out[w]), f32(beta, out[b])
    elif name in BN1_ON:
        gammas, betas = BN1_ON[name]
        CH = out["cnn_encoder.1.weight"].shape[0]
        out["cnn_encoder.1.weight"] = f32(rs.choice(gammas, size=CH), out["cnn_encoder.1.weight"])
        out["cnn_encoder.1.bias"] = f32(rs.choice(betas, size=CH), out["cnn_encoder.1.bias"])
        if name == "conv2_offcentre":                                              # the other 24 rows stay: no case is all-degenerate
            out["cnn_encoder.4.weight"][:ONE_SIGNED] = np.abs(out["cnn_encoder.4.weight"][:ONE_SIGNED])
    elif name == "conv_rows":
        for k in ("cnn_encoder.0.weight", "cnn_encoder.4.weight"):
            for row, scale in zip(rs.permutation(out[k].shape[0])[:len(ROW_SCALES)], ROW_SCALES):
                out[k][row] *= np.asarray(scale, dtype=out[k].dtype)
    else:
        for k, factor in HEAD_SAT.items():
            out[k] = out[k] * np.asarray(factor, dtype=out[k].dtype)
    return out


def bn_channels(params_np, idx):
    """Channels of BatchNorm `idx` (1 or 5) by what the regime made of them: (gamma < 0, gamma == 0 and beta > 0, gamma == 0 and beta < 0)."""
    g, b = np.asarray(params_np[f"cnn_encoder.{idx}.weight"]), np.asarray(params_np[f"cnn_encoder.{idx}.bias"])
    return np.flatnonzero(g < 0), np.flatnonzero((g == 0) & (b > 0)), np.flatnonzero((g == 0) & (b < 0))


def conv_rows_channels(params_np, idx):
    """(zeroed, scaled by 1e-3, scaled by 1e3) output rows of convolution `idx` (0 or 4) under conv_rows, recognised by their norms."""
    w = np.asarray(params_np[f"cnn_encoder.{idx}.weight"], dtype=np.float64)
    norm = np.sqrt((w.reshape(w.shape[0], -1) ** 2).sum(axis=1))
    zero = np.flatnonzero(norm == 0)
    mid = np.median(norm)
    small, large = np.flatnonzero((norm > 0) & (norm < 1e-2 * mid)), np.flatnonzero(norm > 1e2 * mid)
    assert len(zero) == len(small) == len(large) == 1, (zero, small, large)
    return int(zero[0]), int(small[0]), int(large[0])


def _conditioning(y):
    y = np.asarray(y, dtype=np.float64)
    mean, var = y.mean(axis=(0, 2)), y.var(axis=(0, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(var > 0, mean * mean / var, np.where(mean == 0, 0.0, np.inf))


def conv1_conditioning(st64):
    """mean^2 / var per channel of the fp64 oracle's conv1 stage (B, 16, L1): what a one-pass variance E[y^2] - mean^2 loses of its
    relative precision.  0 for a channel that is exactly zero, inf for any other constant channel."""
    return _conditioning(st64["conv1"])


def conv2_conditioning(st64):
    """The same of the conv2 stage (B, 32, L2)."""
    return _conditioning(st64["conv2"])


# bands of conv2's largest mean^2 / var that a case of the regime is named for (conditions on the fp64 oracle's stages, not tolerances)
CONV2_RATIO_BAND = {"bn1_always_on": (16.0, 200.0), "conv2_offcentre": (500.0, np.inf)}
BN_EPS = 1e-5


def assert_stage2_regime_active(regime, params_np, st64):
    """The defining condition of a stage-2 regime in the fp64 oracle's stages (numpy arrays), so that no case passes vacuously."""
    if regime in CONV2_RATIO_BAND:
        ratio, (lo, hi) = conv2_conditioning(st64), CONV2_RATIO_BAND[regime]
        assert lo < ratio.max() < hi, f"conv2: max mean^2 / var = {ratio.max():.1f}, not in ({lo}, {hi})"
        assert ratio.min() < 1.0, f"conv2: min mean^2 / var = {ratio.min():.2f}: no ordinary channel beside the off-centre ones"
    elif regime == "conv_rows":
        for conv, pool, idx in (("conv1", "pool1", 0), ("conv2", "pool2", 4)):
            zero, small, large = conv_rows_channels(params_np, idx)
            y, beta = np.asarray(st64[conv]), float(np.asarray(params_np[f"cnn_encoder.{idx + 1}.bias"])[zero])
            assert (y[:, zero] == 0).all(), f"{conv}: the zeroed row's output is not exactly 0"
            assert (np.asarray(st64[pool])[:, zero] == max(beta, 0.0)).all(), f"{pool}: the zeroed row's channel is not relu(beta)"
            assert y[:, small].var() < BN_EPS, f"{conv}: the 1e-3 row's batch variance is {y[:, small].var():.2e}"
            assert np.abs(y[:, large]).max() > 1e2 * np.median(np.abs(y).max(axis=(0, 2))), f"{conv}: the 1e3 row does not stand out"
    else:
        raise KeyError(regime)


# ---- the frozen stage-2 case tables (shapes chosen for where one-pass sums are weakest — few work items — and for the ragged and
# multi-item paths of pool1_conv2_fwd_kernel; an item is one (window, chunk of 128 conv2 positions)) --------------------------------------
S2_ONE = (1, 6, 2, 256, 0.0)            # one work item: a single fp32-rounded partial, nothing averages
S2_FEW = ((2, 6, 2, 256, 0.5), (4, 3, 2, 256, 0.5))      # 2 and 4 items; C < 4: no gate
S2_MAIN = (24, 6, 2, 256, 0.5)          # the trained-regime tier's main shape, two batch tiles
S2_RAGGED = (37, 3, 3, 72, 0.25)        # L2 = 9: most lanes of the one chunk are masked by t < L2 and must add nothing
S2_CHUNKS = (2, 6, 2, 1027, 0.5)        # L2 = 129: a second conv2 chunk holding one position, unaligned T
S2_MANY = (300, 3, 2, 64, 0.5)          # 300 items: the across-workgroup double reduction over many rows
# (regime, B, C, K, T, p, form): every regime at ONE, FEW and MAIN under both shipped form sets (the front end does not depend on the GRU
# form: "split" alone for the rest)
STAGE2_CASES = ([(r, *s, f) for r in STAGE2_REGIMES for s in (S2_ONE,) + S2_FEW + (S2_MAIN,) for f in ("ws6", "split")]
                + [("conv2_offcentre", *s, "split") for s in (S2_RAGGED, S2_CHUNKS, S2_MANY)])
# (regime, B, T) -> (init_params seed, input seed) where test_trained_regimes_gpu.build_case's defaults leave the gate MLP's one hidden
# unit dead (B = 1), `own` of a gate gradient over OWN_CAP, conv2's largest ratio outside the regime's band (C = 3 under seed 103), or —
# conv_rows at few windows — the 1e3 row's batch mean, which sets the scale of running_mean, a small remainder of its sum (the fp32
# oracle is then itself 2.3e-5 from the fp64 one); chosen with tests/test_stage2_regimes_host.py, which holds every case to those
# conditions, and frozen here.
S2_SEEDS = {(r, 1, 256): (None, 9) for r in STAGE2_REGIMES}
S2_SEEDS.update({("conv_rows", 1, 256): (None, 10), ("conv_rows", 2, 256): (None, 13), ("bn1_always_on", 2, 256): (None, 9), ("conv2_offcentre", 2, 1027): (None, 11), ("conv2_offcentre", 24, 256): (None, 12),
                 ("conv2_offcentre", 300, 64): (102, 1), ("conv2_offcentre", 37, 72): (102, 2)})
S2_FOLD_SHAPE = (8, 6, 2, 256, 0.5, 2)                    # B, C, K, T, p, step of ONE msig_train_step_multi over three folds
# per fold: (regime or None = init_params as they are, init_params seed, input seed, dropout seed)
S2_FOLD_CASES = [("conv2_offcentre", 81, 40, 1000), ("conv_rows", 82, 14, 1001), (None, 83, 42, 1002)]
S2_EVAL_B, S2_EVAL_XSEED = 5, 21        # eval after train: conv2_offcentre at ONE, then an eval forward of 5 other windows
S2_ADAPT = ("cnn_gru_attention", 6, 2)  # kind, C, layers of the AdaBN case (tests/test_adapt_gpu.py's model and windows)


def gru_gates64(params, xs, hs, layer=0, reverse=False):
    """r, 1 - z and n (float64 arrays (B, T', H)) of one GRU direction, from its fp64 input sequence xs (B, T', I) and ITS OWN output
    hs (B, T', H): the previous state of step t is hs[t - 1] (hs[t + 1] in the reverse direction), zero at the first step.
    1 - z is computed as sigmoid(-a), without cancellation."""
    sfx = f"_l{layer}" + ("_reverse" if reverse else "")
    W_ih, W_hh, b_ih, b_hh = (np.asarray(params["gru." + n + sfx], dtype=np.float64) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
    xs, hs = np.asarray(xs, dtype=np.float64), np.asarray(hs, dtype=np.float64)
    H = W_hh.shape[1]
    prev = np.zeros_like(hs)
    if reverse:
        prev[:, :-1] = hs[:, 1:]
    else:
        prev[:, 1:] = hs[:, :-1]
    gi, gh = xs @ W_ih.T + b_ih, prev @ W_hh.T + b_hh
    sig = lambda a: np.where(a >= 0, 1.0 / (1.0 + np.exp(-np.abs(a))), np.exp(-np.abs(a)) / (1.0 + np.exp(-np.abs(a))))
    r = sig(gi[..., :H] + gh[..., :H])
    one_minus_z = sig(-(gi[..., H:2 * H] + gh[..., H:2 * H]))
    n = np.tanh(gi[..., 2 * H:] + r * gh[..., 2 * H:])
    return r, one_minus_z, n
