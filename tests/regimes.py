"""Trained-like parameter regimes for the parity tests (tests/test_trained_regimes_gpu.py; DESIGN.md "Trained-like regimes").

oracle.cnn_gru_oracle.init_params — and nn's default initialisers — leave a model near initialisation: pre-activations of order 1,
BatchNorm gamma positive, logits of order 1.  apply() moves a copy of such a parameter set to where training takes it, one
aspect at a time, on any param_specs layout (two layers of 64 units, one layer of 32, with or without the gate's tensors).
Every regime MIXES saturated and ordinary units: with every unit of a layer saturated, fp32's quantisation of 1 - z alone puts
the fp32 oracle 6e-3 of the largest gradient away from the fp64 one, and a comparison says nothing."""
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
REGIMES = tuple(GATE_BIAS) + ("input_driven", "bn_affine", "head_sat")


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
    else:
        for k, factor in HEAD_SAT.items():
            out[k] = out[k] * np.asarray(factor, dtype=out[k].dtype)
    return out


def bn_channels(params_np, idx):
    """Channels of BatchNorm `idx` (1 or 5) by what the regime made of them: (gamma < 0, gamma == 0 and beta > 0, gamma == 0 and beta < 0)."""
    g, b = np.asarray(params_np[f"cnn_encoder.{idx}.weight"]), np.asarray(params_np[f"cnn_encoder.{idx}.bias"])
    return np.flatnonzero(g < 0), np.flatnonzero((g == 0) & (b > 0)), np.flatnonzero((g == 0) & (b < 0))


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
