"""Input regimes for the parity tests (tests/test_input_regimes_host.py, tests/test_input_regimes_gpu.py; DESIGN.md "Input regimes").

Every other parity test draws its windows as randn * (0.5 + rand) + randn(1, C, 1): unit-scale noise, a per-channel offset of at
most ~2 sigma.  apply() moves a copy of such a batch to where real inputs sit, one aspect at a time:
  offset       a per-channel constant of +-10 x that channel's spread (a temperature or accelerometer column; a test subject under
               --norm-reference baseline:K): the BatchNorm batch statistics of conv1 are then sums of large, nearly equal numbers
  units_small  x * 1e-3: the batch variance of some conv1 channel falls below BatchNorm's eps, so where eps sits matters
  units_large  x * 30 (x * 100 and x * 1e3 are ill-conditioned in the oracle itself: `own` 2.6e-5 and 2.3e-4)
  spikes       about 1 sample in 500 set to +-50
  zero_span    every second window: a span of T / 3 zeroed across all channels; every third window: one whole channel zeroed
               (what --augment mask=..., chandrop=... produce)
  flat         every third window constant in time, each channel at its own value
The CASE tables below are the ONE place that fixes shapes, seeds and offset signs: the host file proves with the oracle alone that
every case is well-conditioned (`own` <= OWN_CAP), active, has a live gate MLP and few fp32 / fp64 pooling disagreements; the GPU
file then holds the HIP path to the project's unchanged tolerances on exactly those cases."""
import numpy as np
import torch

from oracle import cnn_gru_oracle as O

REGIMES = ("offset", "units_small", "units_large", "spikes", "zero_span", "flat")
OFFSET_SPREADS, SMALL, LARGE, SPIKE_RATE, SPIKE_VALUE = 10.0, 1e-3, 30.0, 1.0 / 500.0, 50.0
TRANSFORM_SEED = 9

# thresholds of the activity conditions (conditions on the fp64 oracle's stages, not tolerances)
OFFSET_MIN_MEAN_OVER_STD = 7.0      # conv1: max over channels of |batch mean| / batch std
SMALL_MAX_VAR = 1e-5                # conv1: some channel's batch variance below BatchNorm's eps
SPIKE_MIN_PEAK_OVER_STD = 10.0      # conv1: max |y| / its channel's batch std (11.8 at MAIN; 5.2 - 6.0 in the regimes without spikes)
MIN_EXACT_TIE_WINDOWS = 16          # bn1: pooling windows whose three candidates are exactly equal


def alternating(C):
    return tuple(1.0 if c % 2 == 0 else -1.0 for c in range(C))


def apply(x, name, rs=None, signs=None):
    """A float32 copy of the batch x (B, C, T) in regime `name`.  rs (np.random.RandomState, default seed TRANSFORM_SEED) draws what
    the regime leaves open; signs (length C, default + - + - ...) are the offset regime's."""
    if name not in REGIMES:
        raise KeyError(name)
    rs = np.random.RandomState(TRANSFORM_SEED) if rs is None else rs
    x = np.array(x, dtype=np.float64, copy=True)
    B, C, T = x.shape
    if name == "offset":
        sg = np.asarray(alternating(C) if signs is None else signs, dtype=np.float64)
        assert sg.shape == (C,) and (np.abs(sg) == 1).all()
        x += (OFFSET_SPREADS * sg * x.std(axis=(0, 2)))[None, :, None]
    elif name == "units_small":
        x *= SMALL
    elif name == "units_large":
        x *= LARGE
    elif name == "spikes":
        m = rs.rand(B, C, T) < SPIKE_RATE
        x[m] = SPIKE_VALUE * np.sign(rs.randn(int(m.sum())))
    elif name == "zero_span":
        for b in range(0, B, 2):
            s = rs.randint(0, T - T // 3 + 1)
            x[b, :, s:s + T // 3] = 0.0
        for b in range(1, B, 3):
            x[b, rs.randint(0, C)] = 0.0
    else:
        x[::3] = x[::3, :, :1]
    return x.astype(np.float32)


def base_input(B, C, K, T, xseed):
    """The usual window batch and labels, drawn as tests/test_parity_gpu.py draws them."""
    rs = np.random.RandomState(xseed)
    x = (rs.randn(B, C, T) * (0.5 + rs.rand(1, C, 1)) + rs.randn(1, C, 1)).astype(np.float32)
    y = rs.randint(0, K, size=(B,)).astype(np.int64)
    return x, y


def build_case(regime, B, C, K, T, pseed, xseed, signs=None):
    """(params, x, y): oracle.init_params(seed = pseed) and the base input of seed xseed moved into `regime`."""
    params = {k: v.numpy() for k, v in O.init_params(C, K, seed=pseed).items()}
    x, y = base_input(B, C, K, T, xseed)
    return params, apply(x, regime, signs=signs), y


def exact_tie_windows(bn):
    """Number of MaxPool windows of a BatchNorm output (B, CH, L) whose three candidates are all real and exactly equal."""
    win = O.pool_windows(torch.as_tensor(bn))
    return int(((win[..., 0] == win[..., 1]) & (win[..., 1] == win[..., 2])).sum())


def assert_input_regime_active(regime, st64):
    """The regime's defining condition holds in the fp64 oracle's stages (numpy arrays), so that no case passes vacuously."""
    y = np.asarray(st64["conv1"], dtype=np.float64)
    mean, std = y.mean(axis=(0, 2)), y.std(axis=(0, 2))
    if regime == "offset":
        r = float(np.abs(mean / std).max())
        assert r >= OFFSET_MIN_MEAN_OVER_STD, f"conv1: max |mean / std| = {r:.2f}"
    elif regime == "units_small":
        assert float((std ** 2).min()) < SMALL_MAX_VAR, f"conv1: smallest batch variance {float((std ** 2).min()):.2e}"
    elif regime == "units_large":
        assert float(std.max()) > 10.0, f"conv1: largest batch std {float(std.max()):.2f}"
    elif regime == "spikes":
        r = float((np.abs(y) / std[None, :, None]).max())
        assert r >= SPIKE_MIN_PEAK_OVER_STD, f"conv1: max |y| / std = {r:.1f}"
    else:
        n = exact_tie_windows(st64["bn1"])
        assert n >= MIN_EXACT_TIE_WINDOWS, f"bn1: {n} pooling windows with three exactly equal candidates"


# ---- the frozen case tables ------------------------------------------------------------------------------------------------------------
MAIN = (24, 6, 2, 256, 0.5)
RAGGED = (37, 3, 3, 72, 0.25)
LONG = (4, 6, 2, 3840, 0.5)
MANY = (3100, 6, 2, 64, 0.5)           # many items per thread of the persistent conv grids; default kernel selection
# Seeds and offset signs, chosen with tests/test_input_regimes_host.py and frozen here.  The gate's pre-activation is W1 . mean_t x, so
# an offset's signs decide whether the gate MLP's hidden unit is live and how far its gradients cancel: at MAIN under input seed 4,
# + - + - + - leaves `own` of channel_attention.fc.0.weight at 1.4e-5 and - - - - - - at 3.9e-5 (over OWN_CAP); - + - + - + kills the unit.
PM, MP = (1.0, -1.0), (-1.0, 1.0)
PPMM6, HALVES16 = (1.0, 1.0, -1.0, -1.0, 1.0, 1.0), (1.0,) * 8 + (-1.0,) * 8
PSEED = {6: 82}                        # oracle.init_params seed (default 100 + C): at C = 6 seeds 77 and 78 have a dead gate MLP
XSEED = {(24, 256): 4, (4, 3840): 2}   # input seed (default 7 B + T), as tests/test_trained_regimes_gpu.py has them
# (regime, B, T) -> (input seed, offset signs) where the defaults are ill-conditioned in the oracle itself
OVERRIDE = {("offset", 24, 256): (5, PM * 3), ("units_large", 24, 256): (6, None), ("offset", 3100, 64): (1, PPMM6),
            ("offset", 4, 3840): (2, PPMM6)}
SIGNS = {1: (1.0,), 3: (1.0, -1.0, 1.0), 6: PM * 3, 9: PM * 4 + (1.0,), 16: HALVES16}


def case_signs(regime, B, C, T):
    if regime != "offset":
        return None
    signs = OVERRIDE.get((regime, B, T), (None, None))[1]
    return SIGNS.get(C, alternating(C)) if signs is None else signs


def _case(regime, shape, form):
    B, C, K, T, p = shape
    xseed = OVERRIDE.get((regime, B, T), (None, None))[0]
    xseed = XSEED.get((B, T), 7 * B + T) if xseed is None else xseed
    return (regime, B, C, K, T, p, form, PSEED.get(C, 100 + C), xseed, case_signs(regime, B, C, T))


# (regime, B, C, K, T, p, form, init_params seed, input seed, offset signs); form "auto" = the default selection
STAGE_CASES = ([_case(r, MAIN, f) for r in REGIMES for f in ("ws6", "split")]
               + [_case(r, RAGGED, f) for r in ("offset", "zero_span") for f in ("ws6", "split")]
               + [_case(r, LONG, "ws6") for r in ("offset", "zero_span")]
               + [_case(r, MANY, "auto") for r in ("offset", "zero_span")]
               + [_case("offset", (5, C, 2, 264, 0.5), "split") for C in (1, 3, 16)])
# one msig_train_step_multi: (regime, init_params seed, input seed, dropout seed, offset signs) per fold
FOLD_SHAPE, FOLD_STEP = (64, 6, 2, 256, 0.5), 2
FOLD_CASES = [("offset", 82, 43, 1000, PPMM6), ("units_small", 83, 41, 1001, None), ("zero_span", 81, 42, 1002, None)]
EVAL_CASE = ("offset", 17, 6, 2, 256, 82, 3, PM * 3)               # regime, B, C, K, T, init_params seed, input seed, signs
# regime, B, C, T, torch.manual_seed of the model (nn's initialisation, as tests/test_input_grad_gpu.py builds it): under 11 = C + B the
# gate MLP is dead on the zero_span input
XGRAD_CASES = [("offset", 5, 6, 511, 11), ("zero_span", 5, 6, 511, 14)]
CNN_GRU_CASE = ("offset", 5, 9, 3, 137)                            # regime, B, C, K, T: test_channel_class_range_gpu's cnn_gru helper
ADAPT_CASE = ("cnn_gru_attention", 6, 2, "offset")                 # kind, C, layers, regime (tests/test_adapt_gpu.py)


# ---- what the oracle alone says about a case -------------------------------------------------------------------------------------------
def oracle_report(named, x, y, training=True, **fw):
    """The fp64 and the fp32 oracle on one case: (`own` of every stage, stage gradient and parameter gradient; the fp64 stages as
    numpy arrays; the fp64 gradients; the number of pooling decisions on which the fp64 oracle and a FREE fp32 run disagree — free: no
    decision of either stage adopted, as two independent implementations meet each other)."""
    from gpu_common import rel_err, split_named, to_t
    out, choice = {}, None
    for dt in (torch.float64, torch.float32):
        p, b = split_named(to_t(named, dt))
        for k, v in O.init_buffers(dt).items():
            b.setdefault(k, v)
        xt, yt = torch.as_tensor(x).to(dt), torch.as_tensor(y)
        if training:      # the fp32 run pools through the fp64 run's windows, as gpu_common.run_case has it: `own` measures arithmetic
            _, g, st, _ = O.loss_and_grads(p, b, xt, yt, retain=True, pool_choice=choice, **fw)
        else:
            with torch.no_grad():
                st, _ = O.forward(p, b, xt, training=False, pool_choice=choice)
            g = {}
        if choice is None:
            choice = {"pool" + k[-1]: O.first_argmax(O.pool_windows(torch.clamp_min(st[k].detach(), 0))) for k in ("bn1", "bn2")}
        out[dt] = ({k: v.detach().numpy() for k, v in st.items()}, {k: v.numpy() for k, v in g.items()})
    (st64, g64), (st32, g32) = out[torch.float64], out[torch.float32]
    own = {k: rel_err(st32[k], st64[k]) for k in st64 if k not in ("gate_mean", "gate_pre")}
    own.update({("d_" + k[6:] if k.startswith("stage/") else "grad/" + k): rel_err(g32[k], g64[k]) for k in g64})
    with torch.no_grad():      # p, b, xt are the fp32 run's
        free32, _ = O.forward(p, b, xt, training=training, **(fw if training else {}))
    flips = sum(int((O.first_argmax(O.pool_windows(torch.clamp_min(free32[k], 0))) != choice["pool" + k[-1]]).sum()) for k in ("bn1", "bn2"))
    return own, st64, g64, flips
