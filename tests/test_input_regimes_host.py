"""CPU tier: what keeps tests/test_input_regimes_gpu.py honest, from the oracle alone (tests/input_regimes.py; DESIGN.md "Input regimes").

For every (regime, shape, seeds) of the GPU file's tables:
  - every `own` — the fp32 oracle's disagreement with the fp64 oracle, which the GPU tolerances scale — is at most OWN_CAP, so no case
    is ill-conditioned enough to widen its own tolerance;
  - the regime is active in the fp64 oracle's stages (input_regimes.assert_input_regime_active);
  - at C >= 4 the gate MLP's hidden unit is live: both channel_attention gradients are non-zero in fp64;
  - the fp32 and the fp64 oracle disagree on at most MAX_ADOPTED pooling decisions (gpu_common.run_case's cap on adopted near-ties:
    two correct fp32 implementations differ from fp64 in about as many windows as this one does)."""
import numpy as np
import pytest
import torch

import input_regimes as IR
from gpu_common import rel_err
from oracle import cnn_gru_oracle as O
from test_trained_regimes_gpu import OWN_CAP

MAX_ADOPTED = 8
STAGE_KEYS = sorted({(c[0],) + c[1:6] + c[7:] for c in IR.STAGE_CASES}, key=str)      # without the kernel form: the oracle has none


def _assert_case(regime, own, st64, g64, flips, C, gated=True):
    over = {k: v for k, v in own.items() if not (v <= OWN_CAP)}
    assert not over, f"the fp32 oracle's own error exceeds {OWN_CAP}: {over}"
    IR.assert_input_regime_active(regime, st64)
    if gated and C >= 4 and g64:
        for k in ("channel_attention.fc.0.weight", "channel_attention.fc.2.weight"):
            assert float(np.abs(g64[k]).max()) > 0, f"the gate MLP is dead: the oracle's gradient of {k} is exactly zero"
    assert flips <= MAX_ADOPTED, f"the fp32 and the fp64 oracle disagree on {flips} pooling decisions"


def test_transforms_do_what_they_say():
    x, _ = IR.base_input(12, 6, 2, 96, 1)
    spread = x.astype(np.float64).std(axis=(0, 2))
    off = IR.apply(x, "offset", signs=IR.SIGNS[6]).astype(np.float64)
    assert np.allclose((off - x).mean(axis=(0, 2)), 10.0 * np.asarray(IR.SIGNS[6]) * spread, rtol=1e-5)
    assert np.allclose(off.std(axis=(0, 2)), spread, rtol=1e-4)
    assert np.array_equal(IR.apply(x, "units_small"), (x.astype(np.float64) * 1e-3).astype(np.float32))
    assert np.array_equal(IR.apply(x, "units_large"), (x.astype(np.float64) * 30).astype(np.float32))
    sp = IR.apply(x, "spikes")
    hit = sp != x
    assert 0 < hit.sum() < 0.01 * x.size and (np.abs(sp[hit]) == 50.0).all()
    zs = IR.apply(x, "zero_span")
    for b in range(12):
        col = (zs[b] == 0).all(axis=0)
        assert (col.sum() >= 32) == (b % 2 == 0)                                  # a span of T / 3 across all channels
        assert ((zs[b] == 0).all(axis=1).sum() == 1) == (b % 3 == 1)              # one whole channel
    fl = IR.apply(x, "flat")
    assert (fl[::3] == fl[::3, :, :1]).all() and len(np.unique(fl[0, :, 0])) == 6
    assert np.array_equal(fl[1], x[1]) and np.array_equal(fl[2], x[2])
    assert np.array_equal(IR.apply(x, "spikes"), sp)                              # a fixed seed
    with pytest.raises(KeyError):
        IR.apply(x, "nonsense")


def test_activity_conditions_reject_the_base_input():
    """Each condition fails on the untransformed input of the main shape: it is the regime that makes it true."""
    B, C, K, T, p = IR.MAIN
    params = {k: v.numpy() for k, v in O.init_params(C, K, seed=82).items()}
    x, y = IR.base_input(B, C, K, T, 4)
    _, st64, _, _ = IR.oracle_report(params, x, y, dropout_p=p, seed=1234, step=3)
    for regime in IR.REGIMES:
        with pytest.raises(AssertionError):
            IR.assert_input_regime_active(regime, st64)


@pytest.mark.parametrize("regime,B,C,K,T,p,pseed,xseed,signs", STAGE_KEYS, ids=lambda v: None if isinstance(v, (tuple, type(None))) else str(v))
def test_stage_cases_are_well_conditioned_active_and_live(regime, B, C, K, T, p, pseed, xseed, signs):
    params, x, y = IR.build_case(regime, B, C, K, T, pseed, xseed, signs)
    own, st64, g64, flips = IR.oracle_report(params, x, y, dropout_p=p, seed=1234, step=3)
    _assert_case(regime, own, st64, g64, flips, C)


@pytest.mark.parametrize("regime,pseed,xseed,seed,signs", IR.FOLD_CASES, ids=[c[0] for c in IR.FOLD_CASES])
def test_fold_cases_are_well_conditioned_active_and_live(regime, pseed, xseed, seed, signs):
    B, C, K, T, p = IR.FOLD_SHAPE
    params, x, y = IR.build_case(regime, B, C, K, T, pseed, xseed, signs)
    own, st64, g64, flips = IR.oracle_report(params, x, y, dropout_p=p, seed=seed, step=IR.FOLD_STEP)
    _assert_case(regime, own, st64, g64, flips, C)


def eval_case():
    """(params with foreign running statistics, x) of the eval-mode case: means of +-3, variances of 1e-3, 1 and 50, drawn as
    test_trained_regimes_gpu._bn_affine_eval_case draws them."""
    regime, B, C, K, T, pseed, xseed, signs = IR.EVAL_CASE
    params, x, _ = IR.build_case(regime, B, C, K, T, pseed, xseed, signs)
    rs = np.random.RandomState(7)
    for idx, ch in ((1, 16), (5, 32)):
        params[f"cnn_encoder.{idx}.running_mean"] = rs.choice([-3.0, 3.0], size=ch).astype(np.float32)
        params[f"cnn_encoder.{idx}.running_var"] = rs.choice([1e-3, 1.0, 50.0], size=ch).astype(np.float32)
    return params, x


def test_eval_case_is_well_conditioned_and_active():
    params, x = eval_case()
    own, st64, _, flips = IR.oracle_report(params, x, np.zeros(len(x), dtype=np.int64), training=False)
    assert own["logits"] <= OWN_CAP, own
    IR.assert_input_regime_active(IR.EVAL_CASE[0], st64)
    assert flips <= MAX_ADOPTED


def module_case(kind, regime, B, C, K, T, model_seed, xseed):
    """(state_dict as the oracle reads it, x, y) of a case that runs through the nn.Modules: nn's initialisation under
    torch.manual_seed(model_seed) — what tests/test_input_grad_gpu.py and test_channel_class_range_gpu.py build on the device."""
    from multimodalsignal_amd.models import CnnGruAttentionModel, CnnGruModel
    torch.manual_seed(model_seed)
    m = (CnnGruAttentionModel(C, K, dropout=0.5) if kind == "cnn_gru_attention" else CnnGruModel(C, K))
    named = {k: v.detach().clone() for k, v in m.state_dict().items()}
    if kind == "cnn_gru":
        named["channel_attention.fc.0.weight"], named["channel_attention.fc.2.weight"] = torch.zeros(0, C), torch.zeros(C, 0)
    x, y = IR.base_input(B, C, K, T, xseed)
    return named, torch.as_tensor(IR.apply(x, regime, signs=IR.case_signs(regime, B, C, T))), torch.as_tensor(y)


def _module_report(named, x, y, fw):
    import test_input_grad_gpu as IG
    dx64, g64, st64 = IG._oracle(named, x, y, torch.float64, True, fw)
    choice = {"pool" + k[-1]: O.first_argmax(O.pool_windows(torch.clamp_min(st64[k].detach(), 0))) for k in ("bn1", "bn2")}
    dx32, g32, st32 = IG._oracle(named, x, y, torch.float32, True, fw, pool_choice=choice)
    own = {k: rel_err(st32[k].detach().numpy(), st64[k].detach().numpy()) for k in ("conv1", "pool1", "pool2", "feat", "logits")}
    own.update({"grad/" + k: rel_err(g32[k].numpy(), g64[k].numpy()) for k in g64 if g64[k].numel()})
    own["grad/x"] = rel_err(dx32.numpy(), dx64.numpy())
    _, _, free32 = IG._oracle(named, x, y, torch.float32, True, fw)
    flips = sum(int((O.first_argmax(O.pool_windows(torch.clamp_min(free32[k].detach(), 0))) != choice["pool" + k[-1]]).sum()) for k in ("bn1", "bn2"))
    return own, {k: v.detach().numpy() for k, v in st64.items()}, {k: v.numpy() for k, v in g64.items()}, flips


@pytest.mark.parametrize("regime,B,C,T,mseed", IR.XGRAD_CASES, ids=[c[0] for c in IR.XGRAD_CASES])
def test_input_gradient_cases_are_well_conditioned_active_and_live(regime, B, C, T, mseed):
    K = 2 + (C + B) % 2
    named, x, y = module_case("cnn_gru_attention", regime, B, C, K, T, mseed, 10 * C + B)
    own, st64, g64, flips = _module_report(named, x, y, dict(dropout_p=0.5, seed=1000 + C, step=1))
    _assert_case(regime, own, st64, g64, flips, C)


def test_cnn_gru_case_is_well_conditioned_and_active(monkeypatch):
    regime, B, C, K, T = IR.CNN_GRU_CASE
    monkeypatch.setattr(O, "channel_gate", lambda x_, W1, W2: (x_.mean(dim=2), torch.zeros(x_.shape[0], 0, dtype=x_.dtype),
                                                                torch.ones(x_.shape[0], x_.shape[1], dtype=x_.dtype)))
    named, x, y = module_case("cnn_gru", regime, B, C, K, T, C + T, 7 * B + T)
    own, st64, g64, flips = _module_report(named, x, y, dict(dropout_p=0.5, seed=31, step=1))
    _assert_case(regime, own, st64, g64, flips, C, gated=False)


def test_adapt_case_is_well_conditioned_and_active():
    """The AdaBN case added to tests/test_adapt_gpu.py: `own` of the four adapted statistics in tests/ab_reference.py's two modes."""
    import ab_reference as R
    import test_adapt_gpu as AG
    kind, C, layers, regime = IR.ADAPT_CASE
    named, x = AG._named(kind, C, 20 + C, layers), torch.as_tensor(AG._x_host(C, seed=30 + C, regime=regime))
    r64 = R.adapt(named, O.init_buffers(), x, batch=16, kind=kind)
    r32 = R.adapt(named, O.init_buffers(), x, batch=16, kind=kind, dtype=torch.float32)
    own = {k: rel_err(r32[k].numpy(), r64[k].numpy()) for k in R.KEYS}
    assert max(own.values()) <= OWN_CAP, own
    p64 = {k: torch.as_tensor(v).double() for k, v in named.items()}
    IR.assert_input_regime_active(regime, {"conv1": R.conv1_out(p64, x.double(), kind).numpy()})
