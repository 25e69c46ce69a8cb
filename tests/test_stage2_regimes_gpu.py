"""GPU tier: the HIP path against the fp64 oracle where conv2's channels sit far off centre or have no spread (tests/regimes.py
bn1_always_on, conv2_offcentre, conv_rows; DESIGN.md "Stage-2 regimes").

Stage 1 and stage 2 of the front end form their BatchNorm batch statistics in different kernels (conv1_fwd_kernel,
pool1_conv2_fwd_kernel), and every other parity case leaves conv2's channels at mean^2 / var <= 6.9.  Here BatchNorm-1 has "always on"
channels (small gamma, positive beta) and eight of conv2's output rows are one-signed: conv2's channels reach mean^2 / var of 16 .. 200
(bn1_always_on) and 500 .. 1300 (conv2_offcentre) beside channels below 1, where a one-pass variance E[y^2] - mean^2 loses that factor
of its relative precision; conv_rows has an exactly zero, a 1e-3 and a 1e3 output row in both convolutions (var == 0 and
invstd == 1 / sqrt(eps); var << eps; 1e6 in the fp32 sums of squares).  The shapes (regimes.S2_*) are chosen for where one-pass sums are
weakest — 1, 2 and 4 work items, nothing averages — and for the ragged, two-chunk and many-item paths of pool1_conv2_fwd_kernel.  The
tolerances are the project's own, unchanged (gpu_common.stage_tol / grad_tol, OWN_CAP); tests/test_stage2_regimes_host.py holds every
case, with the oracle alone, to: regime active, `own` <= OWN_CAP, gate MLP live, few pooling disagreements — and predicts the error.
Negative control: make negctl STAGE2=1, tools/negative_controls.sh stage2, profiles/stage2_negative_control.log.

pool1_conv2_fwd's grid is clamped to MSIG_PERSIST_WG = 1024 workgroups, so a thread accumulates more than one item only when
B * ceil(L2 / 128) > 1024.  No case of this file reaches that (the largest has 300 items); the smallest shape that would is
B = 1025 with one conv2 chunk (T <= 1020).  tests/test_input_regimes_gpu.py's (3100, 6, 2, 64) cases run that path on ordinary parameters."""
import ctypes as Ct

import numpy as np
import pytest
import torch

import regimes as RG
import test_trained_regimes_gpu as TR
from oracle import cnn_gru_oracle as O
from test_parity_gpu import FORMS
from test_stage2_regimes_host import (MODULE_CASES, MODULE_FW, adapt_case, build_fold_case, build_stage2_case, eval_after_train_oracle,
                                      eval_case, module_case)
from test_trained_regimes_gpu import OWN_CAP, check_case, run_case_own

pytestmark = pytest.mark.gpu
FORM_PAIRS = dict(FORMS, auto=("auto", "auto"))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tier needs an MI355X"
    return torch.device("cuda:0")


@pytest.fixture
def kernel_forms():
    from multimodalsignal_amd import _lib as L
    yield L.set_kernel_form
    L.set_kernel_form("auto", "auto")


def assert_conv_rows(eng, params, rep, ref):
    """conv_rows: the zeroed rows' channels have batch mean 0 and the stored invstd 1 / sqrt(eps) rounded to fp32, exactly, in both
    stages; their weight-gradient rows are LIVE in the oracle (dL/dw of a zero row is not zero) — and were compared like any other by
    the report — and finite on the device."""
    eps = np.float64(np.float32(1e-5))                       # Batch.bn_eps is a float
    gviews = eng.named_param_views(eng.grads)
    for sname, idx, CH in (("BN1_STAT", 0, 16), ("BN2_STAT", 4, 32)):
        zero, small, large = RG.conv_rows_channels(params, idx)
        stat = eng.region(sname, torch.float32, (4, CH)).cpu().numpy()
        assert stat[0, zero] == 0.0 and stat[1, zero] == np.float32(1.0 / np.sqrt(eps)), (sname, stat[:2, zero])
        assert stat[1, small] > 0.5 * np.float32(1.0 / np.sqrt(eps)), (sname, stat[1, small])      # eps dominates the 1e-3 row's invstd
        key = f"cnn_encoder.{idx}.weight"
        assert float(ref[1][key][zero].abs().max()) > 0, f"the oracle's gradient of the zeroed row of {key} is zero"
        assert bool(torch.isfinite(gviews[key][zero]).all()) and float(gviews[key][zero].abs().max()) > 0
        assert "grad/" + key in rep


@pytest.mark.parametrize("regime,B,C,K,T,p,form", RG.STAGE2_CASES, ids=["-".join(map(str, c)) for c in RG.STAGE2_CASES])
def test_stage2_regime_stages_against_oracle(regime, B, C, K, T, p, form, dev, kernel_forms, monkeypatch, tmp_path):
    from multimodalsignal_amd.runtime import Engine
    kernel_forms(*FORM_PAIRS[form])
    params, x, y = build_stage2_case(regime, B, C, K, T)
    eng = Engine(C, K, dev)
    fw = dict(dropout_p=p, seed=1234, step=3)
    rep, ref, own = run_case_own(monkeypatch, tmp_path, eng, params, x, y, tag=f"stage2_{regime}_{form}", **fw)
    if regime == "conv_rows":
        assert_conv_rows(eng, params, rep, ref)
    check_case(regime, eng, params, x, rep, ref, own, fw)


def test_fold_batch_stage2_regimes_against_oracle(dev, kernel_forms, monkeypatch, tmp_path):
    """ONE msig_train_step_multi over three folds of B = 8 — conv2_offcentre, conv_rows and untouched parameters — built as
    test_trained_regimes_gpu.test_fold_batch_regimes_against_oracle builds its launch: every fold is held to the oracle, so one fold's
    statistics (sums a thousand spreads off centre, a zero-variance channel) must not leak into a companion's rows under blockIdx.z."""
    from multimodalsignal_amd import _lib as L
    from multimodalsignal_amd.runtime import FoldArena
    kernel_forms("auto", "auto")
    (B, Cc, K, T, p, step), NF = RG.S2_FOLD_SHAPE, len(RG.S2_FOLD_CASES)
    arena = FoldArena(Cc, K, dev, NF, B, T)
    engines, cases = [arena.engine(s) for s in range(NF)], [build_fold_case(f) for f in range(NF)]
    for f, (regime, params, x, y, seed) in enumerate(cases):
        engines[f].load_named({k: torch.as_tensor(v) for k, v in params.items()})
        arena.view(f, "x", torch.float32)[:x.size].copy_(torch.as_tensor(x).reshape(-1))
        arena.view(f, "y", torch.int64)[:B].copy_(torch.as_tensor(y))
        engines[f].workspace(B, T, True)
        engines[f]._last = (B, T, True)
    m = arena.multi(list(range(NF)), key_gru=[L.dropout_key(c[4], step, 1) for c in cases],
                    key_head=[L.dropout_key(c[4], step, 2) for c in cases], lr=[1e-3] * NF, steps=[step] * NF)
    desc = arena.batch(B, True, p)
    done = []

    def launch(phase):
        if phase == "fwd" and not done:
            st = Ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            L.check(L.lib().msig_train_step_multi(Ct.byref(desc), Ct.byref(m), arena.ptr("exp_avg"), arena.ptr("exp_avg_sq"),
                                                  0.9, 0.999, 1e-8, 1e-4, step, st), "msig_train_step_multi")
            done.append(1)

    for f, (regime, params, x, y, seed) in enumerate(cases):
        fw = dict(dropout_p=p, seed=seed, step=step)
        rep, ref, own = run_case_own(monkeypatch, tmp_path, engines[f], params, x, y, launch=launch, tag=f"stage2_multi_{regime}", **fw)
        if regime == "conv_rows":
            assert_conv_rows(engines[f], params, rep, ref)
        check_case(regime, engines[f], params, x, rep, ref, own, fw)


@pytest.mark.parametrize("kind,config", MODULE_CASES)
def test_module_paths_conv2_offcentre_against_oracle(kind, config, dev, kernel_forms, monkeypatch):
    """conv2_offcentre through the embedded 32-unit engine and the cnn_gru kind at FEW's (4, 3, 2, 256), through the modules and autograd:
    test_trained_regimes_gpu.test_module_paths_regimes_against_oracle's comparison on the case tests/test_stage2_regimes_host.py judged."""
    def case(kind_, config_, regime, dev_):
        m, moved, x, y = module_case(kind_, config_)
        m = m.to(dev_).train()
        m.set_dropout_seed(MODULE_FW["seed"])
        return m, moved, x, y

    monkeypatch.setattr(TR, "_module_case", case)
    TR.test_module_paths_regimes_against_oracle(kind, config, "conv2_offcentre", "split", dev, kernel_forms, monkeypatch)


def test_eval_forward_after_a_training_forward_on_conv2_offcentre(dev):
    """ONE training forward of one window (one work item) from the default buffers, then an eval forward of five other windows: the
    running statistics of both BatchNorms against the fp64 oracle within FIXED_TOL — running_var of a channel a thousand spreads off
    centre is where a wrong batch variance persists — and the eval logits, which run under them, under stage_tol."""
    from gpu_common import FIXED_TOL, rel_err, stage_tol
    from multimodalsignal_amd.runtime import Engine
    params, x, y, xe = eval_case()
    B, C, T = x.shape
    K = params["classifier.3.weight"].shape[0]
    nb64, l64 = eval_after_train_oracle(params, x, xe, torch.float64)
    nb32, l32 = eval_after_train_oracle(params, x, xe, torch.float32)
    own = rel_err(l32, l64)
    assert own <= OWN_CAP, own
    eng = Engine(C, K, dev)
    eng.load_named({**{k: torch.as_tensor(v) for k, v in params.items()}, **O.init_buffers()})
    eng.forward(torch.as_tensor(x).to(dev), torch.as_tensor(y).to(dev), training=True, dropout_p=0.0, seed=1234, step=3)
    torch.cuda.synchronize()
    bn = eng.bn_state.cpu().numpy()
    for k, sl in (("cnn_encoder.1.running_mean", slice(0, 16)), ("cnn_encoder.1.running_var", slice(16, 32)),
                  ("cnn_encoder.5.running_mean", slice(32, 64)), ("cnn_encoder.5.running_var", slice(64, 96))):
        err, tol = rel_err(bn[sl], nb64[k]), FIXED_TOL["running_var" if "var" in k else "running_mean"]
        print(f"{k:30s} err={err:.3e} tol={tol:.1e} own={rel_err(nb32[k], nb64[k]):.2e}")
        assert err <= tol, (k, err, tol)
    eng.forward(torch.as_tensor(xe).to(dev), None, training=False)
    torch.cuda.synchronize()
    got = eng.region("LOGITS", torch.float32, (len(xe), K)).cpu().numpy()
    err, tol = rel_err(got, l64), stage_tol("logits", own)
    print(f"eval logits err={err:.3e} tol={tol:.1e} own={own:.2e}")
    assert np.isfinite(got).all() and err <= tol, (err, tol, own)
    assert np.array_equal(bn, eng.bn_state.cpu().numpy())                 # the eval forward leaves them alone


def test_adaptation_of_conv2_offcentre_statistics_against_the_float64_restatement():
    """adapt.BnAdapter on conv2_offcentre parameters: ab_merge_kernel reduces pool1_conv2_fwd's partial rows through the same
    bn_batch_sums as bn_finalize_kernel.  The four adapted statistics against tests/ab_reference.py in float64, by
    tests/test_adapt_gpu.py's gate: its rel_err and its stage_tol(name, own of the float32 restatement)."""
    import ab_reference as R
    import test_adapt_gpu as AG
    from multimodalsignal_amd import adapt as A
    kind, C, layers = RG.S2_ADAPT
    named, x = adapt_case()
    model = AG._model(kind, C, 20 + C, layers)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in named.items()}, strict=False)
    model = model.to(AG.DEV).eval()
    ad = A.BnAdapter([dict(model=model, x=torch.as_tensor(x, device=AG.DEV))], alpha=1.0, eval_batch=16)
    got = {k: v.cpu().numpy() for k, v in ad.adapted_buffers(0).items()}
    r64 = R.adapt(named, O.init_buffers(), torch.as_tensor(x), batch=16, kind=kind)
    r32 = R.adapt(named, O.init_buffers(), torch.as_tensor(x), batch=16, kind=kind, dtype=torch.float32)
    bad = {}
    for k in R.KEYS:
        own = AG.rel_err(r32[k].numpy(), r64[k].numpy())
        err, tol = AG.rel_err(got[k], r64[k].numpy()), AG.stage_tol(k, own)
        print(f"{k}: own {own:.3e} gpu {err:.3e} tol {tol:.3e}")
        assert own <= OWN_CAP
        if not err <= tol:
            bad[k] = (err, tol)
    assert not bad, bad
