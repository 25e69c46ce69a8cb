"""GPU tier: the HIP path against the fp64 oracle over INPUT regimes (tests/input_regimes.py; DESIGN.md "Input regimes").

Every other parity test feeds unit-scale noise with a per-channel offset of at most ~2 sigma.  Here the windows carry offsets of 10
spreads per channel (conv1's one-pass BatchNorm sums: E[y^2] - mean^2 cancels), are scaled by 1e-3 (a batch variance below BatchNorm's
eps) and by 30, carry +-50 spikes, exact-zero spans and all-zero channels (what --augment mask / chandrop feed: exact three-way pooling
ties), and windows that are constant in time.  The tolerances are the project's own, unchanged (gpu_common.stage_tol / grad_tol,
OWN_CAP); the cases, seeds and offset signs are input_regimes' tables, which tests/test_input_regimes_host.py holds, with the oracle
alone, to: `own` <= OWN_CAP, the regime active, the gate MLP live, at most 8 fp32 / fp64 pooling disagreements.  Each case asserts the
first three again on what it actually ran.  Negative controls: make negctl INPUT=k, tools/negative_controls.sh input,
profiles/input_negative_control.log."""
import ctypes as Ct

import numpy as np
import pytest
import torch

import input_regimes as IR
from oracle import cnn_gru_oracle as O
from test_input_regimes_host import eval_case, module_case
from test_parity_gpu import FORMS
from test_trained_regimes_gpu import OWN_CAP, assert_own_capped, oracle_stages64, run_case_own

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


def check_case(regime, eng, named, x, rep, ref, own, fw):
    from gpu_common import failures, format_report
    print("\n" + format_report(rep))
    assert_own_capped(own)
    IR.assert_input_regime_active(regime, oracle_stages64(named, x, **fw))
    if eng.C >= 4:
        for k in ("channel_attention.fc.0.weight", "channel_attention.fc.2.weight"):
            assert float(ref[1][k].abs().max()) > 0, f"the gate MLP is dead: the oracle's gradient of {k} is exactly zero"
    assert bool(torch.isfinite(eng.grads).all()), "a gradient of the HIP path is not finite"
    assert not failures(rep), format_report(rep)


@pytest.mark.parametrize("regime,B,C,K,T,p,form,pseed,xseed,signs", IR.STAGE_CASES,
                         ids=["-".join(map(str, c[:7])) for c in IR.STAGE_CASES])
def test_input_regime_stages_against_oracle(regime, B, C, K, T, p, form, pseed, xseed, signs, dev, kernel_forms, monkeypatch, tmp_path):
    from multimodalsignal_amd.runtime import Engine
    kernel_forms(*FORM_PAIRS[form])
    params, x, y = IR.build_case(regime, B, C, K, T, pseed, xseed, signs)
    eng = Engine(C, K, dev)
    fw = dict(dropout_p=p, seed=1234, step=3)
    rep, ref, own = run_case_own(monkeypatch, tmp_path, eng, params, x, y, tag=f"input_{regime}_{form}", **fw)
    check_case(regime, eng, params, x, rep, ref, own, fw)


@pytest.mark.parametrize("forms", [("auto", "auto"), ("ws", "b6")], ids=["offset+units_small+zero_span-auto", "offset+units_small+zero_span-ws_b6"])
def test_fold_batch_input_regimes_against_oracle(forms, dev, kernel_forms, monkeypatch, tmp_path):
    """ONE msig_train_step_multi over three folds whose inputs sit in three different regimes (built as
    test_trained_regimes_gpu.test_fold_batch_regimes_against_oracle builds its launch): every fold is held to the oracle, so one fold's
    BatchNorm statistics — sums 100 times its neighbour's, or a variance below eps — must not leak into another's."""
    from multimodalsignal_amd import _lib as L
    from multimodalsignal_amd.runtime import FoldArena
    kernel_forms(*forms)
    (B, Cc, K, T, p), step, NF = IR.FOLD_SHAPE, IR.FOLD_STEP, len(IR.FOLD_CASES)
    arena = FoldArena(Cc, K, dev, NF, B, T)
    engines, cases = [arena.engine(s) for s in range(NF)], []
    for f, (regime, pseed, xseed, seed, signs) in enumerate(IR.FOLD_CASES):
        params, x, y = IR.build_case(regime, B, Cc, K, T, pseed, xseed, signs)
        engines[f].load_named({k: torch.as_tensor(v) for k, v in params.items()})
        arena.view(f, "x", torch.float32)[:x.size].copy_(torch.as_tensor(x).reshape(-1))
        arena.view(f, "y", torch.int64)[:B].copy_(torch.as_tensor(y))
        engines[f].workspace(B, T, True)
        engines[f]._last = (B, T, True)
        cases.append((regime, params, x, y, seed))
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
        rep, ref, own = run_case_own(monkeypatch, tmp_path, engines[f], params, x, y, launch=launch, tag=f"input_multi_{regime}_{forms[1]}", **fw)
        check_case(regime, engines[f], params, x, rep, ref, own, fw)


def test_eval_mode_offset_input_with_foreign_running_statistics(dev):
    """Engine.forward(training=False) on an offset input with running statistics that are no golden file's own (means of +-3, variances
    of 1e-3, 1 and 50) against the fp64 oracle's eval-mode logits, as test_bn_affine_eval_mode_with_foreign_running_statistics does;
    bn_state is untouched."""
    from gpu_common import rel_err, split_named, stage_tol, to_t
    from multimodalsignal_amd.runtime import Engine
    params, x = eval_case()
    B, C, T = x.shape
    K = params["classifier.3.weight"].shape[0]
    st64 = oracle_stages64(params, x, training=False)
    IR.assert_input_regime_active(IR.EVAL_CASE[0], st64)
    ref = st64["logits"]
    p32, b32 = split_named(to_t(params))
    with torch.no_grad():
        st32, _ = O.forward(p32, {**O.init_buffers(), **b32}, torch.as_tensor(x), training=False)
    own = rel_err(st32["logits"].numpy(), ref)
    assert own <= OWN_CAP, own
    eng = Engine(C, K, dev)
    eng.load_named({k: torch.as_tensor(v) for k, v in params.items()})
    before, count = eng.bn_state.clone(), eng.bn_count.clone()
    assert float(before[:16].abs().min()) == 3.0 and float(before[16:32].min()) == pytest.approx(1e-3)      # the statistics did load
    eng.forward(torch.as_tensor(x).to(dev), None, training=False)
    torch.cuda.synchronize()
    got = eng.region("LOGITS", torch.float32, (B, K)).cpu().numpy()
    err, tol = rel_err(got, ref), stage_tol("logits", own)
    print(f"eval logits err={err:.3e} tol={tol:.1e} own={own:.2e}")
    assert np.isfinite(got).all() and err <= tol, (err, tol, own)
    assert torch.equal(before, eng.bn_state) and torch.equal(count, eng.bn_count)


@pytest.mark.parametrize("regime,B,C,T,mseed", IR.XGRAD_CASES, ids=[c[0] for c in IR.XGRAD_CASES])
def test_train_mode_input_gradient_under_input_regimes(regime, B, C, T, mseed, dev):
    """Train-mode dL/dx and every parameter gradient through CnnGruAttentionModel and autograd, by tests/test_input_grad_gpu.py's
    comparison (T = 511: position-wise staging of dy1), dropout 0.5."""
    import test_input_grad_gpu as IG
    K = 2 + (C + B) % 2
    m = IG._model(C, K, "full", 0.5, dev, seed=mseed).train()
    m.set_dropout_seed(1000 + C)
    named, x, y = module_case("cnn_gru_attention", regime, B, C, K, T, mseed, 10 * C + B)
    for k, v in m.state_dict().items():
        assert torch.equal(v.cpu(), named[k]), k                      # the model the host file judged
    xd = x.to(dev).requires_grad_(True)
    torch.nn.CrossEntropyLoss()(m(xd), y.to(dev)).backward()
    torch.cuda.synchronize()
    assert xd.grad is not None and xd.grad.shape == x.shape and bool(torch.isfinite(xd.grad).all()) and float(xd.grad.abs().max()) > 0
    fw = dict(dropout_p=0.5, seed=1000 + C, step=1)
    IR.assert_input_regime_active(regime, oracle_stages64({k: v.numpy() for k, v in named.items()}, x.numpy(), **fw))
    IG._check_against_oracle(m, named, x, y, xd.grad.cpu().numpy(), True, fw)


def test_cnn_gru_kind_offset_input_against_oracle(dev, monkeypatch):
    """The cnn_gru kind (conv1_fwd_kernel<0, false>: ungated taps, the same statistics code) on an offset input, through
    test_channel_class_range_gpu's helper for that kind with its inputs moved into the regime: stages, loss, every gradient and dL/dx."""
    import test_channel_class_range_gpu as RC
    regime, B, C, K, T = IR.CNN_GRU_CASE
    named, x, y = module_case("cnn_gru", regime, B, C, K, T, C + T, 7 * B + T)
    seen = []

    def inputs(B_, C_, K_, T_, seed):
        xb, yb = IR.base_input(B_, C_, K_, T_, seed)
        assert np.array_equal(yb, y.numpy())
        seen.append(1)
        return x, y

    monkeypatch.setattr(RC, "_inputs", inputs)
    RC.test_cnn_gru_kind_against_oracle(B, C, K, T, dev, monkeypatch)
    assert seen
    st64 = oracle_stages64({k: v.numpy() for k, v in named.items()}, x.numpy(), dropout_p=0.5, seed=31, step=1)      # O.channel_gate is still patched to s = 1
    IR.assert_input_regime_active(regime, st64)
