"""GPU tier: the channel counts 7 and 9..15 and the class counts 5..16 that include/msig.h promises (MSIG_MAX_C = MSIG_MAX_K =
MSIG_MAX_FOLDS = 16) and no other test reaches ("Channel and class range").

C = 9..15 run the CT == 0 form of gate_kernel / conv1_fwd_kernel / conv1_bwd_kernel with a PARTIAL last block: 7C taps padded to
4 KM = 4 ceil(7C / 4) (zero-filled taps) and to 16 NB = 16 ceil(7C / 16) columns (padding columns that alias the last real one, NB16-
strided window records).  At C = 16, the only generic count of the other tests, 7C = 112 = 4 * 28 = 16 * 7 and every guard is always
true.  C = 7 is a compile-time instantiation of its own; Cr = C // 4 = 3 appears at C = 12..15 only; K > 4 (K > 8: dW3's register
slots 2 and 3 in head_bwd_kernel / head_step_kernel) at no other shape.  The tolerances are the project's own, unchanged
(gpu_common.stage_tol / grad_tol / FIXED_TOL / TIE_SLACK); every stage case also asserts, with the oracle alone, that its `own` stays
under OWN_CAP, that the gate MLP is live and that every gradient is finite.  Negative controls: make negctl RANGE=k,
tools/negative_controls.sh range, profiles/range_negative_control.log."""
import ctypes as Ct

import numpy as np
import pytest
import torch

from oracle import cnn_gru_oracle as O
from test_parity_gpu import FORMS, _engine, fused_equals_separate_calls
from test_trained_regimes_gpu import OWN_CAP, assert_own_capped, oracle_stages64, run_case_own

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tier needs an MI355X"
    return torch.device("cuda:0")


@pytest.fixture
def kernel_forms():
    from multimodalsignal_amd import _lib as L
    yield L.set_kernel_form
    L.set_kernel_form("auto", "auto")


# (B, C, K, T, p, form, init_params seed, input seed).  The seeds are 100 + B and 7 B + T (test_random_shapes_with_dropout's rule)
# wherever the gate MLP is live under them (7 of the 14), else the first pair (100 + B + i, 7 B + T + j), j running fastest, under
# which it is: found with the oracle alone (gate_pre = W1 . mean_t x needs nothing else), asserted in every case.  The inputs' per-
# channel offsets dominate gate_pre, so a unit is mostly on for all windows or for none: live means a unit the gradient passes through.
# (5, 7, 5, 137) takes the SECOND such pair: under the first, (105, 173), the gradient of channel_attention.fc.0.weight cancels so far
# that the fp32 oracle's own error in it is 3.7e-6 on one CPU and 1.08e-5 on another (the cap is 1e-5); under (105, 174) 6.4e-7.
CASES = [
    (5, 7, 5, 137, 0.5, "split", 105, 174),      # C = 7 instantiation, T % 4 != 0 (scalar staging, no pipeline)
    (17, 7, 2, 256, 0.5, "ws6", 117, 377),       # C = 7, pipelined staging, two batch tiles (the second ragged)
    (3, 9, 16, 136, 0.0, "split", 103, 158),     # KM = 16 (one padded tap), NB = 4, Cr = 2, K = 16
    (33, 9, 6, 250, 0.5, "ws6", 133, 482),       # the same C at T % 4 != 0, three tiles (the last ragged)
    (16, 10, 13, 208, 0.5, "split", 116, 320),   # KM = 18, NB = 5, K = 13 (dW3 slot 3 partly filled)
    (33, 11, 11, 72, 0.5, "ws6", 133, 303),      # KM = 20, odd T'
    (4, 12, 4, 264, 0.25, "split", 104, 293),    # KM = 21 (odd: the m + 1 < KM guard), Cr = 3
    (2, 13, 2, 137, 0.0, "ws6", 102, 152),       # KM = 23, NB = 6, two-row batch
    (18, 14, 3, 250, 0.5, "split", 118, 376),    # all 14 WESAD channels: KM = 25, NB = 7 with 14 padded columns
    (24, 14, 2, 256, 0.5, "ws6", 124, 424),      # the same under the throughput forms
    (2, 14, 2, 3840, 0.5, "split", 102, 3854),   # the real window: conv1_bwd's eight-segment path on the generic kernel
    (260, 14, 2, 64, 0.5, "split", 360, 1885),   # B >= 256: conv1_bwd_cps = whole windows per item
    (4, 15, 9, 264, 0.25, "ws6", 104, 292),      # KM = 27, K = 9 (dW3 slot 2 partly filled)
    (5, 15, 16, 40, 0.0, "split", 105, 75),      # T' = 3, K = 16
]
LIVE_SHARE = 0.25


def build_case(B, C, K, T, pseed, xseed):
    """(params, x, y): init_params and inputs with per-channel offset and spread, drawn as test_random_shapes_with_dropout draws them."""
    params = {k: v.numpy() for k, v in O.init_params(C, K, seed=pseed).items()}
    rs = np.random.RandomState(xseed)
    x = (rs.randn(B, C, T) * (0.5 + rs.rand(1, C, 1)) + rs.randn(1, C, 1)).astype(np.float32)
    y = rs.randint(0, K, size=(B,)).astype(np.int64)
    return params, x, y


def live_share(params, x):
    """The largest share of windows, over the gate MLP's hidden units, in which the unit's pre-activation is positive — in float64."""
    pre = x.astype(np.float64).mean(axis=2) @ params["channel_attention.fc.0.weight"].astype(np.float64).T      # (B, C // 4)
    return float((pre > 0).mean(axis=0).max())


@pytest.mark.parametrize("B,C,K,T,p,form,pseed,xseed", CASES)
def test_range_stages_against_oracle(B, C, K, T, p, form, pseed, xseed, dev, kernel_forms, monkeypatch, tmp_path):
    from gpu_common import failures, format_report
    kernel_forms(*FORMS[form])
    params, x, y = build_case(B, C, K, T, pseed, xseed)
    eng = _engine(C, K, dev)
    fw = dict(dropout_p=p, seed=1234, step=3)
    rep, ref, own = run_case_own(monkeypatch, tmp_path, eng, params, x, y, tag=f"range_{form}", **fw)
    print("\n" + format_report(rep))
    assert_own_capped(own)
    assert rep["pool_near_ties_adopted"][0] <= 8
    pre = oracle_stages64(params, x, **fw)["gate_pre"]                    # (B, C // 4) of the fp64 oracle
    assert pre.shape == (B, C // 4) and float((pre > 0).mean(axis=0).max()) >= LIVE_SHARE, "the gate MLP is dead in the oracle"
    assert live_share(params, x) >= LIVE_SHARE
    for k in ("channel_attention.fc.0.weight", "channel_attention.fc.2.weight"):
        assert float(ref[1][k].abs().max()) > 0, f"the gate MLP is dead: the oracle's gradient of {k} is exactly zero"
    assert bool(torch.isfinite(eng.grads).all()), "a gradient of the HIP path is not finite"
    assert not failures(rep), format_report(rep)


# ---- the other consumers of the same kernels ------------------------------------------------------------------------------------------
def _inputs(B, C, K, T, seed):
    rs = np.random.RandomState(seed)
    x = (rs.randn(B, C, T) * (0.5 + rs.rand(1, C, 1)) + rs.randn(1, C, 1)).astype(np.float32)
    return torch.as_tensor(x), torch.as_tensor(rs.randint(0, K, size=(B,)).astype(np.int64))


@pytest.mark.parametrize("B,C,K,T", [(5, 9, 3, 137), (18, 14, 5, 250)])
def test_cnn_gru_kind_against_oracle(B, C, K, T, dev, monkeypatch):
    """The cnn_gru kind — conv1_fwd_kernel<0, false> (raw taps in the A registers, `(CT > 0 || m < KM) && k < K`) and
    gate_kernel<0, true> (the parity sums only) — through CnnGruModel and autograd against the fp64 oracle with its gate patched to
    s = 1, as tests/test_cnngru_gpu.py::test_against_fp64_oracle does at C = 12: stages, loss, every gradient and dL/dx."""
    from gpu_common import FIXED_TOL, grad_tol, rel_err, stage_tol
    from multimodalsignal_amd import _lib as L
    from multimodalsignal_amd.models import CnnGruModel
    from test_cnngru_gpu import _grads_and_dx, _hip_pool_choice, _named, _oracle
    monkeypatch.setattr(O, "channel_gate", lambda x_, W1, W2: (x_.mean(dim=2), torch.zeros(x_.shape[0], 0, dtype=x_.dtype),
                                                                torch.ones(x_.shape[0], x_.shape[1], dtype=x_.dtype)))
    torch.manual_seed(C + T)
    model = CnnGruModel(C, K).to(dev)
    model.set_dropout_seed(31)
    xc, yc = _inputs(B, C, K, T, 7 * B + T)
    named = _named(model)
    model.train()
    logits, loss, grads, dx = _grads_and_dx(model, xc.to(dev), yc.to(dev))
    torch.cuda.synchronize()
    fw = dict(dropout_p=0.5, seed=model._seed, step=model._step)
    dx64, g64, st64 = _oracle(named, xc, yc, torch.float64, True, fw)
    choice = _hip_pool_choice(model._engine, st64, B, T)
    if choice is not None:
        dx64, g64, st64 = _oracle(named, xc, yc, torch.float64, True, fw, pool_choice=choice)
    dx32, g32, st32 = _oracle(named, xc, yc, torch.float32, True, fw, pool_choice=choice)
    eng = model._engine
    L1, P1, L2, TP = O.stage_lengths(T)
    stages = {"conv1": eng.region("Y1", torch.float32, (B, L1, 16)).cpu().permute(0, 2, 1),
              "pool1": eng.region("P1", torch.float32, (B, P1, 16)).cpu().permute(0, 2, 1),
              "pool2": eng.region("P2", torch.float32, (B, TP, 32)).cpu().permute(0, 2, 1),
              "feat": eng.region("FEAT", torch.float32, (B, 128)).cpu(), "logits": logits.cpu()}
    own, bad = {}, []
    for k, got in stages.items():
        ref = st64[k].detach().numpy()
        own[k] = rel_err(st32[k].detach().numpy(), ref)
        err, tol = rel_err(got.numpy(), ref), stage_tol(k, own[k])
        print(f"{k:40s} err={err:.3e} tol={tol:.1e} own={own[k]:.2e}")
        if not err <= tol:
            bad.append((k, err, tol))
    loss64 = float(O.cross_entropy(st64["logits"].detach(), yc))
    assert abs(float(loss) - loss64) <= FIXED_TOL["loss"] * max(abs(loss64), 1e-6)
    assert sorted(grads) == sorted(k for k in g64 if k not in L.GATE_KEYS)
    for k, g in list(grads.items()) + [("x", dx)]:
        ref, r32 = (dx64.numpy(), dx32.numpy()) if k == "x" else (g64[k].numpy(), g32[k].numpy())
        own["grad/" + k] = rel_err(r32, ref)
        assert bool(torch.isfinite(g).all()), k
        err, tol = rel_err(g.cpu().numpy(), ref), grad_tol(k, own["grad/" + k])
        print(f"grad/{k:35s} err={err:.3e} tol={tol:.1e} own={own['grad/' + k]:.2e}")
        if not err <= tol:
            bad.append((k, err, tol))
    assert_own_capped(own)
    assert not bad, bad


@pytest.mark.parametrize("B,C,K,T", [(5, 7, 5, 137), (18, 14, 16, 250)])
def test_eval_mode_forward_against_oracle(B, C, K, T, dev):
    """Engine.forward(training=False) of a model whose running statistics are no longer the initial ones (two training steps, as
    tests/test_input_grad_gpu.py::_trained makes them) against the fp64 oracle's eval-mode forward: with labels (ce_kernel: logits,
    mean loss, probabilities, predictions, number correct) and without (softmax_kernel: probabilities and predictions)."""
    from gpu_common import FIXED_TOL, rel_err, split_named, stage_tol, to_t
    from test_input_grad_gpu import _trained
    m = _trained(C, K, "full", dev).eval()
    named = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    assert float(named["cnn_encoder.1.running_mean"].abs().max()) > 0 and float((named["cnn_encoder.5.running_var"] - 1).abs().max()) > 1e-3
    xc, yc = _inputs(B, C, K, T, 99 + C)
    out = {}
    for dt in (torch.float64, torch.float32):
        p, b = split_named(to_t(named, dt))
        with torch.no_grad():
            st, _ = O.forward(p, b, xc.to(dt), training=False)
        out[dt] = (st["logits"].numpy(), torch.softmax(st["logits"], dim=1).numpy(), float(O.cross_entropy(st["logits"], yc)))
    (z64, p64, l64), (z32, p32, l32) = out[torch.float64], out[torch.float32]
    own_z, own_p = rel_err(z32, z64), rel_err(p32, p64)
    assert max(own_z, own_p) <= OWN_CAP, (own_z, own_p)
    top2 = np.sort(z64, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 1e-4 * np.abs(z64).max()          # rows whose prediction no fp32 rounding can change
    assert clear.sum() >= B - 1
    eng = m.engine()
    before = eng.bn_state.clone()
    for labels in (yc.to(dev), None):
        eng.forward(xc.to(dev), labels, training=False)
        torch.cuda.synchronize()
        probs = eng.region("PROBS", torch.float32, (B, K)).cpu().numpy()
        pred = eng.region("PRED", torch.int32, (B,)).cpu().numpy()
        logits = eng.region("LOGITS", torch.float32, (B, K)).cpu().numpy()
        err_z, err_p = rel_err(logits, z64), rel_err(probs, p64)
        print(f"labels={labels is not None} logits err={err_z:.3e} tol={stage_tol('logits', own_z):.1e} probs err={err_p:.3e} tol={stage_tol('probs', own_p):.1e}")
        assert err_z <= stage_tol("logits", own_z) and err_p <= stage_tol("probs", own_p)
        assert (pred[clear] == z64.argmax(axis=1)[clear]).all() and (pred == logits.argmax(axis=1)).all()
        if labels is not None:
            acc = eng.region("LOSS", torch.float32, (3,)).cpu().numpy()
            assert abs(float(acc[0]) - l64) <= FIXED_TOL["loss"] * max(abs(l64), 1e-6), (acc, l64)
            assert int(acc[2]) == int((pred == yc.numpy()).sum())
        assert torch.equal(before, eng.bn_state)


@pytest.mark.parametrize("C,B,T", [(7, 4, 256), (7, 5, 511), (14, 4, 256), (14, 5, 511)])
def test_train_mode_input_gradient_against_oracle(C, B, T, dev):
    """conv1_bwd_dx_kernel at C = 7 and C = 14 (quad and, at T = 511, position-wise staging of dy1), dropout 0.5."""
    import test_input_grad_gpu as IG
    K = 2 + (C + B) % 2
    m = IG._model(C, K, "full", 0.5, dev, seed=C + B).train()
    m.set_dropout_seed(1000 + C)
    x, y = IG._case(B, C, K, T, 10 * C + B)
    named = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    xd = x.to(dev).requires_grad_(True)
    torch.nn.CrossEntropyLoss()(m(xd), y.to(dev)).backward()
    assert xd.grad is not None and xd.grad.shape == x.shape and bool(torch.isfinite(xd.grad).all()) and float(xd.grad.abs().max()) > 0
    IG._check_against_oracle(m, named, x, y, xd.grad.cpu().numpy(), True, dict(dropout_p=0.5, seed=1000 + C, step=1))


def test_eval_mode_input_gradient_against_oracle(dev):
    """Eval-mode backward (keep_for_backward) at C = 14, (B, T) = (5, 511), K = 3, with trained running statistics."""
    import test_input_grad_gpu as IG
    C, K, B, T = 14, 3, 5, 511
    m = IG._trained(C, K, "full", dev).eval()
    x, y = IG._case(B, C, K, T, 99 + C)
    named = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    m.zero_grad()
    xd = x.to(dev).requires_grad_(True)
    torch.nn.CrossEntropyLoss()(m(xd), y.to(dev)).backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(xd.grad).all()) and float(xd.grad.abs().max()) > 0
    IG._check_against_oracle(m, named, x, y, xd.grad.cpu().numpy(), False, dict(dropout_p=0.0, seed=0, step=0))


# ---- the fused step ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [40, 2060])
def test_fused_step_equals_separate_calls_at_c14_k16(B, dev, kernel_forms):
    """Three fused train steps against forward + backward + adam_step, bit for bit (test_parity_gpu's comparison), at C = 14, K = 16,
    T = 64: B = 40 runs head_step_kernel (all four dW3 slots, 16 logits per row), B = 2060 (> 2048 rows) the staged head.  The
    two paths' updates agree to the last bit in the first step only (two compilations of one expression, as that test records), so
    each step starts from the fused engine's parameters and moments: step 3 is then compared in every bit, with moments != 0."""
    kernel_forms(*FORMS["split"])
    fused_equals_separate_calls(B, 14, 16, 64, (1, 2, 3), dev, resync=True)


W16 = tuple(float(w) for w in np.round(np.random.RandomState(16).uniform(0.2, 4.0, size=16), 3))


def test_soft_step_at_c14_k16_matches_fp64_reference(dev):
    """One train step with class weights, label smoothing 0.1 and mixup lambda 0.3 together at (B, C, K, T) = (16, 14, 16, 128)
    against tests/st_reference.py's mix and torch's cross_entropy over the fp64 oracle — the comparison and the preconditions of
    tests/test_soft_targets_gpu.py::test_soft_step_matches_fp64_reference, at that test's tolerances."""
    import st_reference as S
    import test_soft_targets_gpu as ST
    from gpu_common import grad_tol, rel_err, stage_tol
    B, C, K, T, eps, lam = 16, 14, 16, 128, 0.1, 0.3
    e, params = ST._engine(C, K, params=ST._params(C, K))
    x, y = ST._data(B, C, K, T, B + C)
    xm = S.mix(x.cpu().numpy(), np.arange(B), lam)
    e.train_step(torch.as_tensor(xm).to(dev), y, ST.LR, weight_decay=ST.WD, step=1, dropout_p=ST.P, seed=11, class_weight=ST._wt(W16),
                 label_smoothing=eps, mix_lambda=lam)
    torch.cuda.synchronize()
    got_loss = float(e.region("LOSS", torch.float32, (3,))[0])
    got_d = e.region("DLOGITS", torch.float32, (B, K)).cpu().numpy()
    got_g = {k: v.detach().cpu().numpy() for k, v in e.named_param_views(e.grads).items()}
    ref = ST._reference(params, xm, y.cpu().numpy(), W16, eps, lam, ST.ATT, 11, 1)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    l64, k3 = r64["loss"], "classifier.3.weight"
    tol_l = stage_tol("loss", abs(r32["loss"] - l64) / max(abs(l64), 1e-6))
    tol_g3 = grad_tol(k3, rel_err(r32["grads"][k3], r64["grads"][k3]))
    assert abs(r64["plain_loss"] - l64) / max(abs(l64), 1e-6) > 100 * tol_l
    assert rel_err(r64["plain_g3"], r64["grads"][k3]) > 100 * tol_g3
    err_l = abs(got_loss - l64) / max(abs(l64), 1e-6)
    err_d, tol_d = rel_err(got_d, r64["dlogits"]), stage_tol("d_logits", rel_err(r32["dlogits"], r64["dlogits"]))
    print(f"loss err {err_l:.3e} tol {tol_l:.1e} | dlogits err {err_d:.3e} tol {tol_d:.1e}")
    assert err_l <= tol_l, (got_loss, l64)
    assert err_d <= tol_d
    assert set(got_g) == set(r64["grads"])
    for k, g in r64["grads"].items():
        err, tol = rel_err(got_g[k], g), grad_tol(k, rel_err(r32["grads"][k], g))
        assert err <= tol, (k, err, tol)


# ---- the fold limit ------------------------------------------------------------------------------------------------------------------
def test_sixteen_folds_equal_their_single_model_steps(dev):
    """ONE msig_train_step_multi over MSIG_MAX_FOLDS = 16 folds at (B, C, K, T, p) = (8, 14, 3, 64, 0.5), the slots in a non-monotone
    order, every fold with its own weights, inputs, dropout seed, step count and learning rate: each fold's parameters, gradients,
    Adam moments and BatchNorm state are bit-identical to its own single-model train_step."""
    from multimodalsignal_amd import _lib as L
    from multimodalsignal_amd.runtime import Engine, FoldArena
    NF, B, C, K, T, p = 16, 8, 14, 3, 64, 0.5
    assert NF == L.MAX_FOLDS
    order = [5, 12, 0, 9, 15, 3, 7, 1, 14, 10, 2, 8, 13, 4, 11, 6]
    assert sorted(order) == list(range(NF))
    arena = FoldArena(C, K, dev, NF, B, T)
    cases, folds = {}, {s: arena.engine(s) for s in range(NF)}      # made once: a new engine zeroes its arena
    for i, s in enumerate(order):
        params, x, y = build_case(B, C, K, T, 500 + s, 40 + s)
        folds[s].load_named({k: torch.as_tensor(v) for k, v in params.items()})
        arena.view(s, "x", torch.float32)[:x.size].copy_(torch.as_tensor(x).reshape(-1))
        arena.view(s, "y", torch.int64)[:B].copy_(torch.as_tensor(y))
        cases[s] = dict(params=params, x=x, y=y, seed=1000 + 3 * s, step=1 + (5 * i) % 7, lr=1e-3 * (1 + 0.25 * (i % 5)))
    m = arena.multi(order, key_gru=[L.dropout_key(cases[s]["seed"], cases[s]["step"], 1) for s in order],
                    key_head=[L.dropout_key(cases[s]["seed"], cases[s]["step"], 2) for s in order],
                    lr=[cases[s]["lr"] for s in order], steps=[cases[s]["step"] for s in order])
    st = Ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L.check(L.lib().msig_train_step_multi(Ct.byref(arena.batch(B, True, p)), Ct.byref(m), arena.ptr("exp_avg"), arena.ptr("exp_avg_sq"),
                                          0.9, 0.999, 1e-8, 1e-4, cases[order[0]]["step"], st), "msig_train_step_multi")
    torch.cuda.synchronize()
    bits = lambda t: t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()
    for s in order:
        c = cases[s]
        single = Engine(C, K, dev)
        single.load_named({k: torch.as_tensor(v) for k, v in c["params"].items()})
        single.ensure_adam_state()
        single.train_step(torch.as_tensor(c["x"]).to(dev), torch.as_tensor(c["y"]).to(dev), lr=c["lr"], weight_decay=1e-4, step=c["step"],
                          dropout_p=p, seed=c["seed"])
        torch.cuda.synchronize()
        fold = folds[s]
        assert float(single.grads.abs().max()) > 0
        for name in ("params", "grads", "exp_avg", "exp_avg_sq", "bn_state", "bn_count"):
            a, b = bits(getattr(fold, name)), bits(getattr(single, name))
            assert torch.equal(a, b), f"slot {s}: {name}: {int((a != b).sum())} of {a.numel()} words differ"
        assert float(arena.view(s, "acc", torch.float64)[0]) == float(single.loss_acc[0]) > 0
