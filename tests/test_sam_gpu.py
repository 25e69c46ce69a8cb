"""GPU tier of sharpness-aware minimisation (include/msig_sam.h): the perturbation and the restore alone against
tests/sam_reference.py bit for bit, one msig_sam_train_step against the same step built from public calls bit for bit, against the
fp64 oracle differentiated twice, off = the plain step, fold batches = their single calls, and the driver."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import sam_reference as R
from conftest import load_golden_model
from gpu_common import FIXED_TOL, GRAD_FLOOR, K_GRAD, grad_tol, narrow_train_step, rel_err, split_named, to_t
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd.distill import Distillation
from multimodalsignal_amd.runtime import EmbeddedEngine, Engine, FoldArena
from multimodalsignal_amd.sam import Sam
from oracle import cnn_gru_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ATT, CG = "cnn_gru_attention", "cnn_gru"
LR, WD = 1e-3, 1e-4
FORMS = {"ws6": ("ws", "b6"), "split": ("split", "split")}


@pytest.fixture
def kernel_forms():
    yield L.set_kernel_form
    L.set_kernel_form("auto", "auto")


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _dev(a, dtype=None):
    t = torch.as_tensor(a)
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _data(B, Cc, K, T, seed):
    rs = np.random.RandomState(seed)
    y = rs.randint(0, K, size=B).astype(np.int64)
    y[:min(K, B)] = np.arange(min(K, B))
    return _dev(rs.randn(B, Cc, T).astype(np.float32)), _dev(y)


def _engine(Cc, K, hidden=64, layers=2, kind=ATT, seed=3, storage_engine=None):
    params = O.init_params(Cc, K, seed=seed, hidden=hidden, layers=layers)
    if kind == CG:
        params = {k: v for k, v in params.items() if k not in L.GATE_KEYS}
    e = storage_engine
    if e is None:
        e = EmbeddedEngine(Cc, K, DEV, hidden, kind=kind) if layers == 1 else Engine(Cc, K, DEV, kind=kind)
    if layers == 1:
        for k, v in e.small_views().items():
            v.copy_(params[k])
        if storage_engine is not None:
            e.scatter()
    else:
        e.load_named(params)
    return e


def _desc(e, sam):
    state = e.ensure_sam_state()
    return sam.descriptor(e.kind, state.data_ptr(), state.numel() * 8)


# ---- 1. the perturbation and the restore alone ----------------------------------------------------------------------------------
@pytest.mark.parametrize("adaptive", [False, True], ids=["sam", "asam"])
@pytest.mark.parametrize("kind,Cc,K,shift", [(ATT, 6, 2, 0), (ATT, 2, 3, 0), (CG, 6, 3, 0), (ATT, 6, 3, 1)],
                         ids=["att_c6k2", "att_c2k3_empty_gate", "cg_c6k3", "att_c6k3_state_8_mod_16"])
def test_perturb_and_restore_alone(kind, Cc, K, shift, adaptive):
    """shift = 1: a state that is 8-byte but not 16-byte aligned (the backup then moves in 64-bit pieces).  The gradient's padding
    holds NaN: a kernel that read it could not produce a finite norm."""
    rho, eta, B = 0.05, 0.01, 16
    table, n_flat = R.tensor_table(Cc, K, kind)
    mask = R.element_mask(table, n_flat)
    assert not mask.all()
    rs = np.random.RandomState(7 + Cc + K)
    p = np.where(mask, rs.randn(n_flat) * 0.1, 0.0).astype(np.float32)
    g = (rs.randn(n_flat) * 1e-2).astype(np.float32)
    g[~mask] = np.nan
    bn0 = rs.rand(96).astype(np.float32)
    params, grads, bn, cnt = _dev(p), _dev(g), _dev(bn0), _dev(np.array([3, 5], dtype=np.int64))
    loss = _dev(np.array([0.75, 0.75 * B, 9.0, 0.0], dtype=np.float32))
    nbytes = L.sam_state_bytes(Cc, K, kind)
    raw = torch.zeros(nbytes // 8 + 2, dtype=torch.float64, device=DEV)
    state = raw[shift:shift + nbytes // 8]
    assert state.data_ptr() % 16 == 8 * shift
    sd = Sam(rho, adaptive, eta).descriptor(kind, state.data_ptr(), nbytes)
    lib = L.lib()

    def perturb():
        L.check(lib.msig_sam_perturb(params.data_ptr(), grads.data_ptr(), bn.data_ptr(), cnt.data_ptr(), loss.data_ptr(), Cc, K, C.byref(sd),
                                     _stream()), "msig_sam_perturb")
        torch.cuda.synchronize()

    perturb()
    st = state[:L.SAM_NSTAT].cpu().tolist()
    N = st[L.SAM_NORM_LAST]
    assert st[L.SAM_NORM_SUM] == N and st[L.SAM_NORM_MAX] == N and st[L.SAM_STEPS] == 0.0
    # N against a torch fp64 sum over the tensor elements
    tp, tg, tm = torch.as_tensor(p), torch.as_tensor(g), torch.as_tensor(mask)
    u = (tp.abs() + torch.tensor(eta, dtype=torch.float32)) * tg if adaptive else tg
    N64 = float(torch.sqrt((u[tm].double() ** 2).sum()))
    print(f"N {N!r} torch fp64 {N64!r} rel {abs(N - N64) / N64:.2e}")
    assert abs(N - N64) <= 1e-12 * N64
    assert abs(N - R.norm(p, g, mask, adaptive, eta)) <= 1e-12 * N64
    # p' = fadd(p, fmul(coef, ...)) from that N, bit for bit; the padding and the BatchNorm buffers as they were
    got = params.cpu().numpy()
    want = R.perturb(p, g, mask, N, rho, adaptive, eta)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(got[~mask].view(np.int32), p[~mask].view(np.int32)) and not np.array_equal(got[mask], p[mask])
    assert np.array_equal(bn.cpu().numpy(), bn0) and cnt.tolist() == [3, 5] and loss.tolist() == [0.75, 0.75 * B, 9.0, 0.0]
    # what a second pass would leave behind, then the restore
    bn.add_(1.0); cnt.add_(1)
    loss.copy_(_dev(np.array([0.875, 0.875 * B, 11.0, 0.0], dtype=np.float32)))
    L.check(lib.msig_sam_restore(params.data_ptr(), bn.data_ptr(), cnt.data_ptr(), loss.data_ptr(), B, Cc, K, C.byref(sd), _stream()), "msig_sam_restore")
    torch.cuda.synchronize()
    assert np.array_equal(params.cpu().numpy().view(np.int32), p.view(np.int32))
    assert np.array_equal(bn.cpu().numpy().view(np.int32), bn0.view(np.int32)) and cnt.tolist() == [3, 5]
    assert loss.tolist() == [0.75, 0.75 * B, 9.0, 0.0]
    st = state[:L.SAM_NSTAT].cpu().tolist()
    d = R.sharpness(0.875 * B, 0.75 * B, B)
    assert d == 0.125 and st[L.SAM_SHARP_LAST] == d and st[L.SAM_SHARP_SUM] == d and st[L.SAM_STEPS] == 1.0 and st[L.SAM_NORM_LAST] == N
    # a zero gradient leaves p unchanged, and the statistics count it
    grads.copy_(_dev(np.where(mask, 0.0, np.nan).astype(np.float32)))
    perturb()
    assert np.array_equal(params.cpu().numpy().view(np.int32), p.view(np.int32))
    st = state[:L.SAM_NSTAT].cpu().tolist()
    assert st[L.SAM_NORM_LAST] == 0.0 and st[L.SAM_NORM_SUM] == N and st[L.SAM_NORM_MAX] == N


# ---- 2. composition: one msig_sam_train_step = the same step from public calls ---------------------------------------------------------
VARIANTS = {"dropout": dict(p=0.5), "no_dropout": dict(p=0.0),
            "soft": dict(p=0.5, w=(0.3, 2.5), eps=0.1, lam=0.4)}
COMPOSE = [(24, "split", "dropout", ATT, False), (24, "split", "no_dropout", ATT, True), (24, "split", "soft", ATT, False),
           (24, "split", "soft", CG, True), (64, "split", "dropout", ATT, True), (40, "ws6", "dropout", ATT, False), (40, "ws6", "soft", ATT, True),
           (300, "split", "dropout", ATT, False), (2048, "split", "dropout", ATT, False), (2060, "split", "soft", ATT, True)]


@pytest.mark.parametrize("B,form,variant,kind,adaptive", COMPOSE)
def test_sam_step_equals_the_public_calls_bit_for_bit(B, form, variant, kind, adaptive, kernel_forms):
    """The shapes and kernel forms of test_fused_step_equals_separate_calls_bit_for_bit (C = 6, K = 2, T = 384).  Apart: training
    forward + backward at w, msig_sam_perturb, forward + backward at w + e with the same seed and step, msig_sam_restore,
    msig_adam_step (step 1 from zero moments, where the two Adam compilations agree in every bit)."""
    kernel_forms(*FORMS[form])
    Cc, K, T, seed, step = 6, 2, 384, 21, 1
    v = VARIANTS[variant]
    x, y = _data(B, Cc, K, T, 300 + B)
    cw = torch.tensor(v["w"], dtype=torch.float32, device=DEV) if "w" in v else None
    crit = dict(class_weight=cw, label_smoothing=v.get("eps", 0.0), mix_lambda=v.get("lam"))
    sam = Sam(0.05, adaptive)
    fused, apart = _engine(Cc, K, kind=kind, seed=5), _engine(Cc, K, kind=kind, seed=5)
    for e in (fused, apart):
        e.ensure_adam_state()
    w0 = fused.params.clone()
    fused.train_step(x, y, LR, weight_decay=WD, step=step, dropout_p=v["p"], seed=seed, sam=sam, **crit)
    lib, sd = L.lib(), _desc(apart, sam)
    b = apart.forward(x, y, training=True, dropout_p=v["p"], seed=seed, step=step, **crit)
    apart.backward(b)
    acc1 = apart.loss_acc.clone()
    ws_loss = apart.region("LOSS").data_ptr()
    L.check(lib.msig_sam_perturb(apart.params.data_ptr(), apart.grads.data_ptr(), apart.bn_state.data_ptr(), apart.bn_count.data_ptr(), ws_loss,
                                 Cc, K, C.byref(sd), _stream()), "msig_sam_perturb")
    moved = apart.params.clone()
    b = apart.forward(x, y, training=True, dropout_p=v["p"], seed=seed, step=step, **crit)
    apart.backward(b)
    L.check(lib.msig_sam_restore(apart.params.data_ptr(), apart.bn_state.data_ptr(), apart.bn_count.data_ptr(), ws_loss, B, Cc, K, C.byref(sd),
                                 _stream()), "msig_sam_restore")
    apart.adam_step(LR, weight_decay=WD, step=step)
    torch.cuda.synchronize()
    assert not torch.equal(moved, w0)                                      # the second pass ran somewhere else
    for name in ("params", "exp_avg", "exp_avg_sq", "grads", "bn_state", "bn_count"):
        assert torch.equal(_bits(getattr(fused, name)), _bits(getattr(apart, name))), name
    assert torch.equal(_bits(fused.region("LOSS")[:3]), _bits(apart.region("LOSS")[:3]))
    assert torch.equal(fused.sam_state[:L.SAM_NSTAT], apart.sam_state[:L.SAM_NSTAT]) and float(fused.sam_state[L.SAM_STEPS]) == 1.0
    assert float(fused.sam_state[L.SAM_NORM_LAST]) > 0
    assert torch.equal(fused.loss_acc, acc1) and float(fused.loss_acc[0]) > 0      # epoch sums count the batch once, at w
    assert fused.bn_count.tolist() == [1, 1]
    for name, n, dt in (("LOGITS", B * K, torch.float32), ("PROBS", B * K, torch.float32), ("PRED", B, torch.int32)):       # pass 2's
        assert torch.equal(fused.region(name, dt)[:n], apart.region(name, dt)[:n]), name
    # and it is not the plain step: the plain gradient at w differs
    plain = _engine(Cc, K, kind=kind, seed=5)
    plain.train_step(x, y, LR, weight_decay=WD, step=step, dropout_p=v["p"], seed=seed, **crit)
    torch.cuda.synchronize()
    assert not torch.equal(plain.grads, fused.grads) and torch.equal(_bits(plain.bn_state), _bits(fused.bn_state))
    assert torch.equal(plain.loss_acc, fused.loss_acc)


@pytest.mark.parametrize("adaptive", [False, True], ids=["sam", "asam"])
@pytest.mark.parametrize("kind", [ATT, CG])
def test_embedded_padding_stays_exactly_zero_through_sam_steps(kind, adaptive):
    Cc, K, B, T = 3, 2, 16, 256
    e = _engine(Cc, K, 32, 1, kind)
    for s in (1, 2, 3):
        x, y = _data(B, Cc, K, T, 40 + s)
        e.train_step(x, y, LR, weight_decay=WD, step=s, dropout_p=0.5, seed=9, sam=Sam(0.1, adaptive), max_grad_norm=1.0)
    torch.cuda.synchronize()
    for name in ("params", "grads", "exp_avg", "exp_avg_sq"):
        assert int(getattr(e, name)[e.padding].count_nonzero()) == 0, name
    assert float(e.sam_state[L.SAM_STEPS]) == 3.0 and float(e.sam_state[L.SAM_NORM_SUM]) > 0
    assert torch.isfinite(e.small).all()


# ---- 3. against the fp64 oracle, differentiated at w and at w + e --------------------------------------------------------------------
ADAM_EPS, RHO, STEPS = 1e-3, 0.05, 3


def _oracle_sam(oparams, buffers, batches, adaptive, eta, dt, p_drop, seed):
    """STEPS SAM steps of the oracle in dtype dt (autograd through the whole model, Adam with L2 decay and eps = ADAM_EPS in dt).
    Returns the first step's (pass-1 gradient, pass-2 gradient, N, sharpness) and the parameters after the last step."""
    p = {k: v.to(dt).clone() for k, v in oparams.items()}
    bufs = {k: (v.clone() if "num_batches" in k else v.to(dt)) for k, v in buffers.items()}
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    vv = {k: torch.zeros_like(v) for k, v in p.items()}
    first = None
    for s, (x, y) in enumerate(batches, start=1):
        fw = dict(dropout_p=p_drop, seed=seed, step=s)
        xt, yt = torch.as_tensor(x).to(dt), torch.as_tensor(y)
        l1, g1, _, nb = O.loss_and_grads(p, bufs, xt, yt, **fw)
        t = {k: (p[k].abs() + eta) if adaptive else torch.ones_like(p[k]) for k in p}
        u = {k: t[k] * g1[k] for k in p}
        N = torch.sqrt(sum((u[k].double() ** 2).sum() for k in p))
        coef = RHO / (N + 1e-12)
        pe = {k: p[k] + (coef * (t[k] * u[k]).double()).to(dt) for k in p}
        l2, g2, _, _ = O.loss_and_grads(pe, bufs, xt, yt, **fw)
        if first is None:
            first = ({k: v.double().numpy() for k, v in g1.items()}, {k: v.double().numpy() for k, v in g2.items()}, float(N),
                     float(l2) - float(l1), float(l1), float(l2))
        b1, b2 = 0.9, 0.999
        for k in p:
            gd = g2[k] + WD * p[k]
            m[k] = b1 * m[k] + (1 - b1) * gd
            vv[k] = b2 * vv[k] + (1 - b2) * gd * gd
            p[k] = p[k] - LR * (m[k] / (1 - b1 ** s)) / ((vv[k] / (1 - b2 ** s)).sqrt() + ADAM_EPS)
        bufs = nb
    return first, {k: v.double().numpy() for k, v in p.items()}


@pytest.mark.parametrize("adaptive", [False, True], ids=["sam", "asam"])
@pytest.mark.parametrize("name,kind,layers", [("model_c6_k2_t512", ATT, 2), ("model_c2_k3_t256", ATT, 2), ("model_c6_k2_t512", CG, 2),
                                              ("model_c6_k2_t512", ATT, 1)], ids=["attention", "empty_gate_k3", "cnn_gru", "embedded"])
def test_sam_steps_match_the_oracle_differentiated_twice(name, kind, layers, adaptive, monkeypatch):
    """B = 4, T = 256, dropout 0.5, rho = 0.05 on the committed parameters (the one-layer model: the oracle's initialisation).  After
    one step: `grads` against the oracle's gradient AT w + e, N and the sharpness; after three: the parameters.  Gate: gpu_common's —
    K_GRAD x the fp32 oracle's own error against the fp64 oracle, with its floors.  Adam's eps is 1e-3 (test_distill_gpu.py says
    why).  Precondition, from the oracle alone: the gradient at w + e differs from the one at w by more than ten gates in every
    tensor whose gradient is not identically zero (measured: 440 gates at the least), so a plain step cannot pass."""
    meta, params_np, _ = load_golden_model(name)
    Cc, K, T, B, eta, p_drop, seed = meta["C"], meta["K"], 256, 4, 0.01, 0.5, 13
    params, buffers = split_named(to_t(params_np))
    if layers == 1:
        params = O.init_params(Cc, K, seed=3, hidden=32, layers=1)
    oparams = params
    if kind == CG:
        params = {k: v for k, v in params.items() if k not in L.GATE_KEYS}
        oparams = dict(params, **{"channel_attention.fc.0.weight": torch.zeros(0, Cc), "channel_attention.fc.2.weight": torch.zeros(Cc, 0)})
        monkeypatch.setattr(O, "channel_gate", lambda x, W1, W2: (x.mean(dim=2), torch.zeros(x.shape[0], 0, dtype=x.dtype),
                                                                  torch.ones(x.shape[0], x.shape[1], dtype=x.dtype)))
    for k, v in O.init_buffers().items():
        buffers.setdefault(k, v)
    rs = np.random.RandomState(17)
    batches = []
    for _ in range(STEPS):
        x = rs.randn(B, Cc, T).astype(np.float32)
        y = rs.randint(0, K, size=B).astype(np.int64)
        y[:K] = np.arange(K)
        batches.append((x, y))
    (g1_64, g2_64, N64, d64, l1_64, l2_64), p64 = _oracle_sam(oparams, buffers, batches, adaptive, eta, torch.float64, p_drop, seed)
    (_, g2_32, N32, d32, _, _), p32 = _oracle_sam(oparams, buffers, batches, adaptive, eta, torch.float32, p_drop, seed)
    live = [k for k, g in g2_64.items() if g.size and np.abs(g1_64[k]).max() > 0]
    assert len(live) >= len([k for k in g2_64 if g2_64[k].size]) - 2
    for k in live:
        assert rel_err(g1_64[k], g2_64[k]) > 10 * grad_tol(k, rel_err(g2_32[k], g2_64[k])), k

    if layers == 1:
        e = EmbeddedEngine(Cc, K, DEV, 32, kind=kind)
        for k, v in e.small_views().items():
            v.copy_(params[k])
    else:
        e = Engine(Cc, K, DEV, kind=kind)
        e.load_named({**params, **buffers})
    sam = Sam(RHO, adaptive, eta)

    for s, (x, y) in enumerate(batches, start=1):
        e.train_step(_dev(x), _dev(y), LR, eps=ADAM_EPS, weight_decay=WD, step=s, dropout_p=p_drop, seed=seed, sam=sam)
        if s == 1:
            torch.cuda.synchronize()
            got_g = ({k: v.cpu().numpy().copy() for k, v in e.gather_grads().items()} if layers == 1
                     else {k: v.cpu().numpy().copy() for k, v in e.named_param_views(e.grads).items()})
            st = e.sam_stats()
    torch.cuda.synchronize()
    got_p = ({k: v.cpu().numpy().copy() for k, v in e.small_views().items()} if layers == 1
             else {k: v.cpu().numpy() for k, v in e.named_param_views().items()})
    N, d = st[L.SAM_NORM_LAST], st[L.SAM_SHARP_LAST]
    tolN = max(GRAD_FLOOR, K_GRAD * abs(N32 - N64) / N64)
    told = 2 * max(FIXED_TOL["loss"], K_GRAD * abs(d32 - d64) / max(abs(l1_64), abs(l2_64)))
    print(f"N {N:.9g} oracle {N64:.9g} rel {abs(N - N64) / N64:.2e} tol {tolN:.1e} | sharpness {d:.9g} oracle {d64:.9g} "
          f"err/loss {abs(d - d64) / max(abs(l1_64), abs(l2_64)):.2e} tol {told:.1e}")
    assert abs(N - N64) <= tolN * N64
    assert d64 > 0 and abs(d - d64) <= told * max(abs(l1_64), abs(l2_64))
    worst = 0.0
    for k, g in g2_64.items():
        if g.size == 0:
            continue
        err, tol = rel_err(got_g[k], g), grad_tol(k, rel_err(g2_32[k], g))
        errp, tolp = rel_err(got_p[k], p64[k]), grad_tol(k, rel_err(p32[k], p64[k]))
        worst = max(worst, err / tol, errp / tolp)
        print(f"{k:40s} grad err {err:.3e} tol {tol:.1e} | param err {errp:.3e} tol {tolp:.1e}")
        assert err <= tol, (k, err, tol)
        assert errp <= tolp, (k, errp, tolp)
    print(f"worst err / tol {worst:.3f}")


# ---- 4. off = the plain step ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [(ATT, 64, 2), (CG, 64, 2), (ATT, 32, 1)], ids=["attention", "cnn_gru", "embedded"])
def test_none_null_and_rho_zero_are_the_plain_step_bit_for_bit(model):
    """Three steps with eps = 0.1, lam = 0.4, clip and dropout: msig_da_train_step and msig_kd_train_step themselves, msig_sam_train_step
    with a NULL msig_sam and Engine.train_step at rho = 0 leave the same parameters, gradients, moments, BatchNorm state and losses; rho > 0
    does not."""
    kind, hidden, layers = model
    Cc, K, B, T = 3, 2, 16, 256
    engines = {}
    for mode in ("plain", "kd", "null", "zero", "on"):
        e = engines[mode] = _engine(Cc, K, hidden, layers, kind)
        for s in (1, 2, 3):
            x, y = _data(B, Cc, K, T, 10 + s)
            kw = dict(weight_decay=WD, step=s, dropout_p=0.5, seed=7, label_smoothing=0.1, mix_lambda=0.4, max_grad_norm=1.0)
            if mode in ("kd", "null"):
                if layers == 1:
                    e.scatter()
                e.ensure_adam_state()
                b = e._batch(x, y, True, 0.5, 7, s)
                sd = C.byref(e._st(*e._checked(None, 1.0, 0.1, 0.4)))
                tail = (e.exp_avg.data_ptr(), e.exp_avg_sq.data_ptr(), LR, 0.9, 0.999, 1e-8, WD, s, _stream())
                if mode == "kd":
                    L.check(L.lib().msig_kd_train_step(C.byref(b), sd, None, None, *tail), "msig_kd_train_step")
                else:
                    L.check(L.lib().msig_sam_train_step(C.byref(b), sd, None, None, *tail), "msig_sam_train_step")
                if layers == 1:
                    e.gather()
            elif mode == "plain":                                # msig_da_train_step, called directly (Engine.train_step is msig_sc_train_step)
                assert narrow_train_step(e, x, y, LR, **kw) == "msig_da_train_step"
            else:
                e.train_step(x, y, LR, sam={"zero": Sam(0.0), "on": Sam(0.05)}[mode], **kw)
        torch.cuda.synchronize()
    plain = engines["plain"]
    for mode in ("kd", "null", "zero", "on"):
        e = engines[mode]
        same = all(torch.equal(_bits(getattr(plain, n)), _bits(getattr(e, n))) for n in ("params", "grads", "exp_avg", "exp_avg_sq", "bn_state", "bn_count"))
        same_loss = torch.equal(plain.loss_acc, e.loss_acc) and torch.equal(_bits(plain.region("LOSS", torch.float32, (3,))), _bits(e.region("LOSS", torch.float32, (3,))))
        if mode == "on":
            assert not same and float(e.sam_state[L.SAM_STEPS]) == 3.0
        else:
            assert same and same_loss, mode
    assert plain.sam_state is None and not engines["zero"].sam_state[:L.SAM_NSTAT].any()      # rho = 0: nothing launched, nothing reported


@pytest.mark.parametrize("B", [16, 2064])
def test_launch_names(B):
    """By the library's own launch report: sam=None and rho = 0 are the plain step's launches.  rho > 0: every launch of the plain step
    twice, except that the head runs unfused in both passes (head_fwd, ce, head_bwd instead of head_step where that applies:
    B <= 2048), pass 1 reduces without Adam (colsum), and the three launches of this feature run once each."""
    Cc, K, T = 3, 2, 64
    x, y = _data(B, Cc, K, T, 4)
    reports = []
    for sam in (None, Sam(0.0), Sam(0.05)):
        e = _engine(Cc, K)
        e.train_step(x, y, LR, step=1, dropout_p=0.5, seed=7, sam=sam)          # workspaces exist before the count starts
        torch.cuda.synchronize()
        L.profile_enable(True)
        try:
            e.train_step(x, y, LR, step=2, dropout_p=0.5, seed=7, sam=sam)
            torch.cuda.synchronize()
            reports.append({k: v[0] for k, v in L.profile_report().items()})
        finally:
            L.profile_enable(False)
    plain, zero, on = reports
    assert plain == zero and not any(k.startswith("sam_") for k in plain) and sum(plain.values()) > 5
    want = dict(plain)
    if B <= 2048:
        assert want.pop("head_step") == 1 and "head_fwd" not in plain
        want.update(head_fwd=1, ce=1, head_bwd=1)
    assert want.pop("colsum_adam") == 1 and "colsum" not in want
    want = {k: 2 * v for k, v in want.items()}
    want.update(colsum=1, colsum_adam=1, sam_sq=1, sam_perturb=1, sam_restore=1)
    assert on == want
    print(f"B = {B}: plain {sum(plain.values())} launches, SAM {sum(on.values())}")


def test_sam_with_an_adversary_is_refused_before_any_launch():
    from multimodalsignal_amd.adversary import SubjectAdversary
    Cc, K, B, T = 3, 2, 8, 64
    x, y = _data(B, Cc, K, T, 4)
    for e in (_engine(Cc, K), _engine(Cc, K, 32, 1)):
        before = e.params.clone()
        adv = SubjectAdversary(3, lam=0.5, schedule="constant", seed=1)
        adv.set_domains(np.zeros(B, dtype=np.int32))
        adv.bind(DEV)
        with pytest.raises(ValueError, match="adversary"):
            e.train_step(x, y, LR, step=1, sam=Sam(0.05), adversary=adv)
        torch.cuda.synchronize()
        assert torch.equal(e.params, before) and e.sam_state is None and adv.step == 0


# ---- 5. fold batches ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adaptive", [False, True], ids=["sam", "asam"])
@pytest.mark.parametrize("extras", [False, True], ids=["plain", "distill_clip"])
def test_train_step_multi_equals_the_single_calls(extras, adaptive):
    """Three folds in arenas {0, 2, 5} of six, each with its own weights, inputs, dropout keys, step count, learning rate and mixup
    weight (extras: its own teacher table and max_norm too): msig_sam_train_step_multi leaves every fold's parameters, gradients,
    moments, BatchNorm state, losses and SAM statistics with the bits of its msig_sam_train_step."""
    slots, n_arena, B, T, Cc, K, npos = [0, 2, 5], 6, 16, 256, 3, 2, 40
    lams, msteps, lrs = (1.0, 0.4, 0.7), (1, 3, 5), (1e-3, 5e-4, 2e-3)
    norms = (0.05, float("inf"), 1.0)
    alpha, Tk = 0.5, 2.0
    sam = Sam(0.05, adaptive)
    rs = np.random.RandomState(8)
    data = [_data(B, Cc, K, T, 300 + f) for f in slots]
    tables = []
    for _ in slots:
        e_ = np.exp(1.5 * rs.randn(npos, K))
        tables.append((e_ / e_.sum(axis=1, keepdims=True)).astype(np.float32))
    idx = _dev(rs.randint(0, npos, size=(len(slots), B + 3)).astype(np.int64))
    arena = FoldArena(Cc, K, DEV, n_arena, B, T, distill=npos if extras else None, grad_clip=extras, sam=True)
    plain_arena = FoldArena(Cc, K, DEV, n_arena, B, T, distill=npos if extras else None, grad_clip=extras)
    assert list(arena.off)[:-1] == list(plain_arena.off) and list(arena.off)[-1] == "sam" and arena.stride > plain_arena.stride
    assert all(arena.off[k] == plain_arena.off[k] for k in plain_arena.off)
    engs, kds = {}, {}
    for j, f in enumerate(slots):
        engs[f] = _engine(Cc, K, seed=10 + f, storage_engine=arena.engine(f))
        x, y = data[j]
        arena.view(f, "x", torch.float32)[:x.numel()].copy_(x.reshape(-1))
        arena.view(f, "y", torch.int64)[:B].copy_(y)
        if extras:
            d = Distillation(alpha, Tk)
            d.set_teacher(tables[j])
            kds[f] = d.bind(DEV, arena.side_storage("distill", f))
            arena.set_max_norm(f, norms[j])
    m = arena.multi(slots, key_gru=[L.dropout_key(100 + f, msteps[j], 1) for j, f in enumerate(slots)],
                    key_head=[L.dropout_key(100 + f, msteps[j], 2) for j, f in enumerate(slots)], lr=lrs, steps=msteps)
    desc = arena.batch(B, True, 0.5)
    sd = arena.soft(slots, 0.1, lams, clip=arena.clip(slots) if extras else None)
    k = None
    if extras:
        k = arena.kd(alpha, Tk)
        k.idx, k.idx_row_stride = idx.data_ptr(), B + 3
    sm = arena.sam(sam)
    L.check(L.lib().msig_sam_train_step_multi(C.byref(desc), C.byref(m), C.byref(sd), None if k is None else C.byref(k), C.byref(sm),
                                              arena.ptr("exp_avg"), arena.ptr("exp_avg_sq"), 0.9, 0.999, 1e-8, WD, msteps[0], _stream()),
            "msig_sam_train_step_multi")
    torch.cuda.synchronize()
    for j, f in enumerate(slots):
        e = _engine(Cc, K, seed=10 + f)
        d = None
        if extras:
            d = Distillation(alpha, Tk)
            d.set_teacher(tables[j])
            d.bind(DEV)
        x, y = data[j]
        e.train_step(x, y, lrs[j], weight_decay=WD, step=msteps[j], dropout_p=0.5, seed=100 + f, label_smoothing=0.1, mix_lambda=lams[j],
                     max_grad_norm=norms[j] if extras else None, distill=d, batch_index=idx[j, :B].contiguous() if extras else None, sam=sam)
        torch.cuda.synchronize()
        for name in ("params", "grads", "exp_avg", "exp_avg_sq", "bn_state", "bn_count", "loss_acc"):
            assert torch.equal(_bits(getattr(e, name)), _bits(getattr(engs[f], name))), (f, name)
        assert torch.equal(e.sam_state[:L.SAM_NSTAT], engs[f].sam_state[:L.SAM_NSTAT]) and float(e.sam_state[L.SAM_STEPS]) == 1.0, f
        assert float(e.sam_state[L.SAM_NORM_LAST]) > 0 and float(e.sam_state[L.SAM_SHARP_LAST]) != 0.0
        off = L.workspace_layout(B, Cc, T, K, True)[L.WS["LOSS"]]
        assert torch.equal(_bits(arena.view(f, "ws")[off:off + 12].view(torch.float32)), _bits(e.region("LOSS", torch.float32, (3,)))), f
        if extras:
            assert torch.equal(d.stats, kds[f].stats) and float(d.stats[2]) == B, f             # the term reported once, at w
            assert torch.equal(e.gc_state[:L.GC_NSTAT], engs[f].gc_state[:L.GC_NSTAT]), f
    for f in set(range(n_arena)) - set(slots):                                                   # the arenas between them were not touched
        assert not arena.view(f, "sam", torch.float64).any() and not arena.view(f, "grads", torch.float32).any()


# ---- 6. the driver --------------------------------------------------------------------------------------------------------------------
SUBS = ["S2", "S3", "S4"]


def _run(tmp_path, tag, extra):
    from multimodalsignal_amd import main as M
    M.main(["--synthetic", str(tmp_path / "w"), "--synthetic-windows", "24", "--samples", "256", "--subjects", *SUBS, "--epochs", "2",
            "--batch-size", "8"] + extra + ["--out", str(tmp_path / tag)])
    return next((tmp_path / tag).glob("*/run_*"))


def _results(run):
    out = []
    for s in SUBS:
        doc = json.loads((run / f"fold_test_on_{s}" / "fold_result.json").read_text())
        doc = {k: v for k, v in doc.items() if "seconds" not in k and k != "train_windows_per_s"}
        doc["history"] = [{k: v for k, v in h.items() if k != "seconds"} for h in doc["history"]]
        out.append(doc)
    return out


def _weights(run):
    return [torch.load(run / f"fold_test_on_{s}" / "best_model.pt", weights_only=True) for s in SUBS]


def _same_weights(a, b):
    return all(list(wa) == list(wb) and all(torch.equal(wa[k], wb[k]) for k in wa) for wa, wb in zip(a, b))


def test_driver_fold_batches_equal_sequential_and_rho_zero_is_the_plain_run(tmp_path):
    """A two-epoch synthetic LOSO on 3 subjects: --sam 0.05 as one fold batch and with --concurrent-folds 1 gives the same metrics,
    history (sam_* entries included) and weights; --sam 0 is the run without the flag; --sam 0.05 is not."""
    runs = {tag: _run(tmp_path, tag, extra) for tag, extra in (("lock", ["--sam", "0.05", "--concurrent-folds", "3"]),
                                                               ("seq", ["--sam", "0.05", "--concurrent-folds", "1"]),
                                                               ("zero", ["--sam", "0"]), ("plain", []))}
    res = {tag: _results(run) for tag, run in runs.items()}
    assert res["lock"] == res["seq"] and _same_weights(_weights(runs["lock"]), _weights(runs["seq"]))
    assert res["zero"] == res["plain"] and _same_weights(_weights(runs["zero"]), _weights(runs["plain"]))
    assert not _same_weights(_weights(runs["lock"]), _weights(runs["plain"]))
    for doc in res["lock"]:
        assert len(doc["history"]) == 2
        for h in doc["history"]:
            assert h["sam_grad_norm"] > 0 and h["sam_grad_norm_max"] >= h["sam_grad_norm"] and np.isfinite(h["sam_sharpness"])
    assert all("sam_grad_norm" not in h for doc in res["plain"] for h in doc["history"])
    log = (runs["lock"] / "fold_test_on_S2" / "training_log.txt").read_text(encoding="utf-8")
    assert "sam grad norm" in log and "sam sharpness" in log and "sam=0.05" in log
    assert "SAM: 0.05\n" in (runs["lock"] / "cv_summary.txt").read_text(encoding="utf-8")
    assert "SAM" not in (runs["plain"] / "cv_summary.txt").read_text(encoding="utf-8")


@pytest.mark.parametrize("mode", [["--hierarchical"], ["--model", "cnn_gru_attention", "cnn_gru"], ["--ablation"], ["--no-lockstep"],
                                  ["--seeds", "2", "--distill", "--max-grad-norm", "1"]],
                         ids=["hierarchical", "model", "ablation", "no-lockstep", "seeds-distill-clip"])
def test_every_driver_mode_trains_with_sam(tmp_path, mode):
    """Every trainer of every driver — the hierarchical experiment's M1 and its embedded one-layer M2, both model kinds, every
    ablation configuration, sequential folds, seed replicas and their distilled students — logs the epoch's SAM statistics."""
    _run(tmp_path, "o", ["--sam", "0.05:adaptive"] + mode)
    logs = list((tmp_path / "o").rglob("training_log.txt"))
    assert len(logs) >= len(SUBS) * (2 if mode[0] in ("--hierarchical", "--model", "--seeds") else 1)
    for log in logs:
        text = log.read_text(encoding="utf-8")
        assert "sam grad norm" in text and "sam=0.05:adaptive:0.01" in text, log
    checked = 0
    for res in (tmp_path / "o").rglob("fold_result.json"):
        hist = json.loads(res.read_text()).get("history")          # the hierarchical experiment's per-fold file carries no history
        if hist is not None:
            checked += 1
            assert hist and all(h["sam_grad_norm"] > 0 and np.isfinite(h["sam_sharpness"]) for h in hist), res
    assert checked >= len(SUBS) or mode[0] == "--hierarchical"
