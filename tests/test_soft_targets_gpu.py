"""GPU tier: soft targets (include/msig_st.h) through every layer — switched off they are the product as it stands (bits, launches),
the mixed gather equals tests/st_reference.py bit for bit, a soft-target train step matches torch's cross_entropy(label_smoothing=,
weight=) over the fp64 oracle within gpu_common's adaptive tolerances, staged equals fused, folds equal their stand-alone runs, the
clip composes, evaluation smooths without mixing, and the drivers carry both knobs through every mode."""
import ctypes as C
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import st_reference as S
from aug_reference import dropout_key
from gpu_common import grad_tol, legacy_forward, legacy_train_step, rel_err, stage_tol
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd.augment import Augment
from multimodalsignal_amd.mixup import Mixup
from multimodalsignal_amd.multifold import launch_plan
from multimodalsignal_amd.runtime import EmbeddedEngine, Engine, FoldArena
from oracle import cnn_gru_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LR, WD, P = 1e-3, 1e-4, 0.5
W2, W3 = (0.3, 2.5), (1.0, 0.2, 4.0)
ATT, CG = "cnn_gru_attention", "cnn_gru"
AUG_ON = dict(scale=0.1, jitter=0.05, mask_prob=0.5, mask_max=7, chan_drop=0.3)


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _data(B, Cc, K, T, seed):
    rs = np.random.RandomState(seed)
    y = rs.randint(0, K, size=B).astype(np.int64)
    y[:min(K, B)] = np.arange(min(K, B))
    return torch.as_tensor(rs.randn(B, Cc, T).astype(np.float32)).to(DEV), torch.as_tensor(y).to(DEV)


def _params(Cc, K, hidden=64, layers=2, kind=ATT, seed=None, sharp=True):
    """The oracle's initial parameters of a model kind.  sharp: the last layer scaled up and given a bias, so that the logits are far
    from uniform — at the initial scale every criterion is about log K and label smoothing moves the loss by less than the tests'
    precondition asks for."""
    params = O.init_params(Cc, K, seed=Cc + K if seed is None else seed, hidden=hidden, layers=layers)
    if kind == CG:
        params = {k: v for k, v in params.items() if k not in L.GATE_KEYS}
    if sharp:
        params["classifier.3.weight"] = params["classifier.3.weight"] * 30.0
        params["classifier.3.bias"] = torch.linspace(-1.0, 1.0, K, dtype=params["classifier.3.bias"].dtype)
    return params


def _engine(Cc, K, hidden=64, layers=2, seed=3, storage_engine=None, kind=ATT, params=None):
    if params is None:
        params = _params(Cc, K, hidden, layers, kind, seed, sharp=False)
    e = storage_engine
    if e is None:
        e = EmbeddedEngine(Cc, K, DEV, hidden, kind=kind) if layers == 1 else Engine(Cc, K, DEV, kind=kind)
    if layers == 1:
        for k, v in e.small_views().items():
            v.copy_(params[k])
    else:
        e.load_named(params)
    return e, params


def _regions(e, B, K, dlogits=True):
    r = {"LOSS": e.region("LOSS", torch.float32, (3,)), "PROBS": e.region("PROBS", torch.float32, (B, K)),
         "PRED": e.region("PRED", torch.int32, (B,)), "LOGITS": e.region("LOGITS", torch.float32, (B, K))}
    if dlogits:
        r["DLOGITS"] = e.region("DLOGITS", torch.float32, (B, K))
    return r


def _wt(w):
    return None if w is None else torch.tensor(w, dtype=torch.float32, device=DEV)


def _st_train_step(e, x, y, step, smoothing, lam, seed=7, cw=None, clip=None):
    """msig_st_train_step itself, whatever the values."""
    e.ensure_adam_state()
    b = e._batch(x, y, True, P, seed, step)
    s = L.make_st(e.kind, smoothing, e._class_weight(cw), clip, [lam])
    L.check(L.lib().msig_st_train_step(C.byref(b), C.byref(s), e.exp_avg.data_ptr(), e.exp_avg_sq.data_ptr(), LR, 0.9, 0.999, 1e-8, WD, step,
                                       e._stream()), "msig_st_train_step")


def _st_forward(e, x, y, smoothing, lam, keep):
    b = e._batch(x, y, False, 0.0, 0, 0, keep)
    s = L.make_st(e.kind, smoothing, None, None, [lam])
    L.check(L.lib().msig_st_forward(C.byref(b), C.byref(s), e._stream()), "msig_st_forward")


# ---- 1. off is the product as it stands ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(64, 256), (3000, 64)])
def test_off_train_step_is_bit_identical(B, T):
    """msig_st_train_step with eps = 0, lam = 1 against msig_train_step: B = 64 the one-launch head, B = 3000 the separate ce_kernel."""
    Cc, K = 6, 2
    x, y = _data(B, Cc, K, T, 1)
    out = []
    for off in (False, True):
        e, _ = _engine(Cc, K)
        for s in (1, 2):
            if off:
                _st_train_step(e, x, y, s, 0.0, 1.0)
            else:
                assert legacy_train_step(e, x, y, LR, weight_decay=WD, step=s, dropout_p=P, seed=7) == "msig_train_step"
        out.append(e)
    torch.cuda.synchronize()
    a, b = out
    for name in ("params", "grads", "exp_avg", "exp_avg_sq", "bn_state"):
        assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name
    assert torch.equal(a.loss_acc, b.loss_acc)
    ra, rb = _regions(a, B, K), _regions(b, B, K)
    for k in ra:
        assert torch.equal(_bits(ra[k]), _bits(rb[k])), k


def test_off_eval_forward_is_bit_identical():
    Cc, K, B, T = 3, 3, 100, 256
    x, y = _data(B, Cc, K, T, 2)
    for keep in (False, True):
        a, _ = _engine(Cc, K)
        b, _ = _engine(Cc, K)
        assert legacy_forward(a, x, y, keep_for_backward=keep) == "msig_forward"
        _st_forward(b, x, y, 0.0, 1.0, keep)
        torch.cuda.synchronize()
        ra, rb = _regions(a, B, K, keep), _regions(b, B, K, keep)
        for k in ra:
            assert torch.equal(_bits(ra[k]), _bits(rb[k])), (keep, k)
        assert torch.equal(a.loss_acc, b.loss_acc)


def _fold_data(n, B, Cc, K, T, steps=2):
    return [[_data(B, Cc, K, T, 1000 * f + s) for s in range(steps)] for f in range(n)]


def _arena_run(n, B, T, Cc, K, data, soft=None, weights=None, norms=None, steps=2, kind=ATT):
    """n folds in one FoldArena: `steps` train steps — soft = (eps, [lam per fold]): msig_st_train_step_multi (with the arenas' class
    weights and clip when given), None: msig_train_step_multi — then one evaluation pass.  Returns the arena and its engines."""
    arena = FoldArena(Cc, K, DEV, n, B, T, kind=kind, grad_clip=norms is not None)
    engs = [_engine(Cc, K, seed=10 + f, storage_engine=arena.engine(f), kind=kind)[0] for f in range(n)]
    if weights is not None:
        for f in range(n):
            arena.set_class_weight(f, weights[f])
    if norms is not None:
        for f in range(n):
            arena.set_max_norm(f, norms[f])
    cw = arena.ptr("cw") if weights is not None else None
    st, lib, slots = _stream(), L.lib(), list(range(n))
    for s in range(1, steps + 1):
        for f in range(n):
            x, y = data[f][s - 1]
            arena.view(f, "x", torch.float32)[:x.numel()].copy_(x.reshape(-1))
            arena.view(f, "y", torch.int64)[:B].copy_(y)
        m = arena.multi(slots, key_gru=[L.dropout_key(100 + f, s, 1) for f in range(n)],
                        key_head=[L.dropout_key(100 + f, s, 2) for f in range(n)], lr=[LR] * n, steps=[s] * n)
        desc = arena.batch(B, True, P)
        if soft is None:
            rc = lib.msig_train_step_multi(C.byref(desc), C.byref(m), arena.ptr("exp_avg"), arena.ptr("exp_avg_sq"), 0.9, 0.999, 1e-8, WD, s, st)
        else:
            sd = arena.soft(slots, soft[0], soft[1], cw, arena.clip(slots, cw) if norms is not None else None)
            rc = lib.msig_st_train_step_multi(C.byref(desc), C.byref(m), C.byref(sd), arena.ptr("exp_avg"), arena.ptr("exp_avg_sq"), 0.9, 0.999,
                                              1e-8, WD, s, st)
        L.check(rc, "train_step_multi")
    arena.across("acc", 0, torch.float64, 2).zero_()
    desc, m = arena.batch(B, False, 0.0), arena.multi(slots)
    if soft is None:
        L.check(lib.msig_forward_multi(C.byref(desc), C.byref(m), st), "msig_forward_multi")
    else:
        sd = arena.soft(slots, soft[0], None, cw)
        L.check(lib.msig_st_forward_multi(C.byref(desc), C.byref(m), C.byref(sd), st), "msig_st_forward_multi")
    torch.cuda.synchronize()
    return arena, engs


def test_off_fold_batch_is_bit_identical():
    """A 5-fold msig_st_train_step_multi with eps = 0 and every lam = 1, then msig_st_forward_multi, against the msig.h calls: every
    arena byte (soft targets add no region to an arena)."""
    n, B, T, Cc, K = 5, 64, 128, 6, 2
    data = _fold_data(n, B, Cc, K, T)
    a, _ = _arena_run(n, B, T, Cc, K, data)
    b, _ = _arena_run(n, B, T, Cc, K, data, soft=(0.0, [1.0] * n))
    assert a.stride == b.stride and torch.equal(a.mem, b.mem)


@pytest.mark.parametrize("B,T", [(64, 128), (2049, 32)])
def test_soft_targets_add_no_launch(B, T):
    Cc, K = 3, 3
    x, y = _data(B, Cc, K, T, 4)
    reports = []
    for kw in (dict(), dict(label_smoothing=0.1, mix_lambda=0.3)):
        e, _ = _engine(Cc, K)
        e.train_step(x, y, LR, weight_decay=WD, step=1, dropout_p=P, seed=7, **kw)           # workspaces exist before the count starts
        torch.cuda.synchronize()
        L.profile_enable(True)
        try:
            e.train_step(x, y, LR, weight_decay=WD, step=2, dropout_p=P, seed=7, **kw)
            torch.cuda.synchronize()
            reports.append({k: v[0] for k, v in L.profile_report().items()})
        finally:
            L.profile_enable(False)
    assert reports[0] == reports[1] and sum(reports[0].values()) > 5, reports


# ---- 2. the mixed gather ---------------------------------------------------------------------------------------------------------
def _store(N, Cc, T, seed):
    rs = np.random.RandomState(seed)
    s = rs.randn(N, Cc, T).astype(np.float32)
    s[0, 0, :4] = [-0.0, 0.0, -0.0, 1.0]                         # signed zeros: lam = 1 must copy, not compute
    return s, rs.randint(0, 5, size=N).astype(np.int64)


def _gather(store_d, sy_d, idx_d, B, Cc, T, lam, aug=None, key=0):
    ox = torch.full((B, Cc, T), float("nan"), device=DEV)
    oy = torch.full((B,), -1, dtype=torch.int64, device=DEV)
    a = C.byref(Augment(**aug).struct([key])) if aug else None
    L.check(L.lib().msig_st_gather_windows(store_d.data_ptr(), sy_d.data_ptr(), idx_d.data_ptr(), B, Cc, T, ox.data_ptr(), oy.data_ptr(), a,
                                           (C.c_float * 1)(lam), _stream()), "msig_st_gather_windows")
    return ox, oy


LAMS = [0.25, 0.5, float(np.nextafter(np.float32(1.0), np.float32(0.0)))]


@pytest.mark.parametrize("aug", [None, AUG_ON], ids=["plain", "aug"])
@pytest.mark.parametrize("B", [1, 2, 5, 64])
@pytest.mark.parametrize("Cc,T", [(3, 200), (16, 16), (2, 1040)])
def test_mixed_gather_equals_the_restatement(Cc, T, B, aug):
    store, sy = _store(B + 3, Cc, T, 10 * B + Cc)
    rs = np.random.RandomState(B)
    idx = rs.randint(0, B + 3, size=B).astype(np.int64)
    idx[0] = 0
    sd, syd, idd = torch.as_tensor(store).to(DEV), torch.as_tensor(sy).to(DEV), torch.as_tensor(idx).to(DEV)
    key = dropout_key(5, B, 3)
    kw = dict(aug) if aug else {}
    if aug:
        kw["mask_max"] = min(T, aug["mask_max"])
    for lam in LAMS:
        ox, oy = _gather(sd, syd, idd, B, Cc, T, lam, kw or None, key)
        want = S.mix(store, idx, lam, key, **kw)
        assert np.array_equal(ox.cpu().numpy().view(np.int32), want.view(np.int32)), lam
        assert np.array_equal(oy.cpu().numpy(), sy[idx])                                        # the rows' own labels
    ox, oy = _gather(sd, syd, idd, B, Cc, T, 1.0, kw or None, key)                               # lam = 1: the plain / augmented gather's bits
    ref = torch.empty_like(ox)
    if aug:
        a = Augment(**kw).struct([key])
        L.check(L.lib().msig_aug_gather_windows(sd.data_ptr(), syd.data_ptr(), idd.data_ptr(), B, Cc, T, ref.data_ptr(), None, C.byref(a), _stream()), "aug")
    else:
        L.check(L.lib().msig_gather_windows(sd.data_ptr(), syd.data_ptr(), idd.data_ptr(), B, Cc * T, ref.data_ptr(), None, _stream()), "plain")
    assert torch.equal(_bits(ox), _bits(ref)) and np.array_equal(oy.cpu().numpy(), sy[idx])
    assert np.array_equal(ox.cpu().numpy().view(np.int32), S.mix(store, idx, 1.0, key, **kw).view(np.int32))


@pytest.mark.parametrize("aug", [None, AUG_ON], ids=["plain", "aug"])
def test_multi_gather_equals_three_single_calls(aug):
    B, Cc, T, n = 5, 3, 200, 3
    store, sy = _store(20, Cc, T, 77)
    idx = np.random.RandomState(3).randint(0, 20, size=(n, B + 2)).astype(np.int64)
    sd, syd, idd = torch.as_tensor(store).to(DEV), torch.as_tensor(sy).to(DEV), torch.as_tensor(idx).to(DEV)
    lams, keys = [0.25, 1.0, 0.7], [dropout_key(9, f + 1, 3) for f in range(n)]
    xb = B * Cc * T * 4
    yoff = (xb + 255) // 256 * 256
    stride = yoff + 256
    mem = torch.zeros((n + 1, stride), dtype=torch.uint8, device=DEV)
    m = L.Multi()
    m.n, m.stride_bytes = n, stride
    for i, slot in enumerate((2, 0, 3)):
        m.slot[i] = slot
    a = C.byref(Augment(**aug).struct(keys)) if aug else None
    L.check(L.lib().msig_st_gather_windows_multi(sd.data_ptr(), syd.data_ptr(), idd.data_ptr(), B + 2, B, Cc, T, mem.data_ptr(),
                                                 mem.data_ptr() + yoff, C.byref(m), a, (C.c_float * L.MAX_FOLDS)(*lams), _stream()), "multi")
    for i, slot in enumerate((2, 0, 3)):
        ox, oy = _gather(sd, syd, idd[i, :B].contiguous(), B, Cc, T, lams[i], aug, keys[i])
        assert torch.equal(mem[slot, :xb].view(torch.int32), _bits(ox).reshape(-1)), i
        assert torch.equal(mem[slot, yoff:yoff + 8 * B].view(torch.int64), oy), i
    assert int(mem[1].count_nonzero()) == 0                                                      # an arena outside the launch is untouched


# ---- 3. against the fp64 reference -----------------------------------------------------------------------------------------------
TRIPLES = [(0.1, 1.0, None, 2), (0.0, 0.3, None, 3), (0.1, 0.3, W3, 3), (0.2, 0.7, W2, 2)]
_REF = {}


def _soft_loss(z, y, w, eps, lam, dt):
    wt = None if w is None else torch.tensor(w, dtype=dt)
    return lam * F.cross_entropy(z, y, weight=wt, label_smoothing=eps) + (1.0 - lam) * F.cross_entropy(z, y.flip(0), weight=wt, label_smoothing=eps)


def _reference(params, xm, y, w, eps, lam, kind, seed, step):
    """fp64 and fp32 runs of oracle forward over the MIXED input + torch's cross_entropy + autograd:
    {dtype: dict(loss, grads, dlogits, plain_loss, plain_g3)}.  The cnn_gru kind is the attention oracle on 2x with a gate of exactly 1/2
    (channel_attention.fc.2.weight = 0), as tests/test_cnngru_gpu.py establishes."""
    out = {}
    xc, yc = torch.as_tensor(xm), torch.as_tensor(y)
    for dt in (torch.float64, torch.float32):
        full = dict(params)
        if kind == CG:
            full = {**O.init_params(xc.shape[1], int(params["classifier.3.bias"].numel()), seed=1, hidden=params["gru.weight_hh_l0"].shape[1],
                                    layers=2 if "gru.weight_ih_l1" in params else 1), **params}
            full["channel_attention.fc.2.weight"] = torch.zeros_like(full["channel_attention.fc.2.weight"])
        leaf = {k: v.to(dt).clone().requires_grad_(v.numel() > 0) for k, v in full.items()}
        bufs = {k: (v if "num_batches" in k else v.to(dt)) for k, v in O.init_buffers().items()}
        st, _ = O.forward(leaf, bufs, (2.0 * xc if kind == CG else xc).to(dt), training=True, dropout_p=P, seed=seed, step=step)
        z = st["logits"]
        loss = _soft_loss(z, yc, w, eps, lam, dt)
        plain = F.cross_entropy(z, yc, weight=None if w is None else torch.tensor(w, dtype=dt))
        dz = torch.autograd.grad(loss, z, retain_graph=True)[0]
        pg3 = torch.autograd.grad(plain, leaf["classifier.3.weight"], retain_graph=True)[0]
        loss.backward()
        out[dt] = dict(loss=float(loss.detach()), dlogits=dz.double().numpy(), plain_loss=float(plain.detach()), plain_g3=pg3.double().numpy(),
                       grads={k: (v.grad if v.grad is not None else torch.zeros_like(v)).double().numpy() for k, v in leaf.items() if k in params})
    return out


def _case(kind, model, B, Cc, triple):
    """One soft-target train step on the GPU and its reference, computed once per case and shared by the tests below."""
    key = (kind, model, B, Cc, triple)
    if key not in _REF:
        eps, lam, w, K = triple
        hidden, layers = model
        T = 128 if B == 64 else 32
        e, params = _engine(Cc, K, hidden, layers, kind=kind, params=_params(Cc, K, hidden, layers, kind))
        x, y = _data(B, Cc, K, T, B + Cc)
        xm = S.mix(x.cpu().numpy(), np.arange(B), lam)
        e.train_step(torch.as_tensor(xm).to(DEV), y, LR, weight_decay=WD, step=1, dropout_p=P, seed=11, class_weight=_wt(w), label_smoothing=eps,
                     mix_lambda=lam)
        torch.cuda.synchronize()
        got = dict(loss=float(e.region("LOSS", torch.float32, (3,))[0]), dlogits=e.region("DLOGITS", torch.float32, (B, K)).cpu().numpy().copy(),
                   grads={k: v.detach().cpu().numpy().copy() for k, v in (e.gather_grads() if layers == 1 else e.named_param_views(e.grads)).items()})
        _REF[key] = (got, _reference(params, xm, y.cpu().numpy(), w, eps, lam, kind, 11, 1))
    return _REF[key]


@pytest.mark.parametrize("triple", TRIPLES, ids=lambda t: f"eps{t[0]}-lam{t[1]}-{'w' if t[2] else 'u'}{t[3]}")
@pytest.mark.parametrize("Cc", [1, 6])
@pytest.mark.parametrize("B", [64, 2049])
@pytest.mark.parametrize("model", [(64, 2), (32, 1)])
@pytest.mark.parametrize("kind", [ATT, CG])
def test_soft_step_matches_fp64_reference(kind, model, B, Cc, triple):
    """Loss, dlogits and every parameter gradient of msig_st_train_step against torch over the fp64 oracle; the mixed x is the
    restatement's.  Precondition, from the reference alone: the plain criterion's loss and classifier.3.weight gradient on the same
    input differ from the soft-target ones by more than 100 x the tolerance, so a kernel that ignores eps or the partner cannot pass."""
    got, ref = _case(kind, model, B, Cc, triple)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    l64 = r64["loss"]
    tol_l = stage_tol("loss", abs(r32["loss"] - l64) / max(abs(l64), 1e-6))
    k3 = "classifier.3.weight"
    tol_g3 = grad_tol(k3, rel_err(r32["grads"][k3], r64["grads"][k3]))
    assert abs(r64["plain_loss"] - l64) / max(abs(l64), 1e-6) > 100 * tol_l
    assert rel_err(r64["plain_g3"], r64["grads"][k3]) > 100 * tol_g3
    err_l = abs(got["loss"] - l64) / max(abs(l64), 1e-6)
    err_d, tol_d = rel_err(got["dlogits"], r64["dlogits"]), stage_tol("d_logits", rel_err(r32["dlogits"], r64["dlogits"]))
    print(f"loss err {err_l:.3e} tol {tol_l:.1e} | dlogits err {err_d:.3e} tol {tol_d:.1e}")
    assert err_l <= tol_l, (got["loss"], l64)
    assert err_d <= tol_d
    assert set(got["grads"]) == set(r64["grads"])
    for k, g in r64["grads"].items():
        err, tol = rel_err(got["grads"][k], g), grad_tol(k, rel_err(r32["grads"][k], g))
        assert err <= tol, (k, err, tol)


# ---- 4. staged equals fused ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(64, 128), (2049, 32)])
def test_staged_equals_fused(B, T):
    """msig_st_forward(training) + msig_backward(NULL) + msig_adam_step gives msig_st_train_step's bits."""
    Cc, K = 3, 3
    x, y = _data(B, Cc, K, T, 5)
    kw = dict(class_weight=_wt(W3), label_smoothing=0.1, mix_lambda=0.3)
    a, _ = _engine(Cc, K)
    b, _ = _engine(Cc, K)
    a.backward(a.forward(x, y, training=True, dropout_p=P, seed=5, step=1, **kw))
    a.adam_step(LR, weight_decay=WD, step=1)
    b.train_step(x, y, LR, weight_decay=WD, step=1, dropout_p=P, seed=5, **kw)
    torch.cuda.synchronize()
    for name in ("grads", "params", "exp_avg", "exp_avg_sq", "bn_state"):
        assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name
    for r, shape in (("LOSS", (3,)), ("DLOGITS", (B, K)), ("PROBS", (B, K))):
        assert torch.equal(_bits(a.region(r, torch.float32, shape)), _bits(b.region(r, torch.float32, shape))), r
    assert torch.equal(a.loss_acc, b.loss_acc)
    plain, _ = _engine(Cc, K)
    plain.train_step(x, y, LR, weight_decay=WD, step=1, dropout_p=P, seed=5, class_weight=_wt(W3))
    torch.cuda.synchronize()
    assert not torch.equal(_bits(plain.grads), _bits(b.grads))


# ---- 5. folds --------------------------------------------------------------------------------------------------------------------
def test_folds_equal_their_standalone_runs():
    """Three folds with different lam, weight vectors and clip bounds and one eps equal their stand-alone msig_st_train_step runs in
    parameters, moments and BN state; a companion's lam leaves fold 0's arena bytes unchanged; a fold at (eps 0 handled per launch)
    lam = 1 takes its own statements."""
    n, B, T, Cc, K = 3, 64, 128, 3, 3
    data = _fold_data(n, B, Cc, K, T)
    ws = [W3, (0.5, 0.5, 2.0), (3.0, 1.0, 0.25)]
    lams, norms, eps = [0.3, 1.0, 0.85], [0.05, float("inf"), 1.0], 0.1
    arena, engs = _arena_run(n, B, T, Cc, K, data, soft=(eps, lams), weights=ws, norms=norms)
    for f in range(n):
        e, _ = _engine(Cc, K, seed=10 + f)
        for s in (1, 2):
            x, y = data[f][s - 1]
            e.train_step(x, y, LR, weight_decay=WD, step=s, dropout_p=P, seed=100 + f, class_weight=_wt(ws[f]), max_grad_norm=norms[f],
                         label_smoothing=eps, mix_lambda=lams[f])
        torch.cuda.synchronize()
        for name in ("params", "exp_avg", "exp_avg_sq", "bn_state"):
            assert torch.equal(_bits(getattr(e, name)), _bits(getattr(engs[f], name))), (f, name)
    arena2, _ = _arena_run(n, B, T, Cc, K, data, soft=(eps, [0.3, 0.6, 0.85]), weights=ws, norms=norms)
    assert torch.equal(arena.mem[0], arena2.mem[0]) and torch.equal(arena.mem[2], arena2.mem[2])
    assert not torch.equal(arena.mem[1], arena2.mem[1])
    # eps = 0: the fold at lam = 1 is the plain weighted step whatever its companions mix
    arena3, engs3 = _arena_run(n, B, T, Cc, K, data, soft=(0.0, [0.3, 1.0, 0.85]), weights=ws)
    e, _ = _engine(Cc, K, seed=11)
    for s in (1, 2):
        x, y = data[1][s - 1]
        e.train_step(x, y, LR, weight_decay=WD, step=s, dropout_p=P, seed=101, class_weight=_wt(ws[1]))
    torch.cuda.synchronize()
    for name in ("params", "exp_avg", "exp_avg_sq", "bn_state"):
        assert torch.equal(_bits(getattr(e, name)), _bits(getattr(engs3[1], name))), name


def test_ragged_plan_mixes_within_the_launchs_batch():
    """Folds of 70 and 64 training windows at batch 64: one launch of two folds at B = 64, then fold 0 alone at B = 6, whose rows pair
    within those 6.  Gather (msig_st_gather_windows_multi) and step equal the stand-alone loop's."""
    sizes, bs, Cc, K, T = [70, 64], 64, 3, 2, 128
    store, sy = _store(80, Cc, T, 5)
    sy = (sy % K).astype(np.int64)
    sd, syd = torch.as_tensor(store).to(DEV), torch.as_tensor(sy).to(DEV)
    rs = np.random.RandomState(1)
    orders = [rs.permutation(80)[:n].astype(np.int64) for n in sizes]
    mat = torch.as_tensor(np.stack([np.concatenate([o, np.repeat(o[:1], 70 - len(o))]) for o in orders])).to(DEV)
    mix, eps = Mixup(0.4), 0.1
    arena = FoldArena(Cc, K, DEV, 2, bs, T)
    engs = [_engine(Cc, K, seed=20 + f, storage_engine=arena.engine(f))[0] for f in range(2)]
    plan = launch_plan(sizes, bs)
    assert plan == [(0, 64, 0, 2), (64, 6, 0, 1)]
    st, lib = _stream(), L.lib()
    for i, b, r0, nr in plan:
        k = i // bs + 1
        slots = list(range(r0, r0 + nr))
        lams = [mix.lam(500 + f, k) for f in slots]
        m = arena.multi(slots, key_gru=[L.dropout_key(100 + f, k, 1) for f in slots], key_head=[L.dropout_key(100 + f, k, 2) for f in slots],
                        lr=[LR] * nr, steps=[k] * nr)
        L.check(lib.msig_st_gather_windows_multi(sd.data_ptr(), syd.data_ptr(), mat.data_ptr() + 8 * (r0 * 70 + i), 70, b, Cc, T, arena.ptr("x"),
                                                 arena.ptr("y"), C.byref(m), None, (C.c_float * L.MAX_FOLDS)(*lams), st), "gather")
        desc, sdsc = arena.batch(b, True, P), arena.soft(slots, eps, lams)
        L.check(lib.msig_st_train_step_multi(C.byref(desc), C.byref(m), C.byref(sdsc), arena.ptr("exp_avg"), arena.ptr("exp_avg_sq"), 0.9, 0.999,
                                             1e-8, WD, k, st), "step")
    torch.cuda.synchronize()
    for f in range(2):
        e, _ = _engine(Cc, K, seed=20 + f)
        for k, i in enumerate(range(0, sizes[f], bs), start=1):
            idx = orders[f][i:i + bs]
            lam = mix.lam(500 + f, k)
            xm = torch.as_tensor(S.mix(store, idx, lam)).to(DEV)
            ox, oy = _gather(sd, syd, torch.as_tensor(idx).to(DEV), len(idx), Cc, T, lam)
            assert torch.equal(_bits(ox), _bits(xm))
            e.train_step(ox, oy, LR, weight_decay=WD, step=k, dropout_p=P, seed=100 + f, label_smoothing=eps, mix_lambda=lam)
        torch.cuda.synchronize()
        for name in ("params", "exp_avg", "exp_avg_sq", "bn_state"):
            assert torch.equal(_bits(getattr(e, name)), _bits(getattr(engs[f], name))), (f, name)


# ---- 6. with the clip ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(64, 128), (2049, 32)])
def test_infinite_clip_is_the_unclipped_soft_step(B, T):
    Cc, K = 3, 3
    x, y = _data(B, Cc, K, T, 6)
    kw = dict(class_weight=_wt(W3), label_smoothing=0.1, mix_lambda=0.3)
    a, _ = _engine(Cc, K)
    b, _ = _engine(Cc, K)
    for s in (1, 2):
        _st_train_step(a, x, y, s, 0.1, 0.3, seed=5, cw=kw["class_weight"])      # the counterpart: msig_st_train_step itself, no clip
        b.train_step(x, y, LR, weight_decay=WD, step=s, dropout_p=P, seed=5, max_grad_norm=float("inf"), **kw)
    torch.cuda.synchronize()
    for name in ("grads", "params", "exp_avg", "exp_avg_sq", "bn_state"):
        assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name
    assert torch.equal(a.loss_acc, b.loss_acc)
    assert torch.equal(_bits(a.region("LOSS", torch.float32, (3,))), _bits(b.region("LOSS", torch.float32, (3,))))


def test_finite_clip_reports_the_soft_gradients_norm():
    """MSIG_GC_LAST of a clipped soft-target step equals the fp64 norm of the reference's soft-target gradients."""
    kind, model, B, Cc, triple = ATT, (64, 2), 64, 6, TRIPLES[2]
    eps, lam, w, K = triple
    _, ref = _case(kind, model, B, Cc, triple)
    norm = {dt: float(np.sqrt(sum(float((g ** 2).sum()) for g in ref[dt]["grads"].values()))) for dt in ref}
    e, _ = _engine(Cc, K, params=_params(Cc, K))
    x, y = _data(B, Cc, K, 128, B + Cc)
    xm = torch.as_tensor(S.mix(x.cpu().numpy(), np.arange(B), lam)).to(DEV)
    e.train_step(xm, y, LR, weight_decay=WD, step=1, dropout_p=P, seed=11, class_weight=_wt(w), label_smoothing=eps, mix_lambda=lam,
                 max_grad_norm=0.5 * norm[torch.float64])
    torch.cuda.synchronize()
    stats = e.grad_stats()
    n64 = norm[torch.float64]
    tol = grad_tol("", abs(norm[torch.float32] - n64) / n64)
    assert abs(stats["last"] - n64) / n64 <= tol, (stats, n64)
    assert stats["clipped"] == 1


# ---- 7. evaluation ---------------------------------------------------------------------------------------------------------------
def test_eval_loss_is_smoothed_and_predictions_are_not_touched():
    Cc, K, T, eps = 3, 3, 128, 0.1
    e, _ = _engine(Cc, K)
    p, _ = _engine(Cc, K)
    want, correct = 0.0, 0
    e.loss_acc.zero_(), p.loss_acc.zero_()
    for s, Bi in enumerate((64, 64, 22), start=1):
        x, y = _data(Bi, Cc, K, T, 50 + s)
        e.forward(x, y, training=False, label_smoothing=eps)
        p.forward(x, y, training=False)
        lg = e.region("LOGITS", torch.float32, (Bi, K)).double().cpu()
        mean = float(F.cross_entropy(lg, y.cpu(), label_smoothing=eps))
        want += Bi * mean
        lossbuf = e.region("LOSS", torch.float32, (3,)).double().cpu()
        assert abs(float(lossbuf[0]) - mean) <= 2e-6 * abs(mean)
        assert abs(float(lossbuf[1]) - Bi * float(lossbuf[0])) <= 1e-6 * Bi * abs(float(lossbuf[0]))
        assert torch.equal(e.region("PRED", torch.int32, (Bi,)), p.region("PRED", torch.int32, (Bi,)))
        assert torch.equal(_bits(e.region("PROBS", torch.float32, (Bi, K))), _bits(p.region("PROBS", torch.float32, (Bi, K))))
        assert float(lossbuf[0]) != float(p.region("LOSS", torch.float32, (3,))[0])
    assert abs(float(e.loss_acc[0]) - want) <= 1e-6 * abs(want)
    assert float(e.loss_acc[1]) == float(p.loss_acc[1])


# ---- 8. drivers ------------------------------------------------------------------------------------------------------------------
SUBS = ["S2", "S3", "S4", "S5"]
FLAGS = ["--label-smoothing", "0.1", "--mixup", "0.2", "--augment", "scale=0.1,jitter=0.05"]
LINE = "SOFT TARGETS: label_smoothing=0.1 mixup_alpha=0.2\n"


def _common(tmp_path):
    return ["--synthetic", str(tmp_path / "w"), "--synthetic-windows", "12", "--samples", "256", "--subjects", *SUBS, "--epochs", "2",
            "--batch-size", "16"]


def _fold_outputs(run):
    out = []
    for s in SUBS:
        info = json.loads((run / f"fold_test_on_{s}" / "fold_result.json").read_text())
        info.pop("seconds", None), info.pop("train_windows_per_s", None)
        for h in info.get("history", []):
            h.pop("seconds", None)
        out.append((info, torch.load(run / f"fold_test_on_{s}" / "best_model.pt", weights_only=True)))
    return out


def test_lockstep_equals_sequential_with_soft_targets(tmp_path):
    from multimodalsignal_amd import main as M
    runs = {}
    for tag, extra in (("lock", []), ("seq", ["--concurrent-folds", "1"]), ("plain", None)):
        M.main(_common(tmp_path) + (FLAGS + extra if extra is not None else []) + ["--out", str(tmp_path / tag)])
        run = next((tmp_path / tag).glob("*/run_*"))
        txt = (run / "cv_summary.txt").read_text(encoding="utf-8")
        assert (LINE in txt) == (tag != "plain") and ("SOFT TARGETS" in txt) == (tag != "plain")
        runs[tag] = _fold_outputs(run)
    for (ia, wa), (ib, wb) in zip(runs["lock"], runs["seq"]):
        assert ia == ib
        assert list(wa) == list(wb) and all(torch.equal(wa[k], wb[k]) for k in wa)
    assert all(a[0]["history"] != p[0]["history"] for a, p in zip(runs["lock"], runs["plain"]))


@pytest.mark.parametrize("mode", [["--ablation"], ["--hierarchical"], ["--model", "cnn_gru_attention", "cnn_gru"], ["--no-lockstep"]],
                         ids=["ablation", "hierarchical", "model", "no-lockstep"])
def test_every_driver_mode_runs_and_names_the_setting(tmp_path, mode):
    from multimodalsignal_amd import main as M
    M.main(_common(tmp_path) + FLAGS + mode + ["--out", str(tmp_path / "o")])
    summaries = [p for p in (tmp_path / "o").rglob("*summary.txt")]
    assert summaries and all(LINE in p.read_text(encoding="utf-8") for p in summaries), summaries


def test_folds_of_a_batch_must_share_eps_and_alpha(tmp_path):
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.dataset import SubjectStore
    from multimodalsignal_amd.multifold import LockstepTrainer
    from multimodalsignal_amd.synth import make_synthetic_wesad, CHANNELS6
    subs = ["S2", "S3", "S4"]
    d = make_synthetic_wesad(tmp_path / "w", subjects=subs, windows_per_subject=8, T=256)
    names = (d / "_channel_names.txt").read_text().split()
    base = M.default_cfg()
    base.update(data_path=d, channels=list(CHANNELS6), subjects=subs, epochs=1, patience=20, batch_size=16)
    store = SubjectStore(d, subs, base["channels"], names, classification_mode=base["mode"], device=DEV)
    L.profile_enable(True)
    try:
        for key, vals, msg in (("mixup", (0.2, 0.4), "share one mixup alpha"), ("label_smoothing", (0.1, 0.2), "share one label_smoothing")):
            preps = [M.prepare_fold(k, subs[k], tmp_path / key, DEV, names, dict(base, **{key: vals[k]}), store) for k in range(2)]
            with pytest.raises(ValueError, match=msg):
                LockstepTrainer(preps, DEV)
        torch.cuda.synchronize()
        assert L.profile_report() == {}                                                   # before any launch
    finally:
        L.profile_enable(False)


# ---- 9. rejections leave everything as it was ------------------------------------------------------------------------------------
def test_rejections_happen_before_any_launch():
    e, _ = _engine(3, 2)
    x, y = _data(8, 3, 2, 64, 4)
    before = e.params.clone()
    for kw in (dict(label_smoothing=1.0), dict(label_smoothing=-0.1), dict(label_smoothing=float("nan")), dict(mix_lambda=1.5),
               dict(mix_lambda=-0.1), dict(mix_lambda=float("nan")), dict(label_smoothing="0.1")):
        with pytest.raises(ValueError):
            e.train_step(x, y, LR, **kw)
        with pytest.raises(ValueError):
            e.forward(x, y, **kw)
    e.ensure_adam_state()
    b = e._batch(x, y, True, P, 1, 1)
    for eps, lam in ((1.0, 0.5), (float("nan"), 0.5), (0.1, 1.5), (0.1, float("nan"))):
        s = L.make_st(e.kind, 0.0, None, None, [1.0])
        s.smoothing, s.lam[0] = eps, lam
        rc = L.lib().msig_st_train_step(C.byref(b), C.byref(s), e.exp_avg.data_ptr(), e.exp_avg_sq.data_ptr(), LR, 0.9, 0.999, 1e-8, WD, 1, e._stream())
        assert rc == -2
    store, sy = _store(8, 3, 64, 1)
    sd, idd = torch.as_tensor(store).to(DEV), torch.arange(8, device=DEV)
    out = torch.full((8, 3, 64), 7.0, device=DEV)
    for lam in (1.5, -0.5, float("nan")):
        rc = L.lib().msig_st_gather_windows(sd.data_ptr(), None, idd.data_ptr(), 8, 3, 64, out.data_ptr(), None, None, (C.c_float * 1)(lam), _stream())
        assert rc == -2
    with pytest.raises(ValueError):
        FoldArena(3, 2, DEV, 2, 8, 64).soft([0, 1], 0.1, [0.5, 2.0])
    torch.cuda.synchronize()
    assert torch.equal(before, e.params) and int(e.bn_count[0]) == 0 and bool((out == 7.0).all())
    assert float(e.exp_avg.abs().sum()) == 0.0
