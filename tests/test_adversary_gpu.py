"""GPU tier: subject-adversarial training (include/msig_da.h) through every layer — the discriminator's step against the float64
restatement (tests/da_reference.py) at the chunk edges, the ragged tail, the self-paired middle row and the padded S; a step without
a labelled row writes nothing; lambda = 0 is the plain step bit for bit while D trains; the reversed gradient reaches every model
tensor as the oracle says; folds equal their single calls; D learns; the drivers carry the setting and add exactly one launch."""
import ctypes as C
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import da_reference as R
from gpu_common import FIXED_TOL, grad_tol, rel_err, stage_tol
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd.adversary import SubjectAdversary
from multimodalsignal_amd.runtime import EmbeddedEngine, Engine, FoldArena
from oracle import cnn_gru_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LR, WD = 1e-3, 1e-3
ATT, CG = "cnn_gru_attention", "cnn_gru"
B1F, B2F = float(np.float32(0.9)), float(np.float32(0.999))           # the betas as the library's fp32 arguments carry them
ONE_MINUS_B1 = float(np.float32(1.0) - np.float32(0.9))
KEY_OF = {"W0": "classifier.0.weight", "b0": "classifier.0.bias", "W3": "classifier.3.weight", "b3": "classifier.3.bias"}


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _labels(B, S, seed):
    """Domain labels with a fifth of the rows unlabelled (at least one labelled)."""
    rs = np.random.RandomState(seed)
    d = rs.randint(0, S, size=B)
    d[rs.rand(B) < 0.2] = -1
    d[rs.randint(B)] = rs.randint(S)
    return d.astype(np.int32)


def _da(S, dom, params, m, v, stats, lam_rev, lr, step, idx=None, wd=WD):
    a = L.Da()
    a.S, a.weight_decay, a.beta1, a.beta2, a.eps = S, wd, 0.9, 0.999, 1e-8
    a.dom, a.idx = dom.data_ptr(), None if idx is None else idx.data_ptr()
    a.params, a.exp_avg, a.exp_avg_sq = params.data_ptr(), m.data_ptr(), v.data_ptr()
    a.stats = None if stats is None else stats.data_ptr()
    getattr(a, "lambda")[0], a.lr[0], a.step[0] = lam_rev, lr, step
    return a


def _step(S, dom, flat, feat, dfeat, lam, lam_rev, idx=None, lr=LR, step=1, m=None, v=None):
    """One msig_da_step from the given (or zero) moments on copies: returns (params, exp_avg, exp_avg_sq, stats, dfeat) on the host."""
    p = _dev(flat)
    m = torch.zeros_like(p) if m is None else _dev(m)
    v = torch.zeros_like(p) if v is None else _dev(v)
    stats = torch.zeros(3, dtype=torch.float64, device=DEV)
    df = _dev(dfeat)
    keep = (_dev(dom), None if idx is None else _dev(idx), _dev(feat))
    a = _da(S, keep[0], p, m, v, stats, lam_rev, lr, step, keep[1])
    L.check(L.lib().msig_da_step(C.byref(a), keep[2].data_ptr(), df.data_ptr(), feat.shape[0], lam, _stream()), "msig_da_step")
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (p, m, v, stats, df))


# ---- 1. the step alone against the float64 restatement -------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 3, 11, 16])
@pytest.mark.parametrize("B", [1, 2, 15, 16, 17, 64, 255, 256])
def test_step_matches_the_float64_restatement(B, S):
    """From zero moments: the four implied gradients exp_avg / (1 - beta1) (they carry the L2 term wd * p), the loss, the dfeat
    increment and the statistics, for lam in {1, 0.3}, with dom given per row and looked up through idx.  The increment is measured
    from a zero dfeat (0 + t = t exactly) and the same launch on a random dfeat must then give fadd(dfeat, t) bit for bit — the two
    roundings of the header, no FMA."""
    rs = np.random.RandomState(1000 * S + B)
    flat = SubjectAdversary.initial_parameters(S, seed=B).numpy()
    feat = rs.randn(B, 128).astype(np.float32)
    dfeat = rs.randn(B, 128).astype(np.float32)
    d = _labels(B, S, 7 * S + B)
    table = np.concatenate([d, rs.randint(-1, S, size=37).astype(np.int32)])          # looked up through idx: positions 0 .. B + 36
    perm = rs.permutation(B + 37).astype(np.int64)
    table_p = np.empty_like(table)
    table_p[perm] = table                                                              # table_p[perm[b]] = d[b] for b < B
    lam_rev = 0.7
    for lam in (1.0, 0.3):
        P = R.split(flat, S)
        Z = R.zeros_like(P)
        kw = dict(lam=lam, lam_rev=lam_rev, lr=LR, t=1, betas=(B1F, B2F), weight_decay=WD)
        r64 = R.step(P, Z, Z, feat, np.zeros_like(feat), d, **kw)
        r32 = R.step(P, Z, Z, feat, np.zeros_like(feat), d, dtype=np.float32, **kw)
        for form in ("direct", "idx"):
            dom, idx = (d, None) if form == "direct" else (table_p, perm[:B].copy())
            p, m, v, stats, inc = _step(S, dom, flat, feat, np.zeros_like(dfeat), lam, lam_rev, idx)
            tag = (lam, form)
            for k in R.KEYS:
                o = R.layout(S)[R.KEYS.index(k)]
                got = m[o:o + P[k].size].reshape(P[k].shape) / ONE_MINUS_B1
                want = r64["grads"][k] + WD * P[k]
                own = rel_err(r32["grads"][k].astype(np.float64) + np.float32(WD) * P[k].astype(np.float32), want)
                err, tol = rel_err(got, want), grad_tol(KEY_OF[k], own)
                print(f"{tag} grad {k}: err {err:.3e} tol {tol:.1e}")
                assert err <= tol, (tag, k, err, tol)
            err_l = abs(stats[0] / r64["n"] - r64["loss"]) / max(abs(r64["loss"]), 1e-6)
            print(f"{tag} loss err {err_l:.3e}")
            assert err_l <= FIXED_TOL["loss"], (tag, err_l)
            want_inc = -lam_rev * r64["g"]
            err_i, tol_i = rel_err(inc, want_inc), stage_tol("d_feat", rel_err(-np.float32(lam_rev) * r32["g"], want_inc))
            print(f"{tag} dfeat increment err {err_i:.3e} tol {tol_i:.1e}")
            assert err_i <= tol_i, (tag, err_i, tol_i)
            assert float((inc.astype(np.float64) * r64["g"]).sum()) < 0.0                           # reversed: against the discriminator's gradient
            # the counts, exact.  Precondition, from the float64 restatement alone: no row's two largest logits are closer than
            # 1e-5 (fp32 resolves the logits to about 1e-7), so the argmax is the same decision in either precision
            z = np.maximum(feat.astype(np.float64) @ P["W0"].T + P["b0"], 0) @ P["W3"].T + P["b3"]
            top = np.sort(z, axis=1)
            assert (top[:, -1] - top[:, -2]).min() >= 1e-5
            assert stats[2] == float((d >= 0).sum()) == r64["stats"][2]
            assert stats[1] == float(((z.argmax(axis=1) == d) & (d >= 0)).sum()) == r64["stats"][1]
            # the same launch on a random dfeat: parameters, moments and statistics the same bits, dfeat = fadd(dfeat, t)
            p2, m2, v2, stats2, df2 = _step(S, dom, flat, feat, dfeat, lam, lam_rev, idx)
            assert np.array_equal(p2.view(np.int32), p.view(np.int32)) and np.array_equal(m2.view(np.int32), m.view(np.int32))
            assert np.array_equal(v2.view(np.int32), v.view(np.int32)) and np.array_equal(stats2, stats)
            assert np.array_equal(df2.view(np.int32), (dfeat + inc).astype(np.float32).view(np.int32)), tag
            assert not np.array_equal(p, flat)                                                   # D moved


def test_second_step_moments_and_adam_arithmetic():
    """Two consecutive steps, the second from non-zero moments at its own step count.  Both moments against the float64 restatement —
    exp_avg is linear in the gradient and is gated like one (the classifier.0 floor, against the fp32 restatement's own error),
    exp_avg_sq is quadratic: twice that.  The parameters are NOT compared with the float64 run: m / sqrt(v) is ill-conditioned where
    a gradient element happens to be near zero.  They are compared with Adam's statement evaluated in fp32 on the kernel's OWN
    moments, which must agree to a few ulp of the parameter (sqrt and the division round within 1 ulp each; the step is <= lr)."""
    S, B, lr = 11, 37, 1e-2
    rs = np.random.RandomState(5)
    flat = SubjectAdversary.initial_parameters(S, seed=9).numpy()
    P = R.split(flat, S)
    M, V = R.zeros_like(P), R.zeros_like(P)
    P32, M32, V32 = P, M, V
    p, m, v = flat, None, None
    for t in (1, 2):
        feat, d = rs.randn(B, 128).astype(np.float32), _labels(B, S, t)
        kw = dict(lam=0.6, lr=lr, t=t, betas=(B1F, B2F), weight_decay=WD)
        r = R.step(P, M, V, feat, np.zeros_like(feat), d, **kw)
        r32 = R.step(P32, M32, V32, feat, np.zeros_like(feat), d, dtype=np.float32, **kw)
        P, M, V = r["params"], r["exp_avg"], r["exp_avg_sq"]
        P32, M32, V32 = r32["params"], r32["exp_avg"], r32["exp_avg_sq"]
        p_old = p
        p, m, v, _, _ = _step(S, d, p, feat, np.zeros_like(feat), 0.6, 0.0, lr=lr, step=t, m=m, v=v)
    own_m = rel_err(R.join(M32, S, np.float64), R.join(M, S, np.float64))
    own_v = rel_err(R.join(V32, S, np.float64), R.join(V, S, np.float64))
    err_m, err_v = rel_err(m, R.join(M, S, np.float64)), rel_err(v, R.join(V, S, np.float64))
    print(f"exp_avg err {err_m:.3e} own {own_m:.1e} | exp_avg_sq err {err_v:.3e} own {own_v:.1e}")
    assert err_m <= grad_tol("classifier.0.weight", own_m) and err_v <= 2 * grad_tol("classifier.0.weight", own_v)
    f32 = np.float32
    lr_over_bc1, inv_sqrt_bc2 = f32(lr / (1.0 - B1F ** 2)), f32(1.0 / np.sqrt(1.0 - B2F ** 2))
    want = p_old - lr_over_bc1 * (m / (np.sqrt(v) * inv_sqrt_bc2 + f32(1e-8)))
    assert np.abs(p.astype(np.float64) - want.astype(np.float64)).max() <= 4 * np.spacing(f32(np.abs(p).max()))


# ---- 2. no labelled row ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 17, 256])
def test_a_step_without_a_labelled_row_writes_nothing(B):
    S = 5
    rs = np.random.RandomState(B)
    flat = SubjectAdversary.initial_parameters(S, seed=1).numpy()
    feat, dfeat = rs.randn(B, 128).astype(np.float32), rs.randn(B, 128).astype(np.float32)
    m0, v0 = rs.rand(flat.size).astype(np.float32), rs.rand(flat.size).astype(np.float32)
    d = np.full(B, -1, dtype=np.int32)
    d[::3] = S + 4                                                                          # out of range reads as unlabelled
    p, m, v, stats, df = _step(S, d, flat, feat, dfeat, 0.3, 0.7, m=m0, v=v0)
    for got, want in ((p, flat), (m, m0), (v, v0), (df, dfeat)):
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert not stats.any()


# ---- 3. lambda = 0: the model's bits are the plain step's -----------------------------------------------------------------------
def _data(B, Cc, K, T, seed):
    rs = np.random.RandomState(seed)
    y = rs.randint(0, K, size=B).astype(np.int64)
    y[:min(K, B)] = np.arange(min(K, B))
    return torch.as_tensor(rs.randn(B, Cc, T).astype(np.float32)).to(DEV), torch.as_tensor(y).to(DEV)


def _params(Cc, K, hidden=64, layers=2, kind=ATT, seed=3):
    params = O.init_params(Cc, K, seed=seed, hidden=hidden, layers=layers)
    if kind == CG:
        params = {k: v for k, v in params.items() if k not in L.GATE_KEYS}
    return params


def _engine(Cc, K, hidden=64, layers=2, kind=ATT, seed=3, storage_engine=None):
    params = _params(Cc, K, hidden, layers, kind, seed)
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
    return e, params


def _adversary(S, lam, dom, seed=5, step=0):
    a = SubjectAdversary(S, lam=lam, schedule="constant", seed=seed)
    a.set_domains(dom)
    a.step = step
    return a.bind(DEV)


@pytest.mark.parametrize("Cc", [3, 6])
@pytest.mark.parametrize("model", [(64, 2), (32, 1)], ids=["depth2", "embedded"])
@pytest.mark.parametrize("kind", [ATT, CG])
def test_lambda_zero_is_the_plain_step_bit_for_bit(kind, model, Cc):
    """Three msig_da_train_steps at lambda = 0 against three msig_st_train_steps (eps = 0.1, lam = 0.4; for C = 3 also the hard-label
    step): parameters, moments, BatchNorm state and loss, while the discriminator's parameters move."""
    K, B, T, S = 2, 21, 512, 4
    hidden, layers = model
    dom = _labels(B, S, 3)
    for soft in ((0.1, 0.4),) + (((0.0, None),) if Cc == 3 else ()):
        engines, adv = [], _adversary(S, 0.0, dom)
        d0 = adv.params.clone()
        for with_adv in (False, True):
            e, _ = _engine(Cc, K, hidden, layers, kind)
            for s in (1, 2, 3):
                x, y = _data(B, Cc, K, T, 10 + s)
                e.train_step(x, y, LR, weight_decay=1e-4, step=s, dropout_p=0.5, seed=7, label_smoothing=soft[0], mix_lambda=soft[1],
                             adversary=adv if with_adv else None)
            engines.append(e)
        torch.cuda.synchronize()
        a, b = engines
        for name in ("params", "grads", "exp_avg", "exp_avg_sq", "bn_state"):
            assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), (soft, name)
        assert torch.equal(a.bn_count, b.bn_count) and torch.equal(a.loss_acc, b.loss_acc)
        assert torch.equal(_bits(a.region("LOSS", torch.float32, (3,))), _bits(b.region("LOSS", torch.float32, (3,))))
        assert adv.step == 3 and not torch.equal(adv.params, d0) and float(adv.stats[2]) == 3.0 * float((dom >= 0).sum())


# ---- 4. the reversed gradient in every model tensor -----------------------------------------------------------------------------
def _soft_loss(z, y, w, eps, lam, dt):
    wt = None if w is None else torch.tensor(w, dtype=dt)
    return lam * F.cross_entropy(z, y, weight=wt, label_smoothing=eps) + (1.0 - lam) * F.cross_entropy(z, y.flip(0), weight=wt, label_smoothing=eps)


def _oracle(params, x, y, d, dflat, S, lam_rev, lam, w, eps, max_norm):
    """{dtype: {key: gradient}} of L_cls + sum(c * feat), c = -lam_rev * g held constant (g from the restatement on the oracle's own
    feat), after torch's clip_grad_norm_ arithmetic when max_norm is given."""
    out = {}
    for dt, ndt in ((torch.float64, np.float64), (torch.float32, np.float32)):
        leaf = {k: v.to(dt).clone().requires_grad_(v.numel() > 0) for k, v in params.items()}
        bufs = {k: (v if "num_batches" in k else v.to(dt)) for k, v in O.init_buffers().items()}
        st, _ = O.forward(leaf, bufs, torch.as_tensor(x).to(dt), training=True, dropout_p=0.0, seed=0, step=1)
        feat = st["feat"]
        P = R.split(dflat, S)
        if feat.shape[1] == 64:              # the one-layer 32-unit model: its 2 x 32 features are columns 0..31 and 64..95 of the padded row
            P["W0"] = P["W0"][:, np.r_[0:32, 64:96]]
        Z = R.zeros_like(P)
        r = R.step(P, Z, Z, feat.detach().numpy(), np.zeros(tuple(feat.shape)), d, lam=lam, lam_rev=lam_rev, betas=(B1F, B2F), dtype=ndt)
        c = torch.as_tensor((ndt(-lam_rev) * r["g"]).astype(ndt))
        loss = _soft_loss(st["logits"], torch.as_tensor(y), w, eps, lam, dt) + (c * feat).sum()
        loss.backward()
        g = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).double().numpy() for k, v in leaf.items()}
        if max_norm is not None:
            norm = float(np.sqrt(sum(float((v ** 2).sum()) for v in g.values())))
            g = {k: v * min(1.0, max_norm / (norm + 1e-6)) for k, v in g.items()}
        out[dt] = g
    return out


@pytest.mark.parametrize("case", [dict(lam=1.0, w=None, eps=0.0, clip=None), dict(lam=0.4, w=(0.3, 2.5), eps=0.1, clip=0.05)], ids=["plain", "composed"])
def test_reversed_gradient_reaches_every_model_tensor(case):
    """One msig_da_train_step at lambda = 0.7, dropout 0: every model tensor's gradient against the oracle's gradient of
    L_cls + sum(c * feat), c = -lambda * g constant.  Precondition, from the reference alone: without the reversed term
    classifier.0's input side — the GRU's gradient — differs by far more than the tolerance.  Once more with class weights, clip,
    label smoothing and mixup's lam."""
    Cc, K, B, T, S, lam_rev = 3, 2, 21, 512, 4, 0.7
    x, y = _data(B, Cc, K, T, 2)
    d = _labels(B, S, 11)
    e, params = _engine(Cc, K)
    adv = _adversary(S, lam_rev, d)
    dflat = adv.params.cpu().numpy().copy()
    w = None if case["w"] is None else torch.tensor(case["w"], dtype=torch.float32, device=DEV)
    e.train_step(x, y, LR, weight_decay=0.0, step=1, dropout_p=0.0, seed=1, class_weight=w, max_grad_norm=case["clip"],
                 label_smoothing=case["eps"], mix_lambda=case["lam"], adversary=adv)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in e.named_param_views(e.grads).items()}
    xn, yn = x.cpu().numpy(), y.cpu().numpy()
    ref = _oracle(params, xn, yn, d, dflat, S, lam_rev, case["lam"], case["w"], case["eps"], case["clip"])
    without = _oracle(params, xn, yn, d, dflat, S, 0.0, case["lam"], case["w"], case["eps"], case["clip"])[torch.float64]
    r64, r32 = ref[torch.float64], ref[torch.float32]
    k0 = "gru.weight_ih_l1"
    assert rel_err(without[k0], r64[k0]) > 100 * grad_tol(k0, rel_err(r32[k0], r64[k0]))
    if case["clip"] is not None:
        assert e.grad_stats()["clipped"] == 1
    for k, g in r64.items():
        err, tol = rel_err(got[k], g), grad_tol(k, rel_err(r32[k], g))
        print(f"{k:40s} err {err:.3e} tol {tol:.1e}")
        assert err <= tol, (k, err, tol)


def test_reversed_gradient_of_the_embedded_model_matches_the_one_layer_oracle():
    """The one-layer 32-unit model (EmbeddedEngine: padded 64-unit layout) at lambda = 0.7 against the oracle's (32, 1) model, tensor
    by tensor, with D restricted to the real feature columns.  The padded entries of the flat gradient are exactly zero — a non-zero
    reversed term on a padded feature column would train the padded units — and so are D's weights on those columns after the step."""
    Cc, K, B, T, S, lam_rev = 3, 2, 21, 512, 4, 0.7
    x, y = _data(B, Cc, K, T, 2)
    d = _labels(B, S, 11)
    e, params = _engine(Cc, K, 32, 1)
    adv = _adversary(S, lam_rev, d)
    adv.restrict_features(32)
    dflat = adv.params.cpu().numpy().copy()
    assert np.abs(R.split(dflat, S)["W0"][:, np.r_[0:32, 64:96]]).min() > 0
    e.train_step(x, y, LR, weight_decay=0.0, step=1, dropout_p=0.0, seed=1, adversary=adv)
    torch.cuda.synchronize()
    assert int(e.grads[e.padding].count_nonzero()) == 0 and int(e.params[e.padding].count_nonzero()) == 0
    w0 = adv.views()["0.weight"]
    assert int(w0[:, 32:64].count_nonzero()) == 0 and int(w0[:, 96:].count_nonzero()) == 0
    got = {k: v.cpu().numpy().copy() for k, v in e.gather_grads().items()}
    xn, yn = x.cpu().numpy(), y.cpu().numpy()
    ref = _oracle(params, xn, yn, d, dflat, S, lam_rev, 1.0, None, 0.0, None)
    without = _oracle(params, xn, yn, d, dflat, S, 0.0, 1.0, None, 0.0, None)[torch.float64]
    r64, r32 = ref[torch.float64], ref[torch.float32]
    k0 = "gru.weight_ih_l0"
    assert rel_err(without[k0], r64[k0]) > 100 * grad_tol(k0, rel_err(r32[k0], r64[k0]))
    assert set(got) == set(r64)
    for k, g in r64.items():
        err, tol = rel_err(got[k], g), grad_tol(k, rel_err(r32[k], g))
        print(f"{k:40s} err {err:.3e} tol {tol:.1e}")
        assert err <= tol, (k, err, tol)


# ---- 5. fold batches ------------------------------------------------------------------------------------------------------------
def test_step_multi_equals_the_single_calls():
    """msig_da_step_multi over three folds in slots (2, 0, 3) with different lambda, lam, lr and step counts, idx rows of a shared
    matrix: every fold's buffers equal its msig_da_step bit for bit, and the slot outside the launch is untouched."""
    n, B, S, slots = 3, 37, 6, (2, 0, 3)
    rs = np.random.RandomState(3)
    nf = L.da_param_floats(S)
    npos = 90
    off, at = {}, 0
    for name, nb in (("params", nf * 4), ("exp_avg", nf * 4), ("exp_avg_sq", nf * 4), ("stats", 24), ("dom", npos * 4)):
        off[name] = at
        at += (nb + 255) // 256 * 256
    dmem = torch.zeros((4, at), dtype=torch.uint8, device=DEV)
    fstride = (B * 512 + 255) // 256 * 256
    fmem = torch.zeros((4, 2 * fstride), dtype=torch.uint8, device=DEV)                      # per slot: feat, then dfeat
    idx = _dev(rs.randint(0, npos, size=(n, B + 5)).astype(np.int64))
    lam_rev, lams, lrs, steps = (0.0, 0.5, 1.0), (1.0, 0.3, 0.8), (1e-3, 2e-3, 5e-4), (1, 4, 9)
    host = []
    for i, s in enumerate(slots):
        flat = SubjectAdversary.initial_parameters(S, seed=20 + i).numpy()
        rec = dict(flat=flat, m=(rs.rand(nf) * 1e-3).astype(np.float32), v=(rs.rand(nf) * 1e-6).astype(np.float32),
                   dom=rs.randint(-1, S, size=npos).astype(np.int32), feat=rs.randn(B, 128).astype(np.float32), dfeat=rs.randn(B, 128).astype(np.float32))
        host.append(rec)
        for name, key, dt in (("params", "flat", torch.float32), ("exp_avg", "m", torch.float32), ("exp_avg_sq", "v", torch.float32), ("dom", "dom", torch.int32)):
            dmem[s, off[name]:off[name] + rec[key].nbytes].view(dt).copy_(_dev(rec[key]))
        fmem[s, :B * 512].view(torch.float32).copy_(_dev(rec["feat"]).reshape(-1))
        fmem[s, fstride:fstride + B * 512].view(torch.float32).copy_(_dev(rec["dfeat"]).reshape(-1))
    a = L.Da()
    a.S, a.weight_decay, a.beta1, a.beta2, a.eps = S, WD, 0.9, 0.999, 1e-8
    base = dmem.data_ptr()
    a.dom, a.params, a.exp_avg, a.exp_avg_sq, a.stats = (base + off[k] for k in ("dom", "params", "exp_avg", "exp_avg_sq", "stats"))
    a.idx, a.idx_row_stride, a.stride_bytes = idx.data_ptr(), B + 5, at
    m = L.Multi()
    m.n, m.stride_bytes = n, 2 * fstride
    for i, s in enumerate(slots):
        m.slot[i] = s
        getattr(a, "lambda")[i], a.lr[i], a.step[i] = lam_rev[i], lrs[i], steps[i]
    L.check(L.lib().msig_da_step_multi(C.byref(a), C.byref(m), fmem.data_ptr(), fmem.data_ptr() + fstride, B,
                                       (C.c_float * L.MAX_FOLDS)(*lams), _stream()), "msig_da_step_multi")
    torch.cuda.synchronize()
    assert int(dmem[1].count_nonzero()) == 0 and int(fmem[1].count_nonzero()) == 0
    for i, s in enumerate(slots):
        rec = host[i]
        p, mm, v, stats, df = _step(S, rec["dom"], rec["flat"], rec["feat"], rec["dfeat"], lams[i], lam_rev[i], idx[i, :B].cpu().numpy().copy(),
                                    lr=lrs[i], step=steps[i], m=rec["m"], v=rec["v"])
        for name, want in (("params", p), ("exp_avg", mm), ("exp_avg_sq", v)):
            assert np.array_equal(dmem[s, off[name]:off[name] + nf * 4].view(torch.int32).cpu().numpy(), want.view(np.int32)), (i, name)
        assert np.array_equal(dmem[s, off["stats"]:off["stats"] + 24].view(torch.float64).cpu().numpy(), stats), i
        assert np.array_equal(fmem[s, fstride:fstride + B * 512].view(torch.int32).cpu().numpy(), df.view(np.int32).reshape(-1)), i
        if lam_rev[i] == 0.0:
            assert np.array_equal(df.view(np.int32), rec["dfeat"].view(np.int32))


def test_train_step_multi_equals_the_single_calls_and_fold_zero_the_plain_step():
    """NF = 3 with lambda = (0, 0.5, 1), different seeds, model and discriminator step counts, mixup weights and learning rates:
    msig_da_train_step_multi leaves every fold's model and discriminator with the bits of its msig_da_train_step, and fold 0
    (lambda = 0) with the bits of the step without an adversary."""
    n, B, T, Cc, K, S, npos = 3, 21, 512, 3, 2, 4, 60
    lam_rev, lams, msteps, dsteps, lrs = (0.0, 0.5, 1.0), (1.0, 0.4, 0.7), (1, 3, 5), (2, 4, 6), (1e-3, 5e-4, 2e-3)
    rs = np.random.RandomState(8)
    data = [_data(B, Cc, K, T, 300 + f) for f in range(n)]
    doms = [rs.randint(-1, S, size=npos).astype(np.int32) for _ in range(n)]
    idx = _dev(rs.randint(0, npos, size=(n, B + 3)).astype(np.int64))
    arena = FoldArena(Cc, K, DEV, n, B, T, adversary=(S, npos))
    engs = [_engine(Cc, K, seed=10 + f, storage_engine=arena.engine(f))[0] for f in range(n)]
    advs = []
    for f in range(n):
        adv = SubjectAdversary(S, lam=lam_rev[f], schedule="constant", seed=40 + f)
        adv.set_domains(doms[f])
        advs.append(adv.bind(DEV, arena.side_storage("adversary", f)))
        x, y = data[f]
        arena.view(f, "x", torch.float32)[:x.numel()].copy_(x.reshape(-1))
        arena.view(f, "y", torch.int64)[:B].copy_(y)
    slots = list(range(n))
    m = arena.multi(slots, key_gru=[L.dropout_key(100 + f, msteps[f], 1) for f in slots], key_head=[L.dropout_key(100 + f, msteps[f], 2) for f in slots],
                    lr=lrs, steps=msteps)
    desc = arena.batch(B, True, 0.5)
    sd = arena.soft(slots, 0.1, lams)
    a = arena.da(slots, S, lam_rev, lrs, dsteps, (0.9, 0.999), 1e-8, 1e-4)
    a.idx, a.idx_row_stride = idx.data_ptr(), B + 3
    L.check(L.lib().msig_da_train_step_multi(C.byref(desc), C.byref(m), C.byref(sd), C.byref(a), arena.ptr("exp_avg"), arena.ptr("exp_avg_sq"),
                                             0.9, 0.999, 1e-8, 1e-4, msteps[0], _stream()), "msig_da_train_step_multi")
    torch.cuda.synchronize()
    for f in range(n):
        e, _ = _engine(Cc, K, seed=10 + f)
        adv = _adversary(S, lam_rev[f], doms[f], seed=40 + f, step=dsteps[f] - 1)
        x, y = data[f]
        e.train_step(x, y, lrs[f], weight_decay=1e-4, step=msteps[f], dropout_p=0.5, seed=100 + f, label_smoothing=0.1, mix_lambda=lams[f],
                     adversary=adv, batch_index=idx[f, :B].contiguous())
        torch.cuda.synchronize()
        for name in ("params", "grads", "exp_avg", "exp_avg_sq", "bn_state"):
            assert torch.equal(_bits(getattr(e, name)), _bits(getattr(engs[f], name))), (f, name)
        for name in ("params", "exp_avg", "exp_avg_sq"):
            assert torch.equal(_bits(getattr(adv, name)), _bits(getattr(advs[f], name))), (f, name)
        assert torch.equal(adv.stats, advs[f].stats) and float(adv.stats[2]) > 0
    e, _ = _engine(Cc, K, seed=10)
    x, y = data[0]
    e.train_step(x, y, lrs[0], weight_decay=1e-4, step=msteps[0], dropout_p=0.5, seed=100, label_smoothing=0.1, mix_lambda=lams[0])
    torch.cuda.synchronize()
    for name in ("params", "grads", "exp_avg", "exp_avg_sq", "bn_state"):
        assert torch.equal(_bits(getattr(e, name)), _bits(getattr(engs[0], name))), name


def test_embedded_fold_batch_keeps_its_padding_zero_and_equals_the_single_calls():
    """Two folds of the one-layer model in a fold arena (the padded layout is written once and trained in place), three
    msig_da_train_step_multi steps at lambda = (0.7, 0.3): the padded entries of parameters, gradients and both moments stay exactly
    zero, D's padded input columns too, and each fold's padded buffers equal its stand-alone EmbeddedEngine run bit for bit."""
    n, B, T, Cc, K, S, npos, steps = 2, 21, 512, 3, 2, 4, 50, 3
    lam_rev = (0.7, 0.3)
    rs = np.random.RandomState(4)
    data = [[_data(B, Cc, K, T, 500 + 10 * f + s) for s in range(steps)] for f in range(n)]
    doms = [rs.randint(-1, S, size=npos).astype(np.int32) for _ in range(n)]
    idx = _dev(rs.randint(0, npos, size=(n, B)).astype(np.int64))
    arena = FoldArena(Cc, K, DEV, n, B, T, gru_hidden=32, gru_layers=1, adversary=(S, npos))
    engs = [_engine(Cc, K, 32, 1, seed=10 + f, storage_engine=arena.engine(f))[0] for f in range(n)]
    advs = []
    for f in range(n):
        adv = SubjectAdversary(S, lam=lam_rev[f], schedule="constant", seed=40 + f)
        adv.set_domains(doms[f])
        adv.restrict_features(32)
        advs.append(adv.bind(DEV, arena.side_storage("adversary", f)))
    slots = list(range(n))
    sd = arena.soft(slots, 0.0)
    desc = arena.batch(B, True, 0.5)
    for s in range(1, steps + 1):
        for f in range(n):
            x, y = data[f][s - 1]
            arena.view(f, "x", torch.float32)[:x.numel()].copy_(x.reshape(-1))
            arena.view(f, "y", torch.int64)[:B].copy_(y)
        m = arena.multi(slots, key_gru=[L.dropout_key(100 + f, s, 1) for f in slots], key_head=[L.dropout_key(100 + f, s, 2) for f in slots],
                        lr=[LR] * n, steps=[s] * n)
        a = arena.da(slots, S, lam_rev, [LR] * n, [s] * n, (0.9, 0.999), 1e-8, 1e-4)
        a.idx, a.idx_row_stride = idx.data_ptr(), B
        L.check(L.lib().msig_da_train_step_multi(C.byref(desc), C.byref(m), C.byref(sd), C.byref(a), arena.ptr("exp_avg"), arena.ptr("exp_avg_sq"),
                                                 0.9, 0.999, 1e-8, 1e-4, s, _stream()), "msig_da_train_step_multi")
    torch.cuda.synchronize()
    for f in range(n):
        pad = engs[f].padding
        for name in ("params", "grads", "exp_avg", "exp_avg_sq"):
            assert int(getattr(engs[f], name)[pad].count_nonzero()) == 0, (f, name)
        w0 = advs[f].views()["0.weight"]
        assert int(w0[:, 32:64].count_nonzero()) == 0 and int(w0[:, 96:].count_nonzero()) == 0 and int(w0[:, :32].count_nonzero()) == 64 * 32
        e, _ = _engine(Cc, K, 32, 1, seed=10 + f)
        adv = _adversary(S, lam_rev[f], doms[f], seed=40 + f)
        for s in range(1, steps + 1):
            x, y = data[f][s - 1]
            e.train_step(x, y, LR, weight_decay=1e-4, step=s, dropout_p=0.5, seed=100 + f, adversary=adv, batch_index=idx[f].contiguous())
        torch.cuda.synchronize()
        for name in ("params", "grads", "exp_avg", "exp_avg_sq", "bn_state"):
            assert torch.equal(_bits(getattr(e, name)), _bits(getattr(engs[f], name))), (f, name)
        for name in ("params", "exp_avg", "exp_avg_sq"):
            assert torch.equal(_bits(getattr(adv, name)), _bits(getattr(advs[f], name))), (f, name)


# ---- 6. the discriminator learns ------------------------------------------------------------------------------------------------
def test_discriminator_learns_separated_domains():
    S, B = 4, 64
    rs = np.random.RandomState(0)
    d = (np.arange(B) % S).astype(np.int32)
    centres = rs.randn(S, 128).astype(np.float32) * 2.0
    feat = _dev(centres[d] + 0.1 * rs.randn(B, 128).astype(np.float32))
    dfeat = torch.zeros((B, 128), device=DEV)
    adv = _adversary(S, 0.0, d)
    losses = []
    for t in range(1, 201):
        adv.stats.zero_()
        a = adv.descriptor([0.0], [1e-2], [t])
        L.check(L.lib().msig_da_step(C.byref(a), feat.data_ptr(), dfeat.data_ptr(), B, 1.0, _stream()), "msig_da_step")
        if t in (1, 200):
            losses.append(adv.stats.cpu().numpy().copy())
    first, last = losses
    assert last[1] / last[2] == 1.0 and last[0] / last[2] < first[0] / first[2]
    assert not dfeat.any()


# ---- 7. drivers -----------------------------------------------------------------------------------------------------------------
SUBS = ["S2", "S3", "S4", "S5"]
FLAGS = ["--subject-adversarial", "0.1", "--mixup", "0.2"]


def _common(tmp_path):
    return ["--synthetic", str(tmp_path / "w"), "--synthetic-windows", "12", "--samples", "512", "--subjects", *SUBS, "--epochs", "2",
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


def test_fold_batches_equal_sequential_folds_and_the_report_is_well_formed(tmp_path):
    from multimodalsignal_amd import main as M
    runs = {}
    for tag, extra in (("lock", FLAGS), ("seq", FLAGS + ["--concurrent-folds", "1"]), ("plain", ["--mixup", "0.2"])):
        M.main(_common(tmp_path) + extra + ["--out", str(tmp_path / tag)])
        run = next((tmp_path / tag).glob("*/run_*"))
        txt = (run / "cv_summary.txt").read_text(encoding="utf-8")
        assert ("SUBJECT ADVERSARY: lambda=0.1 schedule=ganin" in txt) == (tag != "plain")
        assert (run / "adversary.json").exists() == (tag != "plain")
        runs[tag] = (_fold_outputs(run), run)
    for (ia, wa), (ib, wb) in zip(runs["lock"][0], runs["seq"][0]):
        assert ia == ib
        assert list(wa) == list(wb) and all(torch.equal(wa[k], wb[k]) for k in wa)
    assert all("domain_acc" in h and "domain_loss" in h and "adversary_lambda" in h for f, _ in runs["lock"][0] for h in f["history"])
    assert all("domain_acc" not in h for f, _ in runs["plain"][0] for h in f["history"])
    assert all(a[0]["history"][-1]["train_loss"] != p[0]["history"][-1]["train_loss"] for a, p in zip(runs["lock"][0], runs["plain"][0]))
    assert all(not any(k.startswith("adversary") or "discriminator" in k for k in w) for _, w in runs["lock"][0])      # best_model.pt is the model's alone
    doc = json.loads((runs["lock"][1] / "adversary.json").read_text())
    assert doc == json.loads((runs["seq"][1] / "adversary.json").read_text())
    assert [f["subject"] for f in doc["folds"]] == SUBS and doc["probe"] is False and doc["synthetic"] is True
    for f in doc["folds"]:
        assert f["S"] == 2 and f["chance"] == 0.5 and 0.0 <= f["last_domain_acc"] <= 1.0 and f["first_domain_loss"] > 0
        assert 0.0 < f["final_lambda"] < 0.1 and 0.0 <= f["test_accuracy"] <= 1.0
    assert set(doc["pooled"]) >= {"chance", "first_domain_acc", "last_domain_acc", "test_accuracy"}
    assert "no subject shift" in (runs["lock"][1] / "adversary.txt").read_text(encoding="utf-8")


@pytest.mark.parametrize("mode", [["--ablation"], ["--hierarchical"], ["--model", "cnn_gru_attention", "cnn_gru"], ["--no-lockstep"],
                                  ["--hierarchical", "--concurrent-folds", "1"]],
                         ids=["ablation", "hierarchical", "model", "no-lockstep", "hierarchical-sequential"])
def test_every_driver_mode_runs_with_the_adversary(tmp_path, mode):
    from multimodalsignal_amd import main as M
    M.main(_common(tmp_path) + ["--subject-adversarial", "--max-grad-norm", "1.0", "--label-smoothing", "0.1", "--augment", "scale=0.1"] + mode
           + ["--out", str(tmp_path / "o")])
    summaries = [p for p in (tmp_path / "o").rglob("*summary.txt")]
    assert summaries and all("SUBJECT ADVERSARY: lambda=0.1" in p.read_text(encoding="utf-8") for p in summaries), summaries
    tables = [p for p in (tmp_path / "o").rglob("adversary*.json") if p.name != "adversary_result.json"]
    assert tables and all(json.loads(p.read_text())["folds"] for p in tables), tables


def test_hierarchical_fold_batches_equal_sequential_models(tmp_path):
    """--hierarchical with the adversary: M1 (depth 2) and M2 (the embedded one-layer model) trained as fold batches give the
    checkpoints, histories and decisions of --concurrent-folds 1."""
    from multimodalsignal_amd import main as M
    runs = {}
    for tag, extra in (("lock", []), ("seq", ["--concurrent-folds", "1"])):
        M.main(_common(tmp_path) + ["--subject-adversarial", "0.5", "--adversary-schedule", "constant", "--hierarchical"] + extra
               + ["--out", str(tmp_path / tag)])
        run = next((tmp_path / tag).glob("*/run_*"))
        out = {}
        for sub in SUBS:
            fd = run / f"fold_test_on_{sub}"
            if not (fd / "fold_result.json").exists():          # a fold whose M2 has no training or validation data never decides
                continue
            out[sub] = (json.loads((fd / "fold_result.json").read_text()),
                        {t: torch.load(fd / f"model_{t}" / "best_model.pt", weights_only=True) for t in ("m1", "m2")},
                        {t: json.loads((fd / f"model_{t}" / "adversary_result.json").read_text()) for t in ("m1", "m2")})
        runs[tag] = out
    assert runs["lock"] and list(runs["lock"]) == list(runs["seq"])
    for sub in runs["lock"]:
        (ra, wa, da), (rb, wb, db) = runs["lock"][sub], runs["seq"][sub]
        assert ra == rb and da == db, sub
        for t in ("m1", "m2"):
            assert list(wa[t]) == list(wb[t]) and all(torch.equal(wa[t][k], wb[t][k]) for k in wa[t]), (sub, t)


def test_the_adversary_is_exactly_one_more_launch_per_training_step():
    Cc, K, B, T, S = 3, 2, 21, 512, 4
    x, y = _data(B, Cc, K, T, 4)
    reports = []
    for lam_rev in (None, 0.0, 0.5):
        e, _ = _engine(Cc, K)
        adv = None if lam_rev is None else _adversary(S, lam_rev, _labels(B, S, 1))
        e.train_step(x, y, LR, step=1, dropout_p=0.5, seed=7, adversary=adv)              # workspaces exist before the count starts
        torch.cuda.synchronize()
        L.profile_enable(True)
        try:
            e.train_step(x, y, LR, step=2, dropout_p=0.5, seed=7, adversary=adv)
            torch.cuda.synchronize()
            reports.append({k: v[0] for k, v in L.profile_report().items()})
        finally:
            L.profile_enable(False)
    plain, probe, full = reports
    assert "da_step" not in plain and sum(plain.values()) > 5
    assert probe == full == {**plain, "da_step": 1}


def test_batches_above_256_are_refused_by_the_engine_before_any_launch():
    Cc, K, T, S = 3, 2, 64, 4
    x, y = _data(257, Cc, K, T, 1)
    e, _ = _engine(Cc, K)
    before = e.params.clone()
    with pytest.raises(ValueError, match="at most 256"):
        e.train_step(x, y, LR, step=1, adversary=_adversary(S, 0.1, _labels(257, S, 1)))
    assert torch.equal(e.params, before) and e.exp_avg is None
