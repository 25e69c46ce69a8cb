"""GPU tier: distillation (include/msig_kd.h) through every layer — the teacher table against the fp64 restatement
(tests/kd_reference.py) and msig_en_reduce's bits at T = 1; the term alone against the restatement with and without idx, the blended
target, a teacher row with a zero and poison around what it writes; the train step against the CPU oracle differentiated through
the whole loss; kd = NULL and alpha = 0 are msig_da_train_step bit for bit and launch for launch; folds equal their single calls;
a student learns its teacher."""
import ctypes as C
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kd_reference as R
from conftest import load_golden_model
from gpu_common import FIXED_TOL, grad_tol, narrow_train_step, rel_err, split_named, to_t
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd.adversary import SubjectAdversary
from multimodalsignal_amd.distill import Distillation, teacher_table
from multimodalsignal_amd.runtime import EmbeddedEngine, Engine, FoldArena
from oracle import cnn_gru_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ATT, CG = "cnn_gru_attention", "cnn_gru"
POISON = float("nan")


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


# ---- 1. the teacher table -------------------------------------------------------------------------------------------------------
def _teacher(lg, T, pad=0):
    """msig_kd_teacher on an (M, N, K) stack whose member blocks are N * K + pad floats apart (the padding and both sides of q are
    poison): (N, K) fp32 on the host."""
    M, N, K = lg.shape
    stack = torch.full((M, N * K + pad), POISON, dtype=torch.float32, device=DEV)
    stack[:, :N * K] = _dev(lg).reshape(M, N * K)
    out = torch.full((N * K + 16,), POISON, dtype=torch.float32, device=DEV)
    L.check(L.lib().msig_kd_teacher(stack.data_ptr(), N * K + pad, M, N, K, T, out[8:].data_ptr(), _stream()), "msig_kd_teacher")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[:8]).all()) and bool(torch.isnan(out[8 + N * K:]).all())
    return out[8:8 + N * K].reshape(N, K).cpu().numpy()


def _mean_p(lg):
    M, N, K = lg.shape
    stack, out = _dev(lg), torch.empty((N, K), dtype=torch.float32, device=DEV)
    L.check(L.lib().msig_en_reduce(stack.data_ptr(), N * K, M, N, K, out.data_ptr(), *([None] * 8), _stream()), "msig_en_reduce")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("K", [2, 3, 16])
@pytest.mark.parametrize("M", [1, 2, 7, 256])
def test_teacher_matches_the_restatement_and_is_the_ensemble_mean_at_T_1(M, K):
    """Crafted windows (a saturated member at +-80, an exact tie, equal members) at T in {0.5, 1, 4}: within 2 ulp of fp32 + 1e-12 of
    the fp64 restatement (DESIGN.md section 23's bound for msig_en_reduce); at T = 1 msig_en_reduce's mean_p bit for bit; a padded
    member stride gives the contiguous stack's bits."""
    lg = R.crafted_logits(M, 5, K, seed=100 * M + K)
    worst = 0.0
    for T in (0.5, 1.0, 4.0):
        got, want = _teacher(lg, T), R.teacher(lg, T)
        ratio = float((np.abs(got.astype(np.float64) - want) / (2.0 * R.ulp32(want) + 1e-12)).max())
        worst = max(worst, ratio)
        print(f"M={M} K={K} T={T}: worst error / bound {ratio:.3f}")
        assert R.within_store_rounding(got, want), (T, ratio)
        assert np.allclose(got.sum(axis=1), 1.0, atol=1e-6)
        assert _same_bits(_teacher(lg, T, pad=7), got)
        if T == 1.0:
            assert _same_bits(got, _mean_p(lg))
    assert np.array_equal(_teacher(lg, 4.0)[2], _teacher(np.repeat(lg[:1], M, axis=0), 4.0)[2])      # equal members: one member's row


@pytest.mark.parametrize("M", [1, 3, 16])
def test_teacher_multi_reads_the_members_where_they_lie(M):
    """Members in arenas (slot order not increasing), poison between the blocks and around q: the bits of msig_kd_teacher on the
    gathered stack, and msig_en_reduce_multi's mean_p at T = 1."""
    N, K = 5, 3
    lg = R.crafted_logits(M, N, K, seed=7 + M)
    slots = list(np.random.RandomState(M).permutation(M + 2)[:M])
    stride = 256
    mem = torch.full((M + 2, stride // 4), POISON, dtype=torch.float32, device=DEV)
    for i, s in enumerate(slots):
        mem[int(s), :N * K] = _dev(lg[i]).reshape(-1)
    m = L.Multi()
    m.n, m.stride_bytes = M, stride
    for i, s in enumerate(slots):
        m.slot[i] = int(s)
    for T in (1.0, 2.0):
        out = torch.full((N * K + 16,), POISON, dtype=torch.float32, device=DEV)
        L.check(L.lib().msig_kd_teacher_multi(mem.data_ptr(), C.byref(m), N, K, T, out[8:].data_ptr(), _stream()), "msig_kd_teacher_multi")
        torch.cuda.synchronize()
        assert bool(torch.isnan(out[:8]).all()) and bool(torch.isnan(out[8 + N * K:]).all())
        got = out[8:8 + N * K].reshape(N, K).cpu().numpy()
        assert _same_bits(got, _teacher(lg, T)) and R.within_store_rounding(got, R.teacher(lg, T))
        if T == 1.0:
            mp = torch.empty((N, K), dtype=torch.float32, device=DEV)
            L.check(L.lib().msig_en_reduce_multi(mem.data_ptr(), C.byref(m), N, K, mp.data_ptr(), *([None] * 8), _stream()), "msig_en_reduce_multi")
            torch.cuda.synchronize()
            assert _same_bits(got, mp.cpu().numpy())


def test_teacher_table_helper_is_the_library_call():
    lg = R.crafted_logits(3, 5, 4, seed=3)
    assert _same_bits(teacher_table(_dev(lg), 2.0).cpu().numpy(), _teacher(lg, 2.0))


# ---- 2. the term alone ----------------------------------------------------------------------------------------------------------
def _case(B, K, seed):
    """Logits, a CrossEntropy-sized dlogits, a teacher table of B + 9 positions (one of the batch's rows holds an exact zero) and a
    permutation with gaps that maps the batch's rows into it."""
    rs = np.random.RandomState(seed)
    z = (2.0 * rs.randn(B, K)).astype(np.float32)
    dl = (rs.randn(B, K) / B).astype(np.float32)
    P = B + 9
    e = np.exp(1.5 * rs.randn(P, K))
    table = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    idx = rs.permutation(P)[:B].astype(np.int64)
    for pos in (idx[B // 2], B // 2):                        # the row with the zero, reached with idx and without
        table[pos, 0] = 0.0
        table[pos, 1:] = (table[pos, 1:] / table[pos, 1:].sum()).astype(np.float32)
    return z, dl, table, idx


def _apply(z, dl, table, idx, alpha, T, lam):
    """msig_kd_apply on copies with poison around dlogits and stats: (dlogits, stats) on the host."""
    B, K = z.shape
    buf = torch.full((B * K + 16,), POISON, dtype=torch.float32, device=DEV)
    buf[8:8 + B * K] = _dev(dl).reshape(-1)
    sbuf = torch.full((3 + 4,), POISON, dtype=torch.float64, device=DEV)
    sbuf[2:5] = 0.0
    keep = (_dev(z), _dev(table), None if idx is None else _dev(idx))
    k = L.Kd()
    k.alpha, k.temperature, k.q, k.idx, k.stats = alpha, T, keep[1].data_ptr(), None if idx is None else keep[2].data_ptr(), sbuf[2:].data_ptr()
    L.check(L.lib().msig_kd_apply(C.byref(k), keep[0].data_ptr(), buf[8:].data_ptr(), B, K, lam, _stream()), "msig_kd_apply")
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:8]).all()) and bool(torch.isnan(buf[8 + B * K:]).all())
    assert bool(torch.isnan(sbuf[:2]).all()) and bool(torch.isnan(sbuf[5:]).all())
    assert torch.equal(_bits(keep[0]), _bits(_dev(z))) and torch.equal(_bits(keep[1]), _bits(_dev(table)))      # inputs untouched
    return buf[8:8 + B * K].reshape(B, K).cpu().numpy(), sbuf[2:5].cpu().numpy()


@pytest.mark.parametrize("K", [2, 3, 16])
@pytest.mark.parametrize("B", [1, 2, 15, 16, 17, 64, 255])
def test_apply_matches_the_restatement(B, K):
    """lam in {1, 0.3}, alpha in {0.3, 1}, T in {0.5, 2}, with idx and without.  dlogits: max |got - fp64| <= max(8 x the fp32
    restatement's own max error against the fp64 one, one fp32 ulp of 1 / B) per case.  The counts are exact (precondition, from
    the restatement alone: no row's two largest logits or teacher entries are closer than 1e-5) and L_kd is within
    FIXED_TOL["loss"] relative to max(1, L_kd)."""
    z, dl, table, idx = _case(B, K, 1000 * K + B)
    floor = float(np.spacing(np.float32(1.0 / B)))
    worst = 0.0
    for lam in (1.0, 0.3):
        for use_idx in (True, False):
            qm = R.blend(R.lookup(table, B, idx if use_idx else None), lam)
            assert min(R.argmax_margins(z, qm)) >= 1e-5
            if lam == 1.0 or B % 2 == 1:                      # the row with the zero (blended away unless it is its own partner)
                assert (qm[B // 2] == 0).any()
            for alpha in (0.3, 1.0):
                for T in (0.5, 2.0):
                    r64, r32 = R.apply(z, dl, qm, alpha, T), R.apply(z, dl, qm, alpha, T, dtype=np.float32)
                    got, stats = _apply(z, dl, table, idx if use_idx else None, alpha, T, lam)
                    err = float(np.abs(got.astype(np.float64) - r64["dlogits"]).max())
                    own = float(np.abs(r32["dlogits"].astype(np.float64) - r64["dlogits"]).max())
                    tol = max(8.0 * own, floor)
                    worst = max(worst, err / tol)
                    print(f"B={B} K={K} lam={lam} idx={use_idx} alpha={alpha} T={T}: err {err:.3e} own {own:.3e} tol {tol:.3e}")
                    assert err <= tol, (lam, use_idx, alpha, T, err, tol)
                    assert stats[2] == float(B) and stats[1] == r64["stats"][1]
                    err_l = abs(stats[0] / B - r64["L_kd"]) / max(1.0, r64["L_kd"])
                    assert err_l <= FIXED_TOL["loss"], (lam, use_idx, alpha, T, err_l)
                    assert r64["L_kd"] > 0.0
                    if alpha == 1.0:                          # nothing of the hard gradient is left: dlogits of zeros gives the same bits
                        assert _same_bits(_apply(z, np.zeros_like(dl), table, idx if use_idx else None, alpha, T, lam)[0], got)
    print(f"B={B} K={K}: worst err / tol {worst:.3f}")


def test_apply_accumulates_its_stats_and_leaves_dlogits_alone_without_them():
    B, K = 17, 3
    z, dl, table, idx = _case(B, K, 5)
    keep = (_dev(z), _dev(table), _dev(idx))
    stats = torch.tensor([1.5, 2.0, 3.0], dtype=torch.float64, device=DEV)
    outs = []
    for sp in (stats.data_ptr(), None):
        d = _dev(dl)
        k = L.Kd()
        k.alpha, k.temperature, k.q, k.idx, k.stats = 0.5, 2.0, keep[1].data_ptr(), keep[2].data_ptr(), sp
        L.check(L.lib().msig_kd_apply(C.byref(k), keep[0].data_ptr(), d.data_ptr(), B, K, 0.3, _stream()), "msig_kd_apply")
        torch.cuda.synchronize()
        outs.append(d.cpu().numpy())
    assert _same_bits(outs[0], outs[1])
    want = R.apply(z, dl, R.blend(R.lookup(table, B, idx), 0.3), 0.5, 2.0)["stats"]
    got = stats.cpu().numpy()
    assert got[1] == 2.0 + want[1] and got[2] == 3.0 + B and abs(got[0] - 1.5 - want[0]) <= FIXED_TOL["loss"] * max(B, want[0])


def test_apply_multi_equals_the_single_calls():
    """Three folds in slots (2, 0, 3) with their own lam, teacher tables and a shared idx matrix: every fold's dlogits and stats equal
    its msig_kd_apply bit for bit, and the slot outside the launch is untouched."""
    n, B, K, slots, lams = 3, 37, 3, (2, 0, 3), (1.0, 0.3, 0.8)
    P = B + 9
    rs = np.random.RandomState(2)
    zstride = (B * K * 4 + 255) // 256 * 256
    lmem = torch.zeros((4, 2 * zstride), dtype=torch.uint8, device=DEV)                       # per slot: logits, then dlogits
    koff_q = 256
    kstride = 256 + (P * K * 4 + 255) // 256 * 256                                            # per slot: stats, then q
    kmem = torch.zeros((4, kstride), dtype=torch.uint8, device=DEV)
    idx = _dev(rs.randint(0, P, size=(n, B + 5)).astype(np.int64))
    host = []
    for i, s in enumerate(slots):
        z, dl, table, _ = _case(B, K, 50 + i)
        host.append((z, dl, table))
        lmem[s, :B * K * 4].view(torch.float32).copy_(_dev(z).reshape(-1))
        lmem[s, zstride:zstride + B * K * 4].view(torch.float32).copy_(_dev(dl).reshape(-1))
        kmem[s, koff_q:koff_q + P * K * 4].view(torch.float32).copy_(_dev(table).reshape(-1))
    k = L.Kd()
    k.alpha, k.temperature = 0.5, 2.0
    k.q, k.stats, k.stride_bytes = kmem.data_ptr() + koff_q, kmem.data_ptr(), kstride
    k.idx, k.idx_row_stride = idx.data_ptr(), B + 5
    m = L.Multi()
    m.n, m.stride_bytes = n, 2 * zstride
    for i, s in enumerate(slots):
        m.slot[i] = s
    L.check(L.lib().msig_kd_apply_multi(C.byref(k), C.byref(m), lmem.data_ptr(), lmem.data_ptr() + zstride, B, K,
                                        (C.c_float * L.MAX_FOLDS)(*lams), _stream()), "msig_kd_apply_multi")
    torch.cuda.synchronize()
    assert int(lmem[1].count_nonzero()) == 0 and int(kmem[1].count_nonzero()) == 0
    for i, s in enumerate(slots):
        z, dl, table = host[i]
        want, stats = _apply(z, dl, table, idx[i, :B].cpu().numpy().copy(), 0.5, 2.0, lams[i])
        assert _same_bits(lmem[s, zstride:zstride + B * K * 4].view(torch.float32).cpu().numpy().reshape(B, K), want), i
        assert np.array_equal(kmem[s, :24].view(torch.float64).cpu().numpy(), stats), i
        assert _same_bits(lmem[s, :B * K * 4].view(torch.float32).cpu().numpy().reshape(B, K), z)


# ---- 3. the train step against the oracle ---------------------------------------------------------------------------------------
B1F, B2F = float(np.float32(0.9)), float(np.float32(0.999))
LR, WD, ADAM_EPS = 1e-3, 1e-4, 1e-3
GOLDEN = ("model_c6_k2_t512", "model_c2_k3_t256")
CASES = [dict(lam=1.0, w=None, eps=0.0, clip=None), dict(lam=0.4, w=(0.3, 2.5), eps=0.1, clip=0.05)]


def _soft_loss(z, y, w, eps, lam, dt):
    wt = None if w is None else torch.tensor(w, dtype=dt)
    return lam * F.cross_entropy(z, y, weight=wt, label_smoothing=eps) + (1.0 - lam) * F.cross_entropy(z, y.flip(0), weight=wt, label_smoothing=eps)


def _oracle(params, buffers, x, y, qm, alpha, T, case, w):
    """{dtype: ({key: gradient after the clip}, {key: parameter after Adam's first step})} of
    L = (1 - alpha) L_hard + alpha T^2 KL(qm || softmax(z / T)), batchmean, differentiated by autograd through the whole model."""
    out = {}
    a, Tt = float(np.float32(alpha)), float(np.float32(T))
    for dt in (torch.float64, torch.float32):
        leaf = {k: v.to(dt).clone().requires_grad_(v.numel() > 0) for k, v in params.items()}
        bufs = {k: (v.clone() if "num_batches" in k else v.to(dt)) for k, v in buffers.items()}
        st, _ = O.forward(leaf, bufs, torch.as_tensor(x).to(dt), training=True, dropout_p=0.0, seed=0, step=1)
        z = st["logits"]
        kd = Tt * Tt * F.kl_div(F.log_softmax(z / Tt, dim=1), torch.as_tensor(qm).to(dt), reduction="batchmean")
        loss = (1.0 - a) * _soft_loss(z, torch.as_tensor(y), w, case["eps"], case["lam"], dt) + a * kd
        loss.backward()
        g = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).double().numpy() for k, v in leaf.items()}
        if case["clip"] is not None:
            norm = float(np.sqrt(sum(float((v ** 2).sum()) for v in g.values())))
            g = {k: v * min(1.0, case["clip"] / (norm + 1e-6)) for k, v in g.items()}
        after = {}
        for k, v in g.items():
            p = params[k].double().numpy()
            gd = v + WD * p                                   # Adam's first step from zero moments: m_hat = g', sqrt(v_hat) = |g'|
            after[k] = p - LR * gd / (np.abs(gd) + ADAM_EPS)
        out[dt] = (g, after)
    return out


@pytest.mark.parametrize("case", CASES, ids=["plain", "composed"])
@pytest.mark.parametrize("model", [(ATT, 2), (CG, 2), (ATT, 1)], ids=["attention", "cnn_gru", "embedded"])
@pytest.mark.parametrize("name", GOLDEN)
def test_train_step_matches_the_oracle_differentiated_through_the_whole_loss(name, model, case, monkeypatch):
    """One msig_kd_train_step at alpha = 0.5, T = 2, B = 8, dropout 0, on the committed parameters (the one-layer model has no
    committed parameters: the oracle's initialisation of the same C and K): every parameter gradient and every parameter after
    Adam against the oracle, gated by gpu_common.grad_tol on the fp32 oracle's own error.  Adam's eps is 1e-3 here: the update
    lr g / (|g| + eps) is then Lipschitz in g with constant lr / eps = 1, so an error of the gradient within its tolerance cannot
    exceed it in the parameter (with 1e-8 an element whose gradient is near zero would flip by 2 lr on a rounding).  With K = 3
    the composed case's class weights are (0.3, 2.5, 1.0).  For cnn_gru the oracle's ChannelAttention is replaced by the identity
    (s = 1), as tests/test_cnngru_gpu.py does, without editing oracle/."""
    kind, layers = model
    meta, params_np, _ = load_golden_model(name)
    Cc, K, T, B = meta["C"], meta["K"], meta["T"], 8
    params, buffers = split_named(to_t(params_np))
    if layers == 1:
        params = O.init_params(Cc, K, seed=3, hidden=32, layers=1)
    oparams = params                                          # what the oracle's forward reads: zero-size gate tensors for cnn_gru
    if kind == CG:
        params = {k: v for k, v in params.items() if k not in L.GATE_KEYS}
        oparams = dict(params, **{"channel_attention.fc.0.weight": torch.zeros(0, Cc), "channel_attention.fc.2.weight": torch.zeros(Cc, 0)})
        monkeypatch.setattr(O, "channel_gate", lambda x, W1, W2: (x.mean(dim=2), torch.zeros(x.shape[0], 0, dtype=x.dtype),
                                                                  torch.ones(x.shape[0], x.shape[1], dtype=x.dtype)))
    for k, v in O.init_buffers().items():
        buffers.setdefault(k, v)
    rs = np.random.RandomState(17)
    x = rs.randn(B, Cc, T).astype(np.float32)
    y = rs.randint(0, K, size=B).astype(np.int64)
    y[:K] = np.arange(K)
    z, _, table, idx = _case(B, K, 9)
    alpha, Tk = 0.5, 2.0
    w = None if case["w"] is None else (case["w"] + (1.0,) * (K - 2))
    if layers == 1:
        e = EmbeddedEngine(Cc, K, DEV, 32, kind=kind)
        for k, v in e.small_views().items():
            v.copy_(params[k])
    else:
        e = Engine(Cc, K, DEV, kind=kind)
        e.load_named({**params, **buffers})
    d = Distillation(alpha, Tk)
    d.set_teacher(table)
    d.bind(DEV)
    e.train_step(_dev(x), _dev(y), LR, eps=ADAM_EPS, weight_decay=WD, step=1, dropout_p=0.0, seed=1,
                 class_weight=None if w is None else torch.tensor(w, dtype=torch.float32, device=DEV), max_grad_norm=case["clip"],
                 label_smoothing=case["eps"], mix_lambda=case["lam"], distill=d, batch_index=_dev(idx))
    torch.cuda.synchronize()
    if layers == 1:
        assert int(e.grads[e.padding].count_nonzero()) == 0 and int(e.params[e.padding].count_nonzero()) == 0
        got_g = {k: v.cpu().numpy().copy() for k, v in e.gather_grads().items()}
        got_p = {k: v.cpu().numpy().copy() for k, v in e.small_views().items()}
    else:
        got_g = {k: v.cpu().numpy() for k, v in e.named_param_views(e.grads).items()}
        got_p = {k: v.cpu().numpy() for k, v in e.named_param_views().items()}
    qm = R.blend(R.lookup(table, B, idx), case["lam"])
    ref = _oracle(oparams, buffers, x, y, qm, alpha, Tk, case, w)
    (g64, p64), (g32, p32) = ref[torch.float64], ref[torch.float32]
    # precondition, from the reference alone: without the term the classifier's last layer differs by far more than the tolerance
    without = _oracle(oparams, buffers, x, y, qm, 0.0, Tk, case, w)[torch.float64][0]
    k0 = "classifier.3.weight"
    assert rel_err(without[k0], g64[k0]) > 100 * grad_tol(k0, rel_err(g32[k0], g64[k0]))
    if case["clip"] is not None:
        assert e.grad_stats()["clipped"] == 1
    assert float(d.stats[2]) == B and float(d.stats[0]) > 0
    worst = 0.0
    for k, g in g64.items():
        if g.size == 0:
            continue
        err, tol = rel_err(got_g[k], g), grad_tol(k, rel_err(g32[k], g))
        errp, tolp = rel_err(got_p[k], p64[k]), grad_tol(k, rel_err(p32[k], p64[k]))
        worst = max(worst, err / tol, errp / tolp)
        print(f"{k:40s} grad err {err:.3e} tol {tol:.1e} | param err {errp:.3e} tol {tolp:.1e}")
        assert err <= tol, (k, err, tol)
        assert errp <= tolp, (k, errp, tolp)
    print(f"worst err / tol {worst:.3f}")


# ---- 4. bit identity and launch counts ------------------------------------------------------------------------------------------
def _data(B, Cc, K, T, seed):
    rs = np.random.RandomState(seed)
    y = rs.randint(0, K, size=B).astype(np.int64)
    y[:min(K, B)] = np.arange(min(K, B))
    return torch.as_tensor(rs.randn(B, Cc, T).astype(np.float32)).to(DEV), torch.as_tensor(y).to(DEV)


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


def _distill(alpha, table, T=2.0):
    d = Distillation(alpha, T)
    d.set_teacher(table)
    return d.bind(DEV)


@pytest.mark.parametrize("model", [(ATT, 64, 2), (CG, 64, 2), (ATT, 32, 1)], ids=["attention", "cnn_gru", "embedded"])
def test_null_and_alpha_zero_are_the_plain_step_bit_for_bit(model):
    """Three steps with eps = 0.1, lam = 0.4, clip and dropout: msig_da_train_step itself, msig_kd_train_step with a NULL msig_kd
    and Engine.train_step at alpha = 0 leave the same parameters, gradients, moments, BatchNorm state and loss; alpha = 0.5 does not."""
    kind, hidden, layers = model
    Cc, K, B, T = 3, 2, 21, 512
    _, _, table, idx = _case(B, K, 4)
    idx_d = _dev(idx)
    engines = []
    for mode in ("plain", "null", "zero", "on"):
        e = _engine(Cc, K, hidden, layers, kind)
        d = {"plain": None, "null": None, "zero": _distill(0.0, table), "on": _distill(0.5, table)}[mode]
        for s in (1, 2, 3):
            x, y = _data(B, Cc, K, T, 10 + s)
            kw = dict(weight_decay=1e-4, step=s, dropout_p=0.5, seed=7, label_smoothing=0.1, mix_lambda=0.4, max_grad_norm=1.0)
            if mode == "null":                               # the entry point itself with a NULL msig_kd
                if layers == 1:
                    e.scatter()
                e.ensure_adam_state()
                b = e._batch(x, y, True, 0.5, 7, s)
                cw, mn, sm, lam = e._checked(None, 1.0, 0.1, 0.4)
                L.check(L.lib().msig_kd_train_step(C.byref(b), C.byref(e._st(cw, mn, sm, lam)), None, None, e.exp_avg.data_ptr(),
                                                   e.exp_avg_sq.data_ptr(), LR, 0.9, 0.999, 1e-8, 1e-4, s, _stream()), "msig_kd_train_step")
                if layers == 1:
                    e.gather()
            elif mode == "plain":                            # msig_da_train_step, called directly (Engine.train_step is msig_sc_train_step)
                assert narrow_train_step(e, x, y, LR, **kw) == "msig_da_train_step"
            else:
                e.train_step(x, y, LR, distill=d, batch_index=idx_d, **kw)
        torch.cuda.synchronize()
        engines.append((e, d))
    plain = engines[0][0]
    for (e, d), mode in zip(engines[1:], ("null", "zero", "on")):
        same = all(torch.equal(_bits(getattr(plain, n)), _bits(getattr(e, n))) for n in ("params", "grads", "exp_avg", "exp_avg_sq", "bn_state"))
        same_loss = torch.equal(plain.loss_acc, e.loss_acc) and torch.equal(_bits(plain.region("LOSS", torch.float32, (3,))), _bits(e.region("LOSS", torch.float32, (3,))))
        if mode == "on":
            assert not same and float(d.stats[2]) == 3.0 * B and float(d.stats[0]) > 0
        else:
            assert same and same_loss, mode
            if d is not None:
                assert not d.stats.any()                      # alpha = 0: no launch, nothing reported
    assert not torch.equal(plain.loss_acc, engines[3][0].loss_acc)


@pytest.mark.parametrize("B", [21, 2100])
def test_launch_counts(B):
    """By the library's own launch report: NULL and alpha = 0 are the plain step's launches; alpha > 0 is the plain step's minus
    head_step (where the fused head applies: B <= 2048) plus head_fwd, ce, head_bwd and kd_apply once each."""
    Cc, K, T = 3, 2, 64
    x, y = _data(B, Cc, K, T, 4)
    _, _, table, idx = _case(B, K, 4)
    idx_d = _dev(idx)
    reports = []
    for alpha in (None, 0.0, 0.5):
        e = _engine(Cc, K)
        d = None if alpha is None else _distill(alpha, table)
        e.train_step(x, y, LR, step=1, dropout_p=0.5, seed=7, distill=d, batch_index=idx_d)          # workspaces exist before the count starts
        torch.cuda.synchronize()
        L.profile_enable(True)
        try:
            e.train_step(x, y, LR, step=2, dropout_p=0.5, seed=7, distill=d, batch_index=idx_d)
            torch.cuda.synchronize()
            reports.append({k: v[0] for k, v in L.profile_report().items()})
        finally:
            L.profile_enable(False)
    plain, zero, on = reports
    assert plain == zero and "kd_apply" not in plain and sum(plain.values()) > 5
    want = dict(plain)
    if B <= 2048:
        assert want.pop("head_step") == 1 and "head_fwd" not in plain
        want.update(head_fwd=1, ce=1, head_bwd=1)
    else:
        assert "head_step" not in plain and plain["head_fwd"] == plain["ce"] == plain["head_bwd"] == 1
    want["kd_apply"] = 1
    assert on == want


# ---- 5. fold batches ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_adversary", [False, True], ids=["plain", "adversary"])
def test_train_step_multi_equals_the_single_calls(with_adversary):
    """NF = 3 with per-fold lam, seeds, step counts and learning rates, each fold its own teacher table in the arena's block, idx
    rows of a shared matrix: msig_kd_train_step_multi leaves every fold's parameters, gradients, moments, BatchNorm state and
    distillation statistics (and, with the adversary on, the discriminator's) with the bits of its msig_kd_train_step."""
    n, B, T, Cc, K, S, npos = 3, 21, 512, 3, 2, 4, 60
    lams, msteps, dsteps, lrs, lam_rev = (1.0, 0.4, 0.7), (1, 3, 5), (2, 4, 6), (1e-3, 5e-4, 2e-3), (0.3, 0.5, 1.0)
    alpha, Tk = 0.5, 2.0
    rs = np.random.RandomState(8)
    data = [_data(B, Cc, K, T, 300 + f) for f in range(n)]
    tables = []
    for f in range(n):
        e_ = np.exp(1.5 * rs.randn(npos, K))
        tables.append((e_ / e_.sum(axis=1, keepdims=True)).astype(np.float32))
    doms = [rs.randint(-1, S, size=npos).astype(np.int32) for _ in range(n)]
    idx = _dev(rs.randint(0, npos, size=(n, B + 3)).astype(np.int64))
    arena = FoldArena(Cc, K, DEV, n, B, T, adversary=(S, npos) if with_adversary else None, distill=npos, grad_clip=True)
    engs = [_engine(Cc, K, seed=10 + f, storage_engine=arena.engine(f)) for f in range(n)]
    kds, advs = [], []
    for f in range(n):
        d = Distillation(alpha, Tk)
        d.set_teacher(tables[f])
        kds.append(d.bind(DEV, arena.side_storage("distill", f)))
        if with_adversary:
            adv = SubjectAdversary(S, lam=lam_rev[f], schedule="constant", seed=40 + f)
            adv.set_domains(doms[f])
            advs.append(adv.bind(DEV, arena.side_storage("adversary", f)))
        x, y = data[f]
        arena.view(f, "x", torch.float32)[:x.numel()].copy_(x.reshape(-1))
        arena.view(f, "y", torch.int64)[:B].copy_(y)
        arena.set_max_norm(f, 1.0)
    slots = list(range(n))
    m = arena.multi(slots, key_gru=[L.dropout_key(100 + f, msteps[f], 1) for f in slots], key_head=[L.dropout_key(100 + f, msteps[f], 2) for f in slots],
                    lr=lrs, steps=msteps)
    desc = arena.batch(B, True, 0.5)
    sd = arena.soft(slots, 0.1, lams, clip=arena.clip(slots))
    k = arena.kd(alpha, Tk)
    k.idx, k.idx_row_stride = idx.data_ptr(), B + 3
    a = None
    if with_adversary:
        a = arena.da(slots, S, lam_rev, lrs, dsteps, (0.9, 0.999), 1e-8, 1e-4)
        a.idx, a.idx_row_stride = idx.data_ptr(), B + 3
    L.check(L.lib().msig_kd_train_step_multi(C.byref(desc), C.byref(m), C.byref(sd), None if a is None else C.byref(a), C.byref(k),
                                             arena.ptr("exp_avg"), arena.ptr("exp_avg_sq"), 0.9, 0.999, 1e-8, 1e-4, msteps[0], _stream()),
            "msig_kd_train_step_multi")
    torch.cuda.synchronize()
    for f in range(n):
        e = _engine(Cc, K, seed=10 + f)
        d = _distill(alpha, tables[f], Tk)
        adv = None
        if with_adversary:
            adv = SubjectAdversary(S, lam=lam_rev[f], schedule="constant", seed=40 + f)
            adv.set_domains(doms[f])
            adv.step = dsteps[f] - 1
            adv.bind(DEV)
        x, y = data[f]
        e.train_step(x, y, lrs[f], weight_decay=1e-4, step=msteps[f], dropout_p=0.5, seed=100 + f, label_smoothing=0.1, mix_lambda=lams[f],
                     max_grad_norm=1.0, adversary=adv, distill=d, batch_index=idx[f, :B].contiguous())
        torch.cuda.synchronize()
        for name in ("params", "grads", "exp_avg", "exp_avg_sq", "bn_state"):
            assert torch.equal(_bits(getattr(e, name)), _bits(getattr(engs[f], name))), (f, name)
        assert torch.equal(d.stats, kds[f].stats) and float(d.stats[2]) == B and float(d.stats[0]) > 0, f
        if with_adversary:
            for name in ("params", "exp_avg", "exp_avg_sq"):
                assert torch.equal(_bits(getattr(adv, name)), _bits(getattr(advs[f], name))), (f, name)
            assert torch.equal(adv.stats, advs[f].stats)
    assert torch.equal(arena.side_stats("distill").cpu(), torch.stack([d.stats.cpu() for d in kds]))


# ---- 6. a student learns its teacher --------------------------------------------------------------------------------------------
def test_student_learns_the_teacher_not_the_labels():
    """C = 3, K = 2, T = 512, B = 16, alpha = 1: the labels are a fixed random permutation of a balanced vector, and at alpha = 1 the
    hard loss has weight 0, so only the teacher can explain what the student learns.  The teacher table is built by msig_kd_teacher
    from a fixed second model's eval logits on the same rows, centred per class over the batch and scaled by 20 so that the
    teacher's decisions are spread over both classes (an untrained model gives nearly the same logits for every row).  40 steps on
    the same batch: the mean L_kd of the last 5 steps is below that of the first 5, and the mean agreement with the teacher has risen."""
    Cc, K, T, B, Tk = 3, 2, 512, 16, 2.0
    x, _ = _data(B, Cc, K, T, 21)
    y = _dev(np.random.RandomState(5).permutation(np.arange(B) % K).astype(np.int64))
    teacher = _engine(Cc, K, seed=11)
    teacher.forward(x, None, training=False)
    lg = teacher.region("LOGITS", torch.float32, (B, K)).clone()
    lg = ((lg - lg.mean(dim=0, keepdim=True)) * 20.0).contiguous()
    table = teacher_table(lg[None], Tk)
    assert 0 < int((table.argmax(dim=1) == 0).sum()) < B
    student = _engine(Cc, K, seed=3)
    d = Distillation(1.0, Tk)
    d.set_teacher(table)
    d.bind(DEV)
    losses, agree = [], []
    for s in range(1, 41):
        d.stats.zero_()
        student.train_step(x, y, 3e-3, step=s, dropout_p=0.0, seed=1, distill=d)
        st = d.stats.cpu().numpy()
        losses.append(st[0] / st[2])
        agree.append(st[1] / st[2])
    print("L_kd first 5", losses[:5], "last 5", losses[-5:], "agreement first 5", agree[:5], "last 5", agree[-5:])
    assert np.mean(losses[-5:]) < np.mean(losses[:5])
    assert np.mean(agree[-5:]) > np.mean(agree[:5])


# ---- 7. students through the trainers -------------------------------------------------------------------------------------------
def test_student_fold_batches_equal_sequential_students_and_alpha_zero_is_the_plain_fold(tmp_path):
    """Four folds of a synthetic set, two epochs at B = 16 with a ragged last batch; every fold's teacher table is
    Ensemble.teacher of two untrained models over the whole store (the table is read by store position).  Students trained as one
    fold batch (LockstepTrainer, msig_kd_train_step_multi) give the sequential students' (Trainer.train, msig_kd_train_step)
    metrics, histories — kd_loss and kd_agreement included — and checkpoints bit for bit; alpha = 0 gives the plain fold's
    checkpoint, alpha = 0.5 does not; the plain fold's history has no kd entries."""
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.dataset import SubjectStore
    from multimodalsignal_amd.ensemble import Ensemble
    from multimodalsignal_amd.multifold import LockstepTrainer, lockstep_compatible
    from multimodalsignal_amd.synth import make_synthetic_wesad, CHANNELS6
    subs = ["S2", "S3", "S4", "S5"]
    d = make_synthetic_wesad(tmp_path / "w", subjects=subs, windows_per_subject=23, T=256, difficulty=2.0)
    names = (d / "_channel_names.txt").read_text().split()
    base = M.default_cfg()
    base.update(data_path=d, channels=list(CHANNELS6), subjects=subs, epochs=2, patience=20, batch_size=16)
    store = SubjectStore(d, subs, base["channels"], names, classification_mode=base["mode"], device=DEV)
    tables = []
    for k, sid in enumerate(subs):
        members = [M.prepare_fold(k, sid, tmp_path / f"t{r}", DEV, names, dict(base, replica=r), store) for r in (0, 1)]
        x_all = members[0]["loaders"][0].store
        models = [p["model"].to(DEV).eval() for p in members]
        en = Ensemble(models, eval_batch=40)
        table = en.teacher(x_all, 2.0)
        assert _same_bits(Ensemble(models, batched=False).teacher(x_all, 2.0).cpu().numpy(), table.cpu().numpy())
        assert _same_bits(en.teacher(x_all, 1.0).cpu().numpy(), en.predict(x_all).mean_p.cpu().numpy())
        tables.append(table.cpu())
    out = {}
    for mode, alpha in (("seq", 0.5), ("lock", 0.5), ("seq", 0.0), ("seq", None)):
        preps = [M.prepare_fold(k, sid, tmp_path / f"{mode}{alpha}", DEV, names, base, store) for k, sid in enumerate(subs)]
        if alpha is not None:
            for p, table in zip(preps, tables):
                p["distill"] = Distillation(alpha, 2.0)
                p["distill"].set_teacher(table)
        if mode == "seq":
            infos = [M.train_fold(p, DEV) for p in preps]
        else:
            assert lockstep_compatible(preps)
            infos = LockstepTrainer(preps, DEV).run()
        for i in infos:
            for h in i["history"]:
                h.pop("seconds", None)
        out[mode, alpha] = ([(i["subject"], i["accuracy"], i["f1_score"], i["epochs"], i["history"], i.get("distillation")) for i in infos],
                            [torch.load(tmp_path / f"{mode}{alpha}" / f"fold_test_on_{s}" / "best_model.pt", weights_only=True) for s in subs])
    same = lambda a, b: all(torch.equal(wa[k], wb[k]) for wa, wb in zip(a, b) for k in wa)
    assert out["seq", 0.5][0] == out["lock", 0.5][0] and same(out["seq", 0.5][1], out["lock", 0.5][1])
    assert same(out["seq", 0.0][1], out["seq", None][1]) and not same(out["seq", 0.5][1], out["seq", None][1])
    for rec in out["seq", 0.5][0]:
        assert rec[5] == dict(alpha=0.5, temperature=2.0)
        assert all(h["kd_loss"] > 0 and 0.0 <= h["kd_agreement"] <= 1.0 for h in rec[4])
    assert all("kd_loss" not in h for rec in out["seq", None][0] for h in rec[4]) and all(rec[5] is None for rec in out["seq", None][0])
    assert [[h["val_loss"] for h in r[4]] for r in out["seq", 0.0][0]] == [[h["val_loss"] for h in r[4]] for r in out["seq", None][0]]


# ---- 8. the driver --------------------------------------------------------------------------------------------------------------
SUBS = ["S2", "S3", "S4", "S5", "S6"]


def _common(tmp_path):
    return ["--synthetic", str(tmp_path / "w"), "--synthetic-windows", "24", "--samples", "512", "--subjects", *SUBS, "--epochs", "2",
            "--batch-size", "16", "--seeds", "2"]


def _run(tmp_path, tag, extra):
    from multimodalsignal_amd import main as M
    M.main(_common(tmp_path) + extra + ["--out", str(tmp_path / tag)])
    return next((tmp_path / tag).glob("*/run_*"))


def _weights(run, sub=""):
    return [torch.load(run / sub / f"fold_test_on_{s}" / "best_model.pt", weights_only=True) for s in SUBS]


def _same_weights(a, b):
    return all(list(wa) == list(wb) and all(torch.equal(wa[k], wb[k]) for k in wa) for wa, wb in zip(a, b))


def _without_seconds(v):
    if isinstance(v, dict):
        return {k: _without_seconds(x) for k, x in v.items() if "seconds" not in k and k != "train_windows_per_s"}
    return [_without_seconds(x) for x in v] if isinstance(v, list) else v


def test_driver_fold_batches_equal_sequential_and_alpha_zero_is_replica_zero(tmp_path):
    """--seeds 2 --distill 0.5:2 as fold batches and with --concurrent-folds 1: every student's best_model.pt and distillation.json
    agree.  --distill 0: every student's tensors and metric row are replica 0's bit for bit; with alpha > 0 they differ.  Replica 0
    and seeds.json are what they are without the flag."""
    runs = {tag: _run(tmp_path, tag, extra) for tag, extra in (("lock", ["--distill", "0.5:2"]), ("seq", ["--distill", "0.5:2", "--concurrent-folds", "1"]),
                                                               ("zero", ["--distill", "0"]), ("plain", []))}
    docs = {tag: json.loads((run / "distillation.json").read_text()) for tag, run in runs.items() if tag != "plain"}
    assert not (runs["plain"] / "distillation.json").exists() and not (runs["plain"] / "distilled").exists()
    assert _same_weights(_weights(runs["lock"], "distilled"), _weights(runs["seq"], "distilled")) and docs["lock"] == docs["seq"]
    for tag in ("lock", "seq", "zero"):
        assert _same_weights(_weights(runs[tag]), _weights(runs["plain"])), tag
        assert _same_weights(_weights(runs[tag], "seed_1"), _weights(runs["plain"], "seed_1")), tag
        assert _without_seconds(json.loads((runs[tag] / "seeds.json").read_text())) == _without_seconds(json.loads((runs["plain"] / "seeds.json").read_text())), tag
    assert _same_weights(_weights(runs["zero"], "distilled"), _weights(runs["zero"]))
    assert not _same_weights(_weights(runs["lock"], "distilled"), _weights(runs["lock"]))
    for f in docs["zero"]["folds"]:
        assert f["student"] == f["replica0"] and f["kd_loss"] is None
    doc = docs["lock"]
    assert (doc["alpha"], doc["temperature"], doc["members"], doc["synthetic"]) == (0.5, 2.0, 2, True)
    assert [f["subject"] for f in doc["folds"]] == SUBS
    for f in doc["folds"]:
        assert f["ensemble"]["fidelity"] == 1.0 and f["kd_loss"] > 0 and 0.0 <= f["kd_agreement"] <= 1.0
        assert all(0.0 <= f[sys_][m] <= 1.0 for sys_ in ("ensemble", "mean_member", "replica0", "student") for m in ("accuracy", "f1", "fidelity"))
        assert (runs["lock"] / f"fold_test_on_{f['subject']}" / "distilled_result.json").exists()
        assert (runs["lock"] / "distilled" / f"fold_test_on_{f['subject']}" / "fold_result.json").exists()
    assert set(doc["pooled"]) >= {"ensemble", "mean_member", "replica0", "student", "kd_loss"} and set(doc["paired"]) == {"accuracy", "f1", "nll", "brier", "ece"}
    txt = (runs["lock"] / "distillation.txt").read_text(encoding="utf-8")
    assert txt.startswith("DISTILLATION: alpha=0.5 T=2 members=2") and "shows the machinery, not what WESAD would give" in txt
    hist = json.loads((runs["lock"] / "distilled" / "fold_test_on_S2" / "fold_result.json").read_text())["history"]
    assert all("kd_loss" in h and "kd_agreement" in h for h in hist)
    assert "kd loss" in (runs["lock"] / "distilled" / "fold_test_on_S2" / "training_log.txt").read_text(encoding="utf-8")


@pytest.mark.parametrize("mode", [["--model", "cnn_gru_attention", "cnn_gru"], ["--ablation"], ["--no-lockstep"]], ids=["model", "ablation", "no-lockstep"])
def test_every_driver_mode_runs_with_distillation(tmp_path, mode):
    run = _run(tmp_path, "o", ["--distill"] + mode)
    tables = list((tmp_path / "o").rglob("distillation.json"))
    assert tables and run.exists()
    for t in tables:
        doc = json.loads(t.read_text())
        assert (doc["alpha"], doc["temperature"], doc["members"]) == (0.5, 2.0, 2) and [f["subject"] for f in doc["folds"]] == SUBS
        assert all((t.parent / "distilled" / f"fold_test_on_{s}" / "best_model.pt").exists() for s in SUBS)
    if mode[0] == "--model":
        assert len(tables) == 2
