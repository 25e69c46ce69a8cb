"""GPU tier: group-DRO (include/msig_dro.h) through every layer — the term alone against the fp64 restatement
(tests/dro_reference.py) with poison around every buffer; the structural cases (no present group, one group with q = [1], frozen,
accumulating stats); q following a planted hard group; folds equal their single calls; the train step against the CPU oracle
differentiated through the whole robust loss; NULL and single-group steps are the plain steps bit for bit; launch counts; the
drivers."""
import ctypes as C
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dro_reference as R
from conftest import load_golden_model
from gpu_common import FIXED_TOL, grad_tol, narrow_train_step, rel_err, split_named, to_t
from mc_reference import ulp32, within_store_rounding
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd.adversary import SubjectAdversary
from multimodalsignal_amd.dro import GroupDro
from multimodalsignal_amd.runtime import EmbeddedEngine, Engine, FoldArena
from multimodalsignal_amd.sam import Sam
from oracle import cnn_gru_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ATT, CG = "cnn_gru_attention", "cnn_gru"
GUARD = 64                     # poisoned elements on both sides of every buffer
INT_POISON = -123456789
NS = R.STATS


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class Guarded:
    """A device buffer holding `host` between two poisoned guard zones (NaN for floats, a sentinel for integers)."""

    def __init__(self, host):
        host = np.ascontiguousarray(host)
        self.host, self.n = host, host.size
        poison = float("nan") if host.dtype.kind == "f" else INT_POISON
        self.t = torch.full((self.n + 2 * GUARD,), poison, dtype=torch.from_numpy(host).dtype, device=DEV)
        self.t[GUARD:GUARD + self.n] = _dev(host).reshape(-1)

    def ptr(self):
        return self.t[GUARD:].data_ptr()

    def get(self):
        return self.t[GUARD:GUARD + self.n].cpu().numpy().reshape(self.host.shape)

    def guards_intact(self):
        g = torch.cat([self.t[:GUARD], self.t[GUARD + self.n:]])
        return bool(torch.isnan(g).all()) if self.t.dtype.is_floating_point else bool((g == INT_POISON).all())

    def untouched(self):
        return self.guards_intact() and _same_bits(self.get(), self.host)


# ---- 1. the term alone ----------------------------------------------------------------------------------------------------------
def _case(B, K, G, seed, with_idx, composed):
    """Logits with a saturated row (+-80), labels, the criterion's fp32 dlogits, a group table — with an absent group, a one-row
    group and rows in groups -1 and G where B and G leave room — read by row or through idx with gaps, q, weights and smoothing."""
    rs = np.random.RandomState(seed)
    z = (2.0 * rs.randn(B, K)).astype(np.float32)
    z[B - 1] = np.where(np.arange(K) % 2 == 0, 80.0, -80.0)
    y = rs.randint(0, K, size=B).astype(np.int64)
    w = (0.25 + rs.rand(K)).astype(np.float32) if composed else None
    eps = 0.1 if composed else 0.0
    pool = list(range(G))
    if G >= 3:
        pool.remove(1)                                            # absent
    lone = pool[-1] if len(pool) >= 2 and B >= 4 else None
    rest = [g for g in pool if g != lone]
    rows = np.array([rest[i % len(rest)] for i in range(B)], dtype=np.int32)
    rows = rows[rs.permutation(B)]
    if lone is not None:
        rows[B // 2] = lone                                       # a one-row group
    if B >= 6:
        rows[0], rows[1] = -1, G                                  # in no group
    q = rs.rand(G) + 0.1
    q = (q / q.sum()).astype(np.float32)
    dl = R.criterion_dlogits(z, y, w, eps).astype(np.float32)
    if with_idx:
        P = B + 9
        idx = rs.permutation(P)[:B].astype(np.int64)
        grp = rs.randint(-1, G + 1, size=P).astype(np.int32)
        grp[idx] = rows
    else:
        idx, grp = None, rows
    return dict(z=z, y=y, w=w, eps=eps, grp=grp, idx=idx, q=q, dl=dl, G=G, rows=rows)


def _apply(c, eta, frozen=False, stats0="zeros", q=None, check_inputs=True):
    """msig_dro_apply on guarded copies: (dlogits, q, stats or None) on the host; guards and inputs checked."""
    B, K = c["z"].shape
    bufs = dict(z=Guarded(c["z"]), y=Guarded(c["y"]), grp=Guarded(c["grp"]), dl=Guarded(c["dl"]), q=Guarded(c["q"] if q is None else q))
    if c["w"] is not None:
        bufs["w"] = Guarded(c["w"])
    if c["idx"] is not None:
        bufs["idx"] = Guarded(c["idx"])
    if stats0 is not None:
        bufs["stats"] = Guarded(np.zeros(NS) if isinstance(stats0, str) else stats0)
    d = L.Dro()
    d.G, d.eta, d.frozen = c["G"], eta, int(frozen)
    d.grp, d.q = bufs["grp"].ptr(), bufs["q"].ptr()
    d.idx = bufs["idx"].ptr() if "idx" in bufs else None
    d.stats = bufs["stats"].ptr() if "stats" in bufs else None
    L.check(L.lib().msig_dro_apply(C.byref(d), bufs["z"].ptr(), bufs["y"].ptr(), bufs["w"].ptr() if "w" in bufs else None, c["eps"],
                                   bufs["dl"].ptr(), B, K, _stream()), "msig_dro_apply")
    torch.cuda.synchronize()
    for name, b in bufs.items():
        assert b.guards_intact(), name
        if check_inputs and name in ("z", "y", "grp", "w", "idx"):
            assert b.untouched(), name
    return bufs["dl"].get(), bufs["q"].get(), bufs["stats"].get() if "stats" in bufs else None


def _check_against_restatement(c, eta, got_dl, got_q, got_st, ref):
    B, K = c["z"].shape
    G = c["G"]
    assert within_store_rounding(got_q, ref["q"]), (got_q, ref["q"])
    assert abs(float(got_q.astype(np.float64).sum()) - 1.0) < 1e-6
    # the factors the device's q implies, from the restatement's sums
    implied = np.array([float(np.float32(float(got_q[g]) * ref["Wall"] / ref["W_g"][g])) if g >= 0 and ref["present"][g] else 0.0 for g in ref["groups"]])
    assert within_store_rounding(implied, ref["r"])
    err = np.abs(got_dl.astype(np.float64) - ref["dlogits"])
    ratio = float((err / ulp32(ref["dlogits"])).max())
    print(f"B={B} K={K} G={G} eta={eta}: worst dlogits error {ratio:.3f} fp32 ulps (bound 3)")
    assert np.all(err <= 3.0 * ulp32(ref["dlogits"])), ratio
    if got_st is not None:
        want = ref["stats"]
        assert np.array_equal(got_st[128:192], want[128:192]) and got_st[193] == want[193]
        for sl in (slice(0, 64), slice(64, 128), slice(192, 193)):
            assert np.all(np.abs(got_st[sl] - want[sl]) <= FIXED_TOL["loss"] * np.abs(want[sl])), (sl, got_st[sl], want[sl])


# every B, K, G and eta at least once, the corners, with idx and without, plain and composed (class weights, eps = 0.1)
APPLY_CASES = [(1, 2, 1, False, False, 0.01), (2, 3, 2, True, True, 1.0), (17, 16, 11, True, True, 0.01), (64, 2, 33, False, True, 0.0),
               (255, 3, 64, True, False, 1.0), (256, 16, 64, False, True, 0.01), (2048, 2, 64, True, True, 1.0),
               (2048, 16, 1, False, False, 0.01), (1, 16, 64, True, True, 1.0), (2048, 3, 2, True, False, 0.0)]


@pytest.mark.parametrize("B,K,G,with_idx,composed,eta", APPLY_CASES)
def test_apply_matches_the_restatement(B, K, G, with_idx, composed, eta):
    c = _case(B, K, G, 1000 * B + 10 * K + G, with_idx, composed)
    got_dl, got_q, got_st = _apply(c, eta)
    ref = R.apply(c["z"], c["y"], c["grp"], c["q"], eta, G, c["w"], c["eps"], dlogits=c["dl"], idx=c["idx"], stats=np.zeros(NS))
    assert ref["wrote"]
    if G >= 3:
        assert not ref["present"][1]
    if B >= 6:
        assert ref["groups"][0] == ref["groups"][1] == -1 and not got_dl[:2].any()
    _check_against_restatement(c, eta, got_dl, got_q, got_st, ref)
    if eta == 0.0:                                                # probe: q is renormalised, nothing else
        assert within_store_rounding(got_q, c["q"].astype(np.float64) / c["q"].astype(np.float64).sum())


# ---- 2. structure ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 17, 2048])
def test_a_launch_without_a_present_group_writes_nothing(B):
    c = _case(B, 3, 4, B, True, True)
    c["grp"] = np.where(np.arange(c["grp"].size) % 2 == 0, -1, 4).astype(np.int32)
    ones = np.ones(NS)
    dl, q, st = _apply(c, 1.0, stats0=ones)
    assert _same_bits(dl, c["dl"]) and _same_bits(q, c["q"]) and np.array_equal(st, ones)
    c2 = _case(B, 3, 4, B, False, True)                            # every group's mass is zero: W_g = 0, no group is present
    c2["w"] = np.zeros(3, np.float32)
    dl, q, st = _apply(c2, 1.0, stats0=ones)
    assert _same_bits(dl, c2["dl"]) and _same_bits(q, c2["q"]) and np.array_equal(st, ones)


@pytest.mark.parametrize("B,composed", [(1, False), (64, True), (2048, True)])
def test_one_group_with_unit_weight_leaves_dlogits_bit_identical(B, composed):
    c = _case(B, 3, 1, 7 + B, False, composed)
    c["grp"] = np.zeros(B, np.int32)
    c["q"] = np.ones(1, np.float32)
    for eta in (0.0, 1.0):
        dl, q, st = _apply(c, eta)
        assert _same_bits(dl, c["dl"]) and q[0] == 1.0 and st[128] == B and st[193] == 1.0


def test_frozen_reproduces_the_updating_call_and_stats_accumulate():
    c = _case(255, 3, 11, 3, True, True)
    prior = np.arange(NS, dtype=np.float64)
    dl, q, st = _apply(c, 0.5, stats0=prior)
    assert not _same_bits(q, c["q"])
    dl0, q0, st0 = _apply(c, 0.5)                                   # onto zeros: the difference is the prior content
    assert _same_bits(dl0, dl) and _same_bits(q0, q)
    assert np.allclose(st - prior, st0, rtol=1e-12, atol=1e-9) and np.array_equal((st - prior)[128:192], st0[128:192])
    dln, qn, _ = _apply(c, 0.5, stats0=None)                        # stats = NULL: the same bits
    assert _same_bits(dln, dl) and _same_bits(qn, q)
    dlf, qf, stf = _apply(c, 0.5, frozen=True, stats0=prior, q=q)   # frozen on the q the updating call left
    assert _same_bits(dlf, dl) and _same_bits(qf, q) and np.array_equal(stf, prior)


def test_q_follows_a_planted_hard_group():
    """40 applies on fixed logits, B = 64, G = 4, eta = 0.5, group 2's rows mislabelled: q[2] rises every step and ends largest; the
    trajectory stays within 2 n fp32 ulps of the restatement's at step n (each step stores fp32 once, at most 2 ulps off, and the
    normalisation does not amplify).  The logits favour the true class by a margin of 0.5, so the hard group's loss is about 0.5
    above the others' and 1 - q[2] shrinks by about e^-0.25 per step: after 40 steps it is near 1e-4, far above fp32's spacing at
    1 (6e-8), and every step's rise is representable."""
    B, K, G, eta = 64, 3, 4, 0.5
    rs = np.random.RandomState(11)
    true = rs.randint(0, K, size=B)
    z = (0.1 * rs.randn(B, K)).astype(np.float32)
    z[np.arange(B), true] += 0.5
    grp = (np.arange(B) % G).astype(np.int32)
    y = np.where(grp == 2, (true + 1) % K, true).astype(np.int64)
    dl = R.criterion_dlogits(z, y).astype(np.float32)
    zt, yt, gt, dt = _dev(z), _dev(y), _dev(grp), _dev(dl)
    q = torch.full((G,), 0.25, dtype=torch.float32, device=DEV)
    d = L.Dro()
    d.G, d.eta, d.grp, d.q = G, eta, gt.data_ptr(), q.data_ptr()
    traj = []
    for _ in range(40):
        work = dt.clone()
        L.check(L.lib().msig_dro_apply(C.byref(d), zt.data_ptr(), yt.data_ptr(), None, 0.0, work.data_ptr(), B, K, _stream()), "msig_dro_apply")
        traj.append(q.cpu().numpy().astype(np.float64))
    qr, worst = np.full(G, 0.25, np.float32), 0.0
    for n, got in enumerate(traj, start=1):
        qr = R.apply(z, y, grp, qr, eta, G)["q"]
        ratio = float((np.abs(got - qr) / ulp32(qr)).max())
        worst = max(worst, ratio / (2 * n))
        assert np.all(np.abs(got - qr) <= 2 * n * ulp32(qr)), (n, ratio)
    print(f"worst trajectory error / (2 n ulps): {worst:.3f}; final q {traj[-1]}")
    q2 = [t[2] for t in traj]
    assert all(b > a for a, b in zip([0.25] + q2[:-1], q2)) and int(np.argmax(traj[-1])) == 2


# ---- 3. fold batches of the term ------------------------------------------------------------------------------------------------
def test_apply_multi_equals_the_single_calls_and_leaves_the_other_slot_alone():
    """Three folds in slots (2, 0, 3) of four arenas, each with its own q / grp / stats in a block of its own stride and a row of a
    shared idx matrix: the single calls' bits; slot 1 keeps its poison."""
    B, K, G, n_slots, slots = 255, 3, 11, 4, (2, 0, 3)
    cases = [_case(B, K, G, 50 + i, True, True) for i in range(3)]
    P = cases[0]["grp"].size
    o_z, o_y, o_w, o_dl, stride = 0, 4096, 8192, 8448, 16384
    mem = torch.full((n_slots, stride), 0xA5, dtype=torch.uint8, device=DEV)
    o_q, o_grp, o_st, dstride = 0, 256, 2048, 4096
    dmem = torch.full((n_slots, dstride), 0xA5, dtype=torch.uint8, device=DEV)
    idx = torch.full((3, B + 3), 0, dtype=torch.int64, device=DEV)

    def put(row, off, host):
        t = _dev(host).reshape(-1)
        row[off:off + t.numel() * t.element_size()] = t.view(torch.uint8)

    for i, s in enumerate(slots):
        c = cases[i]
        put(mem[s], o_z, c["z"]); put(mem[s], o_y, c["y"]); put(mem[s], o_w, c["w"]); put(mem[s], o_dl, c["dl"])
        put(dmem[s], o_q, c["q"]); put(dmem[s], o_grp, c["grp"]); put(dmem[s], o_st, np.zeros(NS))
        idx[i, :B] = _dev(c["idx"])
    before1, dbefore1 = mem[1].clone(), dmem[1].clone()
    m = L.Multi()
    m.n, m.stride_bytes = 3, stride
    for i, s in enumerate(slots):
        m.slot[i] = s
    d = L.Dro()
    d.G, d.eta = G, 0.5
    d.q, d.grp, d.stats, d.stride_bytes = dmem.data_ptr() + o_q, dmem.data_ptr() + o_grp, dmem.data_ptr() + o_st, dstride
    d.idx, d.idx_row_stride = idx.data_ptr(), B + 3
    base = mem.data_ptr()
    L.check(L.lib().msig_dro_apply_multi(C.byref(d), C.byref(m), base + o_z, base + o_y, base + o_w, 0.1, base + o_dl, B, K, _stream()),
            "msig_dro_apply_multi")
    torch.cuda.synchronize()
    assert torch.equal(mem[1], before1) and torch.equal(dmem[1], dbefore1)
    for i, s in enumerate(slots):
        dl, q, st = _apply(cases[i], 0.5)
        assert _same_bits(mem[s, o_dl:o_dl + B * K * 4].view(torch.float32).cpu().numpy().reshape(B, K), dl), i
        assert _same_bits(dmem[s, o_q:o_q + G * 4].view(torch.float32).cpu().numpy(), q), i
        assert np.array_equal(dmem[s, o_st:o_st + NS * 8].view(torch.float64).cpu().numpy(), st), i
        assert _same_bits(mem[s, o_z:o_z + B * K * 4].view(torch.float32).cpu().numpy().reshape(B, K), cases[i]["z"])
        assert bool((dmem[s, o_q + G * 4:o_grp] == 0xA5).all()) and bool((mem[s, o_dl + B * K * 4:] == 0xA5).all())
    assert P * 4 <= o_st - o_grp and B * K * 4 <= o_y - o_z and NS * 8 <= dstride - o_st


# ---- 4. the train step against the oracle ---------------------------------------------------------------------------------------
LR, WD, ADAM_EPS = 1e-3, 1e-4, 1e-3
GOLDEN = ("model_c6_k2_t512", "model_c2_k3_t256")
CASES = [dict(w=None, eps=0.0, clip=None), dict(w=(0.3, 2.5), eps=0.1, clip=0.05)]


def _oracle(params, buffers, x, y, groups, q, case, w):
    """{dtype: ({key: gradient after the clip}, {key: parameter after Adam's first step})} of L = sum_g q_g CE(z[g], y[g]) over the
    groups that have rows, q a constant, differentiated by autograd through the whole model."""
    out = {}
    for dt in (torch.float64, torch.float32):
        leaf = {k: v.to(dt).clone().requires_grad_(v.numel() > 0) for k, v in params.items()}
        bufs = {k: (v.clone() if "num_batches" in k else v.to(dt)) for k, v in buffers.items()}
        st, _ = O.forward(leaf, bufs, torch.as_tensor(x).to(dt), training=True, dropout_p=0.0, seed=0, step=1)
        z, yt = st["logits"], torch.as_tensor(y)
        wt = None if w is None else torch.tensor(w, dtype=dt)
        loss = 0.0
        for g in sorted(set(groups) - {-1}):
            rows = torch.tensor([b for b, gb in enumerate(groups) if gb == g])
            loss = loss + float(q[g]) * F.cross_entropy(z[rows], yt[rows], weight=wt, label_smoothing=case["eps"])
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
    """One msig_dro_train_step at eta = 0.5, B = 8, dropout 0, three groups of which one is absent and one row in no group, on the
    committed parameters (the one-layer model: the oracle's initialisation of the same C and K): every parameter gradient and every
    parameter after Adam against the oracle of the robust loss with the post-update q read back from the device, gated by
    gpu_common.grad_tol on the fp32 oracle's own error.  Adam's eps is 1e-3 for the reason test_distill_gpu.py gives."""
    kind, layers = model
    meta, params_np, _ = load_golden_model(name)
    Cc, K, T, B = meta["C"], meta["K"], meta["T"], 8
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
    x = rs.randn(B, Cc, T).astype(np.float32)
    y = rs.randint(0, K, size=B).astype(np.int64)
    y[:K] = np.arange(K)
    groups = [0, 2, 2, -1, 0, 2, 0, 2]                              # G = 3, group 1 absent
    idx = rs.permutation(B + 9)[:B].astype(np.int64)
    table = np.full(B + 9, 1, np.int32)
    table[idx] = groups
    w = None if case["w"] is None else (case["w"] + (1.0,) * (K - 2))
    if layers == 1:
        e = EmbeddedEngine(Cc, K, DEV, 32, kind=kind)
        for k, v in e.small_views().items():
            v.copy_(params[k])
    else:
        e = Engine(Cc, K, DEV, kind=kind)
        e.load_named({**params, **buffers})
    d = GroupDro(0.5).set_groups(table, 3).bind(DEV)
    d.q.copy_(torch.tensor([0.5, 0.2, 0.3]))
    e.train_step(_dev(x), _dev(y), LR, eps=ADAM_EPS, weight_decay=WD, step=1, dropout_p=0.0, seed=1,
                 class_weight=None if w is None else torch.tensor(w, dtype=torch.float32, device=DEV), max_grad_norm=case["clip"],
                 label_smoothing=case["eps"], dro=d, batch_index=_dev(idx))
    torch.cuda.synchronize()
    q = d.q.cpu().numpy().astype(np.float64)
    assert abs(q.sum() - 1.0) < 1e-6 and q[1] < 0.2 and float(d.stats[193]) == 1.0 and d.stats[128:131].tolist() == [3.0, 0.0, 4.0]
    if layers == 1:
        assert int(e.grads[e.padding].count_nonzero()) == 0 and int(e.params[e.padding].count_nonzero()) == 0
        got_g = {k: v.cpu().numpy().copy() for k, v in e.gather_grads().items()}
        got_p = {k: v.cpu().numpy().copy() for k, v in e.small_views().items()}
    else:
        got_g = {k: v.cpu().numpy() for k, v in e.named_param_views(e.grads).items()}
        got_p = {k: v.cpu().numpy() for k, v in e.named_param_views().items()}
    ref = _oracle(oparams, buffers, x, y, groups, q, case, w)
    (g64, p64), (g32, p32) = ref[torch.float64], ref[torch.float32]
    # precondition, from the reference alone: the pooled mean's gradient differs from the robust one by far more than the tolerance
    pooled = _oracle(oparams, buffers, x, y, [0] * B, [1.0], case, w)[torch.float64][0]
    k0 = "classifier.3.weight"
    assert rel_err(pooled[k0], g64[k0]) > 100 * grad_tol(k0, rel_err(g32[k0], g64[k0]))
    if case["clip"] is not None:
        assert e.grad_stats()["clipped"] == 1
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


# ---- 5. bit identity and launch counts ------------------------------------------------------------------------------------------
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


def _dro(table, G, eta=0.5, q=None):
    d = GroupDro(eta).set_groups(table, G).bind(DEV)
    if q is not None:
        d.q.copy_(torch.as_tensor(q, dtype=torch.float32))
    return d


STATE = ("params", "grads", "exp_avg", "exp_avg_sq", "bn_state")


def _same_state(a, b):
    return all(torch.equal(_bits(getattr(a, n)), _bits(getattr(b, n))) for n in STATE) and torch.equal(a.loss_acc, b.loss_acc) \
        and torch.equal(_bits(a.region("LOSS", torch.float32, (3,))), _bits(b.region("LOSS", torch.float32, (3,))))


@pytest.mark.parametrize("with_sam", [False, True], ids=["kd", "sam"])
@pytest.mark.parametrize("model", [(ATT, 64, 2), (CG, 64, 2), (ATT, 32, 1)], ids=["attention", "cnn_gru", "embedded"])
def test_null_and_one_unit_group_are_the_plain_step_bit_for_bit(model, with_sam):
    """Three steps with eps = 0.1, clip and dropout: the narrower entry point without the option called directly (msig_da_train_step,
    or msig_sam_train_step with sam), msig_dro_train_step with a NULL msig_dro, and one group with q = [1] leave the same parameters,
    gradients, moments, BatchNorm state and losses, and the NULL call makes the same launches; three groups do not."""
    kind, hidden, layers = model
    Cc, K, B, T = 3, 2, 21, 512
    sam = Sam(0.05) if with_sam else None
    table3 = (np.arange(B) % 3).astype(np.int32)
    engines, launches = {}, {}
    for mode in ("plain", "null", "one", "three"):
        e = _engine(Cc, K, hidden, layers, kind)
        d = {"plain": None, "null": None, "one": _dro(np.zeros(B, np.int32), 1), "three": _dro(table3, 3)}[mode]
        for s in (1, 2, 3):
            x, y = _data(B, Cc, K, T, 10 + s)
            if s == 3:
                L.profile_enable(True)
            try:
                if mode == "null":                               # the entry point itself with a NULL msig_dro
                    if layers == 1:
                        e.scatter()
                    e.ensure_adam_state()
                    b = e._batch(x, y, True, 0.5, 7, s)
                    cw, mn, sm, lam = e._checked(None, 1.0, 0.1, None)
                    sd = None
                    if sam is not None:
                        state = e.ensure_sam_state()
                        sd = C.byref(sam.descriptor(e.kind, state.data_ptr(), state.numel() * 8))
                    L.check(L.lib().msig_dro_train_step(C.byref(b), C.byref(e._st(cw, mn, sm, lam)), None, None, sd, None, e.exp_avg.data_ptr(),
                                                        e.exp_avg_sq.data_ptr(), LR, 0.9, 0.999, 1e-8, 1e-4, s, _stream()), "msig_dro_train_step")
                    if layers == 1:
                        e.gather()
                elif mode == "plain":                            # the narrower entry point, called directly (Engine.train_step is msig_sc_train_step)
                    name = narrow_train_step(e, x, y, LR, weight_decay=1e-4, step=s, dropout_p=0.5, seed=7, label_smoothing=0.1, max_grad_norm=1.0,
                                             sam=sam)
                    assert name == ("msig_sam_train_step" if with_sam else "msig_da_train_step")
                else:
                    e.train_step(x, y, LR, weight_decay=1e-4, step=s, dropout_p=0.5, seed=7, label_smoothing=0.1, max_grad_norm=1.0, sam=sam, dro=d)
                torch.cuda.synchronize()
                if s == 3:
                    launches[mode] = {k: v[0] for k, v in L.profile_report().items()}
            finally:
                L.profile_enable(False)
        engines[mode] = (e, d)
    plain = engines["plain"][0]
    assert _same_state(plain, engines["null"][0]) and launches["null"] == launches["plain"] and "dro_apply" not in launches["plain"]
    assert all(torch.equal(_bits(getattr(plain, n)), _bits(getattr(engines["one"][0], n))) for n in STATE)
    assert engines["one"][1].q.tolist() == [1.0] and float(engines["one"][1].stats[193]) == 3.0
    assert not torch.equal(_bits(plain.params), _bits(engines["three"][0].params))
    assert torch.equal(plain.loss_acc[1:], engines["one"][0].loss_acc[1:])
    d3 = engines["three"][1]
    assert float(d3.stats[193]) == 3.0 and abs(float(d3.q.sum()) - 1.0) < 1e-6      # under sam too: one update and one report per step
    assert launches["three"]["dro_apply"] == (2 if with_sam else 1)


@pytest.mark.parametrize("B", [21, 2048])
def test_launch_counts(B):
    """By the library's own launch report: group-DRO is the plain step's launches minus head_step plus head_fwd, ce, head_bwd and
    dro_apply once each — the plain step's count plus three — and exactly one launch more than the same step on the unfused route
    (the distilled step's)."""
    from multimodalsignal_amd.distill import Distillation
    Cc, K, T = 3, 2, 64
    x, y = _data(B, Cc, K, T, 4)
    table = (np.arange(B) % 5).astype(np.int32)
    rs = np.random.RandomState(1)
    tq = np.exp(rs.randn(B, K))
    reports = {}
    for mode in ("plain", "kd", "dro", "kd+dro"):
        e = _engine(Cc, K)
        kd = None
        if "kd" in mode:
            kd = Distillation(0.5, 2.0)
            kd.set_teacher((tq / tq.sum(axis=1, keepdims=True)).astype(np.float32))
            kd.bind(DEV)
        d = _dro(table, 5) if "dro" in mode else None
        e.train_step(x, y, LR, step=1, dropout_p=0.5, seed=7, distill=kd, dro=d)          # workspaces exist before the count starts
        torch.cuda.synchronize()
        L.profile_enable(True)
        try:
            e.train_step(x, y, LR, step=2, dropout_p=0.5, seed=7, distill=kd, dro=d)
            torch.cuda.synchronize()
            reports[mode] = {k: v[0] for k, v in L.profile_report().items()}
        finally:
            L.profile_enable(False)
    plain = reports["plain"]
    assert "dro_apply" not in plain and plain["head_step"] == 1 and "head_fwd" not in plain
    want = dict(plain)
    want.pop("head_step")
    want.update(head_fwd=1, ce=1, head_bwd=1, dro_apply=1)
    assert reports["dro"] == want and sum(reports["dro"].values()) == sum(plain.values()) + 3
    assert reports["kd+dro"] == {**reports["kd"], "dro_apply": 1}
    assert sum(reports["dro"].values()) == sum(reports["kd"].values())      # the distilled route's count: one small launch for another


# ---- 6. fold batches of the train step ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", ["plain", "adversary", "sam"])
def test_train_step_multi_equals_the_single_calls(extra):
    """NF = 3 with per-fold seeds, step counts and learning rates, each fold its own q, group table and statistics in the arena's
    block, idx rows of a shared matrix, two steps: msig_dro_train_step_multi leaves every fold's parameters, gradients, moments,
    BatchNorm state, q and statistics (and the discriminator's, with the adversary on) with the bits of its msig_dro_train_step.
    Under SAM q advances once per step: after the first step it has the bits the step without SAM leaves."""
    n, B, T, Cc, K, S, G, npos = 3, 21, 512, 3, 2, 4, 5, 60
    msteps, dsteps, lrs, lam_rev = (1, 3, 5), (2, 4, 6), (1e-3, 5e-4, 2e-3), (0.3, 0.5, 1.0)
    rs = np.random.RandomState(8)
    data = [[_data(B, Cc, K, T, 300 + 10 * f + s) for s in range(2)] for f in range(n)]
    tables = [rs.randint(-1, G, size=npos).astype(np.int32) for _ in range(n)]
    doms = [rs.randint(-1, S, size=npos).astype(np.int32) for _ in range(n)]
    idx = _dev(rs.randint(0, npos, size=(n, B + 3)).astype(np.int64))
    sam = Sam(0.05) if extra == "sam" else None
    arena = FoldArena(Cc, K, DEV, n, B, T, adversary=(S, npos) if extra == "adversary" else None, grad_clip=True, sam=sam is not None,
                      dro=(G, npos))
    engs = [_engine(Cc, K, seed=10 + f, storage_engine=arena.engine(f)) for f in range(n)]
    dros, advs = [], []
    for f in range(n):
        dros.append(GroupDro(0.5).set_groups(tables[f], G).bind(DEV, arena.side_storage("dro", f)))
        if extra == "adversary":
            adv = SubjectAdversary(S, lam=lam_rev[f], schedule="constant", seed=40 + f)
            adv.set_domains(doms[f])
            advs.append(adv.bind(DEV, arena.side_storage("adversary", f)))
        arena.set_max_norm(f, 1.0)
    slots = list(range(n))
    desc = arena.batch(B, True, 0.5)
    sd = arena.soft(slots, 0.1, None, clip=arena.clip(slots))
    q_after_first = None
    for s in range(2):
        for f in range(n):
            x, y = data[f][s]
            arena.view(f, "x", torch.float32)[:x.numel()].copy_(x.reshape(-1))
            arena.view(f, "y", torch.int64)[:B].copy_(y)
        st = [msteps[f] + s for f in slots]
        m = arena.multi(slots, key_gru=[L.dropout_key(100 + f, st[f], 1) for f in slots], key_head=[L.dropout_key(100 + f, st[f], 2) for f in slots],
                        lr=lrs, steps=st)
        dr = arena.dro(0.5)
        dr.idx, dr.idx_row_stride = idx.data_ptr(), B + 3
        a = None
        if extra == "adversary":
            a = arena.da(slots, S, lam_rev, lrs, [dsteps[f] + s for f in slots], (0.9, 0.999), 1e-8, 1e-4)
            a.idx, a.idx_row_stride = idx.data_ptr(), B + 3
        L.check(L.lib().msig_dro_train_step_multi(C.byref(desc), C.byref(m), C.byref(sd), None if a is None else C.byref(a), None,
                                                  None if sam is None else C.byref(arena.sam(sam)), C.byref(dr), arena.ptr("exp_avg"),
                                                  arena.ptr("exp_avg_sq"), 0.9, 0.999, 1e-8, 1e-4, st[0], _stream()), "msig_dro_train_step_multi")
        torch.cuda.synchronize()
        if s == 0:
            q_after_first = [d.q.clone() for d in dros]
    for f in range(n):
        e = _engine(Cc, K, seed=10 + f)
        d = _dro(tables[f], G)
        adv = None
        if extra == "adversary":
            adv = SubjectAdversary(S, lam=lam_rev[f], schedule="constant", seed=40 + f)
            adv.set_domains(doms[f])
            adv.step = dsteps[f] - 1
            adv.bind(DEV)
        for s in range(2):
            x, y = data[f][s]
            e.train_step(x, y, lrs[f], weight_decay=1e-4, step=msteps[f] + s, dropout_p=0.5, seed=100 + f, label_smoothing=0.1,
                         max_grad_norm=1.0, adversary=adv, sam=sam, dro=d, batch_index=idx[f, :B].contiguous())
            torch.cuda.synchronize()
            if s == 0:
                assert torch.equal(_bits(d.q), _bits(q_after_first[f])), f
                if sam is not None:                               # pass 1 is the plain step's forward: q moved once, by that step's amount
                    e0, d0 = _engine(Cc, K, seed=10 + f), _dro(tables[f], G)
                    e0.train_step(x, y, lrs[f], weight_decay=1e-4, step=msteps[f], dropout_p=0.5, seed=100 + f, label_smoothing=0.1,
                                  max_grad_norm=1.0, dro=d0, batch_index=idx[f, :B].contiguous())
                    torch.cuda.synchronize()
                    assert torch.equal(_bits(d0.q), _bits(d.q)) and torch.equal(d0.stats, d.stats)
                    assert not torch.equal(_bits(e0.params), _bits(e.params))
        for name in STATE:
            assert torch.equal(_bits(getattr(e, name)), _bits(getattr(engs[f], name))), (f, name)
        assert torch.equal(_bits(d.q), _bits(dros[f].q)) and torch.equal(d.stats, dros[f].stats) and float(d.stats[193]) == 2.0, f
        if extra == "adversary":
            for name in ("params", "exp_avg", "exp_avg_sq"):
                assert torch.equal(_bits(getattr(adv, name)), _bits(getattr(advs[f], name))), (f, name)
    both = arena.dro_stats().cpu()
    assert torch.equal(both[:, :NS], torch.stack([d.stats.cpu() for d in dros]))
    assert torch.equal(both[:, NS:NS + G].to(torch.float32), torch.stack([d.q.cpu() for d in dros]))


def test_embedded_fold_batch_keeps_its_padding_zero_and_equals_the_single_calls():
    n, B, T, Cc, K, G, npos, steps = 2, 21, 512, 3, 2, 4, 50, 3
    rs = np.random.RandomState(4)
    data = [[_data(B, Cc, K, T, 500 + 10 * f + s) for s in range(steps)] for f in range(n)]
    tables = [rs.randint(-1, G, size=npos).astype(np.int32) for _ in range(n)]
    idx = _dev(rs.randint(0, npos, size=(n, B)).astype(np.int64))
    arena = FoldArena(Cc, K, DEV, n, B, T, gru_hidden=32, gru_layers=1, dro=(G, npos))
    engs = [_engine(Cc, K, 32, 1, seed=10 + f, storage_engine=arena.engine(f)) for f in range(n)]
    dros = [GroupDro(1.0).set_groups(tables[f], G).bind(DEV, arena.side_storage("dro", f)) for f in range(n)]
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
        dr = arena.dro(1.0)
        dr.idx, dr.idx_row_stride = idx.data_ptr(), B
        L.check(L.lib().msig_dro_train_step_multi(C.byref(desc), C.byref(m), C.byref(sd), None, None, None, C.byref(dr), arena.ptr("exp_avg"),
                                                  arena.ptr("exp_avg_sq"), 0.9, 0.999, 1e-8, 1e-4, s, _stream()), "msig_dro_train_step_multi")
    torch.cuda.synchronize()
    for f in range(n):
        pad = engs[f].padding
        for name in ("params", "grads", "exp_avg", "exp_avg_sq"):
            assert int(getattr(engs[f], name)[pad].count_nonzero()) == 0, (f, name)
        e, d = _engine(Cc, K, 32, 1, seed=10 + f), _dro(tables[f], G, eta=1.0)
        for s in range(1, steps + 1):
            x, y = data[f][s - 1]
            e.train_step(x, y, LR, weight_decay=1e-4, step=s, dropout_p=0.5, seed=100 + f, dro=d, batch_index=idx[f].contiguous())
        torch.cuda.synchronize()
        for name in STATE:
            assert torch.equal(_bits(getattr(e, name)), _bits(getattr(engs[f], name))), (f, name)
        assert torch.equal(_bits(d.q), _bits(dros[f].q)) and torch.equal(d.stats, dros[f].stats)
        assert not torch.equal(d.q, torch.full_like(d.q, 0.25))  # the weights moved


def test_mixup_and_oversized_batches_are_refused_by_the_engine_before_any_launch():
    Cc, K, T = 3, 2, 64
    e = _engine(Cc, K)
    before = e.params.clone()
    x, y = _data(8, Cc, K, T, 1)
    with pytest.raises(ValueError, match="mixup"):
        e.train_step(x, y, LR, step=1, mix_lambda=0.4, dro=_dro(np.zeros(8, np.int32), 1))
    x, y = _data(2049, Cc, K, T, 1)
    with pytest.raises(ValueError, match="at most 2048"):
        e.train_step(x, y, LR, step=1, dro=_dro(np.zeros(2049, np.int32), 1))
    assert torch.equal(e.params, before) and e.exp_avg is None


# ---- 7. drivers -----------------------------------------------------------------------------------------------------------------
SUBS = ["S2", "S3", "S4", "S5"]


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


def _check_doc(doc, groups="subject"):
    assert doc["folds"] and doc["settings"]["groups"] == groups and doc["synthetic"] is True
    for f in doc["folds"]:
        assert abs(sum(f["q"]) - 1.0) < 1e-6 and abs(sum(s["q"] for s in f["subjects"]) - 1.0) < 1e-6 and len(f["q"]) == f["G"]
        assert [s["q"] for s in f["subjects"]] == sorted((s["q"] for s in f["subjects"]), reverse=True)
        assert f["heaviest"] == f["subjects"][0]["subject"] and f["subject"] not in [s["subject"] for s in f["subjects"]]
        assert f["robust_loss"] > 0 and f["mean_loss"] > 0 and 0.0 <= f["worst_val_acc"] <= 1.0 and f["worst_val_subject"] in SUBS
    assert sum(h["folds"] for h in doc["pooled"]["heaviest"]) == len(doc["folds"])


def test_fold_batches_equal_sequential_folds_and_the_report_is_well_formed(tmp_path):
    from multimodalsignal_amd import main as M
    flags = ["--group-dro", "0.5", "--label-smoothing", "0.1"]
    runs = {}
    for tag, extra in (("lock", flags), ("seq", flags + ["--concurrent-folds", "1"]), ("plain", ["--label-smoothing", "0.1"])):
        M.main(_common(tmp_path) + extra + ["--out", str(tmp_path / tag)])
        run = next((tmp_path / tag).glob("*/run_*"))
        txt = (run / "cv_summary.txt").read_text(encoding="utf-8")
        assert ("GROUP DRO: eta=0.5 groups=subject" in txt) == (tag != "plain")
        assert (run / "dro.json").exists() == (run / "dro.txt").exists() == (tag != "plain")
        runs[tag] = (_fold_outputs(run), run)
    for (ia, wa), (ib, wb) in zip(runs["lock"][0], runs["seq"][0]):
        assert ia == ib
        assert list(wa) == list(wb) and all(torch.equal(wa[k], wb[k]) for k in wa)
    keys = ("dro_robust_loss", "dro_worst_group_loss", "dro_worst_subject", "dro_q_max", "dro_q_entropy", "val_worst_subject_acc")
    assert all(k in h for f, _ in runs["lock"][0] for h in f["history"] for k in keys)
    assert all(not any(k.startswith("dro") or k.startswith("val_worst") for k in h) for f, _ in runs["plain"][0] for h in f["history"])
    assert all("group_dro" not in f for f, _ in runs["plain"][0])
    assert any(not torch.equal(a[1][k], p[1][k]) for a, p in zip(runs["lock"][0], runs["plain"][0]) for k in a[1])
    for f, _ in runs["lock"][0]:
        g = f["group_dro"]
        assert g["G"] == 2 and abs(sum(g["q"]) - 1.0) < 1e-6 and len(g["subject_loss"]) == 2 and set(g["subjects"]) < set(SUBS)
    doc = json.loads((runs["lock"][1] / "dro.json").read_text())
    assert doc == json.loads((runs["seq"][1] / "dro.json").read_text())
    assert [f["subject"] for f in doc["folds"]] == SUBS and doc["probe"] is False
    _check_doc(doc)
    assert "say nothing about WESAD accuracy" in (runs["lock"][1] / "dro.txt").read_text(encoding="utf-8")
    assert "dro robust loss" in (runs["lock"][1] / "fold_test_on_S2" / "training_log.txt").read_text(encoding="utf-8")


@pytest.mark.parametrize("mode", [["--ablation"], ["--hierarchical"], ["--model", "cnn_gru_attention", "cnn_gru"], ["--no-lockstep"],
                                  ["--hierarchical", "--concurrent-folds", "1"], ["--seeds", "2"], ["--seeds", "2", "--distill"],
                                  ["--sam", "0.05", "--weight-average", "ema"]],
                         ids=["ablation", "hierarchical", "model", "no-lockstep", "hierarchical-sequential", "seeds", "distill", "sam-ema"])
def test_every_driver_mode_runs_with_group_dro(tmp_path, mode):
    from multimodalsignal_amd import main as M
    extra = ["--max-grad-norm", "1.0", "--label-smoothing", "0.1", "--augment", "scale=0.1"]
    if "--hierarchical" not in mode:       # a model of the tiny hierarchical set may see one class only, which 'balanced' refuses
        extra += ["--class-weights", "balanced"]
    if "--sam" not in mode:
        extra += ["--subject-adversarial"]
    M.main(_common(tmp_path) + ["--group-dro", "--dro-groups", "subject-class"] + extra + mode + ["--out", str(tmp_path / "o")])
    summaries = [p for p in (tmp_path / "o").rglob("*summary.txt")]
    assert summaries and all("GROUP DRO: eta=0.01 groups=subject-class" in p.read_text(encoding="utf-8") for p in summaries), summaries
    tables = [p for p in (tmp_path / "o").rglob("dro*.json") if p.name != "dro_result.json"]
    assert tables, list((tmp_path / "o").rglob("*"))
    for p in tables:
        _check_doc(json.loads(p.read_text()), "subject-class")
