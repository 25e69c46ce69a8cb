"""GPU tier: the supervised contrastive term (include/msig_sc.h) through every layer — msig_sc_apply[_multi]
against the fp64 restatement (tests/sc_reference.py), what a launch may and may not write, the planted check; NULL and weight 0 are
the plain step bit for bit; the train step against the CPU oracle differentiated through CE + w L; launch counts; folds equal their
single calls; the embedded model's padding; the engine's refusals; the drivers."""
import ctypes as C
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sc_reference as R
from conftest import load_golden_model
from gpu_common import FIXED_TOL, GRAD_FLOOR, K_GRAD, grad_tol, narrow_train_step, rel_err, split_named, to_t
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd.adversary import SubjectAdversary
from multimodalsignal_amd.runtime import EmbeddedEngine, Engine, FoldArena
from multimodalsignal_amd.sam import Sam
from multimodalsignal_amd.supcon import SupCon
from oracle import cnn_gru_oracle as O

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 97, 257, 2048)      # below, at and across the 32-row and 64-column tile edges, and the limit
MARGIN = 1e-4                                               # N_a and the top-1 count are compared on inputs whose margin exceeds it


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def apply(dev, f, y, table, idx, K, tau, positives, weight=1.0, dfeat=None, stats=None):
    """One msig_sc_apply; returns (dfeat, stats) as CPU tensors.  table None: class mode without a subject table."""
    B = f.shape[0]
    ft, yt = torch.as_tensor(f).to(dev), torch.as_tensor(y).to(dev)
    d = torch.zeros(B, 128, device=dev) if dfeat is None else torch.as_tensor(dfeat).to(dev).clone()
    st = torch.zeros(L.SC_STATS, dtype=torch.float64, device=dev) if stats is None else torch.as_tensor(stats).to(dev).clone()
    scratch = torch.empty(L.lib().msig_sc_scratch_bytes(B), dtype=torch.uint8, device=dev)
    tt = None if table is None else torch.as_tensor(table).to(dev)
    it = None if idx is None else torch.as_tensor(idx).to(dev)
    sc = L.Sc()
    sc.positives, sc.tau = L.SC_POSITIVES[positives], tau
    sc.grp, sc.idx = (None if tt is None else tt.data_ptr()), (None if it is None else it.data_ptr())
    sc.scratch, sc.stats = scratch.data_ptr(), st.data_ptr()
    sc.weight[0] = weight
    L.check(L.lib().msig_sc_apply(C.byref(sc), ft.data_ptr(), yt.data_ptr(), d.data_ptr(), B, K, None), "msig_sc_apply")
    torch.cuda.synchronize()
    return d.cpu(), st.cpu()


def case_with_margin(B, K, tau, positives, use_idx, base_seed):
    """The first of the seeds base_seed, base_seed + 1, ... that has an anchor (B = 1 cannot) and whose fp64 top-1 margin exceeds MARGIN
    (a near-tie between the best positive and the best negative of one anchor is a discrete decision no fp32 implementation has to
    share)."""
    for seed in range(base_seed, base_seed + 50):
        f, y, table, idx = R.make_case(B, K, seed)
        if not use_idx:
            idx = None
        g = table[idx] if idx is not None else table[:B]
        ref = R.restatement(f, y, g, K, tau, positives)
        if ref[4] > MARGIN and (B == 1 or ref[3] > 0):
            return f, y, table, idx, g, ref
    raise AssertionError("no seed with an anchor and a top-1 margin above the bound")


@pytest.mark.parametrize("positives", ["class", "cross-subject"])
@pytest.mark.parametrize("B", SIZES)
def test_apply_matches_the_fp64_restatement(dev, B, positives):
    for tau in (0.1, 0.5):
        for K in (2, 3):
            for use_idx in (True, False):
                f, y, table, idx, g, (L64, df64, st64, na, _) = case_with_margin(B, K, tau, positives, use_idx, 1000 * B + 10 * K)
                L32, df32, _, _, _ = R.restatement(f, y, g, K, tau, positives, torch.float32)
                canary = np.full(4, 7.5)
                d, st = apply(dev, f, y, table, idx, K, tau, positives, stats=canary)
                tag = f"B={B} {positives} tau={tau} K={K} idx={use_idx}"
                if na == 0:
                    assert not d.any() and np.array_equal(st.numpy(), canary), tag
                    continue
                own = rel_err(df32.numpy(), df64.numpy())
                err = rel_err(d.numpy(), df64.numpy())
                tol = max(GRAD_FLOOR, K_GRAD * own)
                own_l = abs(L32 - L64) / max(abs(L64), 1e-6)
                got = st.numpy() - canary
                err_l = abs(got[0] / got[1] - L64) / max(abs(L64), 1e-6)
                print(f"{tag}: df err {err:.3e} own {own:.3e} tol {tol:.1e}; L err {err_l:.3e} own {own_l:.3e}; N_a {na}")
                assert err <= tol, tag
                assert err_l <= max(FIXED_TOL["loss"], K_GRAD * own_l), tag
                assert got[1] == st64[1] and got[2] == st64[2] and got[3] == 1.0, (tag, got, st64)


@pytest.mark.parametrize("B", [1, 17, 2048])
def test_a_launch_with_no_anchor_writes_nothing(dev, B):
    f, _, table, idx = R.make_case(B, 3, B)
    rs = np.random.RandomState(B)
    d0 = rs.randn(B, 128).astype(np.float32)
    canary = np.array([1.5, 2.5, 3.5, 4.5])
    cases = [("class", np.arange(B, dtype=np.int64) % 16, 16 if B <= 16 else None),        # every row a class of its own
             ("class", np.full(B, -1, dtype=np.int64), 3),                                   # no valid row
             ("cross-subject", np.zeros(B, dtype=np.int64), 3)]                              # one class, one subject
    for positives, y, K in cases:
        if K is None:
            continue
        tbl = np.zeros_like(table) if positives == "cross-subject" else table
        d, st = apply(dev, f, y, tbl, idx, K, 0.1, positives, weight=0.5, dfeat=d0, stats=canary)
        assert np.array_equal(d.numpy().view(np.uint32), d0.view(np.uint32)) and np.array_equal(st.numpy(), canary), (positives, B)


def test_zero_weight_is_a_probe_and_the_add_has_two_roundings(dev):
    B, K = 97, 3
    f, y, table, idx = R.make_case(B, K, 5)
    d0 = np.random.RandomState(1).randn(B, 128).astype(np.float32)
    d, st = apply(dev, f, y, table, idx, K, 0.1, "cross-subject", weight=0.0, dfeat=d0)
    assert np.array_equal(d.numpy().view(np.uint32), d0.view(np.uint32))
    df, st1 = apply(dev, f, y, table, idx, K, 0.1, "cross-subject", weight=1.0)
    assert st[1] > 0 and torch.equal(st, st1)
    w = np.float32(0.3)
    d, _ = apply(dev, f, y, table, idx, K, 0.1, "cross-subject", weight=float(w), dfeat=d0)
    assert np.array_equal(d.numpy(), d0 + w * df.numpy())            # numpy rounds the product, then the sum


def test_apply_multi_is_the_single_calls_and_leaves_the_other_slot_alone(dev):
    B, K, n_slots, stride = 65, 3, 3, 1 << 17
    model = torch.zeros(n_slots, stride, dtype=torch.uint8, device=dev)       # per slot: feat, dfeat, labels
    side = torch.zeros(n_slots, stride, dtype=torch.uint8, device=dev)        # per slot: grp, scratch, stats
    o_f, o_d, o_y = 0, B * 512, 2 * B * 512
    positions = 2 * B
    o_g, o_s, o_st = 0, 1024, 1024 + L.lib().msig_sc_scratch_bytes(B)
    assert o_st + 32 <= stride and positions * 4 <= 1024
    folds = {0: R.make_case(B, K, 11, positions=positions), 2: R.make_case(B, K, 12, positions=positions)}
    d0 = np.random.RandomState(3).randn(n_slots, B, 128).astype(np.float32)
    idx_rows = torch.zeros(2, B + 7, dtype=torch.int64, device=dev)
    weights = {0: 0.25, 2: 1.5}
    for z, slot in enumerate((2, 0)):                                          # launch order differs from slot order
        f, y, table, idx = folds[slot]
        model[slot, o_f:o_f + B * 512].view(torch.float32).copy_(torch.as_tensor(f).flatten())
        model[slot, o_y:o_y + B * 8].view(torch.int64).copy_(torch.as_tensor(y))
        side[slot, o_g:o_g + positions * 4].view(torch.int32).copy_(torch.as_tensor(table))
        idx_rows[z, :B].copy_(torch.as_tensor(idx))
    for slot in range(n_slots):
        model[slot, o_d:o_d + B * 512].view(torch.float32).copy_(torch.as_tensor(d0[slot]).flatten())
    side[1].fill_(0xAB)
    before1 = (model[1].clone(), side[1].clone())
    m = L.Multi()
    m.n, m.stride_bytes = 2, stride
    m.slot[0], m.slot[1] = 2, 0
    sc = L.Sc()
    sc.positives, sc.tau = 1, 0.2
    base = side.data_ptr()
    sc.grp, sc.scratch, sc.stats, sc.stride_bytes = base + o_g, base + o_s, base + o_st, stride
    sc.idx, sc.idx_row_stride = idx_rows.data_ptr(), B + 7
    sc.weight[0], sc.weight[1] = weights[2], weights[0]
    mb = model.data_ptr()
    L.check(L.lib().msig_sc_apply_multi(C.byref(sc), C.byref(m), mb + o_f, mb + o_y, mb + o_d, B, K, None), "msig_sc_apply_multi")
    torch.cuda.synchronize()
    assert torch.equal(model[1], before1[0]) and torch.equal(side[1], before1[1])
    for slot in (0, 2):
        f, y, table, idx = folds[slot]
        d, st = apply(dev, f, y, table, idx, K, 0.2, "cross-subject", weight=weights[slot], dfeat=d0[slot])
        got = model[slot, o_d:o_d + B * 512].view(torch.float32).view(B, 128).cpu()
        assert torch.equal(got.view(torch.int32), d.view(torch.int32)), slot
        assert torch.equal(side[slot, o_st:o_st + 32].view(torch.float64).cpu(), st), slot


def test_descent_through_apply_lowers_the_loss_and_raises_top1(dev):
    """Planted check: 50 steps of gradient descent on free features through msig_sc_apply."""
    B, K = 96, 3
    f, y, table, idx = R.make_case(B, K, 21, invalid=0.0)
    f = torch.as_tensor(f)
    first = last = None
    for step in range(50):
        d, st = apply(dev, f.numpy(), y, table, idx, K, 0.2, "cross-subject")
        cur = (float(st[0] / st[1]), float(st[2] / st[1]))
        first = first or cur
        last = cur
        f = f - 2.0 * d
    print("planted:", first, "->", last)
    assert last[0] < first[0] - 0.1 and last[1] > first[1]


# ---- the train steps ------------------------------------------------------------------------------------------------------------
DEV = torch.device("cuda", 0)
ATT, CG = "cnn_gru_attention", "cnn_gru"
LR, WD, ADAM_EPS = 1e-3, 1e-4, 1e-3
STATE = ("params", "grads", "exp_avg", "exp_avg_sq", "bn_state")


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _dev(a):
    return torch.as_tensor(a).to(DEV)


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


def _supcon(weight, table=None, tau=0.1, positives="cross-subject", max_batch=64):
    sc = SupCon(weight, tau, positives)
    if table is not None:
        sc.set_subjects(table)
    return sc.bind(DEV, max_batch=max_batch)


def _same_state(a, b):
    return all(torch.equal(_bits(getattr(a, n)), _bits(getattr(b, n))) for n in STATE) and torch.equal(a.loss_acc, b.loss_acc) \
        and torch.equal(_bits(a.region("LOSS", torch.float32, (3,))), _bits(b.region("LOSS", torch.float32, (3,))))


@pytest.mark.parametrize("with_sam", [False, True], ids=["plain", "sam"])
@pytest.mark.parametrize("model", [(ATT, 64, 2), (CG, 64, 2), (ATT, 32, 1)], ids=["attention", "cnn_gru", "embedded"])
def test_null_and_zero_weight_are_the_plain_step_bit_for_bit(model, with_sam):
    """Three steps with eps = 0.1, clip and dropout: the narrower entry point without the option called directly (msig_da_train_step, or msig_sam_train_step
    with sam), msig_sc_train_step with a NULL msig_sc
    and the term at weight 0 leave the same parameters, gradients, moments, BatchNorm state and losses; the NULL call makes the same
    launches, the probe two more per pass and fills its statistics; weight 0.5 does change the model."""
    kind, hidden, layers = model
    Cc, K, B, T = 3, 2, 21, 512
    sam = Sam(0.05) if with_sam else None
    table = (np.arange(B) % 3).astype(np.int32)
    engines, launches = {}, {}
    for mode in ("plain", "null", "probe", "on"):
        e = _engine(Cc, K, hidden, layers, kind)
        sc = {"plain": None, "null": None, "probe": _supcon(0.0, table), "on": _supcon(0.5, table)}[mode]
        for s in (1, 2, 3):
            x, y = _data(B, Cc, K, T, 10 + s)
            if s == 3:
                L.profile_enable(True)
            try:
                if mode == "null":                               # the entry point itself with a NULL msig_sc
                    if layers == 1:
                        e.scatter()
                    e.ensure_adam_state()
                    b = e._batch(x, y, True, 0.5, 7, s)
                    cw, mn, sm, lam = e._checked(None, 1.0, 0.1, None)
                    sd = None
                    if sam is not None:
                        state = e.ensure_sam_state()
                        sd = C.byref(sam.descriptor(e.kind, state.data_ptr(), state.numel() * 8))
                    L.check(L.lib().msig_sc_train_step(C.byref(b), C.byref(e._st(cw, mn, sm, lam)), None, None, sd, None, None,
                                                       e.exp_avg.data_ptr(), e.exp_avg_sq.data_ptr(), LR, 0.9, 0.999, 1e-8, 1e-4, s, _stream()),
                            "msig_sc_train_step")
                    if layers == 1:
                        e.gather()
                elif mode == "plain":                            # the narrower entry point, called directly (Engine.train_step is msig_sc_train_step)
                    name = narrow_train_step(e, x, y, LR, weight_decay=1e-4, step=s, dropout_p=0.5, seed=7, label_smoothing=0.1, max_grad_norm=1.0,
                                             sam=sam)
                    assert name == ("msig_sam_train_step" if with_sam else "msig_da_train_step")
                else:
                    e.train_step(x, y, LR, weight_decay=1e-4, step=s, dropout_p=0.5, seed=7, label_smoothing=0.1, max_grad_norm=1.0, sam=sam,
                                 supcon=sc)
                torch.cuda.synchronize()
                if s == 3:
                    launches[mode] = {k: v[0] for k, v in L.profile_report().items()}
            finally:
                L.profile_enable(False)
        engines[mode] = (e, sc)
    plain = engines["plain"][0]
    assert _same_state(plain, engines["null"][0]) and launches["null"] == launches["plain"] and "sc_rows" not in launches["plain"]
    assert _same_state(plain, engines["probe"][0])
    passes = 2 if with_sam else 1
    assert launches["probe"] == {**launches["plain"], "sc_rows": passes, "sc_grad": passes}
    for mode in ("probe", "on"):
        st = engines[mode][1].stats.cpu()
        assert float(st[3]) == 3.0 and float(st[1]) > 0 and float(st[0]) > 0, mode        # under sam too: one report per step
    assert not torch.equal(_bits(plain.params), _bits(engines["on"][0].params))
    assert torch.equal(plain.loss_acc[1:], engines["probe"][0].loss_acc[1:])
    if layers == 1:
        e = engines["on"][0]
        assert int(e.grads[e.padding].count_nonzero()) == 0 and int(e.params[e.padding].count_nonzero()) == 0


CASES = [dict(w=None, eps=0.0, clip=None), dict(w=(0.3, 2.5), eps=0.1, clip=0.05)]


def _oracle(params, buffers, x, y, groups, case, w, weight, tau, positives):
    """{dtype: ({key: gradient after the clip}, {key: parameter after Adam's first step})} of CE(logits, y) + weight * L_sc(feat),
    differentiated by autograd through the whole model."""
    out = {}
    K = int(params["classifier.3.bias"].numel())
    for dt in (torch.float64, torch.float32):
        leaf = {k: v.to(dt).clone().requires_grad_(v.numel() > 0) for k, v in params.items()}
        bufs = {k: (v.clone() if "num_batches" in k else v.to(dt)) for k, v in buffers.items()}
        st, _ = O.forward(leaf, bufs, torch.as_tensor(x).to(dt), training=True, dropout_p=0.0, seed=0, step=1)
        wt = None if w is None else torch.tensor(w, dtype=dt)
        loss = F.cross_entropy(st["logits"], torch.as_tensor(y), weight=wt, label_smoothing=case["eps"])
        if weight:
            loss = loss + weight * R.loss_direct(st["feat"], y, groups, K, tau, positives)
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
@pytest.mark.parametrize("layers", [2, 1], ids=["model_c4_k2_t200", "embedded"])
def test_train_step_matches_the_oracle_differentiated_through_ce_plus_the_term(layers, case):
    """One msig_sc_train_step at weight 0.7, tau 0.2, cross-subject positives, B = 8, dropout 0, on the committed parameters (the
    one-layer model: the oracle's initialisation of the same C and K): every parameter gradient and every parameter after Adam
    against autograd of CE + weight * L through the whole model, gated by gpu_common.grad_tol on the fp32 oracle's own error.
    Precondition, from the reference alone: without the term the GRU's gradient differs by far more than the tolerance."""
    meta, params_np, _ = load_golden_model("model_c4_k2_t200")
    Cc, K, T, B = meta["C"], meta["K"], meta["T"], 8
    params, buffers = split_named(to_t(params_np))
    if layers == 1:
        params = O.init_params(Cc, K, seed=3, hidden=32, layers=1)
    for k, v in O.init_buffers().items():
        buffers.setdefault(k, v)
    rs = np.random.RandomState(17)
    x = rs.randn(B, Cc, T).astype(np.float32)
    y = np.array([0, 1, 0, 1, 1, 0, 0, 1], dtype=np.int64)
    groups = [0, 2, 2, -1, 0, 2, 1, 1]
    idx = rs.permutation(B + 9)[:B].astype(np.int64)
    table = np.full(B + 9, 1, np.int32)
    table[idx] = groups
    w = case["w"]
    weight, tau = 0.7, 0.2
    if layers == 1:
        e = EmbeddedEngine(Cc, K, DEV, 32)
        for k, v in e.small_views().items():
            v.copy_(params[k])
    else:
        e = Engine(Cc, K, DEV)
        e.load_named({**params, **buffers})
    sc = _supcon(weight, table, tau)
    e.train_step(_dev(x), _dev(y), LR, eps=ADAM_EPS, weight_decay=WD, step=1, dropout_p=0.0, seed=1,
                 class_weight=None if w is None else torch.tensor(w, dtype=torch.float32, device=DEV), max_grad_norm=case["clip"],
                 label_smoothing=case["eps"], supcon=sc, batch_index=_dev(idx))
    torch.cuda.synchronize()
    assert float(sc.stats[3]) == 1.0 and float(sc.stats[1]) == 7.0
    if layers == 1:
        assert int(e.grads[e.padding].count_nonzero()) == 0 and int(e.params[e.padding].count_nonzero()) == 0
        got_g = {k: v.cpu().numpy().copy() for k, v in e.gather_grads().items()}
        got_p = {k: v.cpu().numpy().copy() for k, v in e.small_views().items()}
    else:
        got_g = {k: v.cpu().numpy() for k, v in e.named_param_views(e.grads).items()}
        got_p = {k: v.cpu().numpy() for k, v in e.named_param_views().items()}
    ref = _oracle(params, buffers, x, y, groups, case, w, weight, tau, "cross-subject")
    (g64, p64), (g32, p32) = ref[torch.float64], ref[torch.float32]
    without = _oracle(params, buffers, x, y, groups, case, w, 0.0, tau, "cross-subject")[torch.float64][0]
    k0 = "gru.weight_ih_l0"
    assert rel_err(without[k0], g64[k0]) > 100 * grad_tol(k0, rel_err(g32[k0], g64[k0]))
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


@pytest.mark.parametrize("B", [21, 2048])
def test_launch_counts(B):
    """By the library's own launch report: the term is the plain step's launches plus sc_rows and sc_grad once each, and the head
    stays fused where it was."""
    Cc, K, T = 3, 2, 64
    x, y = _data(B, Cc, K, T, 4)
    table = (np.arange(B) % 5).astype(np.int32)
    reports = {}
    for mode in ("plain", "supcon"):
        e = _engine(Cc, K)
        sc = _supcon(0.1, table, max_batch=B) if mode == "supcon" else None
        e.train_step(x, y, LR, step=1, dropout_p=0.5, seed=7, supcon=sc)          # workspaces exist before the count starts
        torch.cuda.synchronize()
        L.profile_enable(True)
        try:
            e.train_step(x, y, LR, step=2, dropout_p=0.5, seed=7, supcon=sc)
            torch.cuda.synchronize()
            reports[mode] = {k: v[0] for k, v in L.profile_report().items()}
        finally:
            L.profile_enable(False)
    plain = reports["plain"]
    assert "sc_rows" not in plain
    assert reports["supcon"] == {**plain, "sc_rows": 1, "sc_grad": 1} and sum(reports["supcon"].values()) == sum(plain.values()) + 2
    assert ("head_step" in plain) == ("head_step" in reports["supcon"])


@pytest.mark.parametrize("extra", ["plain", "adversary", "sam"])
def test_train_step_multi_equals_the_single_calls(extra):
    """NF = 3 with per-fold seeds, step counts, learning rates and weights, each fold its own subject table, scratch and statistics in
    the arena's block, idx rows of a shared matrix, two steps: msig_sc_train_step_multi leaves every fold's parameters, gradients,
    moments, BatchNorm state and statistics (and the discriminator's, with the adversary on) with the bits of its
    msig_sc_train_step."""
    n, B, T, Cc, K, S, npos = 3, 21, 512, 3, 2, 4, 60
    msteps, dsteps, lrs, lam_rev, weights = (1, 3, 5), (2, 4, 6), (1e-3, 5e-4, 2e-3), (0.3, 0.5, 1.0), (0.1, 0.0, 0.7)
    rs = np.random.RandomState(8)
    data = [[_data(B, Cc, K, T, 300 + 10 * f + s) for s in range(2)] for f in range(n)]
    tables = [rs.randint(-1, 4, size=npos).astype(np.int32) for _ in range(n)]
    doms = [rs.randint(-1, S, size=npos).astype(np.int32) for _ in range(n)]
    idx = _dev(rs.randint(0, npos, size=(n, B + 3)).astype(np.int64))
    sam = Sam(0.05) if extra == "sam" else None
    arena = FoldArena(Cc, K, DEV, n, B, T, adversary=(S, npos) if extra == "adversary" else None, grad_clip=True, sam=sam is not None,
                      supcon=npos)
    plain_arena = FoldArena(Cc, K, DEV, n, B, T, adversary=(S, npos) if extra == "adversary" else None, grad_clip=True, sam=sam is not None)
    assert (arena.stride, arena.off) == (plain_arena.stride, plain_arena.off)       # the model arenas are what they are without the term
    del plain_arena
    engs = [_engine(Cc, K, seed=10 + f, storage_engine=arena.engine(f)) for f in range(n)]
    scs, advs = [], []
    for f in range(n):
        scs.append(SupCon(weights[f], 0.2, "cross-subject").set_subjects(tables[f]).bind(DEV, arena.side_storage("supcon", f)))
        if extra == "adversary":
            adv = SubjectAdversary(S, lam=lam_rev[f], schedule="constant", seed=40 + f)
            adv.set_domains(doms[f])
            advs.append(adv.bind(DEV, arena.side_storage("adversary", f)))
        arena.set_max_norm(f, 1.0)
    slots = list(range(n))
    desc = arena.batch(B, True, 0.5)
    sd = arena.soft(slots, 0.1, None, clip=arena.clip(slots))
    for s in range(2):
        for f in range(n):
            x, y = data[f][s]
            arena.view(f, "x", torch.float32)[:x.numel()].copy_(x.reshape(-1))
            arena.view(f, "y", torch.int64)[:B].copy_(y)
        st = [msteps[f] + s for f in slots]
        m = arena.multi(slots, key_gru=[L.dropout_key(100 + f, st[f], 1) for f in slots], key_head=[L.dropout_key(100 + f, st[f], 2) for f in slots],
                        lr=lrs, steps=st)
        cd = arena.sc("cross-subject", 0.2, weights)
        cd.idx, cd.idx_row_stride = idx.data_ptr(), B + 3
        a = None
        if extra == "adversary":
            a = arena.da(slots, S, lam_rev, lrs, [dsteps[f] + s for f in slots], (0.9, 0.999), 1e-8, 1e-4)
            a.idx, a.idx_row_stride = idx.data_ptr(), B + 3
        L.check(L.lib().msig_sc_train_step_multi(C.byref(desc), C.byref(m), C.byref(sd), None if a is None else C.byref(a), None,
                                                 None if sam is None else C.byref(arena.sam(sam)), None, C.byref(cd), arena.ptr("exp_avg"),
                                                 arena.ptr("exp_avg_sq"), 0.9, 0.999, 1e-8, 1e-4, st[0], _stream()), "msig_sc_train_step_multi")
        torch.cuda.synchronize()
    for f in range(n):
        e = _engine(Cc, K, seed=10 + f)
        sc = _supcon(weights[f], tables[f], 0.2)
        adv = None
        if extra == "adversary":
            adv = SubjectAdversary(S, lam=lam_rev[f], schedule="constant", seed=40 + f)
            adv.set_domains(doms[f])
            adv.step = dsteps[f] - 1
            adv.bind(DEV)
        for s in range(2):
            x, y = data[f][s]
            e.train_step(x, y, lrs[f], weight_decay=1e-4, step=msteps[f] + s, dropout_p=0.5, seed=100 + f, label_smoothing=0.1,
                         max_grad_norm=1.0, adversary=adv, sam=sam, supcon=sc, batch_index=idx[f, :B].contiguous())
        torch.cuda.synchronize()
        for name in STATE:
            assert torch.equal(_bits(getattr(e, name)), _bits(getattr(engs[f], name))), (f, name)
        assert torch.equal(sc.stats, scs[f].stats) and float(sc.stats[3]) == 2.0 and float(sc.stats[1]) > 0, f
        if extra == "adversary":
            for name in ("params", "exp_avg", "exp_avg_sq"):
                assert torch.equal(_bits(getattr(adv, name)), _bits(getattr(advs[f], name))), (f, name)
    assert torch.equal(arena.side_stats("supcon").cpu(), torch.stack([s.stats.cpu() for s in scs]))


def test_embedded_fold_batch_keeps_its_padding_zero_and_equals_the_single_calls():
    n, B, T, Cc, K, npos, steps = 2, 21, 512, 3, 2, 50, 3
    rs = np.random.RandomState(4)
    data = [[_data(B, Cc, K, T, 500 + 10 * f + s) for s in range(steps)] for f in range(n)]
    tables = [rs.randint(-1, 4, size=npos).astype(np.int32) for _ in range(n)]
    idx = _dev(rs.randint(0, npos, size=(n, B)).astype(np.int64))
    arena = FoldArena(Cc, K, DEV, n, B, T, gru_hidden=32, gru_layers=1, supcon=npos)
    engs = [_engine(Cc, K, 32, 1, seed=10 + f, storage_engine=arena.engine(f)) for f in range(n)]
    scs = [SupCon(0.5, 0.1, "cross-subject").set_subjects(tables[f]).bind(DEV, arena.side_storage("supcon", f)) for f in range(n)]
    slots = list(range(n))
    sd = arena.soft(slots, 0.0)
    desc = arena.batch(B, True, 0.5)
    off = L.workspace_layout(B, Cc, T, K, True)
    for s in range(1, steps + 1):
        for f in range(n):
            x, y = data[f][s - 1]
            arena.view(f, "x", torch.float32)[:x.numel()].copy_(x.reshape(-1))
            arena.view(f, "y", torch.int64)[:B].copy_(y)
        m = arena.multi(slots, key_gru=[L.dropout_key(100 + f, s, 1) for f in slots], key_head=[L.dropout_key(100 + f, s, 2) for f in slots],
                        lr=[LR] * n, steps=[s] * n)
        cd = arena.sc("cross-subject", 0.1, [0.5] * n)
        cd.idx, cd.idx_row_stride = idx.data_ptr(), B
        L.check(L.lib().msig_sc_train_step_multi(C.byref(desc), C.byref(m), C.byref(sd), None, None, None, None, C.byref(cd), arena.ptr("exp_avg"),
                                                 arena.ptr("exp_avg_sq"), 0.9, 0.999, 1e-8, 1e-4, s, _stream()), "msig_sc_train_step_multi")
    torch.cuda.synchronize()
    dfeat = arena.across("ws", off[L.WS["DFEAT"]], torch.float32, B * 128).view(n, B, 128)
    pad_cols = np.r_[32:64, 96:128]
    assert int(dfeat[:, :, pad_cols].count_nonzero()) == 0 and int(dfeat.count_nonzero()) > 0
    for f in range(n):
        pad = engs[f].padding
        for name in ("params", "grads", "exp_avg", "exp_avg_sq"):
            assert int(getattr(engs[f], name)[pad].count_nonzero()) == 0, (f, name)
        e, sc = _engine(Cc, K, 32, 1, seed=10 + f), _supcon(0.5, tables[f])
        for s in range(1, steps + 1):
            x, y = data[f][s - 1]
            e.train_step(x, y, LR, weight_decay=1e-4, step=s, dropout_p=0.5, seed=100 + f, supcon=sc, batch_index=idx[f].contiguous())
        torch.cuda.synchronize()
        for name in STATE:
            assert torch.equal(_bits(getattr(e, name)), _bits(getattr(engs[f], name))), (f, name)
        assert torch.equal(sc.stats, scs[f].stats) and float(sc.stats[1]) > 0


def test_mixup_and_oversized_batches_are_refused_by_the_engine_before_any_launch():
    Cc, K, T = 3, 2, 64
    e = _engine(Cc, K)
    before = e.params.clone()
    x, y = _data(8, Cc, K, T, 1)
    with pytest.raises(ValueError, match="mixup"):
        e.train_step(x, y, LR, step=1, mix_lambda=0.4, supcon=_supcon(0.1, positives="class"))
    x, y = _data(2049, Cc, K, T, 1)
    with pytest.raises(ValueError, match="at most 2048"):
        e.train_step(x, y, LR, step=1, supcon=_supcon(0.1, positives="class", max_batch=2048))
    assert torch.equal(e.params, before) and e.exp_avg is None


# ---- drivers ----------------------------------------------------------------------------------------------------------------------
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


def _check_doc(doc, positives):
    assert doc["folds"] and doc["settings"]["positives"] == positives and doc["synthetic"] is True
    for f in doc["folds"]:
        assert f["supcon_loss"] > 0 and 0.0 <= f["supcon_top1"] <= 1.0 and 0 < f["supcon_anchors"] <= 16 and f["epochs"] >= 1
    assert doc["pooled"]["supcon_loss"] > 0


def test_fold_batches_equal_sequential_folds_and_the_report_is_well_formed(tmp_path):
    from multimodalsignal_amd import main as M
    flags = ["--supcon", "0.1", "--supcon-positives", "cross-subject", "--label-smoothing", "0.1"]
    runs = {}
    for tag, extra in (("lock", flags), ("seq", flags + ["--no-lockstep"]), ("plain", ["--label-smoothing", "0.1"])):
        M.main(_common(tmp_path) + extra + ["--out", str(tmp_path / tag)])
        run = next((tmp_path / tag).glob("*/run_*"))
        txt = (run / "cv_summary.txt").read_text(encoding="utf-8")
        assert ("SUPCON: weight=0.1 tau=0.1 positives=cross-subject" in txt) == (tag != "plain")
        assert (run / "supcon.json").exists() == (run / "supcon.txt").exists() == (tag != "plain")
        runs[tag] = (_fold_outputs(run), run)
    for (ia, wa), (ib, wb) in zip(runs["lock"][0], runs["seq"][0]):
        assert ia == ib
        assert list(wa) == list(wb) and all(torch.equal(wa[k], wb[k]) for k in wa)
    keys = ("supcon_loss", "supcon_top1", "supcon_anchors")
    assert all(k in h for f, _ in runs["lock"][0] for h in f["history"] for k in keys)
    assert all(not any(k.startswith("supcon") for k in h) for f, _ in runs["plain"][0] for h in f["history"])
    assert all("supcon" not in f for f, _ in runs["plain"][0])
    assert any(not torch.equal(a[1][k], p[1][k]) for a, p in zip(runs["lock"][0], runs["plain"][0]) for k in a[1])
    doc = json.loads((runs["lock"][1] / "supcon.json").read_text())
    assert doc == json.loads((runs["seq"][1] / "supcon.json").read_text())
    assert [f["subject"] for f in doc["folds"]] == SUBS and doc["probe"] is False
    _check_doc(doc, "cross-subject")
    assert "say nothing about WESAD accuracy" in (runs["lock"][1] / "supcon.txt").read_text(encoding="utf-8")
    assert "supcon loss" in (runs["lock"][1] / "fold_test_on_S2" / "training_log.txt").read_text(encoding="utf-8")


@pytest.mark.parametrize("mode", [["--ablation"], ["--hierarchical"], ["--model", "cnn_gru_attention", "cnn_gru"],
                                  ["--hierarchical", "--concurrent-folds", "1"], ["--seeds", "2"], ["--seeds", "2", "--distill"],
                                  ["--sam", "0.05", "--weight-average", "ema"]],
                         ids=["ablation", "hierarchical", "model", "hierarchical-sequential", "seeds", "distill", "sam-ema"])
def test_every_driver_mode_runs_with_supcon(tmp_path, mode):
    from multimodalsignal_amd import main as M
    M.main(_common(tmp_path) + ["--supcon", "0.1", "--max-grad-norm", "1.0"] + mode + ["--out", str(tmp_path / "o")])
    summaries = [p for p in (tmp_path / "o").rglob("*summary.txt")]
    assert summaries and all("SUPCON: weight=0.1 tau=0.1 positives=class" in p.read_text(encoding="utf-8") for p in summaries), summaries
    tables = [p for p in (tmp_path / "o").rglob("supcon*.json") if p.name != "supcon_result.json"]
    assert tables, list((tmp_path / "o").rglob("*"))
    for p in tables:
        _check_doc(json.loads(p.read_text()), "class")
