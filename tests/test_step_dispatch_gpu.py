"""GPU tier: the property the host's single dispatch rests on.  Engine.train_step always issues msig_sc_train_step, Engine.forward
msig_st_forward, the lockstep trainer msig_sc_train_step_multi / msig_st_forward_multi, the loaders msig_st_gather_windows whenever
they augment or mix.  Here the bits of each of those widest calls, with a feature off, are held to the bits of the entry point that
the feature's header names as its counterpart, called directly on the library; and with ONE optional term on (adversary,
distillation, SAM, group-DRO) to the bits of the narrowest entry point whose signature has that term — msig_da_, msig_kd_, msig_sam_,
msig_dro_train_step[_multi] — given the same descriptors.  Every comparison is torch.equal: no tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_common import legacy_forward, legacy_train_step, narrow_train_step
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd.adversary import SubjectAdversary
from multimodalsignal_amd.augment import Augment
from multimodalsignal_amd.dataset import DeviceLoader
from multimodalsignal_amd.distill import Distillation
from multimodalsignal_amd.dro import GroupDro
from multimodalsignal_amd.mixup import Mixup
from multimodalsignal_amd.runtime import EmbeddedEngine, Engine, FoldArena
from multimodalsignal_amd.sam import Sam
from multimodalsignal_amd.supcon import SupCon
from oracle import cnn_gru_oracle as O
from test_soft_targets_gpu import AUG_ON, _gather

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CC, K, T, P, SEED, LR, WD = 3, 2, 64, 0.5, 7, 1e-3, 1e-4
W = (0.3, 2.5)
# B = 8: the one-launch head (head.hip head_step_applies: at most 128 groups of 16 rows); B = 2064, 129 groups: the separate head and ce_kernel
CONFIGS = [("full", 8), ("full", 2064), ("cnn_gru", 8), ("embedded", 8)]


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def _data(B, seed=1):
    rs = np.random.RandomState(seed)
    y = rs.randint(0, K, size=B).astype(np.int64)
    y[:min(K, B)] = np.arange(min(K, B))
    return torch.as_tensor(rs.randn(B, CC, T).astype(np.float32)).to(DEV), torch.as_tensor(y).to(DEV)


def _engine(config, seed=3, storage_engine=None):
    """config: "full" (attention model, 64 x 2), "embedded" (attention model, 32 x 1) or "cnn_gru" (the baseline, 64 x 2)."""
    hidden, layers = (32, 1) if config == "embedded" else (64, 2)
    kind = "cnn_gru" if config == "cnn_gru" else "cnn_gru_attention"
    params = O.init_params(CC, K, seed=seed, hidden=hidden, layers=layers)
    if kind == "cnn_gru":
        params = {k: v for k, v in params.items() if k not in L.GATE_KEYS}
    e = storage_engine
    if e is None:
        e = EmbeddedEngine(CC, K, DEV, hidden) if layers == 1 else Engine(CC, K, DEV, kind=kind)
    if layers == 1:
        for k, v in e.small_views().items():
            v.copy_(params[k])
    else:
        e.load_named(params)
    return e


def _gc_train_step(e, x, y, step, max_norm):
    """msig_gc_train_step itself, with EmbeddedEngine's scatter / gather around it."""
    if hasattr(e, "scatter"):
        e.scatter()
    e.ensure_adam_state()
    b, state = e._batch(x, y, True, P, SEED, step), e.ensure_gc_state()
    g = L.GcClip()
    g.kind, g.class_weight, g.state, g.state_bytes = L.GC_KINDS[e.kind], None, state.data_ptr(), state.numel() * 8
    g.max_norm[0] = max_norm
    L.check(L.lib().msig_gc_train_step(C.byref(b), C.byref(g), e.exp_avg.data_ptr(), e.exp_avg_sq.data_ptr(), LR, 0.9, 0.999, 1e-8, WD, step,
                                       e._stream()), "msig_gc_train_step")
    if hasattr(e, "gather"):
        e.gather()


def _assert_same_model(a, b, what):
    for name in ("params", "exp_avg", "exp_avg_sq", "bn_state", "loss_acc"):
        assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), (what, name)
    assert torch.equal(_bits(a.region("LOSS", torch.float32, (3,))), _bits(b.region("LOSS", torch.float32, (3,)))), (what, "LOSS")
    if isinstance(a, EmbeddedEngine):
        assert torch.equal(_bits(a.small), _bits(b.small)), (what, "small")


# ---- one model -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["off", "class_weight", "clip"])
@pytest.mark.parametrize("config,B", CONFIGS)
def test_train_step_has_the_bits_of_the_entry_point_its_header_names(config, B, variant):
    """Three consecutive steps of Engine.train_step against a twin engine driven through msig_train_step (msig_cg_train_step for the
    cnn_gru kind), msig_cw_train_step (a class-weight vector) or msig_gc_train_step (max_grad_norm = 0.5, with its four statistics)."""
    x, y = _data(B)
    cw = torch.tensor(W, dtype=torch.float32, device=DEV) if variant == "class_weight" else None
    mn = 0.5 if variant == "clip" else None
    a, b = _engine(config), _engine(config)
    for s in (1, 2, 3):
        a.train_step(x, y, LR, weight_decay=WD, step=s, dropout_p=P, seed=SEED, class_weight=cw, max_grad_norm=mn)
        if variant == "clip":
            _gc_train_step(b, x, y, s, mn)
        else:
            name = legacy_train_step(b, x, y, LR, weight_decay=WD, step=s, dropout_p=P, seed=SEED, class_weight=cw)
            assert name == ("msig_cg_train_step" if config == "cnn_gru" else "msig_cw_train_step" if cw is not None else "msig_train_step")
    torch.cuda.synchronize()
    _assert_same_model(a, b, (config, B, variant))
    if variant == "clip":
        assert torch.equal(a.gc_state[:L.GC_NSTAT], b.gc_state[:L.GC_NSTAT])
        assert a.grad_stats()["last"] > 0                               # the statistics were written: the clip's launches ran
    else:
        assert a.gc_state is None


S_DOM, G_DRO = 4, 3
TERM_STATE = {"adversary": ("params", "exp_avg", "exp_avg_sq", "stats"), "distill": ("stats",), "dro": ("q", "stats"), "supcon": ("stats",)}
NARROWEST = {"adversary": "msig_da_train_step", "distill": "msig_kd_train_step", "sam": "msig_sam_train_step", "dro": "msig_dro_train_step"}


def _term(name, rows, seed, storage=None):
    """A fresh optional step term over `rows` table entries (read by row, or by the store positions 0 .. rows-1), bound to the device or
    to a fold's side block; the same (name, rows, seed) gives the same initial state."""
    rs = np.random.RandomState(seed)
    if name == "adversary":
        t = SubjectAdversary(S_DOM, lam=0.5, schedule="constant", seed=40 + seed)
        t.set_domains(rs.randint(-1, S_DOM, size=rows).astype(np.int32))
    elif name == "distill":
        q = np.exp(1.5 * rs.randn(rows, K))
        t = Distillation(0.5, 2.0)
        t.set_teacher((q / q.sum(axis=1, keepdims=True)).astype(np.float32))
    elif name == "dro":
        t = GroupDro(0.5).set_groups((np.arange(rows) % G_DRO).astype(np.int32), G_DRO)
    elif name == "supcon":
        t = SupCon(0.5, 0.2, "cross-subject").set_subjects((np.arange(rows) % 3).astype(np.int32))
        return t.bind(DEV, max_batch=rows) if storage is None else t.bind(DEV, storage)
    else:
        return Sam(0.05)
    return t.bind(DEV) if storage is None else t.bind(DEV, storage)


@pytest.mark.parametrize("names", [("adversary",), ("distill",), ("sam",), ("dro",), ("adversary", "distill", "dro", "supcon"),
                                   ("sam", "distill", "dro", "supcon")], ids="+".join)
def test_train_step_with_terms_on_has_the_bits_of_the_narrowest_entry_point(names):
    """Three consecutive steps of Engine.train_step (msig_sc_train_step with NULL for what is off) against a twin engine driven, with
    the same descriptors, through the narrowest entry point whose signature has the term: msig_da_, msig_kd_ (alpha 0.5), msig_sam_
    (rho 0.05), msig_dro_train_step; the widest combinations (adversary or SAM + distillation + group-DRO + supcon) against
    msig_sc_train_step called directly, which guards the argument plumbing.  Dropout 0.5, smoothing 0.1, the clip on.  B = 8: the head
    fuses wherever the terms allow it.  The adversary, the one term of the four that leaves the head fused, would also run at B = 2064
    (129 head groups: the separate head and ce_kernel), but MSIG_DA_MAX_BATCH (256, asserted) admits no batch above 2048 windows, so
    B = 8 is its only row."""
    assert L.DA_MAX_BATCH <= 2048
    B = 8
    x, y = _data(B)
    a, b = _engine("full"), _engine("full")
    ta, tb = ({n: _term(n, B, 5) for n in names} for _ in range(2))
    kw = dict(weight_decay=WD, dropout_p=P, seed=SEED, label_smoothing=0.1, max_grad_norm=0.5)
    for s in (1, 2, 3):
        a.train_step(x, y, LR, step=s, **kw, **ta)
        assert narrow_train_step(b, x, y, LR, step=s, **kw, **tb) == (NARROWEST[names[0]] if len(names) == 1 else "msig_sc_train_step")
    torch.cuda.synchronize()
    _assert_same_model(a, b, names)
    assert torch.equal(_bits(a.grads), _bits(b.grads))
    assert torch.equal(a.gc_state[:L.GC_NSTAT], b.gc_state[:L.GC_NSTAT]) and a.grad_stats()["last"] > 0
    if "sam" in names:
        assert torch.equal(a.sam_state[:L.SAM_NSTAT], b.sam_state[:L.SAM_NSTAT]) and float(a.sam_state[L.SAM_STEPS]) == 3.0
    else:
        assert a.sam_state is None and b.sam_state is None
    for n in names:
        for field in TERM_STATE.get(n, ()):
            assert torch.equal(_bits(getattr(ta[n], field)), _bits(getattr(tb[n], field))), (names, n, field)
        if n != "sam":
            assert ta[n].stats.any(), (names, n)                           # the term ran: its statistics were written
    if "adversary" in names:
        assert ta["adversary"].step == tb["adversary"].step == 3


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("config,B", CONFIGS)
def test_eval_forward_has_the_bits_of_the_entry_point_its_header_names(config, B, weighted):
    """Engine.forward in eval mode against msig_forward / msig_cw_forward (msig_cg_forward for the cnn_gru kind): LOGITS, PRED, loss_acc."""
    x, y = _data(B, seed=2)
    cw = torch.tensor(W, dtype=torch.float32, device=DEV) if weighted else None
    a, b = _engine(config), _engine(config)
    a.forward(x, y, training=False, class_weight=cw)
    name = legacy_forward(b, x, y, class_weight=cw)
    assert name == ("msig_cg_forward" if config == "cnn_gru" else "msig_cw_forward" if weighted else "msig_forward")
    torch.cuda.synchronize()
    assert torch.equal(_bits(a.region("LOGITS", torch.float32, (B, K))), _bits(b.region("LOGITS", torch.float32, (B, K))))
    assert torch.equal(a.region("PRED", torch.int32, (B,)), b.region("PRED", torch.int32, (B,)))
    assert torch.equal(a.loss_acc, b.loss_acc) and float(a.loss_acc[0]) > 0


# ---- a fold batch --------------------------------------------------------------------------------------------------------------------
def _arena_run(widest, term=None):
    """Three folds (own weights, own dropout keys) in one FoldArena of batch 8; two steps, each a launch over folds {0, 1, 2} at B = 8
    and a ragged launch over folds {0, 1} at B = 5.  widest: msig_sc_train_step_multi built as LockstepTrainer._train_epoch builds it
    (FoldArena.soft, NULL for every term that is off, idx rows of an order matrix); else, with everything off, msig_train_step_multi,
    and with `term` on ("adversary", "distill", "sam", "dro") the narrowest *_multi entry point whose signature has it."""
    n, B = 3, 8
    arena = FoldArena(CC, K, DEV, n, B, T, adversary=(S_DOM, B) if term == "adversary" else None, distill=B if term == "distill" else None,
                      sam=term == "sam", dro=(G_DRO, B) if term == "dro" else None)
    for f in range(n):
        _engine("full", seed=10 + f, storage_engine=arena.engine(f))
        if term in TERM_STATE:
            _term(term, B, 20 + f, arena.side_storage(term, f))
    order = torch.arange(B, dtype=torch.int64, device=DEV).repeat(n, 1).contiguous()      # store positions: row r of fold f reads entry r
    lib, st = L.lib(), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    ea, eas, count = arena.ptr("exp_avg"), arena.ptr("exp_avg_sq"), 0
    for s in (1, 2):
        for slots, b in (([0, 1, 2], B), ([0, 1], 5)):
            count += 1
            for f in slots:
                x, y = _data(b, seed=100 * f + count)
                arena.view(f, "x", torch.float32)[:x.numel()].copy_(x.reshape(-1))
                arena.view(f, "y", torch.int64)[:b].copy_(y)
            m = arena.multi(slots, key_gru=[L.dropout_key(100 + f, count, 1) for f in slots],
                            key_head=[L.dropout_key(100 + f, count, 2) for f in slots], lr=[LR] * len(slots), steps=[count] * len(slots))
            desc = arena.batch(b, True, P)
            sd = arena.soft(slots, 0.0, None, None, None)
            d = {"adversary": lambda: arena.da(slots, S_DOM, [0.5] * len(slots), [LR] * len(slots), [count] * len(slots), (0.9, 0.999), 1e-8, WD),
                 "distill": lambda: arena.kd(0.5, 2.0), "sam": lambda: arena.sam(Sam(0.05)), "dro": lambda: arena.dro(0.5), None: lambda: None}[term]()
            if term in TERM_STATE:
                d.idx, d.idx_row_stride = order.data_ptr(), B
            ref, tail = (None if d is None else C.byref(d)), (ea, eas, 0.9, 0.999, 1e-8, WD, count, st)
            if widest:
                terms = [ref if term == t else None for t in ("adversary", "distill", "sam", "dro", "supcon")]
                rc = lib.msig_sc_train_step_multi(C.byref(desc), C.byref(m), C.byref(sd), *terms, *tail)
            elif term is None:
                rc = lib.msig_train_step_multi(C.byref(desc), C.byref(m), *tail)
            elif term == "adversary":
                rc = lib.msig_da_train_step_multi(C.byref(desc), C.byref(m), C.byref(sd), ref, *tail)
            elif term == "distill":
                rc = lib.msig_kd_train_step_multi(C.byref(desc), C.byref(m), C.byref(sd), None, ref, *tail)
            elif term == "sam":
                rc = lib.msig_sam_train_step_multi(C.byref(desc), C.byref(m), C.byref(sd), None, ref, *tail)
            else:
                rc = lib.msig_dro_train_step_multi(C.byref(desc), C.byref(m), C.byref(sd), None, None, None, ref, *tail)
            L.check(rc, "train_step_multi")
    torch.cuda.synchronize()
    return arena


def test_fold_batch_has_the_bits_of_msig_train_step_multi():
    a, b = _arena_run(True), _arena_run(False)
    assert a.stride == b.stride
    for name in ("params", "exp_avg", "exp_avg_sq", "bn_state", "acc"):
        o, nb = a.off[name]
        assert torch.equal(a.mem[:, o:o + nb], b.mem[:, o:o + nb]), name
    assert float(a.across("acc", 0, torch.float64, 2)[2, 0]) > 0 and not torch.equal(a.view(0, "params"), a.view(2, "params"))


@pytest.mark.parametrize("term", ["adversary", "distill", "sam", "dro"])
def test_fold_batch_with_a_term_on_has_the_bits_of_the_narrowest_multi_entry_point(term):
    """The launch as LockstepTrainer._train_epoch builds it, msig_sc_train_step_multi, against msig_da_, msig_kd_, msig_sam_ and
    msig_dro_train_step_multi with the same descriptor: every arena region compared above, the gradients, and the term's own state —
    its whole side block, or for SAM the arenas' "sam" region."""
    a, b = _arena_run(True, term), _arena_run(False, term)
    assert a.stride == b.stride
    for name in ("params", "grads", "exp_avg", "exp_avg_sq", "bn_state", "acc") + (("sam",) if term == "sam" else ()):
        o, nb = a.off[name]
        assert torch.equal(a.mem[:, o:o + nb], b.mem[:, o:o + nb]), (term, name)
    if term == "sam":
        assert float(a.across("sam", 0, torch.float64, L.SAM_NSTAT)[0, L.SAM_STEPS]) == 4.0 and float(a.across("sam", 0, torch.float64, L.SAM_NSTAT)[2, L.SAM_STEPS]) == 2.0
    else:
        assert torch.equal(a.side[term][0].mem, b.side[term][0].mem) and a.side[term][0].stride == b.side[term][0].stride
        assert a.side_stats(term)[2].any()                                  # the term ran in every fold: its statistics were written
    assert float(a.across("acc", 0, torch.float64, 2)[2, 0]) > 0


# ---- the loaders ---------------------------------------------------------------------------------------------------------------------
class _Windows:
    """The least a DeviceLoader needs of a dataset."""

    def __init__(self, x, y):
        self.x, self.labels = torch.from_numpy(x).to(DEV), y
        self.y = torch.from_numpy(y).to(DEV)

    def __len__(self):
        return len(self.labels)

    def device_tensors(self, device):
        return self.x, self.y


def test_a_mixing_loader_serves_the_augmented_gathers_bits_when_lam_is_one():
    """Mixup(0.02) draws lam = 1 exactly for batch 1 of seed 5 and a lam below 1 for batch 2 (a stateless draw, asserted): batch 1 is the
    augmented gather of its rows, by test_soft_targets_gpu's helper (whose lam = 1 case that file holds to msig_aug_gather_windows) and
    by msig_aug_gather_windows itself."""
    n, B, Tw, seed = 8, 4, 64, 5
    rs = np.random.RandomState(3)
    x, y = rs.randn(n, CC, Tw).astype(np.float32), rs.randint(0, K, size=n).astype(np.int64)
    mix, aug = Mixup(0.02), dict(AUG_ON)
    assert mix.lam(seed, 1) == 1.0 and mix.lam(seed, 2) < 1.0
    ds = _Windows(x, y)
    ld = DeviceLoader(ds, B, False, DEV, seed=seed, augment=Augment(**aug), mixup=mix)
    it = iter(ld)
    xb, yb = next(it)
    assert ld.last_lam == 1.0 and ld.aug_step == 1
    idx, key = torch.arange(B, dtype=torch.int64, device=DEV), L.dropout_key(seed, 1, L.AUG_STREAM_ID)
    want, want_y = _gather(ds.x, ds.y, idx, B, CC, Tw, 1.0, aug, key)
    assert torch.equal(_bits(xb), _bits(want)) and torch.equal(yb, want_y)
    ref = torch.empty_like(xb)
    L.check(L.lib().msig_aug_gather_windows(ds.x.data_ptr(), ds.y.data_ptr(), idx.data_ptr(), B, CC, Tw, ref.data_ptr(), None,
                                            C.byref(Augment(**aug).struct([key])), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)), "aug")
    assert torch.equal(_bits(xb), _bits(ref)) and not torch.equal(_bits(xb), _bits(ds.x[:B]))
    next(it)
    assert ld.last_lam == mix.lam(seed, 2)


def test_a_plain_loader_takes_a_window_length_that_is_no_multiple_of_four():
    """A loader that neither augments nor mixes keeps the plain gather, whose rule is on the floats of a window (C * T a multiple of 4),
    not on T: T = 17 is the smallest length past a multiple of 4 that msig_workspace_layout accepts for C = 3 (16 is the smallest it
    accepts at all).  The store has 4 channels — with 3, no such T satisfies the plain gather's own rule.  The augmenting gather
    refuses this T (include/msig_aug.h: T % 4 == 0), so a loader that routed its plain batches through it could not serve them."""
    Tw, Cs, n, B = 17, 4, 7, 4
    for t in (15, 16, 17):
        ok = True
        try:
            L.workspace_layout(B, 3, t, K, True)
        except Exception:
            ok = False
        assert ok == (t >= 16), t
    rs = np.random.RandomState(4)
    x, y = rs.randn(n, Cs, Tw).astype(np.float32), rs.randint(0, K, size=n).astype(np.int64)
    ds = _Windows(x, y)
    got = [(xb.clone(), yb.clone()) for xb, yb in DeviceLoader(ds, B, False, DEV)]
    assert [int(xb.shape[0]) for xb, _ in got] == [4, 3]
    assert np.array_equal(torch.cat([xb for xb, _ in got]).cpu().numpy().view(np.int32), x.view(np.int32))
    assert np.array_equal(torch.cat([yb for _, yb in got]).cpu().numpy(), y)
    out = torch.empty((B, Cs, Tw), device=DEV)
    idx = torch.arange(B, dtype=torch.int64, device=DEV)
    rc = L.lib().msig_st_gather_windows(ds.x.data_ptr(), None, idx.data_ptr(), B, Cs, Tw, out.data_ptr(), None, None,
                                        (C.c_float * 1)(1.0), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == -2                                                    # MSIG_E_SHAPE, before any launch
