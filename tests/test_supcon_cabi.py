"""The supervised contrastive term (include/msig_sc.h), the C ABI checked without a GPU: every call of the header is exported beside
the unchanged headers, the binding's mirror matches the build, and each rejection happens before the first launch (descriptors with
fake, aligned, never dereferenced pointers, as in test_group_dro_cabi.py — the stand-alone calls have no later check to stop at, so
every call of theirs made here carries a defect; the train steps stop at a workspace one byte short)."""
import ctypes as C
import re
from pathlib import Path

import pytest

from multimodalsignal_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "msig_sc.h").read_text()
E_NULL, E_SHAPE, E_ALIGN, E_WORKSPACE = -1, -2, -3, -4
B, CH, T, K = 8, 6, 512, 2
f = C.c_float
NAN = float("nan")

_keep_alive = (C.c_char * 8192)()
A = (C.addressof(_keep_alive) + 255) // 256 * 256          # an aligned address nothing ever reads


def test_msig_sc_header_calls_are_exported_and_the_other_headers_are_unchanged():
    names = sorted(set(re.findall(r"\b(msig_sc_[a-z0-9_]+)\s*\(", HEADER)))
    assert names == ["msig_sc_abi_version", "msig_sc_apply", "msig_sc_apply_multi", "msig_sc_scratch_bytes", "msig_sc_struct_bytes",
                     "msig_sc_train_step", "msig_sc_train_step_multi"]
    lib = L.lib()
    for n in names:
        assert getattr(lib, n) is not None
    assert lib.msig_sc_abi_version() == int(re.search(r"#define MSIG_SC_ABI_VERSION (\d+)", HEADER).group(1)) == L.SC_ABI_VERSION == 1
    assert int(re.search(r"#define MSIG_SC_MAX_BATCH (\d+)", HEADER).group(1)) == L.SC_MAX_BATCH == 2048
    assert int(re.search(r"#define MSIG_SC_STATS (\d+)", HEADER).group(1)) == L.SC_STATS == 4
    assert L.SC_POSITIVES == {"class": 0, "cross-subject": 1}
    assert '#include "msig_dro.h"' in HEADER
    assert len(set(re.findall(r"\b(msig_\w+)\(", (ROOT / "include" / "msig.h").read_text()))) == 26
    assert (lib.msig_abi_version(), lib.msig_cw_abi_version(), lib.msig_cg_abi_version(), lib.msig_ft_abi_version(), lib.msig_gc_abi_version(),
            lib.msig_aug_abi_version(), lib.msig_st_abi_version(), lib.msig_ab_abi_version(), lib.msig_at_abi_version(), lib.msig_mc_abi_version(),
            lib.msig_da_abi_version(), lib.msig_wa_abi_version(), lib.msig_en_abi_version(), lib.msig_nr_abi_version(),
            lib.msig_kd_abi_version(), lib.msig_sam_abi_version(), lib.msig_dro_abi_version()) == (5,) + (1,) * 16
    assert (lib.msig_kd_struct_bytes(), lib.msig_da_struct_bytes(), lib.msig_sam_struct_bytes(), lib.msig_dro_struct_bytes()) == (
        C.sizeof(L.Kd), C.sizeof(L.Da), C.sizeof(L.Sam), C.sizeof(L.Dro))
    assert (lib.msig_struct_bytes(0), lib.msig_struct_bytes(1)) == (C.sizeof(L.Batch), C.sizeof(L.Multi))


def test_mirror_matches_the_header():
    body = re.search(r"typedef struct msig_sc \{(.*?)\} msig_sc;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n for decl in body.split(";") for n in re.findall(r"[\s*,](\w+)(?:\[\w+\])?\s*(?=,|$)", decl.strip())]
    assert fields == [n for n, _ in L.Sc._fields_]
    assert L.lib().msig_sc_struct_bytes() == C.sizeof(L.Sc) == 56 + 4 * L.MAX_FOLDS


def test_scratch_bytes():
    lib = L.lib()
    for Bv in (0, -1, L.SC_MAX_BATCH + 1):
        assert lib.msig_sc_scratch_bytes(Bv) == E_SHAPE
    prev = 0
    for Bv in (1, 2, 31, 32, 33, 64, 257, 2048):
        n = lib.msig_sc_scratch_bytes(Bv)
        assert n % 256 == 0 and n >= Bv * 128 * 4 and n >= prev           # the normalised rows at least; monotonic
        prev = n
    assert prev < 2048 * 1024                                             # and no B x B matrix


def _sc(**kw):
    d = L.Sc()
    d.positives, d.tau = kw.get("positives", 1), kw.get("tau", 0.1)
    for name in ("grp", "idx", "scratch", "stats"):
        setattr(d, name, kw.get(name, A))
    d.idx_row_stride, d.stride_bytes = kw.get("idx_row_stride", 64), kw.get("stride_bytes", 1 << 16)
    for i, w in enumerate(kw.get("weights", (0.1, 0.1))):
        d.weight[i] = w
    return d


def _multi(n=2, stride=1 << 20, slots=None):
    m = L.Multi()
    m.n, m.stride_bytes = n, stride
    for i, s in enumerate(slots if slots is not None else range(min(max(n, 0), L.MAX_FOLDS))):
        m.slot[i] = s
    return m


def _batch(ws_bytes, Bv=B, Kv=K):
    b = L.Batch()
    b.shape = L.Shape(Bv, CH, T, Kv)
    b.training = 1
    for name in ("x", "labels", "params", "grads", "bn_state", "bn_count", "ws"):
        setattr(b, name, A)
    b.ws_bytes = ws_bytes
    b.gru_layers = 2
    return b


def _small(Bv=B):
    """A workspace one byte short: with valid arguments the train steps stop at MSIG_E_WORKSPACE, the last check before a launch."""
    return L.workspace_layout(Bv, CH, T, K, True)[-1] - 1


def _sam():
    s = L.Sam()
    s.kind, s.adaptive, s.rho, s.eta, s.state = 0, 0, 0.05, 0.0, A
    s.state_bytes = L.sam_state_bytes(CH, K, "cnn_gru_attention")
    return s


def _da():
    a = L.Da()
    a.S, a.beta1, a.beta2, a.eps = 3, 0.9, 0.999, 1e-8
    for name in ("dom", "params", "exp_avg", "exp_avg_sq", "stats", "idx"):
        setattr(a, name, A)
    a.idx_row_stride, a.stride_bytes = 64, 1 << 16
    for i in range(2):
        a.step[i] = 1
    return a


def _dro(**kw):
    d = L.Dro()
    d.G, d.eta, d.frozen = kw.get("G", 3), 0.01, 0
    for name in ("grp", "idx", "q", "stats"):
        setattr(d, name, kw.get(name, A))
    d.idx_row_stride, d.stride_bytes = 64, 1 << 16
    return d


def _train_calls(d, Bv=B, lams=(1.0, 1.0), da=None, sam=None, dro=None):
    lib = L.lib()
    b, m = _batch(_small(Bv), Bv), _multi()
    s = L.make_st("cnn_gru_attention", 0.0, None, None, list(lams))
    p = lambda v: C.byref(v) if v is not None else None
    return [lib.msig_sc_train_step(C.byref(b), C.byref(s), p(da), None, p(sam), p(dro), p(d), A, A, f(1e-3), f(0.9), f(0.999), f(1e-8), f(0.0), 1, None),
            lib.msig_sc_train_step_multi(C.byref(b), C.byref(m), C.byref(s), p(da), None, p(sam), p(dro), p(d), A, A, f(0.9), f(0.999), f(1e-8),
                                         f(0.0), 1, None)]


def _apply_calls(d, Bv=B, Kv=K, feat="A", labels="A", dfeat="A", single=True, multi=None):
    """The term alone: [single, fold batch]; single=False where the defect is the fold batch's alone."""
    lib = L.lib()
    dp = C.byref(d) if d is not None else None
    ft, lb, df = (A if feat == "A" else feat), (A if labels == "A" else labels), (A if dfeat == "A" else dfeat)
    m = _multi() if multi is None else multi
    return ([lib.msig_sc_apply(dp, ft, lb, df, Bv, Kv, None)] if single else []) + [lib.msig_sc_apply_multi(dp, C.byref(m), ft, lb, df, Bv, Kv, None)]


def _all(d, **kw):
    return _train_calls(d, **{a: v for a, v in kw.items() if a in ("Bv",)}) + _apply_calls(d, **kw)


def test_valid_arguments_reach_the_counterparts_checks_and_a_null_term_is_the_counterpart():
    assert _train_calls(_sc()) == [E_WORKSPACE] * 2
    assert _train_calls(_sc(idx=None, stats=None)) == [E_WORKSPACE] * 2                       # both optional
    assert _train_calls(_sc(positives=0, grp=None, idx=None)) == [E_WORKSPACE] * 2            # class mode reads no subject table
    assert _train_calls(_sc(tau=1e-3, weights=(0.0, 0.0))) == [E_WORKSPACE] * 2 and _train_calls(_sc(tau=1e3, weights=(1e6, 0.0))) == [E_WORKSPACE] * 2
    assert _train_calls(_sc(stats=A + 8, idx=A + 8, grp=A + 4, scratch=A + 16)) == [E_WORKSPACE] * 2
    assert _train_calls(_sc(idx_row_stride=2048), Bv=2048) == [E_WORKSPACE] * 2
    assert _train_calls(_sc(), sam=_sam()) == [E_WORKSPACE] * 2 and _train_calls(_sc(), da=_da()) == [E_WORKSPACE] * 2
    assert _train_calls(_sc(), dro=_dro()) == [E_WORKSPACE] * 2
    # NULL msig_sc: msig_dro_train_step[_multi] itself — it mixes, and it reaches msig_dro's own checks
    assert _train_calls(None) == [E_WORKSPACE] * 2 and _train_calls(None, lams=(0.4, 0.4)) == [E_WORKSPACE] * 2
    assert _train_calls(None, dro=_dro(G=0)) == [E_SHAPE] * 2 and _train_calls(None, dro=_dro(q=None)) == [E_NULL] * 2
    assert _train_calls(None, dro=_dro(), lams=(0.4, 0.4)) == [E_SHAPE] * 2
    assert _train_calls(None, dro=_dro(q=A + 2)) == [E_ALIGN] * 2


def test_adversary_with_sam_is_refused_with_and_without_the_term():
    assert _train_calls(_sc(), da=_da(), sam=_sam()) == [E_SHAPE] * 2
    assert _train_calls(None, da=_da(), sam=_sam()) == [E_SHAPE] * 2


def test_null_pointers():
    assert _apply_calls(None) == [E_NULL] * 2
    assert _all(_sc(scratch=None)) == [E_NULL] * 4
    assert _all(_sc(grp=None)) == [E_NULL] * 4                                                # cross-subject mode needs the table
    for name in ("feat", "labels", "dfeat"):
        assert _apply_calls(_sc(), **{name: None}) == [E_NULL] * 2, name
    lib = L.lib()
    assert lib.msig_sc_apply_multi(C.byref(_sc()), None, A, A, A, B, K, None) == E_NULL
    b, s = _batch(_small()), L.make_st("cnn_gru_attention", 0.0, None, None, [1.0])
    args = (A, A, f(1e-3), f(0.9), f(0.999), f(1e-8), f(0.0), 1, None)
    assert lib.msig_sc_train_step(C.byref(b), None, None, None, None, None, C.byref(_sc()), *args) == E_NULL
    assert lib.msig_sc_train_step(None, C.byref(s), None, None, None, None, C.byref(_sc()), *args) == E_NULL


@pytest.mark.parametrize("positives", [-1, 2, 1 << 20])
def test_bad_positives_is_a_shape_error(positives):
    assert _all(_sc(positives=positives)) == [E_SHAPE] * 4


@pytest.mark.parametrize("tau", [NAN, 0.0, -0.1, 9.9e-4, 1001.0, float("inf")])
def test_bad_tau_is_a_shape_error(tau):
    assert _all(_sc(tau=tau)) == [E_SHAPE] * 4


@pytest.mark.parametrize("w", [NAN, -0.1, -float("inf")])
def test_bad_weight_is_a_shape_error(w):
    assert _all(_sc(weights=(w, w))) == [E_SHAPE] * 4
    assert _train_calls(_sc(weights=(0.1, w))) == [E_WORKSPACE, E_SHAPE]                        # the single call reads weight[0] alone
    assert _apply_calls(_sc(weights=(0.1, w)), single=False) == [E_SHAPE]


def test_bad_sizes_are_shape_errors():
    for Kv in (-1, 0, 1, L.MAX_K + 1):
        assert _apply_calls(_sc(), Kv=Kv) == [E_SHAPE] * 2, Kv
    for Bv in (0, -3, L.SC_MAX_BATCH + 1):
        assert _apply_calls(_sc(), Bv=Bv) == [E_SHAPE] * 2, Bv
    assert _train_calls(_sc(idx_row_stride=4096), Bv=L.SC_MAX_BATCH + 1) == [E_SHAPE] * 2      # the train step's batch likewise
    assert _apply_calls(_sc(idx_row_stride=B - 1), single=False) == [E_SHAPE]                # the folds' rows of idx would overlap
    assert _train_calls(_sc(idx_row_stride=B - 1)) == [E_WORKSPACE, E_SHAPE]
    assert _apply_calls(_sc(idx_row_stride=0, idx=None), single=False, feat=None) == [E_NULL]      # without idx the stride is not read


@pytest.mark.parametrize("lams", [(0.4, 1.0), (1.0, 0.999), (0.0, 0.0)])
def test_mixup_is_refused(lams):
    """A fold of the launch with lam != 1: MSIG_E_SHAPE (the single call reads lam[0] alone)."""
    assert _train_calls(_sc(), lams=lams) == [E_SHAPE if lams[0] != 1.0 else E_WORKSPACE, E_SHAPE]


def test_misalignment_and_the_order_of_the_checks():
    assert _all(_sc(scratch=A + 8)) == [E_ALIGN] * 4
    assert _all(_sc(grp=A + 2)) == [E_ALIGN] * 4
    for name in ("stats", "idx"):
        assert _all(_sc(**{name: A + 4})) == [E_ALIGN] * 4, name
    assert _apply_calls(_sc(), feat=A + 8) == [E_ALIGN] * 2
    assert _apply_calls(_sc(), dfeat=A + 4) == [E_ALIGN] * 2
    assert _apply_calls(_sc(), labels=A + 4) == [E_ALIGN] * 2
    for stride in (0, -256, 100, 257):
        d = _sc(stride_bytes=stride)                                                          # the stride counts in fold batches only
        assert _train_calls(d) == [E_WORKSPACE, E_ALIGN] and _apply_calls(d, single=False, feat=A + 8) == [E_ALIGN], stride
    # NULL before the shape, the shape before the alignment
    assert _apply_calls(_sc(tau=NAN, scratch=None)) == [E_NULL] * 2 and _apply_calls(_sc(tau=NAN, scratch=A + 8)) == [E_SHAPE] * 2
    assert _apply_calls(_sc(positives=7, grp=A + 2), Bv=0) == [E_SHAPE] * 2
    assert _apply_calls(_sc(), feat=A + 8, Bv=0) == [E_SHAPE] * 2
    # a mixing launch is refused before the term's alignment is looked at
    assert _train_calls(_sc(scratch=A + 8), lams=(0.4, 0.4)) == [E_SHAPE] * 2
    # the term's checks follow msig_dro's
    assert _train_calls(_sc(tau=NAN), dro=_dro(q=A + 2)) == [E_ALIGN] * 2


def test_msig_multis_own_checks_come_first():
    for bad in (_multi(n=0), _multi(n=L.MAX_FOLDS + 1), _multi(slots=[1, 1])):
        assert _apply_calls(_sc(scratch=A + 8), single=False, multi=bad) == [E_SHAPE]
    for bad in (_multi(stride=0), _multi(stride=128)):
        assert _apply_calls(_sc(tau=NAN), single=False, multi=bad) == [E_ALIGN]
