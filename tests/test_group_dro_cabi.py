"""Group-DRO (include/msig_dro.h), the C ABI checked without a GPU: every call of the header is exported beside the unchanged
headers, the binding's mirror matches the build, and each rejection happens before the first launch (descriptors with fake,
aligned, never dereferenced pointers, as in test_distill_cabi.py — the stand-alone calls have no later check to stop at, so every
call of theirs made here carries a defect; the train steps stop at a workspace one byte short)."""
import ctypes as C
import re
from pathlib import Path

import pytest

from multimodalsignal_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "msig_dro.h").read_text()
E_NULL, E_SHAPE, E_ALIGN, E_WORKSPACE = -1, -2, -3, -4
B, CH, T, K = 8, 6, 512, 2
f = C.c_float
NAN = float("nan")

_keep_alive = (C.c_char * 8192)()
A = (C.addressof(_keep_alive) + 255) // 256 * 256          # an aligned address nothing ever reads


def test_msig_dro_header_calls_are_exported_and_the_other_headers_are_unchanged():
    names = sorted(set(re.findall(r"\b(msig_dro_[a-z0-9_]+)\s*\(", HEADER)))
    assert names == ["msig_dro_abi_version", "msig_dro_apply", "msig_dro_apply_multi", "msig_dro_struct_bytes", "msig_dro_train_step",
                     "msig_dro_train_step_multi"]
    lib = L.lib()
    for n in names:
        assert getattr(lib, n) is not None
    assert lib.msig_dro_abi_version() == int(re.search(r"#define MSIG_DRO_ABI_VERSION (\d+)", HEADER).group(1)) == L.DRO_ABI_VERSION == 1
    assert int(re.search(r"#define MSIG_DRO_MAX_GROUPS (\d+)", HEADER).group(1)) == L.DRO_MAX_GROUPS == 64
    assert int(re.search(r"#define MSIG_DRO_MAX_BATCH (\d+)", HEADER).group(1)) == L.DRO_MAX_BATCH == 2048
    assert "#define MSIG_DRO_STATS (3 * MSIG_DRO_MAX_GROUPS + 2)" in HEADER and L.DRO_STATS == 194
    assert len(set(re.findall(r"\b(msig_\w+)\(", (ROOT / "include" / "msig.h").read_text()))) == 26
    assert (lib.msig_abi_version(), lib.msig_cw_abi_version(), lib.msig_cg_abi_version(), lib.msig_ft_abi_version(), lib.msig_gc_abi_version(),
            lib.msig_aug_abi_version(), lib.msig_st_abi_version(), lib.msig_ab_abi_version(), lib.msig_at_abi_version(), lib.msig_mc_abi_version(),
            lib.msig_da_abi_version(), lib.msig_wa_abi_version(), lib.msig_en_abi_version(), lib.msig_nr_abi_version(),
            lib.msig_kd_abi_version(), lib.msig_sam_abi_version()) == (5,) + (1,) * 15
    assert (lib.msig_kd_struct_bytes(), lib.msig_da_struct_bytes(), lib.msig_sam_struct_bytes()) == (C.sizeof(L.Kd), C.sizeof(L.Da), C.sizeof(L.Sam))


def test_mirror_matches_the_header():
    body = re.search(r"typedef struct msig_dro \{(.*?)\} msig_dro;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n for decl in body.split(";") for n in re.findall(r"[\s*,](\w+)(?:\[\w+\])?\s*(?=,|$)", decl.strip())]
    assert fields == [n for n, _ in L.Dro._fields_]
    assert L.lib().msig_dro_struct_bytes() == C.sizeof(L.Dro) == 64


def _dro(**kw):
    d = L.Dro()
    d.G, d.eta, d.frozen = kw.get("G", 3), kw.get("eta", 0.01), kw.get("frozen", 0)
    for name in ("grp", "idx", "q", "stats"):
        setattr(d, name, kw.get(name, A))
    d.idx_row_stride, d.stride_bytes = kw.get("idx_row_stride", 64), kw.get("stride_bytes", 1 << 16)
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


def _train_calls(d, Bv=B, lams=(1.0, 1.0), smoothing=0.0, da=None, sam=None):
    lib = L.lib()
    b, m = _batch(_small(Bv), Bv), _multi()
    s = L.make_st("cnn_gru_attention", smoothing, None, None, list(lams))
    dp = C.byref(d) if d is not None else None
    ap, sp = (C.byref(da) if da is not None else None), (C.byref(sam) if sam is not None else None)
    return [lib.msig_dro_train_step(C.byref(b), C.byref(s), ap, None, sp, dp, A, A, f(1e-3), f(0.9), f(0.999), f(1e-8), f(0.0), 1, None),
            lib.msig_dro_train_step_multi(C.byref(b), C.byref(m), C.byref(s), ap, None, sp, dp, A, A, f(0.9), f(0.999), f(1e-8), f(0.0), 1, None)]


def _apply_calls(d, Bv=B, Kv=K, logits="A", labels="A", cw=None, dlogits="A", smoothing=0.0, single=True, multi=None):
    """The term alone: [single, fold batch]; single=False where the defect is the fold batch's alone."""
    lib = L.lib()
    dp = C.byref(d) if d is not None else None
    lg, lb, dl = (A if logits == "A" else logits), (A if labels == "A" else labels), (A if dlogits == "A" else dlogits)
    m = _multi() if multi is None else multi
    return ([lib.msig_dro_apply(dp, lg, lb, cw, f(smoothing), dl, Bv, Kv, None)] if single else []) + [
        lib.msig_dro_apply_multi(dp, C.byref(m), lg, lb, cw, f(smoothing), dl, Bv, Kv, None)]


def _all(d, **kw):
    return _train_calls(d, **{a: v for a, v in kw.items() if a in ("Bv", "smoothing")}) + _apply_calls(d, **kw)


def test_valid_arguments_reach_the_counterparts_checks_and_a_null_term_is_the_counterpart():
    assert _train_calls(_dro()) == [E_WORKSPACE] * 2
    assert _train_calls(_dro(idx=None, stats=None)) == [E_WORKSPACE] * 2                      # both optional
    assert _train_calls(_dro(G=1, eta=0.0)) == [E_WORKSPACE] * 2 and _train_calls(_dro(G=64, eta=1e6, frozen=1)) == [E_WORKSPACE] * 2
    assert _train_calls(_dro(stats=A + 8, idx=A + 8, q=A + 4, grp=A + 4)) == [E_WORKSPACE] * 2
    assert _train_calls(_dro(idx_row_stride=2048), Bv=2048) == [E_WORKSPACE] * 2
    assert _train_calls(_dro(), smoothing=0.5) == [E_WORKSPACE] * 2
    assert _train_calls(None) == [E_WORKSPACE] * 2                                            # NULL msig_dro: msig_kd_train_step[_multi] itself
    assert _train_calls(None, lams=(0.4, 0.4)) == [E_WORKSPACE] * 2                           # ... which mixes
    assert _train_calls(_dro(), sam=_sam()) == [E_WORKSPACE] * 2 and _train_calls(None, sam=_sam()) == [E_WORKSPACE] * 2
    assert _train_calls(_dro(), da=_da()) == [E_WORKSPACE] * 2


def test_adversary_with_sam_is_refused_with_and_without_the_term():
    assert _train_calls(_dro(), da=_da(), sam=_sam()) == [E_SHAPE] * 2
    assert _train_calls(None, da=_da(), sam=_sam()) == [E_SHAPE] * 2


def test_null_pointers():
    assert _apply_calls(None) == [E_NULL] * 2
    for name in ("grp", "q"):
        assert _all(_dro(**{name: None})) == [E_NULL] * 4, name
    for name in ("logits", "labels", "dlogits"):
        assert _apply_calls(_dro(), **{name: None}) == [E_NULL] * 2, name
    lib = L.lib()
    assert lib.msig_dro_apply_multi(C.byref(_dro()), None, A, A, None, f(0.0), A, B, K, None) == E_NULL
    b, s = _batch(_small()), L.make_st("cnn_gru_attention", 0.0, None, None, [1.0])
    args = (A, A, f(1e-3), f(0.9), f(0.999), f(1e-8), f(0.0), 1, None)
    assert lib.msig_dro_train_step(C.byref(b), None, None, None, None, C.byref(_dro()), *args) == E_NULL
    assert lib.msig_dro_train_step(None, C.byref(s), None, None, None, C.byref(_dro()), *args) == E_NULL


@pytest.mark.parametrize("G", [0, -1, 65, 1 << 20])
def test_bad_group_count_is_a_shape_error(G):
    assert _all(_dro(G=G)) == [E_SHAPE] * 4


@pytest.mark.parametrize("eta", [NAN, -0.01, -float("inf")])
def test_bad_eta_is_a_shape_error(eta):
    assert _all(_dro(eta=eta)) == [E_SHAPE] * 4


def test_bad_sizes_are_shape_errors():
    for Kv in (-1, 0, 1, L.MAX_K + 1):
        assert _apply_calls(_dro(), Kv=Kv) == [E_SHAPE] * 2, Kv
    for Bv in (0, -3, L.DRO_MAX_BATCH + 1):
        assert _apply_calls(_dro(), Bv=Bv) == [E_SHAPE] * 2, Bv
    assert _train_calls(_dro(idx_row_stride=4096), Bv=L.DRO_MAX_BATCH + 1) == [E_SHAPE] * 2      # the train step's batch likewise
    for eps in (NAN, -0.1, 1.0, 1.5):
        assert _apply_calls(_dro(), smoothing=eps) == [E_SHAPE] * 2, eps
    assert _apply_calls(_dro(idx_row_stride=B - 1), single=False) == [E_SHAPE]               # the folds' rows of idx would overlap
    assert _train_calls(_dro(idx_row_stride=B - 1)) == [E_WORKSPACE, E_SHAPE]
    assert _apply_calls(_dro(idx_row_stride=0, idx=None), single=False, logits=None) == [E_NULL]      # without idx the stride is not read


@pytest.mark.parametrize("lams", [(0.4, 1.0), (1.0, 0.999), (0.0, 0.0)])
def test_mixup_is_refused(lams):
    """A fold of the launch with lam != 1: MSIG_E_SHAPE (the single call reads lam[0] alone)."""
    assert _train_calls(_dro(), lams=lams) == [E_SHAPE if lams[0] != 1.0 else E_WORKSPACE, E_SHAPE]


def test_misalignment():
    for name in ("q", "grp"):
        assert _all(_dro(**{name: A + 2})) == [E_ALIGN] * 4, name
    for name in ("stats", "idx"):
        assert _all(_dro(**{name: A + 4})) == [E_ALIGN] * 4, name
    assert _apply_calls(_dro(), logits=A + 2) == [E_ALIGN] * 2
    assert _apply_calls(_dro(), dlogits=A + 1) == [E_ALIGN] * 2
    assert _apply_calls(_dro(), labels=A + 4) == [E_ALIGN] * 2
    assert _apply_calls(_dro(), cw=A + 2) == [E_ALIGN] * 2
    for stride in (0, -256, 100, 257):
        d = _dro(stride_bytes=stride)                                                         # the stride counts in fold batches only
        assert _train_calls(d) == [E_WORKSPACE, E_ALIGN] and _apply_calls(d, single=False, logits=A + 2) == [E_ALIGN], stride
    # NULL before the shape, the shape before the alignment
    assert _apply_calls(_dro(eta=NAN, q=None)) == [E_NULL] * 2 and _apply_calls(_dro(eta=NAN, q=A + 2)) == [E_SHAPE] * 2
    assert _apply_calls(_dro(G=0, grp=A + 2), Bv=0) == [E_SHAPE] * 2


def test_msig_multis_own_checks_come_first():
    for bad in (_multi(n=0), _multi(n=L.MAX_FOLDS + 1), _multi(slots=[1, 1])):
        assert _apply_calls(_dro(q=A + 2), single=False, multi=bad) == [E_SHAPE]
    for bad in (_multi(stride=0), _multi(stride=128)):
        assert _apply_calls(_dro(eta=NAN), single=False, multi=bad) == [E_ALIGN]
