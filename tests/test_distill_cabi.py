"""Distillation (include/msig_kd.h), the C ABI checked without a GPU: every call of the header is exported beside the unchanged
headers, the binding's mirror matches the build, and each rejection happens before the first launch (descriptors with fake,
aligned, never dereferenced pointers, as in test_adversary_cabi.py — the stand-alone calls have no later check to stop at, so every
call of theirs made here carries a defect; the train steps stop at a workspace one byte short)."""
import ctypes as C
import re
from pathlib import Path

import pytest

from multimodalsignal_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "msig_kd.h").read_text()
E_NULL, E_SHAPE, E_ALIGN, E_WORKSPACE = -1, -2, -3, -4
B, CH, T, K = 8, 6, 512, 2
f = C.c_float
NAN = float("nan")

_keep_alive = (C.c_char * 8192)()
A = (C.addressof(_keep_alive) + 255) // 256 * 256          # an aligned address nothing ever reads


def test_msig_kd_header_calls_are_exported_and_the_other_headers_are_unchanged():
    names = sorted(set(re.findall(r"\b(msig_kd_[a-z0-9_]+)\s*\(", HEADER)))
    assert names == ["msig_kd_abi_version", "msig_kd_apply", "msig_kd_apply_multi", "msig_kd_struct_bytes", "msig_kd_teacher",
                     "msig_kd_teacher_multi", "msig_kd_train_step", "msig_kd_train_step_multi"]
    lib = L.lib()
    for n in names:
        assert getattr(lib, n) is not None
    assert lib.msig_kd_abi_version() == int(re.search(r"#define MSIG_KD_ABI_VERSION (\d+)", HEADER).group(1)) == L.KD_ABI_VERSION == 1
    assert int(re.search(r"#define MSIG_KD_MAX_MEMBERS (\d+)", HEADER).group(1)) == L.KD_MAX_MEMBERS == L.EN_MAX_MEMBERS
    assert len(set(re.findall(r"\b(msig_\w+)\(", (ROOT / "include" / "msig.h").read_text()))) == 26
    assert (lib.msig_abi_version(), lib.msig_cw_abi_version(), lib.msig_cg_abi_version(), lib.msig_ft_abi_version(), lib.msig_gc_abi_version(),
            lib.msig_aug_abi_version(), lib.msig_st_abi_version(), lib.msig_ab_abi_version(), lib.msig_at_abi_version(), lib.msig_mc_abi_version(),
            lib.msig_da_abi_version(), lib.msig_wa_abi_version(), lib.msig_en_abi_version(), lib.msig_nr_abi_version()) == (5,) + (1,) * 13
    assert (L.ABI_VERSION, L.DA_ABI_VERSION, L.EN_ABI_VERSION, L.MAX_FOLDS, L.MAX_K) == (5, 1, 1, 16, 16)


def test_mirror_matches_the_header():
    body = re.search(r"typedef struct msig_kd \{(.*?)\} msig_kd;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n for decl in body.split(";") for n in re.findall(r"[\s*,](\w+)(?:\[\w+\])?\s*(?=,|$)", decl.strip())]
    assert fields == [n for n, _ in L.Kd._fields_]
    assert L.lib().msig_kd_struct_bytes() == C.sizeof(L.Kd) == 48


def _kd(**kw):
    k = L.Kd()
    k.alpha, k.temperature = kw.get("alpha", 0.5), kw.get("temperature", 2.0)
    for name in ("q", "idx", "stats"):
        setattr(k, name, kw.get(name, A))
    k.idx_row_stride, k.stride_bytes = kw.get("idx_row_stride", 64), kw.get("stride_bytes", 1 << 16)
    return k


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


def _train_calls(k, Bv=B, lams=(1.0, 1.0), Kv=K):
    lib = L.lib()
    b, m = _batch(_small(Bv), Bv, Kv), _multi()
    s = L.make_st("cnn_gru_attention", 0.0, None, None, list(lams))
    kp = C.byref(k) if k is not None else None
    return [lib.msig_kd_train_step(C.byref(b), C.byref(s), None, kp, A, A, f(1e-3), f(0.9), f(0.999), f(1e-8), f(0.0), 1, None),
            lib.msig_kd_train_step_multi(C.byref(b), C.byref(m), C.byref(s), None, kp, A, A, f(0.9), f(0.999), f(1e-8), f(0.0), 1, None)]


def _apply_calls(k, Bv=B, Kv=K, logits="A", dlogits="A", lam=1.0, single=True, multi=None):
    """The term alone: [single, fold batch]; single=False where the defect is the fold batch's alone."""
    lib = L.lib()
    kp = C.byref(k) if k is not None else None
    lg, dl = (A if logits == "A" else logits), (A if dlogits == "A" else dlogits)
    m = _multi() if multi is None else multi
    return ([lib.msig_kd_apply(kp, lg, dl, Bv, Kv, f(lam), None)] if single else []) + [
        lib.msig_kd_apply_multi(kp, C.byref(m), lg, dl, Bv, Kv, (C.c_float * L.MAX_FOLDS)(lam, lam), None)]


def _all(k, **kw):
    return _train_calls(k, **{a: v for a, v in kw.items() if a in ("Bv",)}) + _apply_calls(k, **kw)


def test_valid_arguments_reach_the_counterparts_checks_and_a_null_or_zero_term_is_the_counterpart():
    assert _train_calls(_kd()) == [E_WORKSPACE] * 2
    assert _train_calls(_kd(idx=None, stats=None)) == [E_WORKSPACE] * 2                       # both optional
    assert _train_calls(_kd(alpha=1.0, temperature=64.0)) == [E_WORKSPACE] * 2
    assert _train_calls(_kd(alpha=0.0, temperature=1.0 / 64.0)) == [E_WORKSPACE] * 2
    assert _train_calls(_kd(stats=A + 8, idx=A + 8, q=A + 4)) == [E_WORKSPACE] * 2
    assert _train_calls(_kd(idx_row_stride=4096), Bv=4096) == [E_WORKSPACE] * 2               # no batch limit: the term streams
    assert _train_calls(None) == [E_WORKSPACE] * 2                                            # NULL msig_kd: msig_da_train_step[_multi] itself


def test_null_pointers():
    assert _apply_calls(None) == [E_NULL] * 2
    assert _all(_kd(q=None)) == [E_NULL] * 4
    assert _apply_calls(_kd(), logits=None) == [E_NULL] * 2
    assert _apply_calls(_kd(), dlogits=None) == [E_NULL] * 2
    lib = L.lib()
    assert lib.msig_kd_apply_multi(C.byref(_kd()), None, A, A, B, K, (C.c_float * L.MAX_FOLDS)(1.0, 1.0), None) == E_NULL
    assert lib.msig_kd_apply_multi(C.byref(_kd()), C.byref(_multi()), A, A, B, K, None, None) == E_NULL
    b, s = _batch(_small()), L.make_st("cnn_gru_attention", 0.0, None, None, [1.0])
    assert lib.msig_kd_train_step(C.byref(b), None, None, C.byref(_kd()), A, A, f(1e-3), f(0.9), f(0.999), f(1e-8), f(0.0), 1, None) == E_NULL
    assert lib.msig_kd_train_step(None, C.byref(s), None, C.byref(_kd()), A, A, f(1e-3), f(0.9), f(0.999), f(1e-8), f(0.0), 1, None) == E_NULL


@pytest.mark.parametrize("alpha", [NAN, -0.1, 1.5, float("inf")])
def test_bad_alpha_is_a_shape_error(alpha):
    assert _all(_kd(alpha=alpha)) == [E_SHAPE] * 4


@pytest.mark.parametrize("temperature", [NAN, 0.0, -2.0, 1.0 / 128.0, 64.5, float("inf")])
def test_bad_temperature_is_a_shape_error(temperature):
    assert _all(_kd(temperature=temperature)) == [E_SHAPE] * 4


def test_bad_sizes_are_shape_errors():
    for Kv in (-1, 0, 1, L.MAX_K + 1):
        assert _apply_calls(_kd(), Kv=Kv) == [E_SHAPE] * 2, Kv
    for Bv in (0, -3):
        assert _apply_calls(_kd(), Bv=Bv) == [E_SHAPE] * 2, Bv
    assert _apply_calls(_kd(idx_row_stride=B - 1), single=False) == [E_SHAPE]                # the folds' rows of idx would overlap
    assert _train_calls(_kd(idx_row_stride=B - 1)) == [E_WORKSPACE, E_SHAPE]
    assert _apply_calls(_kd(idx_row_stride=0, idx=None), single=False, logits=None) == [E_NULL]      # without idx the stride is not read
    for lam in (NAN, -0.1, 1.5):
        assert _apply_calls(_kd(), lam=lam) == [E_SHAPE] * 2, lam


def test_misalignment():
    assert _all(_kd(q=A + 2)) == [E_ALIGN] * 4
    for name in ("stats", "idx"):
        assert _all(_kd(**{name: A + 4})) == [E_ALIGN] * 4, name
    assert _apply_calls(_kd(), logits=A + 2) == [E_ALIGN] * 2
    assert _apply_calls(_kd(), dlogits=A + 1) == [E_ALIGN] * 2
    for stride in (0, -256, 100, 257):
        k = _kd(stride_bytes=stride)                                                          # the stride counts in fold batches only
        assert _train_calls(k) == [E_WORKSPACE, E_ALIGN] and _apply_calls(k, single=False, logits=A + 2) == [E_ALIGN], stride
    # NULL before the shape, the shape before the alignment
    assert _apply_calls(_kd(alpha=NAN, q=None)) == [E_NULL] * 2 and _apply_calls(_kd(alpha=NAN, q=A + 2)) == [E_SHAPE] * 2


def test_msig_multis_own_checks_come_first():
    for bad in (_multi(n=0), _multi(n=L.MAX_FOLDS + 1), _multi(slots=[1, 1])):
        assert _apply_calls(_kd(alpha=NAN), single=False, multi=bad) == [E_SHAPE]
        assert _teacher_multi(multi=bad, logits=None) == E_SHAPE
    for bad in (_multi(stride=0), _multi(stride=128)):
        assert _apply_calls(_kd(alpha=NAN), single=False, multi=bad) == [E_ALIGN]
        assert _teacher_multi(multi=bad, logits=None) == E_ALIGN


# ---- the teacher: msig_en_reduce[_multi]'s conventions and checks, plus the temperature ---------------------------------------------
def _teacher(**kw):
    a = dict(logits=A, stride=5 * 3, M=7, N=5, K=3, T=2.0, q=A)
    a.update(kw)
    return L.lib().msig_kd_teacher(a["logits"], a["stride"], a["M"], a["N"], a["K"], f(a["T"]), a["q"], None)


def _teacher_multi(multi=None, **kw):
    a = dict(logits=A, N=5, K=3, T=2.0, q=A)
    a.update(kw)
    m = _multi(n=3, stride=256) if multi is None else multi
    return L.lib().msig_kd_teacher_multi(a["logits"], None if m is False else C.byref(m), a["N"], a["K"], f(a["T"]), a["q"], None)


def test_teacher_rejections():
    assert _teacher(logits=None) == E_NULL and _teacher(q=None) == E_NULL
    for bad in (dict(M=0), dict(M=-1), dict(M=L.KD_MAX_MEMBERS + 1), dict(N=0), dict(N=-3), dict(K=1), dict(K=L.MAX_K + 1),
                dict(N=1 << 30, M=2, stride=1 << 40), dict(stride=14), dict(stride=0), dict(stride=-1), dict(T=NAN), dict(T=0.0),
                dict(T=1.0 / 128.0), dict(T=65.0)):
        assert _teacher(**bad) == E_SHAPE, bad
    for name in ("logits", "q"):
        for off in (1, 2):
            assert _teacher(**{name: A + off}) == E_ALIGN, (name, off)
    assert _teacher(logits=None, M=0) == E_NULL and _teacher(M=0, q=A + 2) == E_SHAPE


def test_teacher_multi_rejections():
    assert _teacher_multi(multi=False) == E_NULL
    assert _teacher_multi(logits=None) == E_NULL and _teacher_multi(q=None) == E_NULL
    for bad in (dict(N=0), dict(K=1), dict(K=L.MAX_K + 1), dict(N=22), dict(T=NAN), dict(T=100.0)):      # 22 * 3 floats > the 256-byte stride
        assert _teacher_multi(**bad) == E_SHAPE, bad
    for name in ("logits", "q"):
        assert _teacher_multi(**{name: A + 2}) == E_ALIGN, name
