"""Label-free BatchNorm adaptation (include/msig_ab.h), the C ABI checked without a GPU: every call of the header is exported, the
binding's constants match it, and each rejection happens before the first launch (descriptors with fake, aligned, never dereferenced
pointers, as in test_grad_clip_cabi.py)."""
import ctypes as C
import re
from pathlib import Path

import pytest

from multimodalsignal_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "msig_ab.h").read_text()
E_NULL, E_SHAPE, E_ALIGN, E_WORKSPACE = -1, -2, -3, -4
B, CH, T, K = 16, 6, 256, 2
f = C.c_float


def test_header_calls_are_exported_and_constants_match():
    names = sorted(set(re.findall(r"\b(msig_ab_[a-z0-9_]+)\s*\(", HEADER)))
    assert names == ["msig_ab_abi_version", "msig_ab_accumulate", "msig_ab_accumulate_multi", "msig_ab_commit", "msig_ab_commit_multi"]
    lib = L.lib()
    for n in names:
        assert getattr(lib, n) is not None
    assert lib.msig_ab_abi_version() == int(re.search(r"#define MSIG_AB_ABI_VERSION (\d+)", HEADER).group(1)) == L.AB_ABI_VERSION
    const = {k: int(v) for k, v in re.findall(r"#define MSIG_AB_(N1|N2|SUM1|SQ1|SUM2|SQ2|ACC_DOUBLES)\s+(\d+)", HEADER)}
    assert const == {"N1": L.AB_N1, "N2": L.AB_N2, "SUM1": L.AB_SUM1, "SQ1": L.AB_SQ1, "SUM2": L.AB_SUM2, "SQ2": L.AB_SQ2,
                     "ACC_DOUBLES": L.AB_ACC_DOUBLES}
    # the slots tile the accumulator: 2 counts, 16 + 16 and 32 + 32 sums
    assert (L.AB_SUM1, L.AB_SQ1 - L.AB_SUM1, L.AB_SUM2 - L.AB_SQ1, L.AB_SQ2 - L.AB_SUM2, L.AB_ACC_DOUBLES - L.AB_SQ2) == (2, 16, 16, 32, 32)
    # the other headers' calls are still there
    assert (lib.msig_abi_version(), lib.msig_cw_abi_version(), lib.msig_cg_abi_version(), lib.msig_ft_abi_version()) == (5, 1, 1, 1)


def _batch(ws_bytes, training=0, **kw):
    keep_alive = (C.c_char * 8192)()
    addr = (C.addressof(keep_alive) + 255) // 256 * 256
    b = L.Batch()
    b.shape = L.Shape(kw.get("B", B), CH, T, kw.get("K", K))
    b.training = training
    for name in ("x", "params", "bn_state", "bn_count", "ws"):
        setattr(b, name, addr)
    b.ws_bytes = ws_bytes
    b.gru_layers = 2
    return b, keep_alive, addr


def _multi(n=2):
    m = L.Multi()
    m.n, m.stride_bytes = n, 1 << 20
    for i in range(n):
        m.slot[i] = i
    return m


def _acc(b, m, kind, stage, acc):
    lib = L.lib()
    return [lib.msig_ab_accumulate(C.byref(b), kind, stage, acc, None), lib.msig_ab_accumulate_multi(C.byref(b), C.byref(m), kind, stage, acc, None)]


def _commit(acc, stage, alpha, src, dst, m=None):
    lib = L.lib()
    return [lib.msig_ab_commit(acc, stage, f(alpha), src, dst, None),
            lib.msig_ab_commit_multi(acc, stage, f(alpha), src, dst, C.byref(m or _multi()), None)]


def _small():
    """An EVALUATION workspace one byte short: with valid arguments a call stops at MSIG_E_WORKSPACE — the last check before a
    launch — so any other code seen below was returned before anything could have been launched."""
    return L.workspace_layout(B, CH, T, K, False)[-1] - 1


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("stage", [1, 2])
def test_valid_arguments_reach_the_workspace_check_of_the_eval_layout(kind, stage):
    b, _k, addr = _batch(_small())
    assert _acc(b, _multi(), kind, stage, addr) == [E_WORKSPACE] * 2
    assert _acc(b, _multi(), kind, stage, addr + 8) == [E_WORKSPACE] * 2              # 8-byte alignment is enough
    assert L.workspace_layout(B, CH, T, K, False)[-1] < L.workspace_layout(B, CH, T, K, True)[-1]


def test_accumulate_argument_errors():
    lib = L.lib()
    b, _k, addr = _batch(_small())
    m = _multi()
    assert lib.msig_ab_accumulate(None, 0, 1, addr, None) == E_NULL
    assert lib.msig_ab_accumulate_multi(None, C.byref(m), 0, 1, addr, None) == E_NULL
    assert lib.msig_ab_accumulate_multi(C.byref(b), None, 0, 1, addr, None) == E_NULL
    assert _acc(b, m, 0, 1, None) == [E_NULL] * 2
    assert _acc(b, m, 0, 1, addr + 4) == [E_ALIGN] * 2                                 # a misaligned accumulator
    for stage in (0, 3, -1):
        assert _acc(b, m, 0, stage, addr) == [E_SHAPE] * 2, stage
    for kind in (2, -1):
        assert _acc(b, m, kind, 1, addr) == [E_SHAPE] * 2, kind
    bt, _kt, at = _batch(_small(), training=1)                                         # a training descriptor
    assert _acc(bt, m, 0, 1, at) == [E_SHAPE] * 2
    for field in ("x", "params", "bn_state", "bn_count", "ws"):
        bb, _kk, a = _batch(_small())
        setattr(bb, field, None)
        assert _acc(bb, m, 0, 2, a) == [E_NULL] * 2, field
    bb, _kk, a = _batch(_small())
    bb.x = a + 4
    assert _acc(bb, m, 0, 1, a) == [E_ALIGN] * 2
    for kw in (dict(K=1), dict(B=0)):
        bb, _kk, a = _batch(_small(), **kw)
        assert _acc(bb, m, 0, 1, a) == [E_SHAPE] * 2, kw
    bad = _multi(2)
    bad.slot[1] = 0
    assert lib.msig_ab_accumulate_multi(C.byref(b), C.byref(bad), 0, 1, addr, None) == E_SHAPE
    bad = _multi(2)
    bad.stride_bytes = 100
    assert lib.msig_ab_accumulate_multi(C.byref(b), C.byref(bad), 0, 1, addr, None) == E_ALIGN
    bad = _multi(0)
    assert lib.msig_ab_accumulate_multi(C.byref(b), C.byref(bad), 0, 1, addr, None) == E_SHAPE


def test_commit_argument_errors():
    lib = L.lib()
    _b, _k, addr = _batch(0)
    assert _commit(None, 1, 1.0, addr, addr) == [E_NULL] * 2
    assert _commit(addr, 1, 1.0, None, addr) == [E_NULL] * 2
    assert _commit(addr, 1, 1.0, addr, None) == [E_NULL] * 2
    assert lib.msig_ab_commit_multi(addr, 1, f(1.0), addr, addr, None, None) == E_NULL
    for stage in (0, 3):
        assert _commit(addr, stage, 1.0, addr, addr) == [E_SHAPE] * 2
    for alpha in (-0.01, 1.01, float("nan"), float("inf"), -float("inf")):
        assert _commit(addr, 2, alpha, addr, addr) == [E_SHAPE] * 2, alpha
    assert _commit(addr + 4, 1, 0.5, addr, addr) == [E_ALIGN] * 2
    assert _commit(addr, 1, 0.5, addr + 2, addr) == [E_ALIGN] * 2
    assert _commit(addr, 1, 0.5, addr, addr + 1) == [E_ALIGN] * 2
    bad = _multi(2)
    bad.slot[1] = 0
    assert lib.msig_ab_commit_multi(addr, 1, f(1.0), addr, addr, C.byref(bad), None) == E_SHAPE
    bad = _multi(2)
    bad.stride_bytes = 100
    assert lib.msig_ab_commit_multi(addr, 1, f(1.0), addr, addr, C.byref(bad), None) == E_ALIGN
