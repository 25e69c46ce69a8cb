"""Integrated-gradients attribution (include/msig_at.h), the C ABI checked without a GPU: the header's calls are exported, the
binding's constants match it, the other headers' ABI versions are what they were, and each rejection happens before the first
launch (fake, aligned, never dereferenced pointers, as in test_adapt_cabi.py — a call that passed every check would launch, so
only rejected calls are made here)."""
import ctypes as C
import re
from pathlib import Path

from multimodalsignal_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "msig_at.h").read_text()
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
N, P, CH, T, K, BIN = 3, 5, 6, 256, 3, 64

_keep_alive = (C.c_char * 8192)()
A = (C.addressof(_keep_alive) + 255) // 256 * 256          # an aligned address nothing ever reads


def test_header_calls_are_exported_and_constants_match():
    names = sorted(set(re.findall(r"\b(msig_at_[a-z0-9_]+)\s*\(", HEADER)))
    assert names == ["msig_at_abi_version", "msig_at_path", "msig_at_reduce"]
    lib = L.lib()
    for n in names:
        assert getattr(lib, n) is not None
    assert lib.msig_at_abi_version() == int(re.search(r"#define MSIG_AT_ABI_VERSION (\d+)", HEADER).group(1)) == L.AT_ABI_VERSION
    assert int(re.search(r"#define MSIG_AT_MAX_POINTS (\d+)", HEADER).group(1)) == L.AT_MAX_POINTS == 256
    kinds = {k: int(v) for k, v in re.findall(r"#define MSIG_AT_BASE_(ZERO|CHANNEL|SHARED|OWN)\s+(\d+)", HEADER)}
    assert kinds == {"ZERO": L.AT_BASE_ZERO, "CHANNEL": L.AT_BASE_CHANNEL, "SHARED": L.AT_BASE_SHARED, "OWN": L.AT_BASE_OWN}
    assert sorted(kinds.values()) == [0, 1, 2, 3]
    # the shape limits are msig.h's
    msig_h = (ROOT / "include" / "msig.h").read_text()
    assert int(re.search(r"#define MSIG_MAX_C\s+(\d+)", msig_h).group(1)) == L.MAX_C
    assert int(re.search(r"#define MSIG_MAX_K\s+(\d+)", msig_h).group(1)) == L.MAX_K
    # the other headers' calls are still there, at the versions they had
    assert (lib.msig_abi_version(), lib.msig_cw_abi_version(), lib.msig_cg_abi_version(), lib.msig_ft_abi_version(),
            lib.msig_gc_abi_version(), lib.msig_aug_abi_version(), lib.msig_st_abi_version(), lib.msig_ab_abi_version()) == (5, 1, 1, 1, 1, 1, 1, 1)


def _path(**kw):
    a = dict(x=A, base=A, kind=L.AT_BASE_OWN, coef=A, v=A, N=N, P=P, C=CH, T=T, K=K, xp=A, dlogits=A)
    a.update(kw)
    return L.lib().msig_at_path(a["x"], a["base"], a["kind"], a["coef"], a["v"], a["N"], a["P"], a["C"], a["T"], a["K"], a["xp"], a["dlogits"], None)


def _reduce(**kw):
    a = dict(dx=A, x=A, base=A, kind=L.AT_BASE_OWN, w=A, N=N, P=P, C=CH, T=T, bin=BIN, map=A, bins=A, chan=A, total=A, scratch=A)
    a.update(kw)
    return L.lib().msig_at_reduce(a["dx"], a["x"], a["base"], a["kind"], a["w"], a["N"], a["P"], a["C"], a["T"], a["bin"], a["map"],
                                  a["bins"], a["chan"], a["total"], a["scratch"], None)


def test_null_pointers():
    for f in ("x", "coef", "xp", "base"):
        assert _path(**{f: None}) == E_NULL, f
    assert _path(dlogits=None) == E_NULL                       # v without a place for its rows
    for kind in (L.AT_BASE_CHANNEL, L.AT_BASE_SHARED):
        assert _path(base=None, kind=kind) == E_NULL
    for f in ("dx", "x", "w", "bins", "chan", "total", "scratch", "base"):
        assert _reduce(**{f: None}) == E_NULL, f


def test_shape_errors():
    for call in (_path, _reduce):
        for bad in (dict(P=0), dict(P=L.AT_MAX_POINTS + 1), dict(P=-1), dict(C=0), dict(C=L.MAX_C + 1), dict(T=15), dict(T=0), dict(N=0),
                    dict(kind=4), dict(kind=-1), dict(N=1 << 30, P=4)):
            assert call(**bad) == E_SHAPE, (call.__name__, bad)
    for k in (1, 0, L.MAX_K + 1):
        assert _path(K=k) == E_SHAPE, k
    for b in (0, -1):
        assert _reduce(bin=b) == E_SHAPE, b
    assert _path(N=(1 << 31) // 2 - 1, P=1, C=16, T=1 << 20) == E_SHAPE          # more workgroups than a grid has
    assert _path(C=16, T=1 << 27) == E_SHAPE and _reduce(C=16, T=1 << 27) == E_SHAPE      # C * T >= 2^31


def test_alignment():
    for f in ("x", "base", "xp"):
        for off in (4, 8):
            assert _path(**{f: A + off}) == E_ALIGN, (f, off)
    for f in ("coef", "v", "dlogits"):
        assert _path(**{f: A + 2}) == E_ALIGN, f
    for f in ("dx", "x", "base", "map"):
        for off in (4, 8):
            assert _reduce(**{f: A + off}) == E_ALIGN, (f, off)
    for f in ("w", "bins", "chan", "total"):
        assert _reduce(**{f: A + 2}) == E_ALIGN, f
    assert _reduce(scratch=A + 4) == E_ALIGN
