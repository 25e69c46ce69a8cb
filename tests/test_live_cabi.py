"""Sample rings of many sessions and mixed window batches (include/msig_lv.h), the C ABI checked without a GPU: the header's calls
are exported beside the unchanged headers, the versions agree, and each rejection happens before a launch (fake, aligned, never
dereferenced device pointers, as in test_recording_cabi.py — so only calls that must be refused are made here)."""
import ctypes as C
import re
from pathlib import Path

import pytest

from multimodalsignal_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
LV_HEADER = (ROOT / "include" / "msig_lv.h").read_text()
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3


def test_msig_lv_header_calls_are_exported_and_the_other_headers_are_unchanged():
    names = sorted(set(re.findall(r"\b(msig_lv_\w+)\(", re.sub(r"/\*.*?\*/", "", LV_HEADER, flags=re.S))))
    assert names == ["msig_lv_abi_version", "msig_lv_push", "msig_lv_windows_multi"]
    lib = L.lib()
    for n in names:
        assert getattr(lib, n) is not None
    assert lib.msig_lv_abi_version() == int(re.search(r"#define MSIG_LV_ABI_VERSION (\d+)", LV_HEADER).group(1)) == L.LV_ABI_VERSION == 1
    assert int(re.search(r"#define MSIG_LV_MAX_SESSIONS (\d+)", LV_HEADER).group(1)) == L.LV_MAX_SESSIONS
    assert len(set(re.findall(r"\b(msig_\w+)\(", (ROOT / "include" / "msig.h").read_text()))) == 26
    rec = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "msig_rec.h").read_text(), flags=re.S)
    assert len(set(re.findall(r"\b(msig_rec_\w+)\(", rec))) == 6
    assert (lib.msig_abi_version(), lib.msig_nr_abi_version(), lib.msig_en_abi_version(), lib.msig_st_abi_version(),
            lib.msig_rec_abi_version()) == (5, 1, 1, 1, 1)
    assert lib.msig_rec_scratch_bytes() == 512 * 2 * L.MAX_C * 8


def _addr():
    keep_alive = (C.c_char * 8192)()
    return keep_alive, (C.addressof(keep_alive) + 255) // 256 * 256


def _multi(n=2, stride=1 << 20, slots=None):
    m = L.Multi()
    m.n, m.stride_bytes, m.form_folds = n, stride, 1
    for i, s in enumerate(slots if slots is not None else range(max(n, 0))):
        if i < L.MAX_FOLDS:
            m.slot[i] = s
    return m


def _arr(ctype, v):
    return None if v is None else (ctype * max(1, len(v)))(*v)


def _push(addr, **kw):
    """msig_lv_push over fake pointers: a pool of 4 rings of R = 500 rows of 5 columns at addr, the staging buffer at addr + 2048.
    Sessions 2 and 0 hold 1234 and 0 samples and get 500 and 7 more."""
    a = dict(pool=addr, sessions=4, R=500, ring_bytes=500 * 5 * 8, C_all=5, sess=[2, 0], written=[1234, 0], len=[500, 7], n=None,
             staging=addr + 2048)
    a.update(kw)
    n = a["n"] if a["n"] is not None else len(a["len"] or a["sess"])
    return L.lib().msig_lv_push(a["pool"], a["sessions"], a["R"], a["ring_bytes"], a["C_all"], _arr(C.c_int32, a["sess"]),
                                _arr(C.c_int64, a["written"]), _arr(C.c_int64, a["len"]), n, a["staging"], None)


def _windows(addr, **kw):
    """msig_lv_windows_multi over fake pointers: the same pool; T = 100, S = 30; session 1 holds 1000 samples — windows 17 .. 30 are
    complete and still in its ring — and session 3 holds 130: windows 0 and 1."""
    a = dict(pool=addr, sessions=4, R=500, ring_bytes=500 * 5 * 8, C_all=5, cols=[2, 0, 1], C=None, mask=0b10, T=100, S=30, sess=[1, 1, 3, 1],
             win=[17, 18, 1, 30], written=[1000, 1000, 130, 1000], B=None, stats=addr + 1024, out=addr + 2048, m=_multi())
    a.update(kw)
    Cn = a["C"] if a["C"] is not None else (3 if a["cols"] is None else len(a["cols"]))
    B = a["B"] if a["B"] is not None else len(a["win"] or a["sess"])
    return L.lib().msig_lv_windows_multi(a["pool"], a["sessions"], a["R"], a["ring_bytes"], a["C_all"], _arr(C.c_int32, a["cols"]), Cn, a["mask"],
                                         a["T"], a["S"], _arr(C.c_int32, a["sess"]), _arr(C.c_int64, a["win"]), _arr(C.c_int64, a["written"]), B,
                                         a["stats"], a["out"], None if a["m"] is None else C.byref(a["m"]), None)


CALLS = {"push": _push, "windows": _windows}


@pytest.mark.parametrize("which, name", [("push", n) for n in ("pool", "sess", "written", "len", "staging")]
                         + [("windows", n) for n in ("pool", "cols", "sess", "win", "written", "stats", "out", "m")])
def test_null_pointers(which, name):
    _k, addr = _addr()
    assert CALLS[which](addr, **{name: None}) == E_NULL


POOL = [dict(sessions=0), dict(sessions=-1), dict(sessions=L.LV_MAX_SESSIONS + 1), dict(R=0), dict(R=-3), dict(R=1 << 31, ring_bytes=1 << 40),
        dict(C_all=0), dict(ring_bytes=500 * 5 * 8 - 8), dict(ring_bytes=0)]


@pytest.mark.parametrize("which", ["push", "windows"])
@pytest.mark.parametrize("kw", POOL, ids=str)
def test_bad_pools(which, kw):
    _k, addr = _addr()
    assert CALLS[which](addr, **kw) == E_SHAPE


@pytest.mark.parametrize("kw", [dict(len=[501, 7]), dict(len=[500, -1]), dict(sess=[2, 2]), dict(sess=[0, 3, 1, 0], written=[0] * 4, len=[1] * 4),
                                dict(sess=[2, 4]), dict(sess=[-1, 0]), dict(written=[-1, 0]), dict(n=0), dict(n=-2),
                                dict(sess=[0, 1, 2, 3, 0], written=[0] * 5, len=[1] * 5), dict(sess=[0, 1], sessions=1)], ids=str)
def test_push_refuses(kw):
    """A chunk longer than R, the same session twice, a session outside the pool, more chunks than sessions."""
    _k, addr = _addr()
    assert _push(addr, **kw) == E_SHAPE


@pytest.mark.parametrize("kw", [dict(win=[17, 18, 1, 31]),                          # 31 * 30 + 100 = 1030 > 1000: not yet complete
                                dict(win=[17, 18, 2, 30]),                          # session 3: 2 * 30 + 100 = 160 > 130
                                dict(sess=[3], win=[0], written=[99]),              # shorter than one window
                                dict(win=[16, 18, 1, 30]),                          # 16 * 30 = 480 < 1000 - 500: already overwritten
                                dict(win=[0, 18, 1, 30]),
                                dict(sess=[1], win=[0], written=[601]),             # R = 500, T = 100: sample 0 went at 501 samples
                                dict(R=99, ring_bytes=99 * 5 * 8),                  # a ring shorter than a window holds none
                                dict(B=0), dict(B=-1), dict(sess=[1, 4, 3, 1]), dict(sess=[1, -1, 3, 1]), dict(win=[17, -1, 1, 30]),
                                dict(T=0), dict(S=0), dict(S=-1), dict(C=0), dict(C=L.MAX_C + 1, cols=[0] * (L.MAX_C + 1)),
                                dict(cols=[0, 5, 1]), dict(cols=[-1])], ids=str)
def test_windows_refuses(kw):
    _k, addr = _addr()
    assert _windows(addr, **kw) == E_SHAPE


def test_the_ring_specific_bounds_are_exact():
    """With 1000 samples in a ring of 500, T = 100, S = 30: window 30 (samples 900 .. 999) is the last complete one and window 17
    (sample 510 on) the first whole one — both pass the ring's checks and fail only at the deliberately small arena."""
    _k, addr = _addr()
    small = _multi(stride=256)                                                       # < 4 * 1 * 3 * 100 bytes of one row: the LAST check
    assert _windows(addr, sess=[1], win=[30], written=[1000], m=small) == E_SHAPE
    assert _windows(addr, sess=[1], win=[30], written=[1000], m=small, out=addr + 2052) == E_ALIGN       # ... so the ring's checks passed
    assert _windows(addr, sess=[1], win=[17], written=[1000], m=small, out=addr + 2052) == E_ALIGN
    assert _windows(addr, sess=[1], win=[16], written=[1000], m=small, out=addr + 2052) == E_SHAPE
    assert _windows(addr, sess=[1], win=[31], written=[1000], m=small, out=addr + 2052) == E_SHAPE
    assert _windows(addr, sess=[1], win=[0], written=[500], m=small, out=addr + 2052) == E_ALIGN         # nothing overwritten yet


@pytest.mark.parametrize("which, name", [("push", "pool"), ("push", "staging"), ("windows", "pool"), ("windows", "stats")])
def test_misalignment_of_the_float64_buffers(which, name):
    _k, addr = _addr()
    base = {"pool": addr, "stats": addr + 1024, "staging": addr + 2048}[name]
    for off in (1, 4):
        assert CALLS[which](addr, **{name: base + off}) == E_ALIGN


@pytest.mark.parametrize("which", ["push", "windows"])
def test_rings_are_a_multiple_of_8_bytes_apart(which):
    _k, addr = _addr()
    assert CALLS[which](addr, ring_bytes=500 * 5 * 8 + 4) == E_ALIGN


def test_the_batch_is_16_byte_aligned():
    _k, addr = _addr()
    for off in (4, 8):
        assert _windows(addr, out=addr + 2048 + off) == E_ALIGN


def test_msig_multi_is_checked_too_and_a_batch_must_fit_its_arena():
    _k, addr = _addr()
    assert _windows(addr, m=_multi(n=0)) == E_SHAPE
    assert _windows(addr, m=_multi(n=L.MAX_FOLDS + 1)) == E_SHAPE
    assert _windows(addr, m=_multi(slots=[1, 1])) == E_SHAPE
    assert _windows(addr, m=_multi(stride=1000)) == E_ALIGN
    assert _windows(addr, m=_multi(stride=4608)) == E_SHAPE          # 18 * 256 < the 4 * 3 * 100 * 4 = 4 800 bytes of one batch


def test_the_order_of_the_checks():
    """NULL before shape before alignment, the call's own checks before msig_multi's, as the header lists them."""
    _k, addr = _addr()
    assert _push(addr, staging=None, R=0, pool=addr + 4) == E_NULL
    assert _push(addr, sess=[2, 2], pool=addr + 4) == E_SHAPE
    assert _windows(addr, m=None, B=0) == E_NULL
    assert _windows(addr, win=[17, 18, 1, 31], stats=addr + 1028) == E_SHAPE
    assert _windows(addr, out=addr + 2052, m=_multi(n=0)) == E_ALIGN
