"""The decayed running reference (include/msig_rd.h), the C ABI checked without a GPU: the header's calls are exported beside the
unchanged msig_rn.h, the versions and the state layout agree, and each rejection of both entry points happens before a launch (fake,
aligned, never dereferenced device pointers, as in test_running_cabi.py — so only calls that must be refused are made here)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from multimodalsignal_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
RD_HEADER = (ROOT / "include" / "msig_rd.h").read_text()
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
HEAD = 4 * L.MAX_C                   # MSIG_RN_STATE_HEAD
INSIDE = [0.0, -0.0, 1.0, 0.5, float(np.nextafter(1.0, 0.0)), 5e-324, 2.0 ** (-1.0 / 60)]
OUTSIDE = [float(np.nextafter(1.0, 2.0)), -5e-324, -0.5, 2.0, float("inf"), float("-inf"), float("nan")]


def test_msig_rd_header_calls_are_exported_and_msig_rn_is_unchanged():
    code = re.sub(r"/\*.*?\*/", "", RD_HEADER, flags=re.S)
    names = sorted(set(re.findall(r"\b(msig_rd_\w+)\(", code)))
    assert names == ["msig_rd_abi_version", "msig_rd_lv_step", "msig_rd_stats"]
    lib = L.lib()
    for n in names:
        assert getattr(lib, n) is not None
    assert lib.msig_rd_abi_version() == int(re.search(r"#define MSIG_RD_ABI_VERSION (\d+)", RD_HEADER).group(1)) == L.RD_ABI_VERSION == 1
    assert re.search(r"#define MSIG_RD_STATE_C \(3 \* MSIG_MAX_C \+ 2\)", RD_HEADER) and 3 * L.MAX_C + 3 < HEAD       # c and the decay fit the head
    assert lib.msig_rn_state_bytes(0) == HEAD * 8                                                                   # the state block of a session
    rn = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "msig_rn.h").read_text(), flags=re.S)
    assert len(set(re.findall(r"\b(msig_rn_\w+)\(", rn))) == 8
    assert (lib.msig_abi_version(), lib.msig_nr_abi_version(), lib.msig_rec_abi_version(), lib.msig_lv_abi_version(), lib.msig_rn_abi_version()) == (5, 1, 1, 1, 1)


def _addr():
    keep_alive = (C.c_char * 8192)()
    return keep_alive, (C.addressof(keep_alive) + 255) // 256 * 256


def _arr(ctype, v):
    return None if v is None else (ctype * max(1, len(v)))(*v)


# ---- msig_rd_stats ---------------------------------------------------------------------------------------------------------------------
def _stats(addr, **kw):
    """Over fake pointers: sig at addr, the sums at addr + 512, the table at addr + 1024.  L = 1000, T = 100, S = 30: 31 windows."""
    cols = kw.get("cols", [2, 0, 1])
    a = dict(sig=addr, L=1000, C_all=5, cols=_arr(C.c_int32, cols), C=3 if cols is None else len(cols), mask=0b10, T=100, S=30, N=31, decay=0.5,
             sums=addr + 512, table=addr + 1024)
    a.update({k: v for k, v in kw.items() if k != "cols"})
    return L.lib().msig_rd_stats(a["sig"], a["L"], a["C_all"], a["cols"], a["C"], a["mask"], a["T"], a["S"], a["sums"], a["N"], a["decay"], a["table"], None)


@pytest.mark.parametrize("name", ["sig", "cols", "sums", "table"])
def test_stats_null_pointers(name):
    _k, addr = _addr()
    assert _stats(addr, **{name: None}) == E_NULL


SHAPES = [dict(L=0), dict(L=-5), dict(T=0), dict(T=-1), dict(S=0), dict(S=-2), dict(C_all=0), dict(C=0), dict(C=-1), dict(C=L.MAX_C + 1),
          dict(cols=[0, 5, 1]), dict(cols=[-1]), dict(cols=[0, 1, 2], C_all=2), dict(N=0), dict(N=-1), dict(N=32), dict(L=99, N=1)]


@pytest.mark.parametrize("kw", SHAPES + [dict(decay=d) for d in OUTSIDE], ids=str)
def test_stats_refuses(kw):
    _k, addr = _addr()
    assert _stats(addr, **kw) == E_SHAPE


def test_the_stats_bounds_are_exact():
    """What is inside passes every shape check and fails only at a deliberately misaligned table, the last check before a launch."""
    _k, addr = _addr()
    for d in INSIDE:
        assert _stats(addr, decay=d, table=addr + 1028) == E_ALIGN, d
    assert _stats(addr, N=1, table=addr + 1028) == E_ALIGN and _stats(addr, N=31, table=addr + 1028) == E_ALIGN
    assert _stats(addr, N=1, L=100, table=addr + 1028) == E_ALIGN and _stats(addr, N=1, S=2000, table=addr + 1028) == E_ALIGN


@pytest.mark.parametrize("name", ["sig", "sums", "table"])
def test_stats_misaligned_float64_buffers(name):
    _k, addr = _addr()
    base = {"sig": addr, "sums": addr + 512, "table": addr + 1024}[name]
    for off in (1, 4):
        assert _stats(addr, **{name: base + off}) == E_ALIGN


# ---- msig_rd_lv_step -------------------------------------------------------------------------------------------------------------------
def _step(addr, **kw):
    """test_running_cabi's live call: a pool of 4 rings of R = 500 rows of 5 columns at addr, the table at addr + 1024, the states at
    addr + 4096; T = 100, S = 30; session 1 holds 1000 samples (windows 17 .. 30 complete and in its ring), session 3 holds 130."""
    a = dict(pool=addr, sessions=4, R=500, ring_bytes=500 * 5 * 8, C_all=5, cols=[2, 0, 1], C=None, mask=0b10, T=100, S=30, decay=0.5, state=addr + 4096,
             state_bytes=HEAD * 8, sess=[1, 1, 3, 3], win=[17, 18, 0, 1], written=[1000, 1000, 130, 130], next=[17, 17, 0, 0], B=None,
             table=addr + 1024)
    a.update(kw)
    Cn = a["C"] if a["C"] is not None else (3 if a["cols"] is None else len(a["cols"]))
    B = a["B"] if a["B"] is not None else len(a["win"] or a["sess"])
    return L.lib().msig_rd_lv_step(a["pool"], a["sessions"], a["R"], a["ring_bytes"], a["C_all"], _arr(C.c_int32, a["cols"]), Cn, a["mask"], a["T"], a["S"],
                                   a["decay"], a["state"], a["state_bytes"], _arr(C.c_int32, a["sess"]), _arr(C.c_int64, a["win"]),
                                   _arr(C.c_int64, a["written"]), _arr(C.c_int64, a["next"]), B, a["table"], None)


@pytest.mark.parametrize("name", ["pool", "cols", "state", "sess", "win", "written", "next", "table"])
def test_step_null_pointers(name):
    _k, addr = _addr()
    assert _step(addr, **{name: None}) == E_NULL


POOL = [dict(sessions=0), dict(sessions=-1), dict(sessions=L.LV_MAX_SESSIONS + 1), dict(R=0), dict(R=-3), dict(R=1 << 31, ring_bytes=1 << 40),
        dict(C_all=0), dict(ring_bytes=500 * 5 * 8 - 8), dict(ring_bytes=0)]
ROWS = [dict(win=[17, 18, 0, 2]), dict(sess=[1], win=[31], written=[1000], next=[31]), dict(sess=[3], win=[0], written=[99], next=[0]),
        dict(sess=[1], win=[16], written=[1000], next=[16]), dict(sess=[1], win=[0], written=[601], next=[0]), dict(R=99, ring_bytes=99 * 5 * 8),
        dict(B=0), dict(B=-1), dict(sess=[1, 1, 4, 4]), dict(sess=[1, 1, -1, 3]), dict(win=[17, 18, -1, 0]),
        dict(T=0), dict(S=0), dict(S=-1), dict(C=0), dict(C=L.MAX_C + 1, cols=[0] * (L.MAX_C + 1)), dict(cols=[0, 5, 1]), dict(cols=[-1])]
STATE = [dict(state_bytes=HEAD * 8 - 8), dict(state_bytes=0), dict(state_bytes=-8),
         dict(next=[18, 17, 0, 0]), dict(next=[17, 17, 1, 0]), dict(win=[17, 19, 0, 1]), dict(win=[18, 17, 0, 1], next=[18, 18, 0, 0]),
         dict(win=[17, 17, 0, 1]),
         dict(sess=[1, 3, 1, 3], win=[17, 0, 18, 1], written=[1000, 130, 1000, 130], next=[17, 0, 18, 1]),
         dict(sess=[1, 3, 3, 1], win=[17, 0, 1, 18], written=[1000, 130, 130, 1000], next=[17, 0, 0, 18])]


@pytest.mark.parametrize("kw", POOL + ROWS + STATE + [dict(decay=d) for d in OUTSIDE], ids=str)
def test_step_refuses(kw):
    _k, addr = _addr()
    assert _step(addr, **kw) == E_SHAPE


def test_the_step_bounds_are_exact():
    _k, addr = _addr()
    bad = addr + 1028
    for d in INSIDE:
        assert _step(addr, decay=d, table=bad) == E_ALIGN, d
    assert _step(addr, state_bytes=HEAD * 8, table=bad) == E_ALIGN and _step(addr, state_bytes=HEAD * 8 + 800, table=bad) == E_ALIGN
    assert _step(addr, sess=[1], win=[30], written=[1000], next=[30], table=bad) == E_ALIGN
    assert _step(addr, sess=[1], win=[17], written=[1000], next=[17], table=bad) == E_ALIGN
    assert _step(addr, sess=[1], win=[0], written=[500], next=[0], table=bad) == E_ALIGN
    assert _step(addr, sess=[1, 1, 1], win=[17, 18, 19], written=[1000] * 3, next=[17, 0, 0], table=bad) == E_ALIGN


def test_step_misaligned_buffers_and_strides():
    _k, addr = _addr()
    for name, base in (("pool", addr), ("table", addr + 1024), ("state", addr + 4096)):
        for off in (1, 4):
            assert _step(addr, **{name: base + off}) == E_ALIGN
    assert _step(addr, ring_bytes=500 * 5 * 8 + 4) == E_ALIGN and _step(addr, state_bytes=HEAD * 8 + 4) == E_ALIGN


def test_the_order_of_the_checks():
    """NULL before shape before alignment; the decay where msig_rn.h's calls check K."""
    _k, addr = _addr()
    nan = float("nan")
    assert _stats(addr, table=None, decay=nan, L=0, sig=addr + 4) == E_NULL
    assert _stats(addr, decay=nan, table=addr + 1028) == E_SHAPE and _stats(addr, decay=1.5, sig=addr + 4) == E_SHAPE
    assert _stats(addr, N=32, decay=0.5, sums=addr + 516) == E_SHAPE
    assert _step(addr, next=None, B=0, decay=nan) == E_NULL
    assert _step(addr, decay=nan, state=addr + 4100) == E_SHAPE and _step(addr, decay=-1.0, table=addr + 1028) == E_SHAPE
    assert _step(addr, next=[18, 17, 0, 0], state=addr + 4100) == E_SHAPE
    assert _step(addr, win=[17, 18, 0, 2], decay=nan) == E_SHAPE
    assert _step(addr, state=addr + 4100) == E_ALIGN
