"""Gap-tolerant running references (include/msig_gp.h), the C ABI checked without a GPU: the header's calls are exported beside the
unchanged msig_rn.h, msig_rd.h and msig_lv.h, the versions, the mode struct and the state layout agree, and every rejection of every
entry point happens before a launch (fake, aligned, never dereferenced device pointers, as in test_running_cabi.py — so only calls
that must be refused are made here)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from multimodalsignal_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
GP_HEADER = (ROOT / "include" / "msig_gp.h").read_text()
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
HEAD = 6 * L.MAX_C                   # MSIG_GP_STATE_HEAD
PART = 3 * L.MAX_C                   # MSIG_GP_SUM_DOUBLES
EXP, TRAIL, DEC = L.GP_EXPANDING, L.GP_TRAILING, L.GP_DECAYED
MODES_INSIDE = [(EXP, 0, 0.0), (EXP, -7, float("nan")), (TRAIL, 1, 0.0), (TRAIL, L.RN_MAX_K, 5.0), (DEC, 0, 0.0), (DEC, -1, -0.0), (DEC, 0, 1.0),
                (DEC, 0, float(np.nextafter(1.0, 0.0))), (DEC, 0, 5e-324), (DEC, 0, 2.0 ** (-1.0 / 60))]
MODES_OUTSIDE = [(-1, 0, 0.5), (3, 1, 0.5), (TRAIL, 0, 0.5), (TRAIL, -1, 0.5), (TRAIL, L.RN_MAX_K + 1, 0.5), (DEC, 1, float(np.nextafter(1.0, 2.0))),
                 (DEC, 1, -5e-324), (DEC, 1, 2.0), (DEC, 1, float("inf")), (DEC, 1, float("-inf")), (DEC, 1, float("nan"))]


def test_msig_gp_header_calls_are_exported_and_the_other_headers_are_unchanged():
    code = re.sub(r"/\*.*?\*/", "", GP_HEADER, flags=re.S)
    names = sorted(set(re.findall(r"\b(msig_gp_\w+)\(", code)))
    assert names == ["msig_gp_abi_version", "msig_gp_lv_skip", "msig_gp_lv_step", "msig_gp_lv_windows_multi", "msig_gp_pivot", "msig_gp_state_bytes",
                     "msig_gp_stats", "msig_gp_struct_bytes", "msig_gp_sums", "msig_gp_windows", "msig_gp_windows_multi"]
    lib = L.lib()
    for n in names:
        assert getattr(lib, n) is not None
    assert lib.msig_gp_abi_version() == int(re.search(r"#define MSIG_GP_ABI_VERSION (\d+)", GP_HEADER).group(1)) == L.GP_ABI_VERSION == 1
    assert lib.msig_gp_struct_bytes() == C.sizeof(L.GpMode) == 16
    assert re.search(r"#define MSIG_GP_SUM_DOUBLES \(3 \* MSIG_MAX_C\)", GP_HEADER) and re.search(r"#define MSIG_GP_STATE_HEAD \(6 \* MSIG_MAX_C\)", GP_HEADER)
    assert [int(re.search(rf"#define MSIG_GP_{k} (\d)", GP_HEADER).group(1)) for k in ("EXPANDING", "TRAILING", "DECAYED")] == [EXP, TRAIL, DEC]
    for h, count in (("msig_rn.h", 8), ("msig_rd.h", 3), ("msig_lv.h", 3)):
        text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / h).read_text(), flags=re.S)
        assert len(set(re.findall(r"\b(" + h[:-2] + r"_\w+)\(", text))) == count, h
    assert (lib.msig_abi_version(), lib.msig_nr_abi_version(), lib.msig_rec_abi_version(), lib.msig_lv_abi_version(), lib.msig_rn_abi_version(),
            lib.msig_rd_abi_version()) == (5, 1, 1, 1, 1, 1)


def test_state_bytes():
    lib = L.lib()
    assert lib.msig_gp_state_bytes(0) == HEAD * 8 and lib.msig_gp_state_bytes(1) == (HEAD + PART) * 8
    assert lib.msig_gp_state_bytes(L.RN_MAX_K) == (HEAD + L.RN_MAX_K * PART) * 8
    assert lib.msig_gp_state_bytes(-1) == E_SHAPE and lib.msig_gp_state_bytes(L.RN_MAX_K + 1) == E_SHAPE
    assert lib.msig_rn_state_bytes(0) == 4 * L.MAX_C * 8 and lib.msig_rn_state_bytes(2) == (4 * L.MAX_C + 2 * 2 * L.MAX_C) * 8       # unchanged


def _addr():
    keep_alive = (C.c_char * 16384)()
    return keep_alive, (C.addressof(keep_alive) + 255) // 256 * 256


def _arr(ctype, v):
    return None if v is None else (ctype * max(1, len(v)))(*v)


def _mode(m):
    return None if m is None else C.byref(L.GpMode(*m))


# ---- the recording calls ---------------------------------------------------------------------------------------------------------------
def _rec(addr, call, **kw):
    """Over fake pointers: sig at addr, the pivot record at addr + 512, the window records at + 1024, the table at + 2048, the coverage
    at + 3072, out_x at + 4096.  L = 1000, T = 100, S = 30: 31 windows."""
    cols = kw.get("cols", [2, 0, 1])
    a = dict(sig=addr, L=1000, C_all=5, cols=_arr(C.c_int32, cols), C=3 if cols is None else len(cols), mask=0b10, T=100, S=30, N=31, n0=0, B=31,
             mode=(DEC, 0, 0.5), pivot=addr + 512, sums=addr + 1024, table=addr + 2048, coverage=addr + 3072, out=addr + 4096, m="valid")
    a.update({k: v for k, v in kw.items() if k != "cols"})
    head = (a["sig"], a["L"], a["C_all"], a["cols"], a["C"], a["mask"], a["T"], a["S"])
    lib = L.lib()
    if call == "pivot":
        return lib.msig_gp_pivot(*head, a["N"], a["pivot"], None)
    if call == "sums":
        return lib.msig_gp_sums(*head, a["pivot"], a["n0"], a["B"], a["sums"], None)
    if call == "stats":
        return lib.msig_gp_stats(*head, a["pivot"], a["sums"], a["N"], _mode(a["mode"]), a["table"], a["coverage"], None)
    if call == "windows":
        return lib.msig_gp_windows(*head, a["n0"], a["B"], a["table"], a["out"], None)
    multi = None
    if a["m"] is not None:
        multi = L.Multi()
        multi.n, multi.stride_bytes = 2, 1 << 20
        multi.slot[0], multi.slot[1] = 0, 1
        if a["m"] == "small":
            multi.stride_bytes = 4 * a["B"] * a["C"] * a["T"] // 256 * 256 - 256       # a multiple of 256 that one batch does not fit
        multi = C.byref(multi)
    return lib.msig_gp_windows_multi(*head, a["n0"], a["B"], a["table"], a["out"], multi, None)


NULLS = {"pivot": ["sig", "cols", "pivot"], "sums": ["sig", "cols", "pivot", "sums"], "stats": ["sig", "cols", "pivot", "sums", "mode", "table", "coverage"],
         "windows": ["sig", "cols", "table", "out"], "windows_multi": ["sig", "cols", "table", "out", "m"]}


@pytest.mark.parametrize("call,name", [(c, n) for c, ns in NULLS.items() for n in ns])
def test_recording_calls_null_pointers(call, name):
    _k, addr = _addr()
    assert _rec(addr, call, **{name: None}) == E_NULL


SHAPES = [dict(L=0), dict(L=-5), dict(T=0), dict(T=-1), dict(S=0), dict(S=-2), dict(C_all=0), dict(C=0), dict(C=-1), dict(C=L.MAX_C + 1),
          dict(cols=[0, 5, 1]), dict(cols=[-1]), dict(cols=[0, 1, 2], C_all=2)]
COUNT = {"pivot": [dict(N=0), dict(N=-1), dict(N=32), dict(L=99, N=1)], "stats": [dict(N=0), dict(N=-1), dict(N=32), dict(L=99, N=1)],
         "sums": [dict(n0=-1), dict(B=0), dict(B=32), dict(n0=1, B=31), dict(n0=31, B=1)],
         "windows": [dict(n0=-1), dict(B=0), dict(B=32), dict(n0=1, B=31), dict(n0=31, B=1)],
         "windows_multi": [dict(n0=-1), dict(B=0), dict(n0=1, B=31), dict(m="small")]}


@pytest.mark.parametrize("call,kw", [(c, kw) for c in NULLS for kw in SHAPES + COUNT[c]], ids=str)
def test_recording_calls_refuse(call, kw):
    _k, addr = _addr()
    assert _rec(addr, call, **kw) == E_SHAPE


@pytest.mark.parametrize("mode", MODES_OUTSIDE, ids=str)
def test_stats_refuses_a_mode(mode):
    _k, addr = _addr()
    assert _rec(addr, "stats", mode=mode) == E_SHAPE


def test_the_recording_bounds_are_exact():
    """What is inside passes every shape check and fails only at a deliberately misaligned buffer, the last check before a launch."""
    _k, addr = _addr()
    for mode in MODES_INSIDE:
        assert _rec(addr, "stats", mode=mode, coverage=addr + 3076) == E_ALIGN, mode
    for kw in (dict(N=1), dict(N=31), dict(N=1, L=100), dict(N=1, S=2000)):
        assert _rec(addr, "stats", table=addr + 2052, **kw) == E_ALIGN and _rec(addr, "pivot", pivot=addr + 516, **kw) == E_ALIGN
    for kw in (dict(n0=30, B=1), dict(n0=0, B=31), dict(n0=7, B=24)):
        assert _rec(addr, "sums", sums=addr + 1028, **kw) == E_ALIGN and _rec(addr, "windows", out=addr + 4104, **kw) == E_ALIGN


ALIGNED = {"pivot": ["sig", "pivot"], "sums": ["sig", "pivot", "sums"], "stats": ["sig", "pivot", "sums", "table", "coverage"],
           "windows": ["sig", "table"], "windows_multi": ["sig", "table"]}


@pytest.mark.parametrize("call,name", [(c, n) for c, ns in ALIGNED.items() for n in ns])
def test_recording_calls_misaligned_float64_buffers(call, name):
    _k, addr = _addr()
    base = {"sig": addr, "pivot": addr + 512, "sums": addr + 1024, "table": addr + 2048, "coverage": addr + 3072}[name]
    for off in (1, 4):
        assert _rec(addr, call, **{name: base + off}) == E_ALIGN


@pytest.mark.parametrize("call", ["windows", "windows_multi"])
def test_rows_need_a_16_byte_aligned_batch(call):
    _k, addr = _addr()
    for off in (4, 8):
        assert _rec(addr, call, out=addr + 4096 + off) == E_ALIGN


# ---- the live calls --------------------------------------------------------------------------------------------------------------------
def _live(addr, call, **kw):
    """test_running_cabi's live call: a pool of 4 rings of R = 500 rows of 5 columns at addr, the table at addr + 1024, the coverage at
    addr + 2048, the states at addr + 4096, out_x at + 8192; T = 100, S = 30; session 1 holds 1000 samples (windows 17 .. 30 complete
    and in its ring), session 3 holds 130."""
    a = dict(pool=addr, sessions=4, R=500, ring_bytes=500 * 5 * 8, C_all=5, cols=[2, 0, 1], C=None, mask=0b10, T=100, S=30, mode=(DEC, 0, 0.5),
             state=addr + 4096, state_bytes=HEAD * 8, sess=[1, 1, 3, 3], win=[17, 18, 0, 1], written=[1000, 1000, 130, 130], next=[17, 17, 0, 0],
             B=None, table=addr + 1024, coverage=addr + 2048, out=addr + 8192, m="valid")
    a.update(kw)
    Cn = a["C"] if a["C"] is not None else (3 if a["cols"] is None else len(a["cols"]))
    B = a["B"] if a["B"] is not None else len(a["win"] or a["sess"])
    pool = (a["pool"], a["sessions"], a["R"], a["ring_bytes"], a["C_all"])
    rows = (_arr(C.c_int32, a["cols"]), Cn, a["mask"], a["T"], a["S"])
    batch = (_arr(C.c_int32, a["sess"]), _arr(C.c_int64, a["win"]), _arr(C.c_int64, a["written"]))
    if call == "step":
        return L.lib().msig_gp_lv_step(*pool, *rows, _mode(a["mode"]), a["state"], a["state_bytes"], *batch, _arr(C.c_int64, a["next"]), B, a["table"],
                                       a["coverage"], None)
    multi = None
    if a["m"] is not None:
        multi = L.Multi()
        multi.n, multi.stride_bytes = 2, (1 << 20 if a["m"] == "valid" else 4 * B * Cn * a["T"] // 256 * 256 - 256)
        multi.slot[0], multi.slot[1] = 0, 1
        multi = C.byref(multi)
    return L.lib().msig_gp_lv_windows_multi(*pool, *rows, *batch, B, a["table"], a["out"], multi, None)


@pytest.mark.parametrize("call,name", [("step", n) for n in ("pool", "cols", "mode", "state", "sess", "win", "written", "next", "table", "coverage")] +
                         [("windows", n) for n in ("pool", "cols", "sess", "win", "written", "table", "out", "m")])
def test_live_calls_null_pointers(call, name):
    _k, addr = _addr()
    assert _live(addr, call, **{name: None}) == E_NULL


POOL = [dict(sessions=0), dict(sessions=-1), dict(sessions=L.LV_MAX_SESSIONS + 1), dict(R=0), dict(R=-3), dict(R=1 << 31, ring_bytes=1 << 40),
        dict(C_all=0), dict(ring_bytes=500 * 5 * 8 - 8), dict(ring_bytes=0)]
ROWS = [dict(sess=[1], win=[31], written=[1000], next=[31]), dict(sess=[3], win=[0], written=[99], next=[0]),
        dict(sess=[1], win=[16], written=[1000], next=[16]), dict(sess=[1], win=[0], written=[601], next=[0]), dict(R=99, ring_bytes=99 * 5 * 8),
        dict(B=0), dict(B=-1), dict(sess=[1, 1, 4, 4]), dict(sess=[1, 1, -1, 3]), dict(win=[17, 18, -1, 0]),
        dict(T=0), dict(S=0), dict(S=-1), dict(C=0), dict(C=L.MAX_C + 1, cols=[0] * (L.MAX_C + 1)), dict(cols=[0, 5, 1]), dict(cols=[-1])]
STATE = [dict(state_bytes=HEAD * 8 - 8), dict(state_bytes=0), dict(state_bytes=-8), dict(mode=(TRAIL, 2, 0.0), state_bytes=(HEAD + 2 * PART) * 8 - 8),
         dict(win=[17, 18, 0, 2]), dict(next=[18, 17, 0, 0]), dict(next=[17, 17, 1, 0]), dict(win=[17, 19, 0, 1]),
         dict(win=[18, 17, 0, 1], next=[18, 18, 0, 0]), dict(win=[17, 17, 0, 1]),
         dict(sess=[1, 3, 1, 3], win=[17, 0, 18, 1], written=[1000, 130, 1000, 130], next=[17, 0, 18, 1]),
         dict(sess=[1, 3, 3, 1], win=[17, 0, 1, 18], written=[1000, 130, 130, 1000], next=[17, 0, 0, 18])]


@pytest.mark.parametrize("kw", POOL + ROWS + STATE + [dict(mode=m) for m in MODES_OUTSIDE], ids=str)
def test_step_refuses(kw):
    _k, addr = _addr()
    assert _live(addr, "step", **kw) == E_SHAPE


@pytest.mark.parametrize("kw", POOL + ROWS + [dict(m="small")], ids=str)
def test_live_rows_refuse(kw):
    _k, addr = _addr()
    assert _live(addr, "windows", **kw) == E_SHAPE


def test_the_step_bounds_are_exact():
    _k, addr = _addr()
    bad = addr + 1028
    for mode in MODES_INSIDE:
        K = mode[1] if mode[0] == TRAIL else 0
        assert _live(addr, "step", mode=mode, state_bytes=(HEAD + K * PART) * 8, table=bad) == E_ALIGN, mode
    assert _live(addr, "step", state_bytes=HEAD * 8 + 800, table=bad) == E_ALIGN
    assert _live(addr, "step", sess=[1], win=[30], written=[1000], next=[30], table=bad) == E_ALIGN
    assert _live(addr, "step", sess=[1], win=[17], written=[1000], next=[17], table=bad) == E_ALIGN
    assert _live(addr, "step", sess=[1], win=[0], written=[500], next=[0], table=bad) == E_ALIGN
    assert _live(addr, "step", sess=[1, 1, 1], win=[17, 18, 19], written=[1000] * 3, next=[17, 0, 0], table=bad) == E_ALIGN
    assert _live(addr, "windows", sess=[1, 3, 1], win=[30, 0, 17], written=[1000, 130, 1000], table=bad) == E_ALIGN


def test_live_calls_misaligned_buffers_and_strides():
    _k, addr = _addr()
    for name, base in (("pool", addr), ("table", addr + 1024), ("coverage", addr + 2048), ("state", addr + 4096)):
        for off in (1, 4):
            assert _live(addr, "step", **{name: base + off}) == E_ALIGN
    assert _live(addr, "step", ring_bytes=500 * 5 * 8 + 4) == E_ALIGN and _live(addr, "step", state_bytes=HEAD * 8 + 4) == E_ALIGN
    for name, base in (("pool", addr), ("table", addr + 1024)):
        assert _live(addr, "windows", **{name: base + 4}) == E_ALIGN
    assert _live(addr, "windows", out=addr + 8200) == E_ALIGN and _live(addr, "windows", ring_bytes=500 * 5 * 8 + 4) == E_ALIGN


def _skip(addr, **kw):
    a = dict(pool=addr, sessions=4, R=500, ring_bytes=500 * 5 * 8, C_all=5, sess=[1, 3], written=[1000, 130], len=[500, 0], n=None)
    a.update(kw)
    n = a["n"] if a["n"] is not None else len(a["sess"] or a["len"])
    return L.lib().msig_gp_lv_skip(a["pool"], a["sessions"], a["R"], a["ring_bytes"], a["C_all"], _arr(C.c_int32, a["sess"]), _arr(C.c_int64, a["written"]),
                                   _arr(C.c_int64, a["len"]), n, None)


def test_skip_refusals_are_msig_lv_pushs():
    _k, addr = _addr()
    for name in ("pool", "sess", "written", "len"):
        assert _skip(addr, **{name: None}) == E_NULL
    for kw in POOL + [dict(n=0), dict(n=-1), dict(n=5, sess=[0, 1, 2, 3, 0], written=[0] * 5, len=[1] * 5), dict(sess=[1, 4]), dict(sess=[-1, 3]),
                      dict(sess=[1, 1]), dict(written=[-1, 0]), dict(len=[-1, 0]), dict(len=[501, 0])]:
        assert _skip(addr, **kw) == E_SHAPE, kw
    assert _skip(addr, pool=addr + 4) == E_ALIGN and _skip(addr, ring_bytes=500 * 5 * 8 + 4) == E_ALIGN
    assert _skip(addr, pool=addr + 4, len=[501, 0]) == E_SHAPE                                   # shape before alignment
    assert _skip(addr, sess=[1, 3], len=[0, 0]) == 0                                           # nothing to append: no launch, no error


def test_the_order_of_the_checks():
    """NULL before shape before alignment; the mode where msig_rn.h's calls check K."""
    _k, addr = _addr()
    bad_mode = (DEC, 0, float("nan"))
    assert _rec(addr, "stats", table=None, mode=bad_mode, L=0, sig=addr + 4) == E_NULL
    assert _rec(addr, "stats", mode=bad_mode, table=addr + 2052) == E_SHAPE and _rec(addr, "stats", mode=(TRAIL, 0, 0.0), sig=addr + 4) == E_SHAPE
    assert _rec(addr, "stats", N=32, sums=addr + 1028) == E_SHAPE and _rec(addr, "pivot", N=32, pivot=addr + 516) == E_SHAPE
    assert _rec(addr, "sums", B=32, pivot=addr + 516) == E_SHAPE and _rec(addr, "windows", B=32, out=addr + 4100) == E_SHAPE
    assert _live(addr, "step", next=None, B=0, mode=bad_mode) == E_NULL
    assert _live(addr, "step", mode=bad_mode, state=addr + 4100) == E_SHAPE and _live(addr, "step", mode=(7, 0, 0.0), table=addr + 1028) == E_SHAPE
    assert _live(addr, "step", next=[18, 17, 0, 0], state=addr + 4100) == E_SHAPE
    assert _live(addr, "step", win=[17, 18, 0, 2], mode=bad_mode) == E_SHAPE
    assert _live(addr, "step", state=addr + 4100) == E_ALIGN and _live(addr, "step", coverage=addr + 2052) == E_ALIGN
