"""Causal running references (include/msig_rn.h), the C ABI checked without a GPU: the header's calls are exported beside the
unchanged headers, the versions and sizes agree, and each rejection of every entry point happens before a launch (fake, aligned,
never dereferenced device pointers, as in test_recording_cabi.py and test_live_cabi.py — so only calls that must be refused are made
here)."""
import ctypes as C
import re
from pathlib import Path

import pytest

from multimodalsignal_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
RN_HEADER = (ROOT / "include" / "msig_rn.h").read_text()
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
HEAD = 4 * L.MAX_C                   # MSIG_RN_STATE_HEAD


def test_msig_rn_header_calls_are_exported_and_the_other_headers_are_unchanged():
    names = sorted(set(re.findall(r"\b(msig_rn_\w+)\(", re.sub(r"/\*.*?\*/", "", RN_HEADER, flags=re.S))))
    assert names == ["msig_rn_abi_version", "msig_rn_lv_step", "msig_rn_lv_windows_multi", "msig_rn_state_bytes", "msig_rn_stats", "msig_rn_sums",
                     "msig_rn_windows", "msig_rn_windows_multi"]
    lib = L.lib()
    for n in names:
        assert getattr(lib, n) is not None
    assert lib.msig_rn_abi_version() == int(re.search(r"#define MSIG_RN_ABI_VERSION (\d+)", RN_HEADER).group(1)) == L.RN_ABI_VERSION == 1
    assert int(re.search(r"#define MSIG_RN_MAX_K (\d+)", RN_HEADER).group(1)) == L.RN_MAX_K >= 4096
    rec = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "msig_rec.h").read_text(), flags=re.S)
    lv = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "msig_lv.h").read_text(), flags=re.S)
    assert len(set(re.findall(r"\b(msig_rec_\w+)\(", rec))) == 6 and len(set(re.findall(r"\b(msig_lv_\w+)\(", lv))) == 3
    assert (lib.msig_abi_version(), lib.msig_nr_abi_version(), lib.msig_rec_abi_version(), lib.msig_lv_abi_version()) == (5, 1, 1, 1)


def test_state_bytes():
    """The pivot, the carry and two scalars in a head of 4 * MAX_C doubles, then K records of 2 * MAX_C doubles."""
    lib = L.lib()
    for K in (0, 1, 2, 180, L.RN_MAX_K):
        assert lib.msig_rn_state_bytes(K) == (HEAD + K * 2 * L.MAX_C) * 8
    assert lib.msig_rn_state_bytes(-1) == E_SHAPE and lib.msig_rn_state_bytes(L.RN_MAX_K + 1) == E_SHAPE


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


# ---- the recording calls -------------------------------------------------------------------------------------------------------------
def _rec(which, addr, **kw):
    """A recording call over fake pointers: sig at addr, the sums at addr + 512, the table at addr + 1024, out_x at addr + 2048.
    L = 1000, T = 100, S = 30: 31 windows."""
    cols = kw.get("cols", [2, 0, 1])
    a = dict(sig=addr, L=1000, C_all=5, cols=_arr(C.c_int32, cols), C=3 if cols is None else len(cols), mask=0b10, T=100, S=30, n0=3, B=16, N=31,
             K=7, sums=addr + 512, table=addr + 1024, out=addr + 2048, m=_multi())
    a.update({k: v for k, v in kw.items() if k != "cols"})
    head = (a["sig"], a["L"], a["C_all"], a["cols"], a["C"], a["mask"], a["T"], a["S"])
    lib = L.lib()
    if which == "sums":
        return lib.msig_rn_sums(*head, a["n0"], a["B"], a["sums"], None)
    if which == "stats":
        return lib.msig_rn_stats(*head, a["sums"], a["N"], a["K"], a["table"], None)
    if which == "windows":
        return lib.msig_rn_windows(*head, a["n0"], a["B"], a["table"], a["out"], None)
    return lib.msig_rn_windows_multi(*head, a["n0"], a["B"], a["table"], a["out"], None if a["m"] is None else C.byref(a["m"]), None)


REC_CALLS = ["sums", "stats", "windows", "multi"]


@pytest.mark.parametrize("which, name", [("sums", n) for n in ("sig", "cols", "sums")] + [("stats", n) for n in ("sig", "cols", "sums", "table")]
                         + [("windows", n) for n in ("sig", "cols", "table", "out")] + [("multi", n) for n in ("sig", "cols", "table", "out", "m")])
def test_recording_calls_null_pointers(which, name):
    _k, addr = _addr()
    assert _rec(which, addr, **{name: None}) == E_NULL


SHAPES = [dict(L=0), dict(L=-5), dict(T=0), dict(T=-1), dict(S=0), dict(S=-2), dict(C_all=0), dict(C=0), dict(C=-1), dict(C=L.MAX_C + 1),
          dict(cols=[0, 5, 1]), dict(cols=[-1]), dict(cols=[0, 1, 2], C_all=2)]


@pytest.mark.parametrize("which", REC_CALLS)
@pytest.mark.parametrize("kw", SHAPES, ids=str)
def test_recording_calls_bad_shapes(which, kw):
    _k, addr = _addr()
    assert _rec(which, addr, **kw) == E_SHAPE


@pytest.mark.parametrize("which", ["sums", "windows", "multi"])
@pytest.mark.parametrize("kw", [dict(n0=-1), dict(B=0), dict(B=-4), dict(n0=16, B=16), dict(n0=31, B=1), dict(L=99), dict(n0=1, B=1, L=129),
                                dict(n0=1, B=1, S=2000)], ids=str)
def test_windows_outside_the_recording(which, kw):
    """31 windows: [16, 32) reaches past them; L = 129 has one window; S > L leaves window 0 alone."""
    _k, addr = _addr()
    assert _rec(which, addr, **kw) == E_SHAPE


@pytest.mark.parametrize("kw", [dict(N=0), dict(N=-1), dict(N=32), dict(K=-1), dict(K=L.RN_MAX_K + 1), dict(L=99, N=1)], ids=str)
def test_stats_refuses(kw):
    _k, addr = _addr()
    assert _rec("stats", addr, **kw) == E_SHAPE


def test_the_recording_bounds_are_exact():
    """What is inside passes every shape check and fails only at a deliberately misaligned pointer, the last check before a launch."""
    _k, addr = _addr()
    assert _rec("sums", addr, n0=15, B=16, sums=addr + 516) == E_ALIGN
    assert _rec("sums", addr, n0=0, B=31, sums=addr + 516) == E_ALIGN
    assert _rec("sums", addr, n0=0, B=32, sums=addr + 516) == E_SHAPE
    for K in (0, 1, L.RN_MAX_K):
        assert _rec("stats", addr, N=31, K=K, table=addr + 1028) == E_ALIGN
    assert _rec("stats", addr, N=1, K=0, table=addr + 1028) == E_ALIGN
    assert _rec("windows", addr, n0=15, B=16, out=addr + 2052) == E_ALIGN
    assert _rec("windows", addr, n0=0, B=1, S=2000, out=addr + 2052) == E_ALIGN


@pytest.mark.parametrize("which, name", [("sums", "sig"), ("sums", "sums"), ("stats", "sig"), ("stats", "sums"), ("stats", "table"),
                                         ("windows", "sig"), ("windows", "table"), ("multi", "sig"), ("multi", "table")])
def test_recording_calls_misaligned_float64_buffers(which, name):
    _k, addr = _addr()
    base = {"sig": addr, "sums": addr + 512, "table": addr + 1024}[name]
    for off in (1, 4):
        assert _rec(which, addr, **{name: base + off}) == E_ALIGN


@pytest.mark.parametrize("which", ["windows", "multi"])
def test_the_batch_is_16_byte_aligned(which):
    _k, addr = _addr()
    for off in (4, 8):
        assert _rec(which, addr, out=addr + 2048 + off) == E_ALIGN


def test_msig_multi_is_checked_too_and_a_batch_must_fit_its_arena():
    _k, addr = _addr()
    assert _rec("multi", addr, m=_multi(n=0)) == E_SHAPE
    assert _rec("multi", addr, m=_multi(n=L.MAX_FOLDS + 1)) == E_SHAPE
    assert _rec("multi", addr, m=_multi(slots=[1, 1])) == E_SHAPE
    assert _rec("multi", addr, m=_multi(stride=1000)) == E_ALIGN
    assert _rec("multi", addr, m=_multi(stride=19200 - 256)) == E_SHAPE      # one batch: 16 * 3 * 100 * 4 = 19 200 bytes


# ---- the live calls ------------------------------------------------------------------------------------------------------------------
def _lv(which, addr, **kw):
    """A live call over fake pointers: a pool of 4 rings of R = 500 rows of 5 columns at addr, the table at addr + 1024, out_x at
    addr + 2048, the states at addr + 4096; T = 100, S = 30; session 1 holds 1000 samples — windows 17 .. 30 are complete and still in
    its ring — and session 3 holds 130: windows 0 and 1."""
    a = dict(pool=addr, sessions=4, R=500, ring_bytes=500 * 5 * 8, C_all=5, cols=[2, 0, 1], C=None, mask=0b10, T=100, S=30, K=7, state=addr + 4096,
             state_bytes=(HEAD + 7 * 2 * L.MAX_C) * 8, sess=[1, 1, 3, 3], win=[17, 18, 0, 1], written=[1000, 1000, 130, 130], next=[17, 17, 0, 0],
             B=None, table=addr + 1024, out=addr + 2048, m=_multi())
    a.update(kw)
    Cn = a["C"] if a["C"] is not None else (3 if a["cols"] is None else len(a["cols"]))
    B = a["B"] if a["B"] is not None else len(a["win"] or a["sess"])
    pool = (a["pool"], a["sessions"], a["R"], a["ring_bytes"], a["C_all"], _arr(C.c_int32, a["cols"]), Cn, a["mask"], a["T"], a["S"])
    rows = (_arr(C.c_int32, a["sess"]), _arr(C.c_int64, a["win"]), _arr(C.c_int64, a["written"]))
    lib = L.lib()
    if which == "step":
        return lib.msig_rn_lv_step(*pool, a["K"], a["state"], a["state_bytes"], *rows, _arr(C.c_int64, a["next"]), B, a["table"], None)
    return lib.msig_rn_lv_windows_multi(*pool, *rows, B, a["table"], a["out"], None if a["m"] is None else C.byref(a["m"]), None)


@pytest.mark.parametrize("which, name", [("step", n) for n in ("pool", "cols", "state", "sess", "win", "written", "next", "table")]
                         + [("windows", n) for n in ("pool", "cols", "sess", "win", "written", "table", "out", "m")])
def test_live_calls_null_pointers(which, name):
    _k, addr = _addr()
    assert _lv(which, addr, **{name: None}) == E_NULL


POOL = [dict(sessions=0), dict(sessions=-1), dict(sessions=L.LV_MAX_SESSIONS + 1), dict(R=0), dict(R=-3), dict(R=1 << 31, ring_bytes=1 << 40),
        dict(C_all=0), dict(ring_bytes=500 * 5 * 8 - 8), dict(ring_bytes=0)]
ROWS = [dict(win=[17, 18, 0, 2]),                                           # session 3: 2 * 30 + 100 = 160 > 130: not yet complete
        dict(sess=[1], win=[31], written=[1000], next=[31]),                # 31 * 30 + 100 = 1030 > 1000
        dict(sess=[3], win=[0], written=[99], next=[0]),                    # shorter than one window
        dict(sess=[1], win=[16], written=[1000], next=[16]),                # 16 * 30 = 480 < 1000 - 500: already overwritten
        dict(sess=[1], win=[0], written=[601], next=[0]),                   # R = 500, T = 100: sample 0 went at 501 samples
        dict(R=99, ring_bytes=99 * 5 * 8),                                  # a ring shorter than a window holds none
        dict(B=0), dict(B=-1), dict(sess=[1, 1, 4, 4]), dict(sess=[1, 1, -1, 3]), dict(win=[17, 18, -1, 0]),
        dict(T=0), dict(S=0), dict(S=-1), dict(C=0), dict(C=L.MAX_C + 1, cols=[0] * (L.MAX_C + 1)), dict(cols=[0, 5, 1]), dict(cols=[-1])]


@pytest.mark.parametrize("which", ["step", "windows"])
@pytest.mark.parametrize("kw", POOL + ROWS, ids=str)
def test_live_calls_bad_pools_and_rows(which, kw):
    _k, addr = _addr()
    assert _lv(which, addr, **kw) == E_SHAPE


@pytest.mark.parametrize("kw", [dict(K=-1), dict(K=L.RN_MAX_K + 1), dict(state_bytes=(HEAD + 7 * 2 * L.MAX_C) * 8 - 8), dict(K=8), dict(state_bytes=0),
                                dict(K=0, state_bytes=HEAD * 8 - 8),
                                dict(next=[18, 17, 0, 0]),                              # session 1's state stands at 18, the row is window 17
                                dict(next=[17, 17, 1, 0]),
                                dict(win=[17, 19, 0, 1]),                               # a gap inside a session's rows
                                dict(win=[18, 17, 0, 1], next=[18, 18, 0, 0]),          # descending
                                dict(win=[17, 17, 0, 1]),                               # the same window twice
                                dict(sess=[1, 3, 1, 3], win=[17, 0, 18, 1], written=[1000, 130, 1000, 130], next=[17, 0, 18, 1]),      # a session in two separate places
                                dict(sess=[1, 3, 3, 1], win=[17, 0, 1, 18], written=[1000, 130, 130, 1000], next=[17, 0, 0, 18])], ids=str)
def test_step_refuses(kw):
    _k, addr = _addr()
    assert _lv("step", addr, **kw) == E_SHAPE


def test_the_step_bounds_are_exact():
    """What is allowed passes every shape check and fails only at a deliberately misaligned table, the last check before a launch."""
    _k, addr = _addr()
    bad = addr + 1028
    assert _lv("step", addr, table=bad) == E_ALIGN
    assert _lv("step", addr, K=0, state_bytes=HEAD * 8, table=bad) == E_ALIGN
    assert _lv("step", addr, K=L.RN_MAX_K, state_bytes=(HEAD + L.RN_MAX_K * 2 * L.MAX_C) * 8, table=bad) == E_ALIGN
    assert _lv("step", addr, sess=[1], win=[30], written=[1000], next=[30], table=bad) == E_ALIGN         # the last complete window
    assert _lv("step", addr, sess=[1], win=[17], written=[1000], next=[17], table=bad) == E_ALIGN         # the first whole one
    assert _lv("step", addr, sess=[1], win=[0], written=[500], next=[0], table=bad) == E_ALIGN            # nothing overwritten yet
    assert _lv("step", addr, sess=[1, 1, 1], win=[17, 18, 19], written=[1000] * 3, next=[17, 0, 0], table=bad) == E_ALIGN     # next counts at a session's first row
    assert _lv("windows", addr, sess=[1, 3, 1, 3], win=[17, 0, 30, 1], written=[1000, 130, 1000, 130], out=addr + 2052) == E_ALIGN        # any order of rows is a batch


@pytest.mark.parametrize("which, name", [("step", "pool"), ("step", "state"), ("step", "table"), ("windows", "pool"), ("windows", "table")])
def test_live_calls_misaligned_float64_buffers(which, name):
    _k, addr = _addr()
    base = {"pool": addr, "table": addr + 1024, "state": addr + 4096}[name]
    for off in (1, 4):
        assert _lv(which, addr, **{name: base + off}) == E_ALIGN


def test_rings_and_states_are_a_multiple_of_8_bytes_apart():
    _k, addr = _addr()
    for which in ("step", "windows"):
        assert _lv(which, addr, ring_bytes=500 * 5 * 8 + 4) == E_ALIGN
    assert _lv("step", addr, state_bytes=(HEAD + 7 * 2 * L.MAX_C) * 8 + 4) == E_ALIGN


def test_the_live_batch_is_16_byte_aligned_and_msig_multi_is_checked():
    _k, addr = _addr()
    for off in (4, 8):
        assert _lv("windows", addr, out=addr + 2048 + off) == E_ALIGN
    assert _lv("windows", addr, m=_multi(n=0)) == E_SHAPE
    assert _lv("windows", addr, m=_multi(slots=[1, 1])) == E_SHAPE
    assert _lv("windows", addr, m=_multi(stride=1000)) == E_ALIGN
    assert _lv("windows", addr, m=_multi(stride=4608)) == E_SHAPE          # 18 * 256 < the 4 * 3 * 100 * 4 = 4 800 bytes of one batch


def test_the_order_of_the_checks():
    """NULL before shape before alignment, the call's own checks before msig_multi's, as the header lists them."""
    _k, addr = _addr()
    assert _rec("sums", addr, sums=None, L=0, sig=addr + 4) == E_NULL
    assert _rec("stats", addr, K=-1, table=addr + 1028) == E_SHAPE
    assert _rec("multi", addr, m=None, B=0) == E_NULL
    assert _rec("multi", addr, out=addr + 2052, m=_multi(n=0)) == E_ALIGN
    assert _lv("step", addr, next=None, B=0) == E_NULL
    assert _lv("step", addr, next=[18, 17, 0, 0], state=addr + 4100) == E_SHAPE
    assert _lv("windows", addr, m=None, B=0) == E_NULL
    assert _lv("windows", addr, win=[17, 18, 0, 2], table=addr + 1028) == E_SHAPE
    assert _lv("windows", addr, out=addr + 2052, m=_multi(n=0)) == E_ALIGN
