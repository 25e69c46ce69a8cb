"""The "same session twice" check of the live calls at 300 entries in a pool of 4096 rings (include/msig_lv.h, msig_rn.h, msig_rd.h,
msig_gp.h, msig_rs.h), without a GPU: fake, aligned, never dereferenced device pointers as in test_live_cabi.py, so only calls that
must be refused are made.  The bitmap behind the check has 64 words; the other tests use sessions 0, 1 and 3, all in word 0.  Here
the duplicate sits in word 1, in word 63 and 298 entries apart, in every call that keeps such a bitmap.  That the refusal is the
duplicate's is shown by the same call without it on a misaligned pool: alignment is checked after the shapes, so it answers
MSIG_E_ALIGN where the call with the duplicate answers MSIG_E_SHAPE.  (A call without a duplicate on an aligned pool would launch;
tests/test_live_scale_gpu.py makes it.)"""
import ctypes as C

import pytest

import lv_scale_cases as SC
from multimodalsignal_amd import _lib as L

T, S, RN = 16, 4, 37
N = SC.P
assert N > 2 * SC.GROUP, "300 entries are meant to span three launch groups"


def _addr():
    keep_alive = (C.c_char * 8192)()
    return keep_alive, (C.addressof(keep_alive) + 255) // 256 * 256


def _i32(v):
    return (C.c_int32 * len(v))(*v)


def _i64(v):
    return (C.c_int64 * len(v))(*v)


def _pool(addr, sessions):
    return addr, sessions, RN, RN * 8 * 8, 8


def _push(addr, sess, sessions):
    return L.lib().msig_lv_push(*_pool(addr, sessions), _i32(sess), _i64([40] * len(sess)), _i64([3] * len(sess)), len(sess), addr + 2048, None)


def _skip(addr, sess, sessions):
    return L.lib().msig_gp_lv_skip(*_pool(addr, sessions), _i32(sess), _i64([40] * len(sess)), _i64([3] * len(sess)), len(sess), None)


def _rs_push(addr, sess, sessions):
    """ratio 2 / 3, half = 30: 31 tail rows."""
    return L.lib().msig_rs_lv_push(*_pool(addr, sessions), addr + 1024, 31, 31 * 8 * 8, addr + 3072, 2, 3, 30, _i32(sess), _i64([40] * len(sess)),
                                   _i64([3] * len(sess)), len(sess), addr + 2048, None)


def _rows(sess):
    """One row per entry: window 0 of a session that holds exactly one window, expected next."""
    n = len(sess)
    return _i32(sess), _i64([0] * n), _i64([T] * n), _i64([0] * n), n


def _rn_step(addr, sess, sessions):
    lib = L.lib()
    return lib.msig_rn_lv_step(*_pool(addr, sessions), _i32([5, 1, 4]), 3, 0b10, T, S, 2, addr + 1024, lib.msig_rn_state_bytes(2), *_rows(sess),
                               addr + 2048, None)


def _rd_step(addr, sess, sessions):
    lib = L.lib()
    return lib.msig_rd_lv_step(*_pool(addr, sessions), _i32([5, 1, 4]), 3, 0b10, T, S, 0.5, addr + 1024, lib.msig_rn_state_bytes(0), *_rows(sess),
                               addr + 2048, None)


def _gp_step(addr, sess, sessions):
    lib = L.lib()
    return lib.msig_gp_lv_step(*_pool(addr, sessions), _i32([5, 1, 4]), 3, 0b10, T, S, C.byref(L.GpMode(1, 2, 0.0)), addr + 1024,
                               lib.msig_gp_state_bytes(2), *_rows(sess), addr + 2048, addr + 3072, None)


CALLS = {"msig_lv_push": _push, "msig_gp_lv_skip": _skip, "msig_rs_lv_push": _rs_push, "msig_rn_lv_step": _rn_step, "msig_rd_lv_step": _rd_step,
         "msig_gp_lv_step": _gp_step}
# (the session that comes twice, the two entries): in bitmap word 1 across the first group's end, in word 63, and 298 entries apart
DUPLICATES = {"64-in-word-1": (64, 126, 129), "4095-in-word-63": (4095, 5, 7), "200-at-both-ends": (200, 0, N - 1)}


def _distinct():
    """300 distinct sessions of the 4096, the order of the GPU tests, without the ids planted below."""
    order = [s for s in SC.slot_order(N + 3) if s not in (64, 200, 4095)][:N]
    assert len(order) == N and len(set(order)) == N
    return order


@pytest.mark.parametrize("which", list(DUPLICATES))
@pytest.mark.parametrize("call", list(CALLS))
def test_a_duplicate_among_300_entries_is_refused(call, which):
    _k, addr = _addr()
    sid, a, b = DUPLICATES[which]
    once = _distinct()
    once[a] = sid
    assert CALLS[call](addr + 4, once, SC.POOL_SLOTS) == SC.E_ALIGN          # every shape check passed: the entries are fine
    twice = list(once)
    twice[b] = sid
    assert abs(a - b) > 1 and len(set(twice)) == N - 1
    assert CALLS[call](addr, twice, SC.POOL_SLOTS) == SC.E_SHAPE
    assert CALLS[call](addr + 4, twice, SC.POOL_SLOTS) == SC.E_SHAPE         # ... and before the alignment


@pytest.mark.parametrize("call", list(CALLS))
def test_aliases_modulo_64_are_not_duplicates(call):
    """5, 69, 133 and 4037 share a bit position, not a word: the call gets as far as the alignment."""
    _k, addr = _addr()
    once = _distinct()
    assert set(SC.FAMILY) <= set(once) and len({s & 63 for s in SC.FAMILY}) == 1 and len({s >> 6 for s in SC.FAMILY}) == len(SC.FAMILY)
    assert CALLS[call](addr + 4, once, SC.POOL_SLOTS) == SC.E_ALIGN


@pytest.mark.parametrize("call", list(CALLS))
def test_one_entry_more_than_the_pool_has_sessions(call):
    """n = sessions + 1 in a pool of 299: the append calls refuse the count; a step takes any number of rows, but 300 rows of
    distinct sessions do not fit 299 rings, so the ids 0 .. 299 are refused for the last one."""
    _k, addr = _addr()
    sess = list(range(N))[::-1]
    assert CALLS[call](addr, sess, N - 1) == SC.E_SHAPE
    assert CALLS[call](addr + 4, sess, N) == SC.E_ALIGN
