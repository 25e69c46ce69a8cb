"""The monitoring calls at scale (include/msig_lv.h, msig_rn.h, msig_rd.h, msig_gp.h, msig_rs.h, msig_rec.h).

A. More than one launch group.  Every live call chops its per-session or per-run table into launches of MSIG_LV_GROUP entries.  Here
300 sessions of a pool of 4096 slots — in a fixed pseudo-random order of slots that holds 0, 63, 64, 127, 128, 191, 192, 4095 and
the family 5, 69, 133, 4037 that is equal modulo 64 — go through ONE call per tick: ragged chunks with zero lengths on both sides of
a group's end, over a whole group and over the first group; mixed window batches of 300 runs; the steps of the running references.
Session k's recording is rows [5 k, 5 k + L_k) of one long recording, so a row in the wrong ring or from the wrong staging offset has
wrong bits.
B. The second pass of every grid-stride loop.  Each case takes the smallest size that is over the kernel's cap on gridDim.x; the
reference is the same call in pieces that stay under it.
D. 300 wearers in one LiveMonitor against three Monitor.run.

Every comparison is of raw bits, except one numpy cross-check at the tolerance tests/test_live_gpu.py uses.  The group size and the
caps are read from the header and the sources (tests/lv_scale_cases.py), and every case asserts that it is over them."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import gp_reference as G
import lv_reference as LV
import lv_scale_cases as SC
import rn_reference as RN
from multimodalsignal_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MC = L.MAX_C
NAMES8 = LV.NAMES8
GROUP, P = SC.GROUP, SC.P
FILL = np.frombuffer(b"\x5a" * 8, dtype=np.float64)[0]                   # a ring row nobody wrote
QNAN = 0x7ff8000000000000
T, S, RING = 16, 4, 37                                                   # R is no multiple of S or T
COLS = LV.COLS["8of8"]
CN = len(COLS)
ORDER = SC.slot_order()
DECAY = float(np.exp2(-1.0 / 3))
FS = 64.0


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "the gpu tier needs an MI355X"
    assert P > 2 * GROUP, "300 entries are meant to take three launches"


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _i32(v):
    return (C.c_int32 * len(v))(*[int(x) for x in v])


def _i64(v):
    return (C.c_int64 * len(v))(*[int(x) for x in v])


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[x.dtype.itemsize])


def _same_bits(a, b):
    """Two device tensors hold the same bytes."""
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)))


def _selected(rec, Cn):
    return np.concatenate([rec[..., :Cn], rec[..., MC:MC + Cn], rec[..., 2 * MC:]], axis=-1)


def _head(dev, cols, Tn, Sn, mask=None):
    return (dev.data_ptr(), dev.shape[0], dev.shape[1] if dev.dim() == 2 else 1, _i32(cols), len(cols), LV.mask_of(cols) if mask is None else mask,
            Tn, Sn)


def _runs(rows):
    """The runs the host code forms: maximal stretches of consecutive windows of one session."""
    return 1 + sum(1 for a, b in zip(rows, rows[1:]) if a[0] != b[0] or b[1] != a[1] + 1)


# ---- the 300 sessions' recordings ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _base(gappy=False):
    """One long (L, 8) recording and its device copy; `gappy`: 4 % of the samples missing, and the first row of every fifth session."""
    sig = LV.recording(5 * P + 200, 4242)
    if gappy:
        sig[np.random.RandomState(77).rand(*sig.shape) < 0.04] = np.nan
        sig[np.arange(0, 5 * P, 25)] = np.nan
    return sig, torch.from_numpy(sig).to(DEV)


def _lengths(least):
    return [least + (7 * k) % 23 for k in range(P)]


def _rec(k, n, gappy=False):
    """Session k's recording of n rows: host, device."""
    sig, dev = _base(gappy)
    return sig[5 * k:5 * k + n], dev[5 * k:5 * k + n]


def _ticks(total, limit=None, dense=()):
    """(tick, rows every entry holds so far, this tick's chunk lengths) until every session has delivered its `total` rows.  `limit(j, n)`
    cuts entry j's chunk to what its ring takes; at the ticks of `dense` every entry delivers at least one stride."""
    at, tick = [0] * P, 0
    while any(a < t for a, t in zip(at, total)):
        lens = [min(max(n, S) if tick in dense else n, total[j] - at[j]) for j, n in enumerate(SC.chunk_lengths(tick))]
        if limit is not None:
            lens = [limit(j, n) if n else 0 for j, n in enumerate(lens)]
        if tick == 1:
            assert lens[GROUP - 1] == lens[GROUP] == 0 and lens[GROUP - 2] > 0 and lens[GROUP + 1] > 0
        if tick == 2:
            assert not any(lens[GROUP:2 * GROUP]) and any(lens[:GROUP]) and any(lens[2 * GROUP:])
        if tick == 3:
            assert not any(lens[:GROUP]) and any(lens[GROUP:2 * GROUP])
        yield tick, list(at), lens
        at = [a + n for a, n in zip(at, lens)]
        tick += 1
    assert tick > 3


class Pool:
    """A caller-owned pool of `sessions` rings of Rn rows of C_all float64, filled with 0x5A."""

    def __init__(self, Rn, sessions=SC.POOL_SLOTS, C_all=8):
        self.R, self.sessions, self.C_all = Rn, sessions, C_all
        self.mem = torch.full((sessions, Rn * C_all * 8), 0x5A, dtype=torch.uint8, device=DEV)

    def args(self):
        return self.mem.data_ptr(), self.sessions, self.R, self.R * self.C_all * 8, self.C_all

    def rings(self):
        torch.cuda.synchronize()
        return self.mem.cpu().numpy().view(np.float64).reshape(self.sessions, self.R, self.C_all)

    def push(self, sess, written, lens, chunks):
        """ONE msig_lv_push: chunks[j] is entry j's (len[j], C_all) host rows, back to back in one staging buffer with a canary row."""
        staging = torch.from_numpy(np.concatenate(list(chunks) + [np.full((1, self.C_all), -7.25)])).to(DEV)
        assert staging.shape[0] == sum(lens) + 1
        L.check(L.lib().msig_lv_push(*self.args(), _i32(sess), _i64(written), _i64(lens), len(sess), staging.data_ptr(), _stream()), "msig_lv_push")

    def skip(self, sess, written, lens):
        L.check(L.lib().msig_gp_lv_skip(*self.args(), _i32(sess), _i64(written), _i64(lens), len(sess), _stream()), "msig_gp_lv_skip")


def _expected_rings(rings, sessions=SC.POOL_SLOTS):
    """(sessions, R, C_all): the restatement's ring of entry j in slot ORDER[j], 0x5A everywhere else."""
    want = np.full((sessions,) + rings[0].rows.shape, FILL)
    for j, ring in enumerate(rings):
        want[ORDER[j]] = ring.rows
    return want


# ---- A.1, A.6: msig_lv_push ------------------------------------------------------------------------------------------------------------
def test_push_of_300_ragged_chunks_fills_every_ring_as_the_restatement_does():
    """300 chunks a call, one call a tick, until every ring has wrapped three times: every ring equals lv_reference.Ring filled row by
    row, every slot that was never opened is still 0x5A.  On the way a call whose entry 299 repeats an earlier session — one of the
    family that is equal modulo 64, which the call has just taken as distinct — is refused and leaves the pool as it was."""
    pool = Pool(RING)
    total = _lengths(3 * RING + 10)
    rings = [LV.Ring(RING, 8, FILL) for _ in range(P)]
    assert set(SC.FAMILY) <= set(ORDER) and set(SC.NAMED) <= set(ORDER)
    for tick, at, lens in _ticks(total):
        chunks = [_rec(j, total[j])[0][at[j]:at[j] + lens[j]] for j in range(P)]
        pool.push(ORDER, at, lens, chunks)
        for j in range(P):
            rings[j].push(chunks[j])
        if tick == 4:
            before = pool.rings().copy()
            twice = list(ORDER[:-1]) + [SC.FAMILY[3] if ORDER[-1] != SC.FAMILY[3] else SC.FAMILY[0]]
            written = [r.written for r in rings]
            staging = torch.zeros((13 * P, 8), dtype=torch.float64, device=DEV)
            rc = L.lib().msig_lv_push(*pool.args(), _i32(twice), _i64(written), _i64([3] * P), P, staging.data_ptr(), _stream())
            assert rc == SC.E_SHAPE and len(set(twice)) == P - 1
            assert L.lib().msig_gp_lv_skip(*pool.args(), _i32(twice), _i64(written), _i64([3] * P), P, _stream()) == SC.E_SHAPE
            assert np.array_equal(_bits(pool.rings()), _bits(before))
    got = pool.rings()
    assert all(r.written == n > 3 * RING for r, n in zip(rings, total))
    assert np.array_equal(_bits(got), _bits(_expected_rings(rings)))
    untouched = np.ones(SC.POOL_SLOTS, dtype=bool)
    untouched[ORDER] = False
    assert untouched.sum() == SC.POOL_SLOTS - P and np.all(_bits(got[untouched]) == _bits(FILL))


# ---- A.2: msig_gp_lv_skip --------------------------------------------------------------------------------------------------------------
def test_skip_of_300_ragged_stretches_is_a_push_of_nan_rows():
    """The same pattern of lengths through msig_gp_lv_skip and through msig_lv_push with NaN staging rows: the same pools, byte for
    byte, and the restatement's rings.  Some rings wrap here and some are not even full."""
    a, b = Pool(RING), Pool(RING)
    total = _lengths(20)
    rings = [LV.Ring(RING, 8, FILL) for _ in range(P)]
    nan = np.full((13, 8), np.nan)
    assert np.all(_bits(nan) == QNAN)
    for _tick, at, lens in _ticks(total):
        a.skip(ORDER, at, lens)
        b.push(ORDER, at, lens, [nan[:n] for n in lens])
        for j in range(P):
            rings[j].push(nan[:lens[j]])
    got = a.rings()
    assert min(total) < RING < max(total)
    assert np.array_equal(_bits(got), _bits(b.rings())) and np.array_equal(_bits(got), _bits(_expected_rings(rings)))
    assert int(np.isnan(got).sum()) == sum(min(n, RING) for n in total) * 8


# ---- A.3, B: msig_rs_lv_push -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rs(fs_in, fs_out):
    from multimodalsignal_amd.resample import FirResampler
    return FirResampler(fs_in, fs_out, DEV)


def _resample(dev, r):
    """msig_rs_resample of the (n, C_all) device rows; the row behind the last output keeps its canary."""
    n_out = r.out_count(dev.shape[0])
    y = torch.full((n_out + 1, dev.shape[1]), -7.25, dtype=torch.float64, device=DEV)
    L.check(L.lib().msig_rs_resample(dev.data_ptr(), dev.shape[0], dev.shape[1], *r.ratio_args(), y.data_ptr(), n_out, _stream()), "msig_rs_resample")
    return y, n_out


def _wrapped(rows, Rn, width=8):
    """(Rn, width): row i of `rows` in ring row i % Rn, the last Rn of them; 0x5A where none was written."""
    want = np.full((Rn, width), FILL)
    i = np.arange(max(0, rows.shape[0] - Rn), rows.shape[0])
    want[i % Rn] = rows[i]
    return want


@pytest.mark.parametrize("missing", [False, True], ids=["staging", "no-staging"])
def test_resampled_push_of_300_raw_chunks_is_the_offline_resampler(missing):
    """Ratio 2 / 3, the same ragged raw lengths: every ring row is msig_rs_resample's of the session's linear raw recording, every
    tail row the raw row, in bits; without a staging buffer the raw rows are NaN.  Untouched rings and tails stay 0x5A."""
    r = _rs(3, 2)
    assert (r.L, r.M) == (2, 3)
    pool = Pool(RING)
    tails = torch.full((SC.POOL_SLOTS, r.tail_rows * 8 * 8), 0x5A, dtype=torch.uint8, device=DEV)
    total = _lengths(3 * RING + 10)
    nan_dev = torch.full((max(total), 8), float("nan"), dtype=torch.float64, device=DEV)
    raws = [(np.full((n, 8), np.nan), nan_dev[:n]) if missing else _rec(j, n) for j, n in enumerate(total)]
    for _tick, at, lens in _ticks(total):
        staging = torch.from_numpy(np.concatenate([raws[j][0][at[j]:at[j] + lens[j]] for j in range(P)] + [np.full((1, 8), -7.25)])).to(DEV)
        L.check(L.lib().msig_rs_lv_push(*pool.args(), tails.data_ptr(), r.tail_rows, r.tail_rows * 64, *r.ratio_args(), _i32(ORDER), _i64(at),
                                        _i64(lens), P, None if missing else staging.data_ptr(), _stream()), "msig_rs_lv_push")
    offline = [_resample(raws[j][1], r) for j in range(P)]
    want, want_tails = np.full((SC.POOL_SLOTS, RING, 8), FILL), np.full((SC.POOL_SLOTS, r.tail_rows, 8), FILL)
    torch.cuda.synchronize()
    for j, (y, n_out) in enumerate(offline):
        host = y.cpu().numpy()
        assert n_out > RING and np.all(host[n_out] == -7.25)
        want[ORDER[j]] = _wrapped(host[:n_out], RING)
        want_tails[ORDER[j]] = _wrapped(raws[j][0], r.tail_rows)
    assert np.array_equal(_bits(pool.rings()), _bits(want))
    assert np.array_equal(_bits(tails.cpu().numpy()).reshape(-1), _bits(want_tails).view(np.uint8).reshape(-1))
    if missing:
        assert np.all(np.isnan(want[ORDER])) and np.all(_bits(want_tails[ORDER]) == QNAN)


# ---- A.4: msig_lv_windows_multi --------------------------------------------------------------------------------------------------------
def _stats_table(slots, seed):
    """A statistics table of the whole pool: NaN, and a record of its own for every slot of `slots`."""
    rs = np.random.RandomState(seed)
    tab = np.full((SC.POOL_SLOTS, 2 * MC + 1), np.nan)
    for s in slots:
        tab[s, :MC], tab[s, MC:2 * MC], tab[s, 2 * MC] = rs.randn(MC), 0.5 + rs.rand(MC), 7
    return torch.from_numpy(tab).to(DEV)


def _check_windows(pool, Tn, Sn, rows, written, recs, stats, launches):
    """ONE msig_lv_windows_multi of `rows` [(entry, window)] into arena slots [2, 0] of three against msig_rec_windows on each entry's
    linear recording (recs[entry]: device rows) with the session's record."""
    from multimodalsignal_amd.runtime import Arenas
    B = len(rows)
    assert _runs(rows) > (launches - 1) * GROUP and _runs(rows) <= launches * GROUP
    arenas = Arenas(3, DEV, (("other", 1000), ("x", B * CN * Tn * 4), ("tail", 256)))
    arenas.mem.fill_(0x5A)
    L.check(L.lib().msig_lv_windows_multi(*pool.args(), _i32(COLS), CN, LV.mask_of(COLS), Tn, Sn, _i32([ORDER[j] for j, _w in rows]),
                                          _i64([w for _j, w in rows]), _i64([written[j] for j, _w in rows]), B, stats.data_ptr(), arenas.ptr("x"),
                                          C.byref(arenas.multi([2, 0])), _stream()), "msig_lv_windows_multi")
    ref = torch.full((B + 1, CN, Tn), -77.0, dtype=torch.float32, device=DEV)
    for b, (j, w) in enumerate(rows):
        L.check(L.lib().msig_rec_windows(*_head(recs[j], COLS, Tn, Sn), w, 1, stats[ORDER[j]].data_ptr(), ref[b].data_ptr(), _stream()), "msig_rec_windows")
    torch.cuda.synchronize()
    want = ref.cpu().numpy()
    assert np.all(want[B] == -77.0) and np.all(np.isfinite(want[:B]))
    for s in (0, 2):
        x = arenas.view(s, "x", torch.float32).cpu().numpy()
        assert np.array_equal(_bits(x[:B * CN * Tn]), _bits(want[:B].reshape(-1))), s
        assert np.all(x[B * CN * Tn:].view(np.uint8) == 0x5A), "wrote past the batch"
        assert np.all(arenas.view(s, "other").cpu().numpy() == 0x5A) and np.all(arenas.view(s, "tail").cpu().numpy() == 0x5A)
    assert np.all(arenas.mem[1].cpu().numpy() == 0x5A)


def test_one_mixed_batch_of_300_runs():
    """All 300 sessions with their last 1 to 3 complete windows, rings wrapped: 300 runs, three launches."""
    pool = Pool(RING)
    written = [50 + k % 9 for k in range(P)]
    recs = [_rec(j, written[j]) for j in range(P)]
    pool.push(ORDER, [0] * P, [RING] * P, [recs[j][0][:RING] for j in range(P)])
    pool.push(ORDER, [RING] * P, [n - RING for n in written], [recs[j][0][RING:] for j in range(P)])
    rows = []
    for j in range(P):
        last = LV.count(written[j], T, S) - 1
        rows += [(j, w) for w in range(last - j % 3, last + 1)]
    assert len(rows) == 2 * P and all(w * S >= written[j] - RING for j, w in rows)
    _check_windows(pool, T, S, rows, written, [d for _h, d in recs], _stats_table(ORDER, 3), launches=3)
    untouched = np.ones(SC.POOL_SLOTS, dtype=bool)
    untouched[ORDER] = False
    assert np.all(_bits(pool.rings()[untouched]) == _bits(FILL))


def test_130_single_row_runs_of_one_session():
    """130 windows of the session in slot 4095 in descending order, S = 1: no two rows are consecutive, so 130 runs and two launches."""
    Rn, Sn, n = 130 + T + 4, 1, 130 + T + 24
    pool = Pool(Rn)
    j = ORDER.index(4095)
    host, dev = _rec(j, n)
    pool.push([4095], [0], [Rn], [host[:Rn]])
    pool.push([4095], [Rn], [n - Rn], [host[Rn:]])
    last = LV.count(n, T, Sn) - 1
    rows = [(j, w) for w in range(last, last - 130, -1)]
    assert rows[-1][1] * Sn >= n - Rn and 130 > GROUP
    _check_windows(pool, T, Sn, rows, {j: n}, {j: dev}, _stats_table([4095], 5), launches=2)


# ---- A.5: the steps of the running references -------------------------------------------------------------------------------------------
STEP_MODES = {"rn-expanding": ("rn", 0), "rn-trailing2": ("rn", 2), "rd-decayed": ("rd", DECAY), "gp-expanding": ("gp", (G.EXPANDING, 0, 0.0)),
              "gp-trailing2": ("gp", (G.TRAILING, 2, 0.0)), "gp-decayed": ("gp", (G.DECAYED, 0, DECAY))}


def _offline_chain(family, mode, total):
    """The offline chain on every session's linear recording, all launches first and one copy back: per entry the table (N, 33), the
    coverage (N, 16; gp) and the rows (N, C, T) — msig_rn_sums / msig_rn_stats or msig_rd_stats / msig_rn_windows, or msig_gp_pivot /
    msig_gp_sums / msig_gp_stats / msig_gp_windows."""
    lib = L.lib()
    Ns = [LV.count(n, T, S) for n in total]
    at = [int(a) for a in np.concatenate([[0], np.cumsum(Ns)])]
    sums = torch.zeros((at[-1], 3 * MC), dtype=torch.float64, device=DEV)
    table = torch.full((at[-1], 2 * MC + 1), float("nan"), dtype=torch.float64, device=DEV)
    cov = torch.full((at[-1], MC), float("nan"), dtype=torch.float64, device=DEV)
    pivot = torch.full((P, 2 * MC), float("nan"), dtype=torch.float64, device=DEV)
    out = torch.empty((at[-1], CN, T), dtype=torch.float32, device=DEV)
    for j in range(P):
        head, a, N = _head(_rec(j, total[j], family == "gp")[1], COLS, T, S), int(at[j]), Ns[j]
        if family == "gp":
            L.check(lib.msig_gp_pivot(*head, N, pivot[j].data_ptr(), _stream()), "msig_gp_pivot")
            L.check(lib.msig_gp_sums(*head, pivot[j].data_ptr(), 0, N, sums[a].data_ptr(), _stream()), "msig_gp_sums")
            L.check(lib.msig_gp_stats(*head, pivot[j].data_ptr(), sums[a].data_ptr(), N, C.byref(L.GpMode(*mode)), table[a].data_ptr(), cov[a].data_ptr(),
                                      _stream()), "msig_gp_stats")
            L.check(lib.msig_gp_windows(*head, 0, N, table[a].data_ptr(), out[a].data_ptr(), _stream()), "msig_gp_windows")
            continue
        L.check(lib.msig_rn_sums(*head, 0, N, sums[a].data_ptr(), _stream()), "msig_rn_sums")
        if family == "rd":
            L.check(lib.msig_rd_stats(*head, sums[a].data_ptr(), N, mode, table[a].data_ptr(), _stream()), "msig_rd_stats")
        else:
            L.check(lib.msig_rn_stats(*head, sums[a].data_ptr(), N, mode, table[a].data_ptr(), _stream()), "msig_rn_stats")
        L.check(lib.msig_rn_windows(*head, 0, N, table[a].data_ptr(), out[a].data_ptr(), _stream()), "msig_rn_windows")
    torch.cuda.synchronize()
    return at, table.cpu().numpy(), cov.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize("name", list(STEP_MODES))
def test_steps_of_300_sessions_in_one_call_give_the_offline_tables_and_rows(name):
    """tests/test_running_live_gpu.py's test_live_tables_and_rows_are_the_offline_ones at 300 sessions: per tick ONE append, ONE step and
    ONE *_lv_windows_multi for all sessions' newly complete windows.  Every table record, coverage record and output row equals the
    offline chain's on the session's linear recording, for all 300 sessions — the group boundaries' neighbours (entries 126 .. 129,
    254 .. 257) and the named slots among them; the record behind the last keeps its canary, the states of unopened slots stay NaN."""
    from multimodalsignal_amd.live import RingBook
    from multimodalsignal_amd.runtime import Arenas
    family, mode = STEP_MODES[name]
    lib = L.lib()
    gp = family == "gp"
    K = mode if family == "rn" else (mode[1] if gp and mode[0] == G.TRAILING else 0)
    state_bytes = lib.msig_gp_state_bytes(K) if gp else lib.msig_rn_state_bytes(K)
    total = _lengths(60)
    at_of, want_tab, want_cov, want_out = _offline_chain(family, mode, total)
    pool = Pool(RING)
    state = torch.full((SC.POOL_SLOTS, state_bytes // 8), float("nan"), dtype=torch.float64, device=DEV)
    books = [RingBook(RING, T, S, 0) for _ in range(P)]
    nxt = [0] * P
    arenas = Arenas(3, DEV, (("other", 1000), ("x", 4 * P * CN * T * 4), ("tail", 256)))
    rows_args = (_i32(COLS), CN, LV.mask_of(COLS), T, S)
    most_runs, checked, seen_entries = 0, 0, set()
    for _tick, at, lens in _ticks(total, limit=lambda j, n: books[j].segment(n), dense=(9, 12)):      # at tick 9 every session holds a window
        pool.push(ORDER, at, lens, [_rec(j, total[j], gp)[0][at[j]:at[j] + lens[j]] for j in range(P)])
        rows = []
        for j in range(P):
            rows += [(j, w) for w in books[j].advance(lens[j])[1]]
        if not rows:
            continue
        B = len(rows)
        assert B <= 4 * P
        sess, win = _i32([ORDER[j] for j, _w in rows]), _i64([w for _j, w in rows])
        written, nx = _i64([books[j].written for j, _w in rows]), _i64([nxt[j] for j, _w in rows])
        table = torch.full((B + 1, 2 * MC + 1), float("nan"), dtype=torch.float64, device=DEV)
        cov = torch.full((B + 1, MC), float("nan"), dtype=torch.float64, device=DEV)
        pool_args = pool.args()
        if gp:
            L.check(lib.msig_gp_lv_step(*pool_args, *rows_args, C.byref(L.GpMode(*mode)), state.data_ptr(), state_bytes, sess, win, written, nx, B,
                                        table.data_ptr(), cov.data_ptr(), _stream()), "msig_gp_lv_step")
        elif family == "rd":
            L.check(lib.msig_rd_lv_step(*pool_args, *rows_args, mode, state.data_ptr(), state_bytes, sess, win, written, nx, B, table.data_ptr(),
                                        _stream()), "msig_rd_lv_step")
        else:
            L.check(lib.msig_rn_lv_step(*pool_args, *rows_args, mode, state.data_ptr(), state_bytes, sess, win, written, nx, B, table.data_ptr(),
                                        _stream()), "msig_rn_lv_step")
        arenas.mem.fill_(0x5A)
        fill = lib.msig_gp_lv_windows_multi if gp else lib.msig_rn_lv_windows_multi
        L.check(fill(*pool_args, *rows_args, sess, win, written, B, table.data_ptr(), arenas.ptr("x"), C.byref(arenas.multi([2, 0])), _stream()),
                "*_lv_windows_multi")
        for j, _w in rows:
            nxt[j] += 1
        torch.cuda.synchronize()
        where = np.array([at_of[j] + w for j, w in rows])
        got = table.cpu().numpy()
        assert np.all(np.isnan(got[B])), "wrote past the table"
        assert np.array_equal(_bits(_selected(got[:B], CN)), _bits(_selected(want_tab[where], CN)))
        assert np.all(np.isnan(got[:B, CN:MC])) and np.all(np.isnan(got[:B, MC + CN:2 * MC]))
        if gp:
            gcov = cov.cpu().numpy()
            assert np.all(np.isnan(gcov[B])) and np.array_equal(_bits(gcov[:B, :CN]), _bits(want_cov[where, :CN])) and np.all(np.isnan(gcov[:B, CN:]))
        n = B * CN * T
        ref = _bits(want_out[where].reshape(-1))
        for s in (0, 2):
            x = arenas.view(s, "x", torch.float32).cpu().numpy()
            assert np.array_equal(_bits(x[:n]), ref), s
            assert np.all(x[n:].view(np.uint8) == 0x5A), "wrote past the batch"
            assert np.all(arenas.view(s, "other").cpu().numpy() == 0x5A) and np.all(arenas.view(s, "tail").cpu().numpy() == 0x5A)
        assert np.all(arenas.mem[1].cpu().numpy() == 0x5A)
        most_runs = max(most_runs, len({j for j, _w in rows}))
        if len({j for j, _w in rows}) > 2 * GROUP:
            seen_entries |= {j for j, _w in rows}
        checked += B
    assert checked == at_of[-1] and most_runs > 2 * GROUP
    assert set(SC.BOUNDARY) <= seen_entries and {ORDER.index(s) for s in SC.NAMED} <= seen_entries      # ... in calls of three launches
    st = state.cpu().numpy()
    opened = np.zeros(SC.POOL_SLOTS, dtype=bool)
    opened[ORDER] = True
    assert np.all(np.isnan(st[~opened]))
    assert np.array_equal(st[ORDER, G.STATE_NEXT if gp else 3 * MC], np.array([LV.count(n, T, S) for n in total], dtype=np.float64))
    assert np.all(_bits(pool.rings()[~opened]) == _bits(FILL))
    if gp:
        assert np.isnan(_base(True)[0]).any() and (want_cov[:, :CN] < 1.0).any() and np.all(np.isfinite(want_out))


# ---- B. the second pass of the grid-stride loops ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", ["msig_lv_push", "msig_gp_lv_skip"])
def test_a_chunk_over_the_append_kernels_cap(call):
    """One chunk of 32 800 rows of 8 columns into a ring of as many rows, from a row that makes it wrap, and beside it in the same call
    a chunk of 3 rows that wraps its own ring: the short chunk's threads all fall out of a grid sized for the long one."""
    Rn = 32800
    kernel = {"msig_lv_push": ("live.hip", "lv_push_kernel"), "msig_gp_lv_skip": ("gaps.hip", "gp_lv_skip_kernel")}[call]
    assert SC.blocks(Rn * 8) > SC.cap(*kernel) >= SC.blocks((Rn - 256) * 8)
    pool = Pool(Rn, sessions=3)
    rs = np.random.RandomState(8)
    long, short = rs.randn(Rn, 8), rs.randn(3, 8)
    if call == "msig_gp_lv_skip":
        long[:], short[:] = np.nan, np.nan
        pool.skip([2, 0], [Rn - 1, 12345], [3, Rn])
    else:
        pool.push([2, 0], [Rn - 1, 12345], [3, Rn], [short, long])
    rings = [LV.Ring(Rn, 8, FILL) for _ in range(3)]
    rings[0].written, rings[2].written = 12345, Rn - 1
    rings[0].push(long)
    rings[2].push(short)
    got = pool.rings()
    assert np.array_equal(_bits(got), _bits(np.stack([r.rows for r in rings])))
    assert np.all(_bits(got[1]) == _bits(FILL)) and np.all(_bits(got[2, 2:Rn - 1]) == _bits(FILL))
    assert np.array_equal(_bits(got[0, 12345]), _bits(long[0])) and np.array_equal(_bits(got[0, 12344]), _bits(long[Rn - 1]))


def test_a_raw_chunk_over_the_resampling_append_kernels_caps():
    """Ratio 3 / 2, a tail of 40 000 rows: one chunk of 40 001 raw rows — about 60 000 outputs of 8 columns, and 40 000 tail rows of 8
    columns, both over 1024 x 256 — behind 50 rows pushed earlier, and a 1-row chunk of another session before it in the same call.
    The ring is 5 rows longer than the long chunk's outputs, so it wraps."""
    r = _rs(2, 3)
    assert (r.L, r.M) == (3, 2)
    tail_rows, first, n = 40000, 50, 40001
    outs = r.out_count(first + n) - r.out_count(first)
    Rn = outs + 5
    assert SC.blocks(outs * 8) > SC.cap("resample.hip", "rs_lv_push_kernel") and SC.blocks(tail_rows * 8) > SC.cap("resample.hip", "rs_lv_tail_kernel")
    assert n > tail_rows >= r.tail_rows and r.out_count(first + n) > Rn
    pool = Pool(Rn, sessions=3)
    tails = torch.full((3, tail_rows * 64), 0x5A, dtype=torch.uint8, device=DEV)
    sig = LV.recording(first + n, 91)
    other = LV.recording(21, 92)
    dev, dev_other = torch.from_numpy(sig).to(DEV), torch.from_numpy(other).to(DEV)

    def push(sess, raw, lens, staging):
        L.check(L.lib().msig_rs_lv_push(*pool.args(), tails.data_ptr(), tail_rows, tail_rows * 64, *r.ratio_args(), _i32(sess), _i64(raw), _i64(lens),
                                        len(sess), staging.data_ptr(), _stream()), "msig_rs_lv_push")

    push([2, 0], [0, 0], [first, 20], torch.cat([dev[:first], dev_other[:20]]))
    push([0, 2], [20, first], [1, n], torch.cat([dev_other[20:], dev[first:]]))
    y, n_out = _resample(dev, r)
    y0, n0 = _resample(dev_other, r)
    torch.cuda.synchronize()
    got, got_tails = pool.rings(), tails.cpu().numpy().view(np.float64).reshape(3, tail_rows, 8)
    assert np.array_equal(_bits(got[2]), _bits(_wrapped(y.cpu().numpy()[:n_out], Rn)))
    assert 0 < n0 < Rn and np.array_equal(_bits(got[0]), _bits(_wrapped(y0.cpu().numpy()[:n0], Rn)))
    assert np.array_equal(_bits(got_tails[2]), _bits(_wrapped(sig, tail_rows))) and np.array_equal(_bits(got_tails[0]), _bits(_wrapped(other, tail_rows)))
    assert np.all(_bits(got[1]) == _bits(FILL)) and np.all(_bits(got_tails[1]) == _bits(FILL))
    assert r.out_count(20) < r.out_count(21), "the 1-row chunk yields an output"


def test_a_run_over_the_window_kernels_cap():
    """C_all = 1, T = 16, S = 64, one run of 16 385 consecutive windows: a span of 1 048 592 samples, over 4096 x 256.  msig_rec_windows
    on the linear recording and msig_lv_windows_multi on its wrapped ring, in one call each, against msig_rec_windows in pieces of
    1000 windows; and against lv_reference.normalised at tests/test_live_gpu.py's tolerance for fp32 rounding of fp64 statistics."""
    from multimodalsignal_amd.runtime import Arenas
    Tn, Sn, B, n0 = 16, 64, 16385, 16
    span = (B - 1) * Sn + Tn
    for source, kernel in (("record.hip", "rec_windows_kernel"), ("live.hip", "lv_windows_kernel")):
        assert SC.blocks(span) > SC.cap(source, kernel) >= SC.blocks(span - 256)
    written = (n0 + B - 1) * Sn + Tn
    Rn = span + 8
    assert written - Rn <= n0 * Sn and written > Rn
    rs = np.random.RandomState(17)
    sig = np.ascontiguousarray(rs.randn(written, 1) * 1.5 + 0.7 + np.sin(np.arange(written) / 5000.0)[:, None])
    dev = torch.from_numpy(sig).to(DEV)
    stats = torch.full((2 * MC + 1,), float("nan"), dtype=torch.float64, device=DEV)
    stats[0], stats[MC], stats[2 * MC] = float(sig.mean()), 1.0 / float(sig.std()), 7
    head = _head(dev, [0], Tn, Sn, mask=0)
    pieces = torch.empty((B, 1, Tn), dtype=torch.float32, device=DEV)
    for a in range(0, B, 1000):
        b = min(1000, B - a)
        assert SC.blocks((b - 1) * Sn + Tn) <= SC.cap("record.hip", "rec_windows_kernel")
        L.check(L.lib().msig_rec_windows(*head, n0 + a, b, stats.data_ptr(), pieces[a].data_ptr(), _stream()), "msig_rec_windows")
    whole = torch.full((B * Tn + 64,), -77.0, dtype=torch.float32, device=DEV)
    L.check(L.lib().msig_rec_windows(*head, n0, B, stats.data_ptr(), whole.data_ptr(), _stream()), "msig_rec_windows")
    assert _same_bits(whole[:B * Tn], pieces.reshape(-1)) and bool((whole[B * Tn:] == -77.0).all())
    # the ring of session 1 of two: sample i in row i % R, the last R samples
    pool = Pool(Rn, sessions=2, C_all=1)
    i = torch.arange(written - Rn, written, device=DEV)
    pool.mem[1].view(torch.float64)[i % Rn] = dev[i, 0]
    table = torch.full((2, 2 * MC + 1), float("nan"), dtype=torch.float64, device=DEV)
    table[1] = stats
    arenas = Arenas(3, DEV, (("other", 1000), ("x", B * Tn * 4), ("tail", 256)))
    arenas.mem.fill_(0x5A)
    L.check(L.lib().msig_lv_windows_multi(*pool.args(), _i32([0]), 1, 0, Tn, Sn, _i32([1] * B), _i64(range(n0, n0 + B)), _i64([written] * B), B,
                                          table.data_ptr(), arenas.ptr("x"), C.byref(arenas.multi([2, 0])), _stream()), "msig_lv_windows_multi")
    torch.cuda.synchronize()
    for s in (0, 2):
        assert _same_bits(arenas.view(s, "x", torch.float32)[:B * Tn], pieces.reshape(-1)), s
        assert bool((arenas.view(s, "x")[B * Tn * 4:] == 0x5A).all()) and bool((arenas.view(s, "other") == 0x5A).all())
        assert bool((arenas.view(s, "tail") == 0x5A).all())
    assert bool((arenas.mem[1] == 0x5A).all()) and bool((pool.mem[0] == 0x5A).all())
    got = pieces.cpu().numpy()
    mean, inv = [float(stats[0])], [float(stats[MC])]
    for b in sorted(set(range(0, B, 97)) | set(range(B - 6, B))):         # the last windows lie in the loop's second pass
        ref = LV.normalised(sig[(n0 + b) * Sn:(n0 + b) * Sn + Tn], [0], 0, mean, inv)
        assert np.abs(got[b] - ref).max() <= 2e-6 * max(1.0, np.abs(ref).max()), b


@pytest.mark.parametrize("family", ["rn", "gp"])
def test_a_run_over_the_row_kernels_cap_behind_its_step(family):
    """T = 256, S = 1, 3 of 8 columns: a session takes windows 0 .. 44, then ONE step and ONE *_lv_windows_multi take the run of 4097
    windows behind them (4097 x 256 elements, over 4096 x 256) from a ring that has wrapped: the offline chain's records and rows,
    whose own grids stay under their caps."""
    from multimodalsignal_amd.runtime import Arenas
    lib = L.lib()
    gp = family == "gp"
    Tn, Sn, cols, B, before = 256, 1, LV.COLS["3of8"], 4097, 45
    Cn, mask = len(cols), LV.mask_of(cols)
    kernel = ("gaps.hip", "gp_lv_windows_kernel") if gp else ("running.hip", "rn_lv_windows_kernel")
    offline_kernel = ("gaps.hip", "gp_windows_kernel") if gp else ("running.hip", "rn_windows_kernel")
    assert SC.blocks(B * Tn) > SC.cap(*kernel) >= SC.blocks((B - 1) * Tn) and SC.blocks(B * Tn) <= SC.cap(*offline_kernel)
    N = before + B
    n = N - 1 + Tn
    Rn = n - before + 8
    sig = LV.recording(n, 23)
    if gp:
        sig[np.random.RandomState(24).rand(*sig.shape) < 0.03] = np.nan
    dev = torch.from_numpy(sig).to(DEV)
    head = _head(dev, cols, Tn, Sn)
    mode = (G.EXPANDING, 0, 0.0) if gp else 2
    want_tab = torch.zeros((N, 2 * MC + 1), dtype=torch.float64, device=DEV)
    want_cov = torch.zeros((N, MC), dtype=torch.float64, device=DEV)
    want_out = torch.empty((B, Cn, Tn), dtype=torch.float32, device=DEV)
    sums = torch.zeros((N, 3 * MC), dtype=torch.float64, device=DEV)
    assert N <= SC.cap("running.hip", "rn_sums_kernel")
    if gp:
        pivot = torch.zeros(2 * MC, dtype=torch.float64, device=DEV)
        L.check(lib.msig_gp_pivot(*head, N, pivot.data_ptr(), _stream()), "msig_gp_pivot")
        L.check(lib.msig_gp_sums(*head, pivot.data_ptr(), 0, N, sums.data_ptr(), _stream()), "msig_gp_sums")
        L.check(lib.msig_gp_stats(*head, pivot.data_ptr(), sums.data_ptr(), N, C.byref(L.GpMode(*mode)), want_tab.data_ptr(), want_cov.data_ptr(),
                                  _stream()), "msig_gp_stats")
        L.check(lib.msig_gp_windows(*head, before, B, want_tab[before].data_ptr(), want_out.data_ptr(), _stream()), "msig_gp_windows")
    else:
        L.check(lib.msig_rn_sums(*head, 0, N, sums.data_ptr(), _stream()), "msig_rn_sums")
        L.check(lib.msig_rn_stats(*head, sums.data_ptr(), N, mode, want_tab.data_ptr(), _stream()), "msig_rn_stats")
        L.check(lib.msig_rn_windows(*head, before, B, want_tab[before].data_ptr(), want_out.data_ptr(), _stream()), "msig_rn_windows")
    slot, sessions = 69, 70
    pool = Pool(Rn, sessions=sessions)
    state_bytes = lib.msig_gp_state_bytes(0) if gp else lib.msig_rn_state_bytes(2)
    state = torch.full((sessions, state_bytes // 8), float("nan"), dtype=torch.float64, device=DEV)
    arenas = Arenas(3, DEV, (("other", 1000), ("x", B * Cn * Tn * 4), ("tail", 256)))
    rows_args = (_i32(cols), Cn, mask, Tn, Sn)

    def step(first, count, written):
        sess, win, wr, nx = _i32([slot] * count), _i64(range(first, first + count)), _i64([written] * count), _i64([first] * count)
        table = torch.full((count + 1, 2 * MC + 1), float("nan"), dtype=torch.float64, device=DEV)
        cov = torch.full((count + 1, MC), float("nan"), dtype=torch.float64, device=DEV)
        if gp:
            L.check(lib.msig_gp_lv_step(*pool.args(), *rows_args, C.byref(L.GpMode(*mode)), state.data_ptr(), state_bytes, sess, win, wr, nx, count,
                                        table.data_ptr(), cov.data_ptr(), _stream()), "msig_gp_lv_step")
        else:
            L.check(lib.msig_rn_lv_step(*pool.args(), *rows_args, mode, state.data_ptr(), state_bytes, sess, win, wr, nx, count, table.data_ptr(),
                                        _stream()), "msig_rn_lv_step")
        return sess, win, wr, table, cov

    held = before - 1 + Tn
    pool.push([slot], [0], [held], [sig[:held]])
    step(0, before, held)
    pool.push([slot], [held], [n - held], [sig[held:]])
    assert n - held <= Rn and n > Rn and before * Sn >= n - Rn
    sess, win, wr, table, cov = step(before, B, n)
    arenas.mem.fill_(0x5A)
    fill = lib.msig_gp_lv_windows_multi if gp else lib.msig_rn_lv_windows_multi
    L.check(fill(*pool.args(), *rows_args, sess, win, wr, B, table.data_ptr(), arenas.ptr("x"), C.byref(arenas.multi([2, 0])), _stream()),
            "*_lv_windows_multi")
    torch.cuda.synchronize()
    got = table.cpu().numpy()
    assert np.all(np.isnan(got[B])) and np.array_equal(_bits(_selected(got[:B], Cn)), _bits(_selected(want_tab.cpu().numpy()[before:], Cn)))
    if gp:
        gcov = cov.cpu().numpy()
        assert np.all(np.isnan(gcov[B])) and np.array_equal(_bits(gcov[:B, :Cn]), _bits(want_cov.cpu().numpy()[before:, :Cn])) and (gcov[:B, :Cn] < 1).any()
    for s in (0, 2):
        assert _same_bits(arenas.view(s, "x", torch.float32)[:B * Cn * Tn], want_out.reshape(-1)), s
        assert bool((arenas.view(s, "other") == 0x5A).all()) and bool((arenas.view(s, "tail") == 0x5A).all())
    assert bool((arenas.mem[1] == 0x5A).all()) and bool((pool.mem[:slot] == 0x5A).all()) and bool(torch.isnan(state[:slot]).all())


@pytest.mark.parametrize("family", ["rn", "gp"])
def test_sums_and_trailing_statistics_of_65_600_windows(family):
    """T = 16, S = 1, N = 65 600 windows, trailing:2 — a workgroup (sums) or a wave (statistics) per window, over the cap of 65 536.
    The sums against the call in two pieces.  The statistics against the call in two pieces as well: a trailing:2 record is a function
    of the pivot and of the records of windows n - 1 and n, so msig_*_stats on the sums from window 39 990 on gives, from its second
    record on, the records of windows 39 991 ...  Beside it the reference modules' restatement on some 300 windows, windows 65 535 ..
    65 540 among them, where its additions are the device's: W1 of the columns without log1p, the window count, the mean (p + W1 /
    count; 1 / std passes W2, which the device forms with fma and numpy does not) and, with gaps, the counts and the coverage."""
    lib = L.lib()
    gp = family == "gp"
    Tn, Sn, N, cols = 16, 1, 65600, LV.COLS["3of8"]
    Cn, mask = len(cols), LV.mask_of(cols)
    src = "gaps.hip" if gp else "running.hip"
    assert N > SC.cap(src, f"{family}_sums_kernel") >= N - 256 and N > SC.cap(src, f"{family}_stats_kernel") >= N - 256
    sig = LV.recording(N - 1 + Tn, 31)
    if gp:
        sig[np.random.RandomState(32).rand(*sig.shape) < 0.03] = np.nan
    dev = torch.from_numpy(sig).to(DEV)
    head = _head(dev, cols, Tn, Sn)
    width = 3 * MC if gp else 2 * MC
    pivot = torch.zeros(2 * MC, dtype=torch.float64, device=DEV)
    mode = C.byref(L.GpMode(G.TRAILING, 2, 0.0))
    if gp:
        L.check(lib.msig_gp_pivot(*head, N, pivot.data_ptr(), _stream()), "msig_gp_pivot")

    def sums_of(n0, B):
        out = torch.full((B + 1, width), float("nan"), dtype=torch.float64, device=DEV)
        if gp:
            L.check(lib.msig_gp_sums(*head, pivot.data_ptr(), n0, B, out.data_ptr(), _stream()), "msig_gp_sums")
        else:
            L.check(lib.msig_rn_sums(*head, n0, B, out.data_ptr(), _stream()), "msig_rn_sums")
        return out

    def stats_of(sums, n):
        tab = torch.full((n + 1, 2 * MC + 1), float("nan"), dtype=torch.float64, device=DEV)
        cov = torch.full((n + 1, MC), float("nan"), dtype=torch.float64, device=DEV)
        if gp:
            L.check(lib.msig_gp_stats(*head, pivot.data_ptr(), sums.data_ptr(), n, mode, tab.data_ptr(), cov.data_ptr(), _stream()), "msig_gp_stats")
        else:
            L.check(lib.msig_rn_stats(*head, sums.data_ptr(), n, 2, tab.data_ptr(), _stream()), "msig_rn_stats")
        return tab, cov

    whole = sums_of(0, N)
    cut = 40000
    parts = torch.cat([sums_of(0, cut)[:cut], sums_of(cut, N - cut)[:N - cut]])
    torch.cuda.synchronize()
    assert bool(torch.isnan(whole[N]).all()), "wrote past the records"
    sel = [c + part * MC for part in range(width // MC) for c in range(Cn)]
    assert _same_bits(whole[:N, sel], parts[:, sel])
    tab, cov = stats_of(whole, N)
    lo, _c = stats_of(whole, cut)
    hi, hi_cov = stats_of(whole[cut - 10:], N - cut + 10)
    torch.cuda.synchronize()
    got = tab.cpu().numpy()
    assert np.all(np.isnan(got[N])), "wrote past the table"
    want = np.concatenate([lo.cpu().numpy()[:cut], hi.cpu().numpy()[10:N - cut + 10]])
    assert np.array_equal(_bits(_selected(got[:N], Cn)), _bits(_selected(want, Cn)))
    assert np.all(got[1:N, 2 * MC] == 2) and got[0, 2 * MC] == 1
    # the restatement
    some = sorted(set(range(1, N, 219)) | set(range(65530, 65545)) | {N - 1})
    plain = [c for c, col in enumerate(cols) if NAMES8[col] != "chest_EDA"]
    host_sums = whole.cpu().numpy()
    if gp:
        gcov = cov.cpu().numpy()
        assert np.all(np.isnan(gcov[N])) and np.array_equal(_bits(gcov[cut:N, :Cn]), _bits(hi_cov.cpu().numpy()[10:N - cut + 10, :Cn]))
        v, ok = G.transformed(sig, cols, mask)
        p, found = G.pivot(v, ok, Tn, Sn, 40)
        assert found.all() and np.array_equal(_bits(pivot.cpu().numpy()[:Cn][plain]), _bits(p[plain]))
    else:
        v = RN.transformed(sig, cols, mask)
        ok, p = np.ones(v.shape, dtype=bool), v[0]

    def record(k):
        m = ok[k * Sn:k * Sn + Tn]
        return RN._ordered(np.where(m, v[k * Sn:k * Sn + Tn] - p, 0.0)), RN._ordered(m.astype(np.float64))

    for k in some:
        (a1, an), (b1, bn) = record(k - 1), record(k)
        assert np.array_equal(_bits(host_sums[k, :Cn][plain]), _bits(b1[plain])), k
        count = (an / Tn + bn / Tn) * Tn
        assert np.all(count > 0)
        assert np.array_equal(_bits(got[k, :Cn][plain]), _bits((p + (a1 + b1) / count)[plain])), k
        if gp:
            assert np.array_equal(host_sums[k, 2 * MC:2 * MC + Cn], bn) and np.array_equal(_bits(gcov[k, :Cn]), _bits(bn / Tn)), k
    if gp:
        assert (host_sums[:N, 2 * MC:2 * MC + Cn] < Tn).any()


@pytest.mark.parametrize("family", ["rn", "gp"])
def test_rows_of_65_600_windows_with_a_record_each(family):
    """T = 256, S = 1, one column, B = 65 600: B x T / 256 blocks, over 65 536.  Against the call in two pieces, on the device."""
    lib = L.lib()
    gp = family == "gp"
    Tn, Sn, B, cols = 256, 1, 65600, [3]
    src = ("gaps.hip", "gp_windows_kernel") if gp else ("running.hip", "rn_windows_kernel")
    assert SC.blocks(B * Tn) > SC.cap(*src) >= SC.blocks((B - 64) * Tn)
    sig = LV.recording(B - 1 + Tn, 41)
    if gp:
        sig[np.random.RandomState(42).rand(*sig.shape) < 0.03] = np.nan
    dev = torch.from_numpy(sig).to(DEV)
    head = _head(dev, cols, Tn, Sn)
    rs = np.random.RandomState(43)
    tab = np.zeros((B, 2 * MC + 1))
    tab[:, 0], tab[:, MC], tab[:, 2 * MC] = 33.0 + 0.01 * rs.randn(B), 10.0 + rs.rand(B), 1
    table = torch.from_numpy(tab).to(DEV)
    call = lib.msig_gp_windows if gp else lib.msig_rn_windows
    whole = torch.full((B * Tn + 64,), -77.0, dtype=torch.float32, device=DEV)
    L.check(call(*head, 0, B, table.data_ptr(), whole.data_ptr(), _stream()), "msig_*_windows")
    pieces = torch.empty((B, Tn), dtype=torch.float32, device=DEV)
    cut = 30000
    for a, b in ((0, cut), (cut, B - cut)):
        assert SC.blocks(b * Tn) <= SC.cap(*src)
        L.check(call(*head, a, b, table[a].data_ptr(), pieces[a].data_ptr(), _stream()), "msig_*_windows")
    torch.cuda.synchronize()
    assert _same_bits(whole[:B * Tn], pieces.reshape(-1)) and bool((whole[B * Tn:] == -77.0).all())
    last = pieces[B - 1].cpu().numpy()
    v = sig[B - 1:B - 1 + Tn, 3]
    ref = np.where(np.isnan(v), np.float32(0), ((v - tab[B - 1, 0]) * tab[B - 1, MC]).astype(np.float32))
    assert np.array_equal(_bits(last), _bits(ref.astype(np.float32)))          # plain IEEE operations: the restatement's bits
    assert bool(torch.isfinite(pieces).all()) and (not gp or bool((pieces == 0).any()))


def test_resample_of_64_columns_over_the_cap():
    """Ratio 3 / 2, C_all = 64, 262 145 outputs or a few more: n_out x C_all over 65 536 x 256.  Columns 0, 37 and 63 against the call
    on contiguous single-column copies, far under the cap."""
    r = _rs(2, 3)
    C_all = 64
    n_in = r.max_rows(262144) + 1
    n_out = r.out_count(n_in)
    cap = SC.cap("resample.hip", "rs_resample_kernel")
    assert SC.blocks(n_out * C_all) > cap >= SC.blocks((n_out - 8) * C_all) and SC.blocks(n_out) <= cap
    torch.manual_seed(51)
    x = torch.randn((n_in, C_all), dtype=torch.float64, device=DEV) + torch.arange(C_all, dtype=torch.float64, device=DEV)
    y, _n = _resample(x, r)
    for c in (0, 37, 63):
        one, _n = _resample(x[:, c:c + 1].contiguous(), r)
        assert _same_bits(y[:n_out, c], one[:n_out, 0]), c
    torch.cuda.synchronize()
    assert bool((y[n_out] == -7.25).all()), "wrote past the last output"
    assert bool(torch.isfinite(y[:n_out]).all()) and not _same_bits(y[:n_out, 0], y[:n_out, 1])


# ---- D. 300 wearers in one LiveMonitor --------------------------------------------------------------------------------------------------
TL_FIELDS = ("t_end", "mean_p", "std_p", "pred", "entropy", "mutual_info", "votes", "score", "smoothed", "state", "warmup")


def _same(a, b, what=""):
    for k in TL_FIELDS + (("coverage", "valid", "lost") if a.coverage is not None or b.coverage is not None else ()):
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)
    assert a.events == b.events, what


END_TO_END = [("head:7", False, False), ("expanding", True, False), ("decayed:4", False, False), ("trailing:5", False, True)]


@pytest.mark.parametrize("reference,gapped,resampled", END_TO_END, ids=["head7", "expanding-gaps", "decayed4", "trailing5-resampled"])
def test_300_wearers_in_one_live_monitor_have_monitor_runs_timelines(reference, gapped, resampled):
    """LiveMonitor(max_sessions=320, eval_batch=256), 300 open sessions, T = 64, S = 16, 3 of 8 columns, one member.  Session k is fed
    recording k % 3 of three from tick k % 7 on in chunks whose length depends on k, so a tick's batch mixes sessions at different
    windows, with none, one or several new ones: over 256 rows in two pieces, a piece of more than 128 runs.  With gaps one stretch
    of recording 1 arrives as skip() calls in every session that is fed it.  Ten sessions in slots 64 .. 299 are closed midway and
    others opened in their slots.  Every open session's timeline is Monitor.run's of its recording in every field and in its events;
    Monitor.run is made three times."""
    from multimodalsignal_amd.live import LiveMonitor, replay_pieces
    from multimodalsignal_amd.monitor import Gaps, Monitor
    Tn, Sn, windows = 64, 16, 20
    channels = [NAMES8[c] for c in LV.COLS["3of8"]]
    models = LV.models("cnn_gru_attention", 3, 2, 1, DEV)
    r = _rs(96, 64) if resampled else None
    rows = (windows - 1) * Sn + Tn + 2
    spans = [(7 * Sn + 5, 7 * Sn + 5 + 3 * Sn + Tn)] if gapped else []
    if resampled:
        assert (r.L, r.M) == (2, 3)
        rows = r.max_rows(rows)
    recs = []
    for i in range(3):
        sig = LV.recording(rows + 3 * i, 700 + i)
        if gapped:
            sig[np.random.RandomState(710 + i).rand(*sig.shape) < 0.02] = np.nan
            if i == 1:
                sig[spans[0][0]:spans[0][1]] = np.nan
        recs.append((sig, torch.from_numpy(sig).to(DEV)))
    common = dict(window_s=Tn / FS, stride_s=Sn / FS, reference=reference, eval_batch=256, channels=channels, halflife=2, min_on=2,
                  gaps=Gaps(0.75, 2) if gapped else None, resampler=r)
    sm = Monitor(models, FS, on=0.55, off=0.45, **common).run(recs[0][1], NAMES8).smoothed
    sm = sm[np.isfinite(sm)]
    off, on = float(np.percentile(sm, 40)), float(np.percentile(sm, 60))
    if not off < on:
        off, on = 0.45, 0.55
    mon = Monitor(models, FS, on=on, off=off, **common)
    live = LiveMonitor(models, FS, max_sessions=320, on=on, off=off, **common)
    offline = [mon.run(recs[i][1], NAMES8) for i in range(3)]
    assert all(len(o.t_end) >= windows - 1 for o in offline)
    lengths = [11, Sn, Sn + 5, 2 * Sn + 3, 3 * Sn + 1]
    if resampled:
        lengths = [n * 3 // 2 for n in lengths]
    todo, rec_of, late = {}, {}, {}

    def enrol(sid, i, length, start):
        live.open(sid, NAMES8)
        n = recs[i][0].shape[0]
        todo[sid] = [p for a in range(0, n, length) for p in replay_pieces(a, min(a + length, n), spans if i == 1 else [])]
        rec_of[sid], late[sid] = i, start

    for k in range(P):
        enrol(k, k % 3, lengths[k % 5], k % 7)
        assert live.sessions[k].slot == k
    reused = [64, 65, 100, 127, 128, 129, 191, 192, 255, 299]
    tick, most_rows, most_sessions, skipped = 0, 0, 0, 0
    while any(todo.values()):
        if tick == 12:
            for k in reused:
                assert live.sessions[k].book.written > 0                 # the slot's ring, state and tail are in use
                live.close(k)
                del todo[k]
            for k in reused:
                enrol(("again", k), (k + 1) % 3, lengths[(k + 2) % 5], tick)
            assert [live.sessions[("again", k)].slot for k in reused] == reused and len(live.sessions) == P
        push, skip = {}, {}
        for sid, pieces in todo.items():
            if tick >= late[sid] and pieces:
                a, b, gone = pieces.pop(0)
                if gone:
                    skip[sid] = b - a
                else:
                    push[sid] = recs[rec_of[sid]][1][a:b]
        ups = [live.push(push)] if push else []
        if skip:
            ups.append(live.skip(skip))
            skipped += len(skip)
        for out in ups:
            most_rows = max(most_rows, sum(len(u) for u in out.values()))
            most_sessions = max(most_sessions, sum(1 for u in out.values() if u))
        tick += 1
    assert most_rows > 256 and most_sessions > GROUP and (not gapped or skipped >= P // 3)
    for sid in live.sessions:
        _same(live.timeline(sid), offline[rec_of[sid]], sid)
    if gapped:
        assert offline[1].lost.any() and not offline[1].valid.all()
