"""Mixed-rate streams on the GPU (include/msig_mx.h, multimodalsignal_amd/resample.py, live.py, monitor.py).  The
oracle is the existing single-rate call: every stream resampled on its own by msig_rs_resample, truncated to the slowest stream and laid
side by side (tests/mx_reference.py), which tests/test_resample_gpu.py ties to the np.longdouble restatement.  Every comparison is
uint64 or uint32 equality: the mixed calls form an output with the device function of the single-rate calls, so there is no tolerance."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

import lv_reference as R
import mx_reference as MX
import rs_reference as RS
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd.resample import FirResampler, MixedResampler, Stream

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FS = MX.FS
NAMES8 = R.NAMES8
SHAPES = [(256, 64, "8of8"), (200, 37, "3of8")]
K_HEAD = 7
POOL_SLOTS, SESSIONS = 4, (0, 1, 3)          # three sessions in a pool of four: ring 2 and tail 2 are never touched
TL_FIELDS = ("t_end", "mean_p", "std_p", "pred", "entropy", "mutual_info", "votes", "score", "smoothed", "state", "warmup")
CHANNELS6 = ["chest_ECG", "chest_EDA", "chest_Resp", "wrist_BVP", "chest_ACC_x", "wrist_EDA"]
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
CHEST, ACC, BVP, SLOW = range(4)             # the streams of mx_reference.STREAMS by index


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "the gpu tier needs an MI355X"


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _ring(T, S):
    return (K_HEAD - 1) * S + T + 41 + 256          # test_resample_gpu.py's ring and 256 rows for the streams' latency spread (176)


@functools.lru_cache(maxsize=None)
def _mx():
    mx = MX.resampler(DEV)
    assert [(g.L, g.M, g.half) for g in mx.streams] == [(16, 175, 1750), (2, 1, 20), (1, 1, 0), (16, 1, 160)] and mx.names == MX.ORDER
    return mx


@functools.lru_cache(maxsize=None)
def _raw(T, S, k):
    """Session k's raw streams: a little more than three rings of outputs, another length and other values per session — on the host
    and on the device."""
    host = MX.raw_streams(_mx(), 3 * _ring(T, S) + 17 + 29 * k, 1000 * T + 10 * S + k)
    return host, {n: torch.from_numpy(x).to(DEV) for n, x in host.items()}


def _head(dev, cols, mask, T, S):
    return dev.data_ptr(), dev.shape[0], dev.shape[1], (C.c_int32 * len(cols))(*cols), len(cols), mask, T, S


@functools.lru_cache(maxsize=None)
def _offline(T, S, key, k):
    """The oracle of session k, computed once: the streams' own msig_rs_resample outputs, their assembly, msig_rec_stats over windows
    [0, K_HEAD) of it and msig_rec_windows of every window."""
    mx, lib = _mx(), L.lib()
    ys = MX.stream_outputs(mx, _raw(T, S, k)[1], DEV)
    y = MX.assembly(mx, _raw(T, S, k)[1], DEV)
    cols, mask = MX.cols_of(key)
    N = R.count(y.shape[0], T, S)
    stats = torch.full((2 * L.MAX_C + 1,), float("nan"), dtype=torch.float64, device=DEV)
    scratch = torch.empty(lib.msig_rec_scratch_bytes(), dtype=torch.uint8, device=DEV)
    L.check(lib.msig_rec_stats(*_head(y, cols, mask, T, S), 0, K_HEAD, stats.data_ptr(), scratch.data_ptr(), _stream()), "msig_rec_stats")
    out = torch.empty((N, len(cols), T), dtype=torch.float32, device=DEV)
    L.check(lib.msig_rec_windows(*_head(y, cols, mask, T, S), 0, N, stats.data_ptr(), out.data_ptr(), _stream()), "msig_rec_windows")
    torch.cuda.synchronize()
    return {n: v.cpu().numpy() for n, v in ys.items()}, y.cpu().numpy(), stats, out.cpu().numpy()


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- 1. one group is the single-rate call ---------------------------------------------------------------------------------------------
def test_one_group_of_all_columns_is_the_single_rate_call():
    """One stream holding all eight columns at 16 / 175.  msig_mx_lv_push leaves the ring and tail bytes of msig_rs_lv_push under the same
    chunking (three sessions, ragged chunks, a stretch without a staging buffer); msig_mx_resample with n_out = out_count is
    msig_rs_resample, and with a smaller n_out it leaves the rows after it untouched."""
    T, S = 256, 64
    Rn = _ring(T, S)
    one = MixedResampler([Stream("all", 700, NAMES8)], FS, device=DEV)
    r = FirResampler(700, 64, DEV)
    g = one.streams[0]
    assert (g.L, g.M, g.half, g.tail_rows, g.col0, g.ncols, g.h_off, g.tail_off) == (16, 175, 1750, r.tail_rows, 0, 8, 0, 0)
    recs = {k: torch.from_numpy(R.recording(r.max_rows(2 * Rn + 50 + 31 * k), 7 + k)).to(DEV) for k in SESSIONS}
    mxp = MX.MxPool(one, Rn, POOL_SLOTS, SESSIONS, DEV)
    mem = torch.full((POOL_SLOTS, Rn * 64), 0x5A, dtype=torch.uint8, device=DEV)
    tails = torch.full((POOL_SLOTS, r.tail_rows * 64), 0x5A, dtype=torch.uint8, device=DEV)
    assert tails.shape == mxp.tails.shape and mem.shape == mxp.mem.shape
    raw = {k: 0 for k in SESSIONS}
    rs = np.random.RandomState(2)
    calls = 0
    while any(raw[k] < recs[k].shape[0] for k in SESSIONS):
        missing = calls % 5 == 3
        ks = [k for k in SESSIONS if raw[k] < recs[k].shape[0] and rs.rand() < 0.7]
        if not ks:
            continue
        ks = [ks[i] for i in rs.permutation(len(ks))]
        lens = {k: min(int(rs.choice([1, 7, r.tail_rows - 1, r.tail_rows + 1, 3 * r.tail_rows + 7, 4000])), recs[k].shape[0] - raw[k]) for k in ks}
        chunks = {k: recs[k][raw[k]:raw[k] + lens[k]] for k in ks}
        n = len(ks)
        staging = torch.cat([chunks[k] for k in ks]) if n > 1 else chunks[ks[0]]
        L.check(L.lib().msig_rs_lv_push(mem.data_ptr(), POOL_SLOTS, Rn, Rn * 64, 8, tails.data_ptr(), r.tail_rows, r.tail_rows * 64, *r.ratio_args(),
                                        (C.c_int32 * n)(*ks), (C.c_int64 * n)(*[raw[k] for k in ks]), (C.c_int64 * n)(*[lens[k] for k in ks]), n,
                                        None if missing else staging.data_ptr(), _stream()), "msig_rs_lv_push")
        mxp.push([(k, 0, chunks[k]) for k in ks], missing=missing)
        for k in ks:
            raw[k] += lens[k]
        calls += 1
    torch.cuda.synchronize()
    assert calls > 10 and all(mxp.raw[k] == [raw[k]] and r.out_count(raw[k]) > 2 * Rn for k in SESSIONS)
    assert torch.equal(mxp.mem, mem) and torch.equal(mxp.tails, tails)
    assert bool((mem[2] == 0x5A).all()) and not bool((mem[0] == 0x5A).all()) and not bool((tails[3] == 0x5A).all())
    # offline
    x = recs[0]
    n_in, n_out = x.shape[0], r.out_count(x.shape[0])
    want = torch.empty((n_out, 8), dtype=torch.float64, device=DEV)
    L.check(L.lib().msig_rs_resample(x.data_ptr(), n_in, 8, *r.ratio_args(), want.data_ptr(), n_out, _stream()), "msig_rs_resample")
    grp = g.group()
    for n in (n_out, n_out - 1, 300, 1, 0):
        y = torch.full((n_out + 1, 8), -7.25, dtype=torch.float64, device=DEV)          # the rows after the last output keep the canary
        L.check(L.lib().msig_mx_resample(x.data_ptr(), n_in, one.h.data_ptr(), C.byref(grp), y.data_ptr(), n, 8, _stream()), "msig_mx_resample")
        torch.cuda.synchronize()
        assert np.array_equal(_u64(y[:n].cpu().numpy()), _u64(want[:n].cpu().numpy())), n
        assert bool((y[n:] == -7.25).all()), n
    assert np.array_equal(_u64(one.apply({"all": x}).cpu().numpy()), _u64(want.cpu().numpy()))


# ---- 2. every way of chunking ---------------------------------------------------------------------------------------------------------
def _check_batch(pool, cols, mask, T, S, stats, rows, arenas, want, what):
    """ONE msig_lv_windows_multi over rows [(session, window)] with the sessions' `written` = their slowest stream's count; slots 2 and
    0 of three hold the rows' offline bits; slot 1 and the rest of every arena keep 0x5A."""
    arenas.mem.fill_(0x5A)
    B = len(rows)
    L.check(L.lib().msig_lv_windows_multi(*pool.args(), (C.c_int32 * len(cols))(*cols), len(cols), mask, T, S, (C.c_int32 * B)(*[k for k, _n in rows]),
                                          (C.c_int64 * B)(*[n for _k, n in rows]), (C.c_int64 * B)(*[pool.written(k) for k, _n in rows]), B,
                                          stats.data_ptr(), arenas.ptr("x"), C.byref(arenas.multi([2, 0])), _stream()), "msig_lv_windows_multi")
    torch.cuda.synchronize()
    n = B * len(cols) * T
    ref = np.concatenate([want[k][w].reshape(-1) for k, w in rows]).view(np.uint32)
    for s in (0, 2):
        x = arenas.view(s, "x", torch.float32).cpu().numpy()
        assert np.array_equal(x[:n].view(np.uint32), ref), (what, s, rows)
        assert np.all(x[n:].view(np.uint8) == 0x5A), (what, "wrote past the batch")
    assert np.all(arenas.mem[1].cpu().numpy() == 0x5A)


def _next_prime(n):
    n += 1
    while any(n % d == 0 for d in range(2, int(n ** 0.5) + 1)):
        n += 1
    return n


@pytest.mark.parametrize("T,S,key", SHAPES, ids=[f"t{T}-s{S}" for T, S, _k in SHAPES])
def test_every_way_of_chunking_gives_the_offline_bits(T, S, key):
    """Three sessions' raw streams into slots 0, 1 and 3 of a pool of four, each session cut its own way, the streams of a session
    arriving in different calls and in a shuffled order within a call:
      session 0 — single rows on the 4 Hz and 32 Hz streams, sevens on the 64 Hz stream, and the 700 Hz stream row by row for about
                  one ring of outputs and in sevens after that;
      session 1 — a prime near each stream's tail_rows for the first ring and a half, then chunks longer than tail_rows;
      session 3 — as much as the ring allows, with the 4 Hz stream first as far AHEAD of the others as the ring allows and, from the
                  middle on, as far BEHIND: it moves only when no other stream can.
    A stream may take a chunk while its output count stays at or below next window * S + R (no row a window still to be checked
    needs is overwritten).  After every call the newly complete windows of all sessions — complete in EVERY stream — as one
    msig_lv_windows_multi batch with `written` = the slowest stream's count: the bits of msig_rec_windows on the offline assembly.
    At the end every stream's column block in every ring row is the stream's own msig_rs_resample output (the streams of a session
    end at different rows) and every tail row the raw stream's row; ring 2 and tail 2 keep 0x5A."""
    from multimodalsignal_amd.runtime import Arenas
    mx, Rn = _mx(), _ring(T, S)
    G = len(mx.streams)
    off = {k: _offline(T, S, key, k) for k in SESSIONS}
    want = {k: off[k][3] for k in SESSIONS}
    cols, mask = MX.cols_of(key)
    stats = torch.full((POOL_SLOTS, 2 * L.MAX_C + 1), float("nan"), dtype=torch.float64, device=DEV)
    for k in SESSIONS:
        stats[k].copy_(off[k][2])
    pool = MX.MxPool(mx, Rn, POOL_SLOTS, SESSIONS, DEV)
    devs = {k: [_raw(T, S, k)[1][g.name] for g in mx.streams] for k in SESSIONS}
    arenas = Arenas(3, DEV, (("other", 1000), ("x", 40 * len(cols) * T * 4), ("tail", 256)))
    rs = np.random.RandomState(11)
    done = {k: 0 for k in SESSIONS}
    left = lambda k, g: devs[k][g].shape[0] - pool.raw[k][g]                                  # noqa: E731
    room = lambda k, g: mx.streams[g].max_rows(done[k] * S + Rn) - pool.raw[k][g]            # noqa: E731
    prime = [_next_prime(max(g.tail_rows, 21)) for g in mx.streams]

    early = lambda k: pool.written(k) < 3 * Rn // 2                                           # noqa: E731

    def way(k, g):
        """The chunk length session k's way asks for on stream g now."""
        c = pool.counts(k)[g]
        if k == 0:
            return 7 if g == BVP or (g == CHEST and c >= Rn) else 1
        if k == 1:
            return prime[g] if c < 3 * Rn // 2 else 2 * max(mx.streams[g].tail_rows, 21) + 5
        if early(k):
            return 1 << 40 if g == SLOW else int(mx.streams[g].fs)    # the 4 Hz stream runs ahead: the others take a second a call
        return 1 if g == SLOW else 1 << 40                            # and behind: the others take what the ring allows

    def wants(k, g, target):
        """Whether stream g of session k delivers in this call."""
        if not left(k, g):
            return False
        if k != 3:
            return pool.counts(k)[g] < target
        others = [h for h in range(G) if h != SLOW and left(k, h)]
        if g != SLOW or early(k):
            return True                                               # ahead: the 4 Hz stream takes what the ring allows, always
        return not others or all(room(k, h) < 1 for h in others)       # behind: only when nothing else can move

    checked = mixed = calls = 0
    longest = {k: [0] * G for k in SESSIONS}
    ahead = behind = 0
    tick = 0
    while any(left(k, g) for k in SESSIONS for g in range(G)):
        tick += 1
        assert tick < 400
        target = {k: 16 * (tick - 3 * j) for j, k in enumerate(SESSIONS)}          # session j starts 3 j ticks late; 16 outputs a tick
        others_run = any(left(k, g) for k in SESSIONS[:2] for g in range(G))
        active3 = True
        while True:
            chunks = []
            for k in SESSIONS:
                if k == 3 and not active3:
                    continue
                for g in range(G):
                    if wants(k, g, target[k]):
                        n = min(way(k, g), room(k, g), left(k, g))
                        if n >= 1:
                            chunks.append((k, g, devs[k][g][pool.raw[k][g]:pool.raw[k][g] + n]))
                            longest[k][g] = max(longest[k][g], n)
            if not chunks:
                break
            late = [c for c in chunks if c[0] != 3 and rs.rand() < 0.2]          # a fifth of the chunks arrive a call later
            chunks = [c for c in chunks if not any(c is d for d in late)] or chunks
            pool.push([chunks[i] for i in rs.permutation(len(chunks))])
            calls += 1
            c3 = pool.counts(3)
            ahead = max(ahead, c3[SLOW] - max(c3[:SLOW]))
            behind = max(behind, min(c3[:SLOW]) - c3[SLOW])
            rows = []
            for k in SESSIONS:
                assert max(pool.counts(k)) <= done[k] * S + Rn
                now = R.count(pool.written(k), T, S)
                rows += [(k, w) for w in range(done[k], now)]
                done[k] = now
            if rows:
                assert len(rows) <= 40
                _check_batch(pool, cols, mask, T, S, stats, rows, arenas, want, f"call {calls}")
                checked += len(rows)
                mixed += len({k for k, _w in rows}) > 1
            if others_run:
                active3 = False                                       # one call of session 3 a tick while the others run; then on its own
    assert checked == sum(want[k].shape[0] for k in SESSIONS) and mixed > 0
    assert longest[0][CHEST] == 7 and longest[0][SLOW] == 1 and longest[0][ACC] == 1
    assert all(longest[1][g] > max(mx.streams[g].tail_rows, 21) for g in range(G)) and longest[3][CHEST] > 10 * mx.streams[CHEST].tail_rows
    assert ahead >= Rn - T - S - 32 and behind >= Rn - T - 32, (ahead, behind)          # as far as the ring allows, both ways
    torch.cuda.synchronize()
    for k in SESSIONS:
        ring, counts = pool.ring(k), pool.counts(k)
        assert pool.written(k) == off[k][1].shape[0] > 3 * Rn and len(set(counts)) > 1
        for gi, g in enumerate(mx.streams):
            y, raw = off[k][0][g.name], _raw(T, S, k)[0][g.name]
            assert pool.raw[k][gi] == raw.shape[0] and counts[gi] == y.shape[0]
            i = np.arange(y.shape[0] - Rn, y.shape[0])
            assert np.array_equal(_u64(ring[i % Rn][:, g.col0:g.col0 + g.ncols]), _u64(y[i])), (k, g.name)
            if g.tail_rows:
                j = np.arange(raw.shape[0] - g.tail_rows, raw.shape[0])
                assert np.array_equal(_u64(pool.tail(k, gi)[j % g.tail_rows]), _u64(raw[j])), (k, g.name)
    assert np.all(pool.mem[2].cpu().numpy() == 0x5A) and np.all(pool.tails[2].cpu().numpy() == 0x5A)


# ---- 3. the identity stream copies ----------------------------------------------------------------------------------------------------
def test_identity_stream_keeps_every_bit():
    """-0.0, +0.0, denormals, infinities and NaNs with payloads through the 64 Hz stream: the ring and apply's output hold the raw
    bits (a product with a unit tap and a sum from +0.0 would turn -0.0 into +0.0 and may quieten a signalling NaN)."""
    mx = _mx()
    bits = np.array([0x8000000000000000, 0x0000000000000000, 0x0000000000000001, 0x800fffffffffffff, 0x7ff8000000000123, 0xfff800000000beef,
                     0x7ff0000000000001, 0x7ff0000000000000, 0xfff0000000000000, 0x3ff0000000000000, 0x7ff4000000000000, 0x0010000000000000],
                    dtype=np.uint64)
    x = np.tile(bits, 5)[:57].copy()
    dev = torch.from_numpy(x.view(np.float64).reshape(-1, 1).copy()).to(DEV)
    pool = MX.MxPool(mx, 40, POOL_SLOTS, SESSIONS, DEV)
    for lo, hi in [(0, 1), (1, 8), (8, 31), (31, 57)]:                # 57 rows into a ring of 40: it wraps
        pool.push([(1, BVP, dev[lo:hi])])
    torch.cuda.synchronize()
    g = mx.streams[BVP]
    ring = pool.ring(1)
    i = np.arange(17, 57)
    assert np.array_equal(_u64(ring[i % 40][:, g.col0]), x[i])
    other = np.delete(pool.mem[1].cpu().numpy().reshape(40, 8, 8), g.col0, axis=1)
    assert np.all(other == 0x5A) and np.all(pool.tails.cpu().numpy() == 0x5A)          # no other column, and the identity keeps no tail
    streams = {n: torch.zeros((mx.stream[n].max_rows(57) + 1, mx.stream[n].ncols), dtype=torch.float64, device=DEV) for n in ("chest", "acc", "slow")}
    y = mx.apply(dict(streams, bvp=dev)).cpu().numpy()
    assert y.shape == (57, 8) and np.array_equal(_u64(y[:, g.col0]), x)
    y = mx.apply(dict(streams, bvp=dev[:, 0].cpu().numpy())).cpu().numpy()              # 1-D, numpy
    assert np.array_equal(_u64(y[:, g.col0]), x)


# ---- 4. one missing raw sample --------------------------------------------------------------------------------------------------------
def test_one_missing_row_of_the_4hz_stream_reaches_exactly_its_outputs():
    """One NaN in column 0 of raw row j of the 4 Hz stream: the outputs whose support holds row j — the set comes from the definition —
    are not finite in that column, and every other value of every stream keeps the clean run's bits; offline (apply) and live in
    chunks of three rows of that stream."""
    mx = _mx()
    slow = mx.streams[SLOW]
    n_out = 16 * 60
    clean = MX.raw_streams(mx, n_out, 77)
    j = 31
    hurt = {n: x.copy() for n, x in clean.items()}
    hurt["slow"][j, 0] = np.nan
    want = mx.apply(clean).cpu().numpy()
    total = want.shape[0]
    hit = RS.holds(j, 16, 1, 160, total)
    assert n_out <= total and len(hit) == 2 * 160 + 1 and 0 < hit[0] and hit[-1] < total - 1 and np.all(np.isfinite(want))
    col = slow.col0

    def check(got, what):
        bad = ~np.isfinite(got)
        assert sorted(np.flatnonzero(bad[:, col])) == hit, what
        bad[:, col] = False
        assert not bad.any(), what
        keep = np.ones(got.shape, dtype=bool)
        keep[hit, col] = False
        assert np.array_equal(_u64(got)[keep], _u64(want)[keep]), what

    check(mx.apply(hurt).cpu().numpy(), "offline")
    pool = MX.MxPool(mx, total + 40, POOL_SLOTS, SESSIONS, DEV)      # a ring that holds every output: no wrap
    dev = [torch.from_numpy(hurt[g.name]).to(DEV) for g in mx.streams]
    step = [3 * int(g.fs) // 4 for g in mx.streams]                   # three rows of the 4 Hz stream and the same time of the others
    at = [0] * 4
    while any(at[g] < dev[g].shape[0] for g in range(4)):
        pool.push([(3, g, dev[g][at[g]:at[g] + step[g]]) for g in (2, 0, 3, 1) if at[g] < dev[g].shape[0]])
        at = [a + s for a, s in zip(at, step)]
    torch.cuda.synchronize()
    assert pool.written(3) == total
    check(pool.ring(3)[:total], "live")


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------------
def _monitors(T, S, M, reference, gaps, models=None, **kw):
    """A LiveMonitor and the offline Monitor over the same random members, settings and mixed resampler."""
    from multimodalsignal_amd.live import LiveMonitor
    from multimodalsignal_amd.monitor import Monitor
    models = models if models is not None else R.models("cnn_gru_attention", 6, 2, M, DEV)
    common = dict(window_s=T / FS, stride_s=S / FS, reference=reference, eval_batch=16, channels=CHANNELS6, halflife=2,
                  on=kw.pop("on", 0.55), off=kw.pop("off", 0.45), min_on=2, gaps=gaps, resampler=_mx())
    kw.setdefault("ring_s", _ring(T, S) / FS)
    kw.setdefault("max_sessions", POOL_SLOTS)
    return LiveMonitor(models, FS, **common, **kw), Monitor(models, FS, **common), models


def _same(a, b, what=""):
    for k in TL_FIELDS + (("coverage", "valid", "lost") if a.coverage is not None or b.coverage is not None else ()):
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)
    assert a.events == b.events, what


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("reference,gapped", [(f"head:{K_HEAD}", False), ("expanding", False), ("trailing:5", False), ("decayed:4", True)],
                         ids=["head7", "expanding", "trailing5", "decayed4-gaps"])
def test_live_timelines_updates_and_alarms_are_the_offline_ones(reference, gapped, M):
    """Three sessions pushed interleaved and ragged — a random subset of a session's streams per call, each a random stretch of up to
    what room() allows —, sessions 0 and 3 as device tensors, session 1 as numpy arrays.  Under `gaps`: scattered missing raw samples in
    every stream and, per session, nine seconds delivered as skip on the 4 Hz stream alone — the wrist strap drops out, the chest belt
    keeps sending: windows become invalid, and against the same run without the stretch coverage drops in that stream's channel only."""
    from multimodalsignal_amd.live import alarms_of_events, alarms_of_gaps
    from multimodalsignal_amd.reference import Gaps
    T, S = 256, 64
    mx = _mx()
    G = len(mx.streams)
    gaps = Gaps(0.75, 2) if gapped else None
    recs, spans, before = {}, {}, {}
    for k in SESSIONS:
        host = {n: x.copy() for n, x in _raw(T, S, k)[0].items()}
        if gapped:
            rs = np.random.RandomState(40 + k)
            for g in mx.streams:
                x = host[g.name]
                few = 2 if g.name == "slow" else 8                   # a missing 4 Hz sample costs its column five seconds of outputs
                x[rs.randint(0, x.shape[0], few), rs.randint(0, g.ncols, few)] = np.nan
            before[k] = {n: x.copy() for n, x in host.items()}
            a = int(host["slow"].shape[0] * (0.3 + 0.1 * k))
            spans[k] = (a, a + 4 * 9 + k)                             # nine seconds: more than two windows of four seconds lie inside
            host["slow"][spans[k][0]:spans[k][1]] = np.nan
        recs[k] = (host, {n: torch.from_numpy(x).to(DEV) for n, x in host.items()})
    _live, mon, models = _monitors(T, S, M, reference, gaps)
    sm = mon.run(recs[0][1]).smoothed
    sm = sm[np.isfinite(sm)]
    off, on = float(np.percentile(sm, 40)), float(np.percentile(sm, 60))
    if not off < on:
        off, on = 0.45, 0.55
    live, mon, _m = _monitors(T, S, M, reference, gaps, models, on=on, off=off)
    offline = {k: mon.run(recs[k][1 if k != 3 else 0], mx.names if k == 0 else None) for k in SESSIONS}      # session 3's recording: numpy arrays
    for k in SESSIONS:
        live.open(k, mx.names if k == 1 else None)
    rs = np.random.RandomState(5)
    at, ups = {k: [0] * G for k in SESSIONS}, {k: [] for k in SESSIONS}
    total = lambda k, g: recs[k][0][mx.streams[g].name].shape[0]                              # noqa: E731
    calls = 0
    while any(at[k][g] < total(k, g) for k in SESSIONS for g in range(G)):
        calls += 1
        assert calls < 3000
        chunks, gone = {}, {}
        for k in SESSIONS:
            room = live.room(k)
            for gi in rs.permutation(G):
                g = mx.streams[gi]
                if at[k][gi] >= total(k, gi) or rs.rand() < 0.4:
                    continue
                sec = float(rs.choice([0.0, 0.25, 1.0, 2.5, 3.0 + 0.01, 11.0]))
                lo = at[k][gi]
                hi = min(lo + min(int(sec * g.fs) + int(rs.randint(0, 2)), room[g.name]), total(k, gi))
                if gapped and gi == SLOW and lo < spans[k][1] and hi > spans[k][0]:          # up to the stretch; then the stretch itself, skipped
                    hi = spans[k][0] if lo < spans[k][0] else min(hi, spans[k][1])
                    if lo >= spans[k][0]:
                        gone.setdefault(k, {})[g.name] = hi - lo
                if not (k in gone and g.name in gone[k]):
                    x = recs[k][1 if k != 1 else 0][g.name][lo:hi]                            # session 1 pushes numpy arrays
                    chunks.setdefault(k, {})[g.name] = x[:, 0] if g.ncols == 1 and rs.rand() < 0.5 else x      # a one-column stream may be 1-D
                at[k][gi] = hi
        for k, u in live.push(chunks).items():
            ups[k] += u
        if gone:
            for k, u in live.skip(gone).items():
                ups[k] += u
    for k in SESSIONS:
        tl, want = live.timeline(k), offline[k]
        _same(tl, want, k)
        assert tl.meta == want.meta
        raw = {g.name: total(k, gi) for gi, g in enumerate(mx.streams)}
        assert tl.meta["resampler"] == mx.spelling and tl.meta["resampler_latency_s"] == 2.75 == mx.latency_s
        assert tl.meta["raw_samples"] == raw and tl.meta["samples"] == mx.out_count(raw) == _offline(T, S, "8of8", k)[1].shape[0]
        json.dumps(tl.meta)
        N = len(want.t_end)
        assert N == R.count(mx.out_count(raw), T, S) > 20
        assert [u.window for u in ups[k]] == list(range(N)) and all(u.sid == k for u in ups[k])
        for u in ups[k]:
            n = u.window
            row = (want.t_end[n], want.score[n], want.std_p[n, 1], want.entropy[n], want.mutual_info[n], want.pred[n], want.smoothed[n], want.warmup[n])
            got = (u.t_end, u.score, u.std, u.entropy, u.mutual_info, u.pred, u.smoothed, u.warmup)
            assert all(a == b or (a != a and b != b) for a, b in zip(got, (v.item() for v in row))), (k, n)
        if gapped:
            implied = alarms_of_gaps(want.state, want.valid, gaps.lost_after, mon.min_on)
            assert (~want.valid).sum() >= 2 and [u.valid for u in ups[k]] == list(want.valid)
            clean = mon.run(before[k])                                # the same streams without the stretch
            c = CHANNELS6.index("wrist_EDA")
            rest = [i for i in range(6) if i != c]
            assert np.array_equal(want.coverage[:, rest], clean.coverage[:, rest])
            assert np.all(want.coverage[:, c] <= clean.coverage[:, c]) and (want.coverage[:, c] == 0).sum() >= 2
            assert (want.coverage[:, c] < clean.coverage[:, c]).any() and (~want.valid).sum() >= (~clean.valid).sum()
        else:
            implied = alarms_of_events(want.state, mon.min_on)
        assert [(a.kind, a.window, a.start_window) for a in live.alarms(k)] == implied
        raised = [a for u in ups[k] for a in (u.alarms if gapped else ([u.alarm] if u.alarm is not None else []))]
        assert raised == live.alarms(k)


def test_monitor_run_is_apply_then_run_and_apply_is_the_assembly():
    from multimodalsignal_amd.monitor import Monitor
    T, S = 256, 64
    mx = _mx()
    host, dev = _raw(T, S, 1)
    want = _offline(T, S, "8of8", 1)[1]
    assert np.array_equal(_u64(mx.apply(dev).cpu().numpy()), _u64(want)) and np.array_equal(_u64(mx.apply(host).cpu().numpy()), _u64(want))
    short = dict(dev, slow=dev["slow"][:40])                          # the slowest stream cuts the recording
    got = mx.apply(short).cpu().numpy()
    assert got.shape[0] == mx.stream["slow"].out_count(40) == mx.out_count({n: x.shape[0] for n, x in short.items()}) < want.shape[0]
    assert np.array_equal(_u64(got), _u64(want[:got.shape[0]]))
    assert mx.apply(dict(dev, slow=dev["slow"][:10])).shape == (0, 8)
    models = R.models("cnn_gru_attention", 6, 2, 1, DEV)
    kw = dict(window_s=T / FS, stride_s=S / FS, reference="recording", eval_batch=16, channels=CHANNELS6)
    with_mx, plain = Monitor(models, FS, resampler=mx, **kw), Monitor(models, FS, **kw)
    a, b = with_mx.run(dev), plain.run(torch.from_numpy(want).to(DEV), mx.names)
    _same(a, b)
    assert "resampler" not in b.meta and {k: v for k, v in a.meta.items() if not k.startswith("r")} == {k: v for k, v in b.meta.items() if not k.startswith("r")}
    with pytest.raises(ValueError):
        with_mx.run(dev, NAMES8)                                      # the columns are the resampler's
    with pytest.raises(ValueError):
        with_mx.run(dev["chest"], mx.names)
    with pytest.raises(ValueError):
        mx.apply({n: x for n, x in dev.items() if n != "acc"})


# ---- 6. a push that would get stuck ---------------------------------------------------------------------------------------------------
def test_a_push_that_would_get_stuck_is_refused_and_changes_nothing():
    T, S = 256, 64
    mx = _mx()
    host, dev = _raw(T, S, 0)
    live, mon, _m = _monitors(T, S, 1, f"head:{K_HEAD}", None)
    live.open("a")
    live.open("b")
    n0 = {g.name: int(5 * g.fs) for g in mx.streams}
    live.push({"a": {n: dev[n][:k] for n, k in n0.items()}, "b": {"chest": dev["chest"][:900]}})
    room = live.room("a")
    assert all(v > 0 for v in room.values())
    # the statistics are pending: the chest stream may fill the ring, R rows, and not a row more
    assert room["chest"] == mx.stream["chest"].max_rows(live.R) - n0["chest"] and room["bvp"] == live.R - n0["bvp"]
    slot = live.sessions["a"].slot

    def state():
        torch.cuda.synchronize()
        tl = live.timeline("a")
        return (list(live.sessions["a"].mx.raw), live.sessions["a"].book.written, len(tl.t_end), tl.meta["raw_samples"],
                live.pool[slot].cpu().numpy().tobytes(), live.tails[slot].cpu().numpy().tobytes(), list(live.sessions["b"].mx.raw))

    was = state()
    refused = {"chest": dev["chest"][n0["chest"]:n0["chest"] + room["chest"] + 1], "acc": dev["acc"][n0["acc"]:n0["acc"] + 7]}
    for attempt in ({"b": {"chest": dev["chest"][900:1000]}, "a": refused}, ):
        with pytest.raises(ValueError) as e:
            live.push(attempt)
        assert "'a'" in str(e.value) and "'chest'" in str(e.value) and "ring_s" in str(e.value) and " s ahead" in str(e.value)
        assert state() == was                                         # session b's chunk of the same call was not appended either
    with pytest.raises(ValueError):
        live.push("a", refused)
    assert state() == was and live.room("a") == room
    # the lagging streams catch up to 13.5 s — the 4 Hz stream then covers the head span — and the refused push goes through: the
    # statistics are taken and windows handed out in the middle of it, which frees the rows the chest stream's last row needs
    pos = dict(n0)
    live.push("a", {"acc": dev["acc"][pos["acc"]:pos["acc"] + 7]})
    pos["acc"] += 7
    assert live.push("a", {n: dev[n][pos[n]:int(13.5 * mx.stream[n].fs)] for n in ("acc", "bvp", "slow")}) == []
    pos.update({n: int(13.5 * mx.stream[n].fs) for n in ("acc", "bvp", "slow")})
    assert live.room("a")["chest"] > room["chest"] + 1
    ups = live.push("a", {"chest": refused["chest"]})
    pos["chest"] += room["chest"] + 1
    assert [u.window for u in ups] == list(range(len(ups))) and len(ups) >= K_HEAD
    while any(pos[n] < dev[n].shape[0] for n in pos):                # the rest, a second of every stream a call
        step = {n: int(mx.stream[n].fs) for n in pos}
        live.push("a", {n: dev[n][pos[n]:pos[n] + step[n]] for n in pos})
        pos = {n: pos[n] + step[n] for n in pos}
    _same(live.timeline("a"), mon.run(dev), "after the refusal")
    assert live.timeline("a").meta["raw_samples"] == {n: x.shape[0] for n, x in host.items()}
    # an explicit ring without room for the spread is refused at construction; the default ring has it
    from multimodalsignal_amd.live import LiveMonitor
    head = (K_HEAD - 1) * S + T
    with pytest.raises(ValueError):
        _monitors(T, S, 1, f"head:{K_HEAD}", None, ring_s=(head + 176 + 15) / FS)
    assert _monitors(T, S, 1, f"head:{K_HEAD}", None, ring_s=(head + 176 + 16) / FS)[0].R == head + 192
    models = R.models("cnn_gru_attention", 6, 2, 1, DEV)
    assert LiveMonitor(models, FS, window_s=4, stride_s=1, reference=f"head:{K_HEAD}", channels=CHANNELS6, resampler=mx).R == head + 8 * S + 176
    with pytest.raises(ValueError):
        LiveMonitor(models, FS, window_s=4, stride_s=1, reference="expanding", channels=CHANNELS6, resampler=mx).skip("x", {"slow": 4})      # needs gaps
    with pytest.raises(ValueError):
        live.push("a", {"wrist": dev["slow"][:4]})                   # no such stream
    with pytest.raises(ValueError):
        live.push("a", {"slow": dev["slow"][:4, :1]})                # a two-column stream
    with pytest.raises(ValueError):
        live.open("c", NAMES8)                                       # the columns are the resampler's
    with pytest.raises(ValueError):
        live.push("a", dev["chest"][:4])


# ---- 7. refusals of the C ABI ---------------------------------------------------------------------------------------------------------
def _set(mx, i, **fields):
    """The resampler's group table with fields of group i replaced."""
    table = mx.groups()
    for f, v in fields.items():
        setattr(table[i], f, v)
    return table


def test_live_call_refuses_before_any_launch():
    """Every check of msig_mx_lv_push; after each refused call the pool and the tails are what they were.  The rings and the tail
    blocks lie 8 bytes further apart than they are long: the padding is never written.  The longest admissible chunk is taken."""
    mx = _mx()
    Rn = 100
    p = MX.MxPool(mx, Rn, POOL_SLOTS, SESSIONS, DEV, pad=8)
    pool, tails = p.mem, p.tails
    staging = torch.zeros(40000, dtype=torch.float64, device=DEV)
    i32, i64 = lambda *v: (C.c_int32 * len(v))(*v), lambda *v: (C.c_int64 * len(v))(*v)      # noqa: E731
    chest, slow = mx.streams[CHEST], mx.streams[SLOW]
    base = dict(pool=pool.data_ptr(), sessions=POOL_SLOTS, R=Rn, ring_bytes=Rn * 64 + 8, C_all=8, tails=tails.data_ptr(), tail_bytes=mx.tail_doubles * 8 + 8,
                h=mx.h.data_ptr(), groups=mx.groups(), G=4, sess=i32(0, 3, 3), group=i32(SLOW, CHEST, BVP), raw=i64(0, 500, 20), len=i64(12, 700, 9), n=3,
                staging=staging.data_ptr())
    most = chest.max_rows(chest.out_count(500) + Rn) - 500            # the longest chunk after 500 rows that yields R outputs
    last = mx.tail_doubles                                            # the tail ranges end here
    G8 = (L.MxGroup * 9)(*([mx.streams[BVP].group()] * 9))
    cases = [("pool", None, E_NULL), ("tails", None, E_NULL), ("h", None, E_NULL), ("groups", None, E_NULL), ("sess", None, E_NULL), ("group", None, E_NULL),
             ("raw", None, E_NULL), ("len", None, E_NULL),
             ("sessions", 0, E_SHAPE), ("sessions", L.LV_MAX_SESSIONS + 1, E_SHAPE), ("R", 0, E_SHAPE), ("R", 1 << 31, E_SHAPE), ("C_all", 0, E_SHAPE),
             ("ring_bytes", Rn * 64 - 8, E_SHAPE), ("G", 0, E_SHAPE), ("G", 9, E_SHAPE), ("groups", G8, E_SHAPE),
             ("C_all", 7, E_SHAPE)]                                                              # the last group's column lies outside the row
    cases += [("groups", _tab, E_SHAPE) for _tab in (
        _set(mx, CHEST, col0=-1), _set(mx, SLOW, col0=7), _set(mx, ACC, ncols=0), _set(mx, ACC, col0=3),      # outside the row; two ranges overlap
        _set(mx, BVP, col0=4), _set(mx, BVP, half=1), _set(mx, BVP, tail_rows=1),                           # an identity with a half or a tail
        _set(mx, CHEST, L=0), _set(mx, CHEST, L=4097), _set(mx, CHEST, M=0), _set(mx, CHEST, M=4097), _set(mx, CHEST, L=175), _set(mx, CHEST, L=35),
        _set(mx, CHEST, half=174), _set(mx, CHEST, half=L.RS_MAX_HALF + 1), _set(mx, ACC, L=2, M=2), _set(mx, CHEST, h_off=-1),
        _set(mx, CHEST, tail_rows=chest.tail_rows - 1), _set(mx, SLOW, tail_rows=20), _set(mx, CHEST, tail_rows=1 << 31),
        _set(mx, SLOW, tail_off=-1), _set(mx, SLOW, tail_off=slow.tail_off + 2), _set(mx, SLOW, tail_rows=22),      # beyond the block
        _set(mx, SLOW, tail_off=slow.tail_off - 1), _set(mx, ACC, tail_off=0))]                              # two tail ranges overlap
    cases += [("tail_bytes", last * 8 - 8, E_SHAPE), ("tail_bytes", -8, E_SHAPE),
              ("n", 0, E_SHAPE), ("n", POOL_SLOTS * 4 + 1, E_SHAPE), ("sess", i32(0, 4, 3), E_SHAPE), ("sess", i32(-1, 3, 3), E_SHAPE),
              ("group", i32(SLOW, CHEST, 4), E_SHAPE), ("group", i32(SLOW, -1, BVP), E_SHAPE), ("group", i32(SLOW, CHEST, CHEST), E_SHAPE),      # a pair twice
              ("raw", i64(0, -1, 20), E_SHAPE), ("len", i64(12, -1, 9), E_SHAPE), ("len", i64(12, 1 << 31, 9), E_SHAPE), ("raw", i64(0, 1 << 48, 20), E_SHAPE),
              ("len", i64(12, most + 1, 9), E_SHAPE), ("len", i64(12, 700, Rn + 1), E_SHAPE), ("len", i64(17, 700, 9), E_SHAPE),
              ("pool", pool.data_ptr() + 4, E_ALIGN), ("tails", tails.data_ptr() + 4, E_ALIGN), ("h", mx.h.data_ptr() + 4, E_ALIGN),
              ("staging", staging.data_ptr() + 4, E_ALIGN), ("ring_bytes", Rn * 64 + 12, E_ALIGN), ("tail_bytes", last * 8 + 12, E_ALIGN)]
    order = ("pool", "sessions", "R", "ring_bytes", "C_all", "tails", "tail_bytes", "h", "groups", "G", "sess", "group", "raw", "len", "n", "staging")
    for name, value, code in cases:
        a = dict(base, **{name: value})
        rc = L.lib().msig_mx_lv_push(*[a[k] for k in order], _stream())
        assert rc == code, (name, value, rc)
    torch.cuda.synchronize()
    assert bool((pool == 0x5A).all()) and bool((tails == 0x5A).all())
    assert slow.out_count(16) == 96 <= Rn < slow.out_count(17)         # (the 4 Hz chunk one row shorter than the refused one)
    ok = dict(base, len=i64(16, most, Rn))                            # the longest chunks are taken, and write
    assert L.lib().msig_mx_lv_push(*[ok[k] for k in order], _stream()) == 0
    only = dict(base, groups=(L.MxGroup * 1)(mx.streams[BVP].group()), G=1, h=None, sess=i32(1), group=i32(0), raw=i64(5), len=i64(3), n=1)
    assert L.lib().msig_mx_lv_push(*[only[k] for k in order], _stream()) == 0          # identity groups alone need no taps
    torch.cuda.synchronize()
    ring = lambda k: pool[k, :Rn * 64].view(torch.float64).view(Rn, 8)                # noqa: E731
    untouched = lambda t: bool((t.contiguous().view(torch.uint8) == 0x5A).all())      # noqa: E731
    sc, bc, ac = slow.col0, mx.streams[BVP].col0, mx.streams[ACC].col0
    assert (sc, bc, ac) == (6, 5, 4)
    assert bool((ring(0)[:96, sc:sc + 2] == 0).all()) and untouched(ring(0)[96:]) and untouched(ring(0)[:, :sc])          # 96 outputs of zeros
    # the chest chunk: outputs 36 .. 135, every ring row once.  Outputs 56 and later have their whole support inside the chunk of zeros
    # (56 * 175 - 1750 = 16 * 500); the first twenty reach into a tail nobody wrote — 0x5A bytes as numbers — and are not zero
    zero = [m % Rn for m in range(56, 136)]
    assert bool((ring(3)[zero, :4] == 0).all()) and not bool((ring(3)[36:56, :4].contiguous().view(torch.uint8) == 0x5A).all(dim=-1).any())
    assert bool((ring(3)[:, bc] == 0).all()) and untouched(ring(3)[:, ac]) and untouched(ring(3)[:, sc:])
    assert bool((ring(1)[5:8, bc] == 0).all()) and untouched(ring(1)[8:]) and untouched(ring(1)[:5]) and untouched(ring(1)[5:8, :bc])
    assert untouched(pool[2]) and untouched(pool[:, Rn * 64:])
    tail = lambda k, g: tails[k, g.tail_off * 8:(g.tail_off + g.tail_rows * g.ncols) * 8]      # noqa: E731
    assert bool((tail(3, chest) == 0).all()) and bool((tail(0, slow)[:16 * 2 * 8] == 0).all()) and untouched(tail(0, slow)[16 * 2 * 8:])
    assert untouched(tail(0, chest)) and untouched(tail(3, slow)) and untouched(tails[1:3]) and untouched(tails[:, last * 8:])


def test_offline_call_refuses():
    mx = _mx()
    chest = mx.streams[CHEST]
    x = torch.zeros((5000, 4), dtype=torch.float64, device=DEV)
    y = torch.full((449, 8), -7.25, dtype=torch.float64, device=DEV)
    grp = lambda **f: C.pointer(_set(mx, CHEST, **f)[CHEST])          # noqa: E731
    base = dict(x=x.data_ptr(), n_in=5000, h=mx.h.data_ptr(), g=grp(), y=y.data_ptr(), n_out=448, C_all=8)
    order = ("x", "n_in", "h", "g", "y", "n_out", "C_all")
    assert chest.out_count(5000) == 448
    cases = [("x", None, E_NULL), ("y", None, E_NULL), ("h", None, E_NULL), ("g", None, E_NULL), ("n_in", -1, E_SHAPE), ("n_in", (1 << 48) + 1, E_SHAPE),
             ("C_all", 0, E_SHAPE), ("C_all", 3, E_SHAPE), ("n_out", 449, E_SHAPE), ("n_out", -1, E_SHAPE), ("g", grp(L=0), E_SHAPE),
             ("g", grp(M=4097), E_SHAPE), ("g", grp(L=175), E_SHAPE), ("g", grp(L=35), E_SHAPE), ("g", grp(half=174), E_SHAPE), ("g", grp(h_off=-1), E_SHAPE),
             ("g", grp(col0=5), E_SHAPE), ("g", grp(col0=-1), E_SHAPE), ("g", grp(ncols=0), E_SHAPE), ("g", grp(L=1, M=1), E_SHAPE),
             ("x", x.data_ptr() + 4, E_ALIGN), ("y", y.data_ptr() + 4, E_ALIGN), ("h", mx.h.data_ptr() + 4, E_ALIGN)]
    for name, value, code in cases:
        a = dict(base, **{name: value})
        assert L.lib().msig_mx_resample(*[a[k] for k in order], _stream()) == code, (name, value)
    torch.cuda.synchronize()
    assert bool((y == -7.25).all())
    assert L.lib().msig_mx_resample(None, 0, mx.h.data_ptr(), grp(), None, 0, 8, _stream()) == 0      # nothing in, nothing out
    same = C.pointer(mx.groups()[BVP])
    assert L.lib().msig_mx_resample(x.data_ptr(), 449, None, same, y.data_ptr(), 449, 8, _stream()) == 0      # the identity needs no taps
    torch.cuda.synchronize()
    assert bool((y[:, mx.streams[BVP].col0] == 0).all()) and bool((y[:, :5] == -7.25).all()) and bool((y[:, 6:] == -7.25).all())


# ---- 8. a reused slot -----------------------------------------------------------------------------------------------------------------
def test_a_reused_slot_has_no_memory_of_the_closed_sessions_tails():
    T, S = 200, 37
    mx = _mx()
    recs = {k: _raw(T, S, k)[1] for k in SESSIONS}
    cut = lambda d, a, b: {g.name: d[g.name][int(a * g.fs):int(b * g.fs)] for g in mx.streams}      # noqa: E731  seconds a .. b of every stream

    def monitor():
        from multimodalsignal_amd.live import LiveMonitor
        models = R.models("cnn_gru_attention", 3, 2, 1, DEV)
        return LiveMonitor(models, FS, window_s=T / FS, stride_s=S / FS, reference=f"head:{K_HEAD}", eval_batch=16,
                           channels=[NAMES8[c] for c in R.COLS["3of8"]], halflife=2, on=0.55, off=0.45, min_on=2, resampler=mx,
                           ring_s=_ring(T, S) / FS, max_sessions=2)

    secs = int(max(recs[3][g.name].shape[0] / g.fs for g in mx.streams)) + 1
    alone = monitor()
    alone.open("solo")
    for t in range(secs):
        alone.push("solo", cut(recs[3], t, t + 1))
    live = monitor()
    live.open("first")
    live.open("left")
    slot = live.sessions["left"].slot
    live.push({"first": cut(recs[0], 0, 9), "left": cut(recs[1], 0, 9.3)})       # left ends mid-support: its tails hold rows a successor must not see
    assert len(live.timeline("left").t_end) > 0 and live.sessions["left"].mx.raw == [int(9.3 * g.fs) for g in mx.streams]
    assert bool(live.tails[slot].any())
    live.close("left")
    with pytest.raises(ValueError):
        live.push("left", cut(recs[1], 10, 11))
    live.open("new")
    assert live.sessions["new"].slot == slot and live.sessions["new"].mx.raw == [0] * 4 and len(live.timeline("new").t_end) == 0
    assert not bool(live.tails[slot].any())
    for t in range(secs):
        live.push({"new": cut(recs[3], t, t + 1), "first": cut(recs[0], 9 + t / 2, 9.5 + t / 2)})
    _same(live.timeline("new"), alone.timeline("solo"), "in a reused slot")
    assert live.timeline("new").meta["raw_samples"] == {n: x.shape[0] for n, x in recs[3].items()}
    assert len(live.timeline("new").t_end) > 40


# ---- 9. the command line --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run_dir(tmp_path_factory):
    """A run directory of saved random state_dicts: folds S2 and S10."""
    from multimodalsignal_amd.synth import CHANNELS6 as SYNTH6
    root = tmp_path_factory.mktemp("run")
    for seed, sid in ((40, "S2"), (41, "S10")):
        d = root / f"fold_test_on_{sid}"
        d.mkdir(parents=True)
        torch.save(R.models("cnn_gru_attention", 6, 2, 1, DEV, seed)[0].state_dict(), d / "best_model.pt")
    (root / "cv_summary.txt").write_text(f"实验配置:\nSEED: 42\nCHANNELS_TO_USE: {list(SYNTH6)}\n", encoding="utf-8")
    return root


def test_cli_replays_the_synthetic_streams(run_dir, tmp_path, capsys):
    from multimodalsignal_amd import live, monitor
    spec = "chest=700:chest_ECG,chest_EDA,chest_Resp,chest_EMG;bvp=64:wrist_BVP;eda=4:wrist_EDA"
    args = ["--run", str(run_dir), "--synthetic-recording", "--streams", spec, "--window-s", "8", "--stride-s", "8", "--reference", "expanding",
            "--gaps", "--synthetic-gaps", "drop=0.0002,all=900:70,stream=eda:1500:40"]
    tl = live.main(args + ["--sessions", "2", "--chunk-s", "20", "--out", str(tmp_path / "live")])
    said = capsys.readouterr().out
    want = monitor.main(args + ["--out", str(tmp_path / "offline")])
    mx = MixedResampler([Stream("chest", 700, ["a"]), Stream("bvp", 64, ["b"]), Stream("eda", 4, ["c"])], 64, device="cpu")
    raw = {"chest": 40 * 60 * 700, "bvp": 40 * 60 * 64, "eda": 40 * 60 * 4}
    n = (mx.out_count(raw) - 512) // 512 + 1
    assert mx.out_count(raw) == mx.stream["eda"].out_count(raw["eda"]) and len(tl.t_end) == n == len(want.t_end)
    _same(tl, want, "cli")
    assert (tmp_path / "live" / "timeline.csv").read_text() == (tmp_path / "offline" / "timeline.csv").read_text()
    doc = json.loads((tmp_path / "live" / "timeline.json").read_text())
    assert doc == json.loads((tmp_path / "offline" / "timeline.json").read_text())
    assert doc["resampler_latency_s"] == 2.75 and doc["raw_samples"] == raw and doc["samples"] == mx.out_count(raw) and doc["lost_windows"] > 0
    assert doc["resampler"].startswith("mixed->64") and all(k + "=" in doc["resampler"] for k in raw)
    wrist = tl.coverage[:, 5]                                          # wrist_EDA: off for 40 s more than the others
    assert (wrist == 0).sum() >= (tl.coverage[:, 0] == 0).sum() + 3
    line = [ln for ln in said.splitlines() if "Monitor.run's" in ln]
    assert len(line) == 1 and line[0].endswith(": equal bit for bit") and "NOT" not in line[0]
    assert any(f"'eda': {(70 + 40) * 4}" in ln and f"'chest': {70 * 700}" in ln for ln in said.splitlines())
    np.savez(tmp_path / "rec.npz", chest=np.abs(np.random.RandomState(0).randn(700 * 40, 4)), bvp=np.random.RandomState(1).randn(64 * 40),
             eda=np.abs(np.random.RandomState(2).randn(4 * 40, 1)))
    args = ["--run", str(run_dir), "--recording", str(tmp_path / "rec.npz"), "--streams", spec, "--window-s", "4", "--stride-s", "2", "--reference", "head:3"]
    a, b = live.main(args + ["--out", str(tmp_path / "l2"), "--chunk-s", "1.5"]), monitor.main(args + ["--out", str(tmp_path / "o2")])
    _same(a, b, "npz")
    assert len(a.t_end) == (mx.stream["eda"].out_count(160) - 256) // 128 + 1 and "equal bit for bit" in capsys.readouterr().out
