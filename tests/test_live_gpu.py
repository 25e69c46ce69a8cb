"""Live monitoring on the GPU (include/msig_lv.h, multimodalsignal_amd/live.py): the rings and the mixed
batches bit for bit against msig_rec_windows on each session's linear recording, the statistics of a split push against
msig_rec_stats, and LiveMonitor's timelines, updates and alarms against Monitor.run on the same samples as one recording — under
ragged, out-of-phase chunks, catch-up, every way of chunking, interleaved and reused sessions, and the command line."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import lv_reference as R
from multimodalsignal_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES8, COLS = R.NAMES8, R.COLS
K_HEAD = 7
SHAPES = [(256, 64, "8of8"), (200, 37, "3of8"), (200, 300, "1of8"), (256, 1, "3of8")]
IDS = [f"t{T}-s{S}-{key}" for T, S, key in SHAPES]
POOL_SLOTS, SESSIONS = 4, (0, 1, 3)          # three sessions in a pool of four: ring 2 is never touched
FS = 64.0
TL_FIELDS = ("t_end", "mean_p", "std_p", "pred", "entropy", "mutual_info", "votes", "score", "smoothed", "state", "warmup")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "the gpu tier needs an MI355X"


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _ring(T, S):
    return (K_HEAD - 1) * S + T + 41          # no multiple of S, T or 256: every ring wraps several times, at odd places


@functools.lru_cache(maxsize=None)
def _recording(T, S, k):
    """Session k's recording: a little more than three rings long, another length and other values per session."""
    sig = R.recording(3 * _ring(T, S) + 17 + 29 * k, 1000 * T + 10 * S + k)
    return sig, torch.from_numpy(sig).to(DEV)


def _head(dev, cols, T, S):
    return dev.data_ptr(), dev.shape[0], dev.shape[1], (C.c_int32 * len(cols))(*cols), len(cols), R.mask_of(cols), T, S


@functools.lru_cache(maxsize=None)
def _offline(T, S, key, k):
    """msig_rec_stats over windows [0, K_HEAD) and msig_rec_windows of every window of session k's LINEAR recording — computed once."""
    sig, dev = _recording(T, S, k)
    cols, lib = COLS[key], L.lib()
    N = R.count(sig.shape[0], T, S)
    stats = torch.full((2 * L.MAX_C + 1,), float("nan"), dtype=torch.float64, device=DEV)
    scratch = torch.empty(lib.msig_rec_scratch_bytes(), dtype=torch.uint8, device=DEV)
    L.check(lib.msig_rec_stats(*_head(dev, cols, T, S), 0, K_HEAD, stats.data_ptr(), scratch.data_ptr(), _stream()), "msig_rec_stats")
    out = torch.empty((N, len(cols), T), dtype=torch.float32, device=DEV)
    L.check(lib.msig_rec_windows(*_head(dev, cols, T, S), 0, N, stats.data_ptr(), out.data_ptr(), _stream()), "msig_rec_windows")
    torch.cuda.synchronize()
    return stats, out.cpu().numpy()


class Pool:
    """A caller-owned pool of POOL_SLOTS rings filled with 0x5A, the statistics table, and the host's counts of samples written."""

    def __init__(self, T, S, key, Rn, stats_of):
        self.T, self.S, self.R, self.cols = T, S, Rn, COLS[key]
        self.mem = torch.full((POOL_SLOTS, Rn * 8 * 8), 0x5A, dtype=torch.uint8, device=DEV)
        self.stats = torch.full((POOL_SLOTS, 2 * L.MAX_C + 1), float("nan"), dtype=torch.float64, device=DEV)
        for k in SESSIONS:
            self.stats[k].copy_(stats_of(k))
        self.written = {k: 0 for k in SESSIONS}

    def args(self):
        return self.mem.data_ptr(), POOL_SLOTS, self.R, self.R * 8 * 8, 8

    def push(self, chunks):
        """chunks: {session: (n, 8) device rows} — ONE msig_lv_push, the chunks back to back in one staging buffer."""
        ks = list(chunks)
        staging = torch.cat([chunks[k] for k in ks] + [torch.zeros((1, 8), dtype=torch.float64, device=DEV)]).contiguous()
        n = len(ks)
        L.check(L.lib().msig_lv_push(*self.args(), (C.c_int32 * n)(*ks), (C.c_int64 * n)(*[self.written[k] for k in ks]),
                                     (C.c_int64 * n)(*[int(chunks[k].shape[0]) for k in ks]), n, staging.data_ptr(), _stream()), "msig_lv_push")
        for k in ks:
            self.written[k] += int(chunks[k].shape[0])

    def windows(self, rows, arenas, slots):
        """rows: [(session, window)] — ONE msig_lv_windows_multi into the arena slots `slots`."""
        B = len(rows)
        L.check(L.lib().msig_lv_windows_multi(*self.args(), (C.c_int32 * len(self.cols))(*self.cols), len(self.cols), R.mask_of(self.cols),
                                              self.T, self.S, (C.c_int32 * B)(*[k for k, _n in rows]), (C.c_int64 * B)(*[n for _k, n in rows]),
                                              (C.c_int64 * B)(*[self.written[k] for k, _n in rows]), B, self.stats.data_ptr(), arenas.ptr("x"),
                                              C.byref(arenas.multi(slots)), _stream()), "msig_lv_windows_multi")


def _check_batch(pool, rows, arenas, want, what):
    """Slots 2 and 0 of three hold the rows' offline bits; slot 1, the rest of every arena and the pool's fourth ring keep 0x5A."""
    arenas.mem.fill_(0x5A)
    pool.windows(rows, arenas, [2, 0])
    torch.cuda.synchronize()
    Cn, T = len(pool.cols), pool.T
    n = len(rows) * Cn * T
    ref = np.concatenate([want[k][w].reshape(-1) for k, w in rows]).view(np.uint32)
    for s in (0, 2):
        x = arenas.view(s, "x", torch.float32).cpu().numpy()
        assert np.array_equal(x[:n].view(np.uint32), ref), (what, s, rows)
        assert np.all(x[n:].view(np.uint8) == 0x5A), (what, "wrote past the batch")
        assert np.all(arenas.view(s, "other").cpu().numpy() == 0x5A) and np.all(arenas.view(s, "tail").cpu().numpy() == 0x5A)
    assert np.all(arenas.mem[1].cpu().numpy() == 0x5A)
    assert np.all(pool.mem[2].cpu().numpy() == 0x5A)


# ---- 1. ring and batch bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S,key", SHAPES, ids=IDS)
def test_ragged_out_of_phase_pushes_give_the_offline_bits(T, S, key):
    """Three recordings into sessions 0, 1 and 3 in ragged chunks; after each push the newly complete windows of all sessions as one
    mixed batch: every row is msig_rec_windows' on that session's linear recording."""
    from multimodalsignal_amd.runtime import Arenas
    Rn = _ring(T, S)
    pool = Pool(T, S, key, Rn, lambda k: _offline(T, S, key, k)[0])
    want = {k: _offline(T, S, key, k)[1] for k in SESSIONS}
    devs = {k: _recording(T, S, k)[1] for k in SESSIONS}
    arenas = Arenas(3, DEV, (("other", 1000), ("x", 40 * len(COLS[key]) * T * 4), ("tail", 256)))
    rs = np.random.RandomState(7)
    lengths = [1, 5, S - 1, S, S + 1, 3 * S + 7]
    done = {k: 0 for k in SESSIONS}             # windows checked so far
    rings = {k: R.Ring(Rn, 8) for k in SESSIONS}      # the restatement's rings, filled sample by sample
    tick, checked, mixed = 0, 0, 0
    while any(pool.written[k] < devs[k].shape[0] for k in SESSIONS):
        chunks = {}
        for j, k in enumerate(SESSIONS):
            if tick >= 3 * j and pool.written[k] < devs[k].shape[0]:      # session j starts 3 j pushes late
                n = min(int(lengths[rs.randint(len(lengths))]), devs[k].shape[0] - pool.written[k])
                chunks[k] = devs[k][pool.written[k]:pool.written[k] + n]
        tick += 1
        pool.push(chunks)
        for k, chunk in chunks.items():
            rings[k].push(_recording(T, S, k)[0][rings[k].written:rings[k].written + chunk.shape[0]])
        rows = []
        for k in SESSIONS:
            now = R.count(pool.written[k], T, S)
            rows += [(k, w) for w in range(done[k], now)]
            done[k] = now
        if rows:
            assert len(rows) <= 40
            _check_batch(pool, rows, arenas, want, f"push {tick}")
            checked += len(rows)
            mixed += len({k for k, _w in rows}) > 1
    assert checked == sum(want[k].shape[0] for k in SESSIONS) and mixed > 0
    assert all(pool.written[k] > 3 * Rn for k in SESSIONS)                 # every ring wrapped three times
    # the rings are the restatement's — the last R samples of their recordings, sample i in row i % R — and the last window read back
    # from the restatement's ring and normalised in numpy is the device's row to fp32 rounding of the same fp64 statistics
    torch.cuda.synchronize()
    cols = COLS[key]
    for k in SESSIONS:
        ring, sig = pool.mem[k].view(torch.float64).view(Rn, 8).cpu().numpy(), _recording(T, S, k)[0]
        assert rings[k].written == pool.written[k] == sig.shape[0]
        assert np.array_equal(ring.view(np.uint64), rings[k].rows.view(np.uint64))
        i = np.arange(sig.shape[0] - Rn, sig.shape[0])
        assert np.array_equal(ring[i % Rn].view(np.uint64), sig[i].view(np.uint64))
        st = pool.stats[k].cpu().numpy()
        last = want[k].shape[0] - 1
        ref = R.normalised(rings[k].window(last, T, S), cols, R.mask_of(cols), st[:len(cols)], st[L.MAX_C:L.MAX_C + len(cols)])
        assert np.abs(want[k][last] - ref).max() <= 2e-6 * max(1.0, np.abs(ref).max())


# ---- 2. catch-up ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S,key", SHAPES, ids=IDS)
def test_catch_up_of_nine_consecutive_windows_beside_single_ones(T, S, key):
    """One push completes 9 consecutive windows of session 0 (one run: each sample read once) beside one window each of sessions 1 and
    3: the same bits.  The ring is 10 S + T + 41 rows here — nine consecutive windows must fit — and session 0's has wrapped."""
    from multimodalsignal_amd.runtime import Arenas
    Rn = 10 * S + T + 41
    pool = Pool(T, S, key, Rn, lambda k: _offline(T, S, key, k)[0])
    want = {k: _offline(T, S, key, k)[1] for k in SESSIONS}
    devs = {k: _recording(T, S, k)[1] for k in SESSIONS}
    arenas = Arenas(3, DEV, (("other", 1000), ("x", 16 * len(COLS[key]) * T * 4), ("tail", 256)))
    q = 41 // S + 4                                        # session 0 first gets q + 1 windows; the next nine wrap its ring
    first = {0: q * S + T, 1: 2 * S + T - 1, 3: T - 1}
    assert first[0] + 9 * S <= devs[0].shape[0] and first[0] + 9 * S > Rn
    while any(pool.written[k] < first[k] for k in SESSIONS):          # a chunk is at most R rows
        pool.push({k: devs[k][pool.written[k]:min(first[k], pool.written[k] + Rn)] for k in SESSIONS if pool.written[k] < first[k]})
    before = {k: R.count(pool.written[k], T, S) for k in SESSIONS}
    assert before == {0: q + 1, 1: 2, 3: 0}
    pool.push({0: devs[0][first[0]:first[0] + 9 * S], 1: devs[1][first[1]:first[1] + 1], 3: devs[3][first[3]:first[3] + 1]})
    after = {k: R.count(pool.written[k], T, S) for k in SESSIONS}
    assert after == {0: q + 10, 1: 3, 3: 1}
    run = [(0, w) for w in range(q + 1, q + 10)]
    _check_batch(pool, [(1, 2)] + run + [(3, 0)], arenas, want, "one run between two single rows")
    _check_batch(pool, run[:4] + [(3, 0)] + run[4:] + [(1, 2)], arenas, want, "the run cut in two")
    _check_batch(pool, run[::-1], arenas, want, "no two rows consecutive")


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------
def _monitors(T, S, key, M=1, kind="cnn_gru_attention", reference=f"head:{K_HEAD}", models=None, **kw):
    """A LiveMonitor and the offline Monitor over the same random members and settings."""
    from multimodalsignal_amd.live import LiveMonitor
    from multimodalsignal_amd.monitor import Monitor
    channels = [NAMES8[c] for c in COLS[key]] if isinstance(key, str) else key
    models = models if models is not None else R.models(kind, len(channels), 2, M, DEV)
    common = dict(window_s=T / FS, stride_s=S / FS, reference=reference, eval_batch=16, channels=channels, halflife=kw.pop("halflife", 2),
                  on=kw.pop("on", 0.55), off=kw.pop("off", 0.45), min_on=kw.pop("min_on", 2))
    kw.setdefault("ring_s", _ring(T, S) / FS)
    kw.setdefault("max_sessions", POOL_SLOTS)
    live = LiveMonitor(models, FS, **common, **kw)
    assert (live.T, live.S, live.R) == (T, S, int(round(kw["ring_s"] * FS)))
    return live, Monitor(models, FS, **common)


def _same(a, b, what=""):
    for k in TL_FIELDS:
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)
    assert a.events == b.events, what


def _feed(live, sid, dev, chunk):
    out = []
    for i in range(0, dev.shape[0], chunk):
        out += live.push(sid, dev[i:i + chunk])
    return out


# ---- 3. the statistics' order --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S,key", SHAPES, ids=IDS)
def test_statistics_of_a_push_far_past_the_head_are_the_offline_ones(T, S, key):
    """head:7, the whole recording — three rings long — in a single push: the Python layer splits it, and the statistics are taken
    before the append that wraps over the head."""
    live, _mon = _monitors(T, S, key)
    sig, dev = _recording(T, S, 1)
    live.open("a", NAMES8)
    live.open("b", NAMES8)
    ups = live.push({"b": sig})                  # numpy: uploaded by push
    want = _offline(T, S, key, 1)[0].cpu().numpy()
    got = live.session_stats("b").cpu().numpy()
    Cn = len(COLS[key])
    for sl in (slice(0, Cn), slice(L.MAX_C, L.MAX_C + Cn), slice(2 * L.MAX_C, 2 * L.MAX_C + 1)):
        assert np.array_equal(got[sl].view(np.uint64), want[sl].view(np.uint64))
    assert got[2 * L.MAX_C] == K_HEAD
    N = R.count(sig.shape[0], T, S)
    assert [u.window for u in ups["b"]] == list(range(N)) and [u.warmup for u in ups["b"]] == [True] * K_HEAD + [False] * (N - K_HEAD)
    assert live.timeline("a").t_end.shape == (0,) and live.timeline("b").meta["samples"] == sig.shape[0]


# ---- 4. chunking invariance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S,key", SHAPES, ids=IDS)
def test_every_way_of_chunking_gives_the_same_timeline(T, S, key):
    live, mon = _monitors(T, S, key)
    _sig, dev = _recording(T, S, 0)
    ways = {"strides": S, "one push": dev.shape[0]}
    if (T, S) == (200, 37):
        ways["sample by sample"] = 1
    for sid, chunk in ways.items():
        live.open(sid, NAMES8)
        _feed(live, sid, dev, chunk)
    base = mon.run(dev, NAMES8)
    for sid in ways:
        _same(live.timeline(sid), base, sid)


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------------
FIELDS = ("mean_p", "std_p", "pred", "entropy", "mutual_info", "votes")
CHANNELS = {6: ["chest_ECG", "chest_EDA", "chest_Resp", "wrist_BVP", "chest_ACC_x", "wrist_EDA"], 2: ["chest_Temp", "chest_EDA"]}


def _host(p):
    torch.cuda.synchronize()
    return {k: getattr(p, k).cpu().numpy() for k in FIELDS}


@pytest.mark.parametrize("given", [False, True], ids=["head7", "statistics"])
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("kind,Cin", [("cnn_gru_attention", 6), ("cnn_gru", 2)])
def test_live_timelines_updates_and_alarms_are_the_offline_ones(kind, Cin, M, given):
    from multimodalsignal_amd.ensemble import Ensemble
    from multimodalsignal_amd.live import alarms_of_events
    from multimodalsignal_amd.monitor import RecordingWindows
    T, S = 256, 64
    recs = {k: _recording(T, S, k) for k in SESSIONS}
    reference = f"head:{K_HEAD}"
    if given:                   # wearers enrolled earlier: one statistics tensor, from windows [3, 11) of session 0's recording
        reference = RecordingWindows(recs[0][1], NAMES8, CHANNELS[Cin], T, S, reference=(3, 11)).stats.clone()
    models = R.models(kind, Cin, 2, M, DEV)
    own = torch.from_numpy(np.random.RandomState(9).randn(37, Cin, T).astype(np.float32)).to(DEV)
    before = _host(Ensemble(models, eval_batch=16).predict(own))                  # before any live code has run
    _live, mon = _monitors(T, S, CHANNELS[Cin], M, kind, reference, models)
    # thresholds that the scores of these never-trained members cross: the 40th and 60th percentile of session 0's offline smoothed score
    sm = mon.run(recs[0][1], NAMES8).smoothed
    off, on = float(np.percentile(sm, 40)), float(np.percentile(sm, 60))
    if not off < on:
        off, on = 0.45, 0.55
    live, mon = _monitors(T, S, CHANNELS[Cin], M, kind, reference, models, on=on, off=off)
    offline = {k: mon.run(recs[k][1], NAMES8) for k in SESSIONS}
    for k in SESSIONS:
        live.open(k, NAMES8)
    rs = np.random.RandomState(5)
    at, ups = {k: 0 for k in SESSIONS}, {k: [] for k in SESSIONS}
    while any(at[k] < recs[k][1].shape[0] for k in SESSIONS):           # interleaved, ragged, sometimes without one of the three
        chunks = {}
        for k in SESSIONS:
            n = int(rs.choice([0, 1, S - 1, S, 3 * S + 7, 700]))
            if rs.rand() < 0.8:
                chunks[k] = recs[k][1 if k != 1 else 0][at[k]:at[k] + n]     # session 1 pushes numpy arrays
                at[k] += chunks[k].shape[0]
        for k, u in live.push(chunks).items():
            ups[k] += u
    warm = 0 if given else K_HEAD
    for k in SESSIONS:
        tl, want = live.timeline(k), offline[k]
        _same(tl, want, k)
        for f in FIELDS:
            assert np.array_equal(getattr(tl, f).view(np.uint32), getattr(want, f).view(np.uint32)), (k, f)
        assert tl.meta == want.meta
        N = len(want.t_end)
        assert [u.window for u in ups[k]] == list(range(N)) and all(u.sid == k for u in ups[k])
        for u in ups[k]:                   # each update is the timeline's row
            n = u.window
            row = (want.t_end[n], want.score[n], want.std_p[n, 1], want.entropy[n], want.mutual_info[n], want.pred[n], want.smoothed[n], want.warmup[n])
            assert (u.t_end, u.score, u.std, u.entropy, u.mutual_info, u.pred, u.smoothed, u.warmup) == tuple(v.item() for v in row), (k, n)
            assert u.warmup == (n < warm)
        implied = alarms_of_events(want.state, mon.min_on)
        assert implied == R.alarms(want.smoothed, on, off, mon.min_on)
        assert [(a.kind, a.window, a.start_window) for a in live.alarms(k)] == implied
        assert [u.alarm for u in ups[k] if u.alarm is not None] == live.alarms(k)
        for a in live.alarms(k):
            assert (a.t_s, a.start_s) == (want.t_end[a.window], want.t_end[a.start_window])
        edges = np.diff(np.r_[0, want.state.astype(np.int8), 0])
        for a, b in zip(np.flatnonzero(edges == 1), np.flatnonzero(edges == -1)):       # `on`: the state from the onset on
            assert [u.on for u in ups[k][a:b]] == [False] * (mon.min_on - 1) + [True] * (b - a - mon.min_on + 1)
        assert sum(u.on for u in ups[k]) == int(want.state.sum()) - (mon.min_on - 1) * len(want.events)
    after = _host(Ensemble(models, eval_batch=16).predict(own))
    for f in FIELDS:
        assert np.array_equal(after[f].view(np.uint32), before[f].view(np.uint32)), f


# ---- 6. sessions are independent -----------------------------------------------------------------------------------------------------
def test_sessions_are_independent_and_a_reused_slot_has_no_memory():
    T, S, key = 200, 37, "3of8"
    recs = {k: _recording(T, S, k)[1] for k in SESSIONS}
    alone = {}
    for k in (0, 3):
        live, _mon = _monitors(T, S, key, max_sessions=3)
        live.open("solo", NAMES8)
        _feed(live, "solo", recs[k], 2 * S + 3)
        alone[k] = live.timeline("solo")
    live, _mon = _monitors(T, S, key, max_sessions=3)
    for sid in ("first", "left", "right"):
        live.open(sid, NAMES8)
    slot = live.sessions["left"].slot
    chunk, half = 2 * S + 3, recs[0].shape[0] // 2 // (2 * S + 3) * (2 * S + 3)
    for i in range(0, half, chunk):
        live.push({"first": recs[0][i:i + chunk], "left": recs[1][i:i + 80], "right": recs[1][i:i + chunk + 9]})
    assert len(live.timeline("left").t_end) > K_HEAD                      # the slot's ring and statistics are in use
    live.close("left")
    with pytest.raises(ValueError):
        live.push("left", recs[1][:5])
    live.open("new", NAMES8)
    assert live.sessions["new"].slot == slot and len(live.timeline("new").t_end) == 0
    ticks = range(half, recs[0].shape[0], chunk)
    for i in ticks:
        live.push({"first": recs[0][i:i + chunk], "new": recs[3][i - half:i - half + chunk], "right": recs[1][i:i + 11]})
    _feed(live, "new", recs[3][len(ticks) * chunk:], chunk)
    _same(live.timeline("first"), alone[0], "with companions")
    _same(live.timeline("new"), alone[3], "in a reused slot")


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
def test_live_monitor_refuses_what_it_cannot_take():
    from multimodalsignal_amd.live import LiveMonitor
    T, S, key = 200, 37, "3of8"
    channels = [NAMES8[c] for c in COLS[key]]
    models = R.models("cnn_gru_attention", 3, 2, 1, DEV)
    kw = dict(window_s=T / FS, stride_s=S / FS, eval_batch=16, channels=channels, max_sessions=2)
    with pytest.raises(ValueError):
        LiveMonitor(models, FS, reference="recording", **kw)                                  # not causal
    with pytest.raises(ValueError):
        LiveMonitor(models, FS, reference=(0, 7), **kw)
    with pytest.raises(ValueError):
        LiveMonitor(models, FS, reference="head:7", ring_s=((K_HEAD - 1) * S + T - 1) / FS, **kw)      # R smaller than the head span
    with pytest.raises(ValueError):
        LiveMonitor(models, FS, reference=torch.zeros(5, dtype=torch.float64), **kw)
    with pytest.raises(ValueError):
        LiveMonitor(models, FS, reference="head:7", **dict(kw, max_sessions=0))
    live = LiveMonitor(models, FS, reference="head:7", ring_s=_ring(T, S) / FS, **kw)
    _sig, dev = _recording(T, S, 0)
    with pytest.raises(ValueError):
        live.open("a", NAMES8[:2])                                                            # the models' channels are not all there
    live.open("a", NAMES8)
    with pytest.raises(ValueError):
        live.open("a", NAMES8)
    with pytest.raises(ValueError):
        live.open("b", NAMES8[::-1])                                                          # other columns than the first session's
    live.open("b")
    with pytest.raises(ValueError):
        live.open("c", NAMES8)                                                                # more sessions than the pool has slots
    with pytest.raises(ValueError):
        live.push("a", dev[:10].cpu())                                                        # a CPU tensor: no fallback
    with pytest.raises(ValueError):
        live.push("a", dev[:10].float())
    with pytest.raises(ValueError):
        live.push("a", dev[:10, :7])                                                          # wrong column count
    with pytest.raises(ValueError):
        live.push({"a": dev[:10], "nobody": dev[:10]})                                        # an unknown sid: nothing is appended
    with pytest.raises(ValueError):
        live.timeline("nobody")
    assert live.sessions["a"].book.written == 0
    assert live.push("a", dev[:0]) == [] and live.push({}) == {}
    # where the library refuses: a window that is not in the ring
    from multimodalsignal_amd.live import LiveBatch
    live.push("a", dev[:T + 5])
    with pytest.raises(RuntimeError):
        live.ensemble.predict(LiveBatch(live, [(live.sessions["a"].slot, 1, T + 5)]))        # window 1 is not complete yet


# ---- 8. the command line -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run_dir(tmp_path_factory):
    """A run directory of saved random state_dicts: folds S2 and S10, replica 0 and seed_1/."""
    from multimodalsignal_amd.synth import CHANNELS6
    root = tmp_path_factory.mktemp("run")
    seed = 40
    for rep in ("", "seed_1"):
        for sid in ("S2", "S10"):
            d = root / rep / f"fold_test_on_{sid}"
            d.mkdir(parents=True)
            torch.save(R.models("cnn_gru_attention", 6, 2, 1, DEV, seed)[0].state_dict(), d / "best_model.pt")
            seed += 1
    (root / "cv_summary.txt").write_text(f"实验配置:\nSEED: 42\nCHANNELS_TO_USE: {list(CHANNELS6)}\n", encoding="utf-8")
    return root


def test_cli_replays_the_synthetic_recording_into_three_sessions(run_dir, tmp_path, capsys):
    import json
    from multimodalsignal_amd import live, monitor
    args = ["--run", str(run_dir), "--synthetic-recording", "--window-s", "8", "--stride-s", "8", "--reference", "head:6"]
    tl = live.main(args + ["--sessions", "3", "--chunk-s", "3", "--out", str(tmp_path / "live")])
    said = capsys.readouterr().out
    want = monitor.main(args + ["--out", str(tmp_path / "offline")])
    n = (40 * 60 * 64 - 512) // 512 + 1
    rows = (tmp_path / "live" / "timeline.csv").read_text().splitlines()
    assert len(tl.t_end) == n and len(rows) == n + 1
    assert rows == (tmp_path / "offline" / "timeline.csv").read_text().splitlines()
    assert json.loads((tmp_path / "live" / "timeline.json").read_text()) == json.loads((tmp_path / "offline" / "timeline.json").read_text())
    _same(tl, want, "cli")
    line = [ln for ln in said.splitlines() if "Monitor.run" in ln]
    assert len(line) == 1 and line[0].endswith(": equal bit for bit") and "NOT" not in line[0]
    alarms = json.loads((tmp_path / "live" / "alarms.json").read_text())
    assert set(alarms) == {"0", "1", "2"} and alarms["0"] == alarms["1"] == alarms["2"]
    assert [(a["kind"], a["window"], a["start_window"]) for a in alarms["0"]] == live.alarms_of_events(want.state, 2)
