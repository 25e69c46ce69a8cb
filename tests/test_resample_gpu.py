"""The causal polyphase FIR resampler on the GPU (include/msig_rs.h, multimodalsignal_amd/resample.py, live.py, monitor.py, DESIGN.md
section 39): msig_rs_resample against the np.longdouble restatement (tests/rs_reference.py) with the float64 restatement's own error
as the yardstick; msig_rs_lv_push under every way of chunking bit for bit against msig_rs_resample followed by msig_rec_windows on
the linear stream; LiveMonitor(resampler=...) against Monitor(resampler=...) in every field; missing raw samples; and the refusals."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import lv_reference as R
import rs_reference as RS
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd.resample import FirResampler

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES8, COLS = R.NAMES8, R.COLS
RATIOS = [(16, 175), (2, 3), (3, 2), (1, 7), (7, 1)]
LIVE_RATIOS = [(16, 175), (2, 3)]
SHAPES = [(256, 64, "8of8"), (200, 37, "3of8")]
K_HEAD = 7
POOL_SLOTS, SESSIONS = 4, (0, 1, 3)          # three sessions in a pool of four: ring 2 and tail 2 are never touched
FS = 64.0
TL_FIELDS = ("t_end", "mean_p", "std_p", "pred", "entropy", "mutual_info", "votes", "score", "smoothed", "state", "warmup")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "the gpu tier needs an MI355X"


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


@functools.lru_cache(maxsize=None)
def _rs(up, down):
    """The resampler of ratio up / down (fs_in = down, fs_out = up)."""
    r = FirResampler(down, up, DEV)
    assert (r.L, r.M, r.half) == (up, down, 10 * max(up, down))
    return r


def _resample(dev, n_in, r):
    """msig_rs_resample on the first n_in rows of `dev` through the C ABI; the row after the last output keeps its canary."""
    n_out = RS.out_count_brute(n_in, r.L, r.M, r.half)
    y = torch.full((n_out + 1, dev.shape[1]), -7.25, dtype=torch.float64, device=DEV)
    L.check(L.lib().msig_rs_resample(dev.data_ptr(), n_in, dev.shape[1], *r.ratio_args(), y.data_ptr(), n_out, _stream()), "msig_rs_resample")
    torch.cuda.synchronize()
    assert bool((y[n_out] == -7.25).all()), "wrote past the last output"
    return y[:n_out]


# ---- 1. the offline call against the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_all", [1, 3, 8])
@pytest.mark.parametrize("up,down", RATIOS, ids=[f"{u}over{d}" for u, d in RATIOS])
def test_offline_call_against_the_longdouble_restatement(up, down, C_all):
    """msig_rs_resample on prefixes of one stream: none, the last length without an output, the first lengths with one and with two
    (where the ratio has such lengths: one raw row of an up-sampler yields several), one below, at and one above the length that
    completes output 5's support, and a few hundred outputs.  Bound, per column, in the maximum norm: 8 x the float64 restatement's
    own error against np.longdouble.  The yardstick is taken over the case's longest prefix, of which every shorter prefix's
    outputs are a head — the outputs are a causal function of the stream, which is asserted bit for bit —, since the ratio of two
    roundings of ONE output is unbounded whenever the restatement's happens to land on the reference (tests/test_running_gpu.py's
    yardstick is taken over a case's windows for the same reason)."""
    r = _rs(up, down)
    first = lambda k: r.max_rows(k - 1) + 1      # noqa: E731  the shortest stream with k outputs
    big = first(300) + 3
    rs = np.random.RandomState(1000 * up + 10 * down + C_all)
    x = np.cumsum(rs.randn(big, C_all), axis=0)
    x = np.ascontiguousarray(x * (16.0 / np.abs(x).max()) + 3.0 * rs.randn(C_all))
    y64 = RS.resample(x, r.taps, up, down, r.half, np.float64)
    yld = RS.resample(x, r.taps, up, down, r.half, np.longdouble)
    own = np.abs(y64 - yld).max(axis=0).astype(np.float64)
    assert np.all(own > 0)
    dev = torch.from_numpy(x).to(DEV)
    full = _resample(dev, big, r).cpu().numpy()
    assert full.shape == y64.shape and full.shape[0] >= 300
    lengths = sorted({0, r.max_rows(0), first(1), first(2), first(5) - 1, first(5), first(5) + 1, big})
    outs, worst = set(), 0.0
    for n in lengths:
        got = _resample(dev, n, r).cpu().numpy()
        n_out = got.shape[0]
        outs.add(n_out)
        assert n_out == r.out_count(n) == L.lib().msig_rs_out_count(n, up, down, r.half)
        assert np.array_equal(got.view(np.uint64), full[:n_out].view(np.uint64)), n
        if n_out:
            err = np.abs(got - yld[:n_out]).max(axis=0).astype(np.float64)
            worst = max(worst, float((err / own).max()))
            assert np.all(err <= 8 * own), (n, err / own)
    assert 0 in outs and (up > down or {1, 2} <= outs)
    print(f"msig_rs_resample {up}/{down} C_all={C_all}: error {worst:.3f} x the float64 restatement's own (bound 8)")


def test_apply_and_resample_signal_are_the_call():
    from multimodalsignal_amd import preprocess
    r = _rs(16, 175)
    x = R.recording(5000, 3)
    want = _resample(torch.from_numpy(x).to(DEV), 5000, r).cpu().numpy()
    assert want.shape == (448, 8)
    assert np.array_equal(r.apply(x).cpu().numpy().view(np.uint64), want.view(np.uint64))
    assert np.array_equal(r.apply(torch.from_numpy(x[:, 2].copy()).to(DEV)).cpu().numpy().view(np.uint64), want[:, 2].copy().view(np.uint64))
    assert r.apply(x[:100]).shape == (0, 8)
    got = preprocess.resample_signal(x, 175, 16, device=DEV, method="fir")
    assert isinstance(got, np.ndarray) and np.array_equal(got.view(np.uint64), want.view(np.uint64))


# ---- 2. chunking, bits ----------------------------------------------------------------------------------------------------------------
def _ring(T, S):
    return (K_HEAD - 1) * S + T + 41          # no multiple of S, T or 256: every ring wraps several times, at odd places


@functools.lru_cache(maxsize=None)
def _raw(up, down, T, S, k):
    """Session k's raw recording: a little more than three rings of outputs, another length and other values per session."""
    r = _rs(up, down)
    sig = R.recording(r.max_rows(3 * _ring(T, S) + 17 + 29 * k) - k, 1000 * T + 10 * S + k + up)
    return sig, torch.from_numpy(sig).to(DEV)


def _head(dev, cols, T, S):
    return dev.data_ptr(), dev.shape[0], dev.shape[1], (C.c_int32 * len(cols))(*cols), len(cols), R.mask_of(cols), T, S


@functools.lru_cache(maxsize=None)
def _offline(up, down, T, S, key, k):
    """msig_rs_resample of session k's whole raw recording, then msig_rec_stats over windows [0, K_HEAD) and msig_rec_windows of every
    window of the LINEAR resampled stream — computed once."""
    _sig, dev = _raw(up, down, T, S, k)
    y = _resample(dev, dev.shape[0], _rs(up, down)).contiguous()
    cols, lib = COLS[key], L.lib()
    N = R.count(y.shape[0], T, S)
    stats = torch.full((2 * L.MAX_C + 1,), float("nan"), dtype=torch.float64, device=DEV)
    scratch = torch.empty(lib.msig_rec_scratch_bytes(), dtype=torch.uint8, device=DEV)
    L.check(lib.msig_rec_stats(*_head(y, cols, T, S), 0, K_HEAD, stats.data_ptr(), scratch.data_ptr(), _stream()), "msig_rec_stats")
    out = torch.empty((N, len(cols), T), dtype=torch.float32, device=DEV)
    L.check(lib.msig_rec_windows(*_head(y, cols, T, S), 0, N, stats.data_ptr(), out.data_ptr(), _stream()), "msig_rec_windows")
    torch.cuda.synchronize()
    return y.cpu().numpy(), stats, out.cpu().numpy()


class Pool:
    """A caller-owned pool of POOL_SLOTS rings and tails filled with 0x5A, the statistics table, and the host's raw counts."""

    def __init__(self, r, T, S, key, Rn, stats_of=None, tail_rows=None):
        self.r, self.T, self.S, self.R, self.cols = r, T, S, Rn, COLS[key]
        self.tail_rows = r.tail_rows if tail_rows is None else tail_rows
        self.mem = torch.full((POOL_SLOTS, Rn * 8 * 8), 0x5A, dtype=torch.uint8, device=DEV)
        self.tails = torch.full((POOL_SLOTS, self.tail_rows * 8 * 8), 0x5A, dtype=torch.uint8, device=DEV)
        self.stats = torch.full((POOL_SLOTS, 2 * L.MAX_C + 1), float("nan"), dtype=torch.float64, device=DEV)
        for k in SESSIONS:
            if stats_of is not None:
                self.stats[k].copy_(stats_of(k))
        self.raw = {k: 0 for k in SESSIONS}

    def written(self, k):
        return self.r.out_count(self.raw[k])

    def args(self):
        return self.mem.data_ptr(), POOL_SLOTS, self.R, self.R * 8 * 8, 8

    def tail_args(self):
        return self.tails.data_ptr(), self.tail_rows, self.tail_rows * 8 * 8

    def push(self, chunks, missing=False):
        """chunks: {session: (n, 8) device rows} — ONE msig_rs_lv_push, the chunks back to back in one staging buffer (`missing`: no
        staging buffer, every row is missing)."""
        ks = list(chunks)
        n = len(ks)
        staging = chunks[ks[0]] if n == 1 else torch.cat([chunks[k] for k in ks])
        L.check(L.lib().msig_rs_lv_push(*self.args(), *self.tail_args(), *self.r.ratio_args(), (C.c_int32 * n)(*ks),
                                        (C.c_int64 * n)(*[self.raw[k] for k in ks]), (C.c_int64 * n)(*[int(chunks[k].shape[0]) for k in ks]), n,
                                        None if missing else staging.data_ptr(), _stream()), "msig_rs_lv_push")
        for k in ks:
            self.raw[k] += int(chunks[k].shape[0])

    def windows(self, rows, arenas, slots):
        """rows: [(session, window)] — ONE msig_lv_windows_multi into the arena slots `slots`."""
        B = len(rows)
        L.check(L.lib().msig_lv_windows_multi(*self.args(), (C.c_int32 * len(self.cols))(*self.cols), len(self.cols), R.mask_of(self.cols),
                                              self.T, self.S, (C.c_int32 * B)(*[k for k, _n in rows]), (C.c_int64 * B)(*[n for _k, n in rows]),
                                              (C.c_int64 * B)(*[self.written(k) for k, _n in rows]), B, self.stats.data_ptr(), arenas.ptr("x"),
                                              C.byref(arenas.multi(slots)), _stream()), "msig_lv_windows_multi")

    def ring(self, k):
        return self.mem[k].view(torch.float64).view(self.R, 8).cpu().numpy()

    def tail(self, k):
        return self.tails[k].view(torch.float64).view(self.tail_rows, 8).cpu().numpy()


def _check_batch(pool, rows, arenas, want, what):
    """Slots 2 and 0 of three hold the rows' offline bits; slot 1 and the rest of every arena keep 0x5A."""
    arenas.mem.fill_(0x5A)
    pool.windows(rows, arenas, [2, 0])
    torch.cuda.synchronize()
    n = len(rows) * len(pool.cols) * pool.T
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


def _ways(r, rs):
    """Chunk lengths in raw rows by name; `room` is the longest chunk the ring allows at that moment."""
    return {"ones": lambda room: 1, "sevens": lambda room: 7, "prime": lambda room: _next_prime(r.tail_rows),
            "long": lambda room: 2 * r.tail_rows + 5, "most": lambda room: room,
            "ragged": lambda room: int(rs.choice([1, 5, r.tail_rows - 1, r.tail_rows, r.tail_rows + 1, 3 * r.tail_rows + 7]))}


GROUPS = {"short": ("ones", "sevens", "prime"), "long": ("long", "most", "ragged")}


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("T,S,key", SHAPES, ids=[f"t{T}-s{S}" for T, S, _k in SHAPES])
@pytest.mark.parametrize("up,down", LIVE_RATIOS, ids=[f"{u}over{d}" for u, d in LIVE_RATIOS])
def test_every_way_of_chunking_gives_the_offline_bits(up, down, T, S, key, group):
    """Three raw recordings into sessions 0, 1 and 3 of a pool of four, each cut its own way — rows one by one, sevens, a prime near
    tail_rows; or chunks longer than tail_rows, as long as the ring allows, ragged — session j starting 3 j pushes late, one
    msig_rs_lv_push per tick for all of them.  After each push the newly complete windows of all sessions as one mixed batch: every
    row is msig_rec_windows' on msig_rs_resample's output for the linear recording.  At the end every ring row and every tail row."""
    from multimodalsignal_amd.runtime import Arenas
    r, Rn = _rs(up, down), _ring(T, S)
    off = {k: _offline(up, down, T, S, key, k) for k in SESSIONS}
    want = {k: off[k][2] for k in SESSIONS}
    pool = Pool(r, T, S, key, Rn, lambda k: off[k][1])
    devs = {k: _raw(up, down, T, S, k)[1] for k in SESSIONS}
    arenas = Arenas(3, DEV, (("other", 1000), ("x", 40 * len(COLS[key]) * T * 4), ("tail", 256)))
    ways = _ways(r, np.random.RandomState(11))
    done = {k: 0 for k in SESSIONS}
    tick, checked, mixed, longest = 0, 0, 0, {k: 0 for k in SESSIONS}
    while any(pool.raw[k] < devs[k].shape[0] for k in SESSIONS):
        chunks = {}
        for j, k in enumerate(SESSIONS):
            if tick >= 3 * j and pool.raw[k] < devs[k].shape[0]:
                room = r.max_rows(pool.written(k) + Rn - T) - pool.raw[k]        # a window completed by this push is still in the ring
                n = min(ways[GROUPS[group][j]](room), room, devs[k].shape[0] - pool.raw[k])
                assert n >= 1
                chunks[k] = devs[k][pool.raw[k]:pool.raw[k] + n]
                longest[k] = max(longest[k], n)
        tick += 1
        pool.push(chunks)
        rows = []
        for k in SESSIONS:
            now = R.count(pool.written(k), T, S)
            rows += [(k, w) for w in range(done[k], now)]
            done[k] = now
        if rows:
            assert len(rows) <= 40
            _check_batch(pool, rows, arenas, want, f"push {tick}")
            checked += len(rows)
            mixed += len({k for k, _w in rows}) > 1
    assert checked == sum(want[k].shape[0] for k in SESSIONS)
    if group == "long":
        assert mixed > 0 and all(longest[k] > r.tail_rows for k in SESSIONS)
    torch.cuda.synchronize()
    for k in SESSIONS:
        y, sig = off[k][0], _raw(up, down, T, S, k)[0]
        assert pool.raw[k] == sig.shape[0] and pool.written(k) == y.shape[0] > 3 * Rn          # every ring wrapped three times
        i = np.arange(y.shape[0] - Rn, y.shape[0])
        assert np.array_equal(pool.ring(k)[i % Rn].view(np.uint64), y[i].view(np.uint64)), k
        j = np.arange(sig.shape[0] - r.tail_rows, sig.shape[0])
        assert np.array_equal(pool.tail(k)[j % r.tail_rows].view(np.uint64), sig[j].view(np.uint64)), k
    assert np.all(pool.mem[2].cpu().numpy() == 0x5A) and np.all(pool.tails[2].cpu().numpy() == 0x5A)


# ---- 3. end to end --------------------------------------------------------------------------------------------------------------------
CHANNELS6 = ["chest_ECG", "chest_EDA", "chest_Resp", "wrist_BVP", "chest_ACC_x", "wrist_EDA"]


def _monitors(r, T, S, M, reference, gaps, models=None, **kw):
    """A LiveMonitor and the offline Monitor over the same random members, settings and resampler."""
    from multimodalsignal_amd.live import LiveMonitor
    from multimodalsignal_amd.monitor import Monitor
    models = models if models is not None else R.models("cnn_gru_attention", 6, 2, M, DEV)
    common = dict(window_s=T / FS, stride_s=S / FS, reference=reference, eval_batch=16, channels=CHANNELS6, halflife=2,
                  on=kw.pop("on", 0.55), off=kw.pop("off", 0.45), min_on=2, gaps=gaps, resampler=r)
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
    """700 -> 64 Hz.  Three raw recordings pushed interleaved, ragged, as device tensors and as numpy arrays; under `gaps` with
    scattered missing raw samples and, per session, a stretch in which nothing arrived, delivered as skip calls."""
    from multimodalsignal_amd.live import alarms_of_events, alarms_of_gaps
    from multimodalsignal_amd.reference import Gaps
    T, S = 256, 64
    r = FirResampler(700, 64, DEV)
    gaps = Gaps(0.75, 2) if gapped else None
    recs, spans = {}, {}
    for k in SESSIONS:
        sig = _raw(16, 175, T, S, k)[0].copy()
        if gapped:
            rs = np.random.RandomState(40 + k)
            sig[rs.randint(0, sig.shape[0], 30), rs.randint(0, 8, 30)] = np.nan
            a = int(sig.shape[0] * (0.3 + 0.1 * k))
            spans[k] = (a, a + 700 * 9 + 13 * k)                     # nine seconds: more than two windows hold nothing else
            sig[spans[k][0]:spans[k][1]] = np.nan
        recs[k] = (sig, torch.from_numpy(sig).to(DEV))
    _live, mon, models = _monitors(r, T, S, M, reference, gaps)
    sm = mon.run(recs[0][1], NAMES8).smoothed
    off, on = float(np.percentile(sm, 40)), float(np.percentile(sm, 60))
    if not off < on:
        off, on = 0.45, 0.55
    live, mon, _m = _monitors(r, T, S, M, reference, gaps, models, on=on, off=off)
    offline = {k: mon.run(recs[k][1 if k != 3 else 0], NAMES8) for k in SESSIONS}          # session 3's recording is a numpy array
    for k in SESSIONS:
        live.open(k, NAMES8)
    rs = np.random.RandomState(5)
    at, ups = {k: 0 for k in SESSIONS}, {k: [] for k in SESSIONS}
    while any(at[k] < recs[k][0].shape[0] for k in SESSIONS):
        chunks, gone = {}, {}
        for k in SESSIONS:
            n = int(rs.choice([0, 1, 699, 700, 1750, 3 * 700 + 7, 8000]))
            if rs.rand() < 0.8:
                lo, hi = at[k], min(at[k] + n, recs[k][0].shape[0])
                if gapped and lo < spans[k][1] and hi > spans[k][0]:             # up to the stretch; then the stretch itself, skipped
                    hi = spans[k][0] if lo < spans[k][0] else min(hi, spans[k][1])
                    if lo >= spans[k][0]:
                        gone[k] = hi - lo
                if k not in gone:
                    chunks[k] = recs[k][1 if k != 1 else 0][lo:hi]               # session 1 pushes numpy arrays
                at[k] = hi
        for k, u in live.push(chunks).items():
            ups[k] += u
        if gone:
            for k, u in live.skip(gone).items():
                ups[k] += u
    for k in SESSIONS:
        tl, want = live.timeline(k), offline[k]
        _same(tl, want, k)
        assert tl.meta == want.meta
        assert tl.meta["resampler"] == r.spelling and tl.meta["resampler_latency_s"] == r.latency_s
        assert tl.meta["raw_samples"] == recs[k][0].shape[0] and tl.meta["samples"] == r.out_count(recs[k][0].shape[0])
        N = len(want.t_end)
        assert N == R.count(r.out_count(recs[k][0].shape[0]), T, S) > 20
        assert [u.window for u in ups[k]] == list(range(N)) and all(u.sid == k for u in ups[k])
        for u in ups[k]:
            n = u.window
            row = (want.t_end[n], want.score[n], want.std_p[n, 1], want.entropy[n], want.mutual_info[n], want.pred[n], want.smoothed[n], want.warmup[n])
            got = (u.t_end, u.score, u.std, u.entropy, u.mutual_info, u.pred, u.smoothed, u.warmup)
            assert all(a == b or (a != a and b != b) for a, b in zip(got, (v.item() for v in row))), (k, n)
        if gapped:
            implied = alarms_of_gaps(want.state, want.valid, gaps.lost_after, mon.min_on)
            assert (~want.valid).sum() >= 2 and want.lost.any()
            assert [u.valid for u in ups[k]] == list(want.valid)
        else:
            implied = alarms_of_events(want.state, mon.min_on)
        assert [(a.kind, a.window, a.start_window) for a in live.alarms(k)] == implied
        raised = [a for u in ups[k] for a in (u.alarms if gapped else ([u.alarm] if u.alarm is not None else []))]
        assert raised == live.alarms(k)


def test_monitor_run_is_apply_then_run():
    from multimodalsignal_amd.monitor import Monitor
    T, S = 256, 64
    r = FirResampler(700, 64, DEV)
    sig, dev = _raw(16, 175, T, S, 0)
    models = R.models("cnn_gru_attention", 6, 2, 1, DEV)
    kw = dict(window_s=T / FS, stride_s=S / FS, reference="recording", eval_batch=16, channels=CHANNELS6)
    with_rs, plain = Monitor(models, FS, resampler=r, **kw), Monitor(models, FS, **kw)
    a, b = with_rs.run(dev, NAMES8), plain.run(r.apply(dev), NAMES8)
    _same(a, b)
    assert "resampler" not in b.meta and {k: v for k, v in a.meta.items() if not k.startswith("r")} == {k: v for k, v in b.meta.items() if not k.startswith("r")}


# ---- 4. missing samples ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up,down", LIVE_RATIOS, ids=[f"{u}over{d}" for u, d in LIVE_RATIOS])
def test_one_missing_raw_sample_reaches_exactly_its_outputs(up, down):
    """One NaN in column 5 of raw row j: the outputs whose support holds row j — the set comes from the definition — are not finite in
    column 5, and every other value keeps the clean run's bits; offline, and live in chunks of seven rows."""
    r = _rs(up, down)
    n_in = r.max_rows(120) + 2
    clean = R.recording(n_in, 77 + up)
    j = r.max_rows(60)
    hurt = clean.copy()
    hurt[j, 5] = np.nan
    hit = RS.holds(j, up, down, r.half, r.out_count(n_in))
    assert 2 * r.half // down <= len(hit) <= 2 * r.half // down + 1 and 0 < hit[0] and hit[-1] < r.out_count(n_in) - 1
    dc, dh = torch.from_numpy(clean).to(DEV), torch.from_numpy(hurt).to(DEV)
    want = _resample(dc, n_in, r).cpu().numpy()
    assert np.all(np.isfinite(want))

    def check(got, what):
        bad = ~np.isfinite(got)
        assert sorted(np.flatnonzero(bad[:, 5])) == hit, what
        bad[:, 5] = False
        assert not bad.any(), what
        keep = np.ones(got.shape, dtype=bool)
        keep[hit, 5] = False
        assert np.array_equal(got.view(np.uint64)[keep], want.view(np.uint64)[keep]), what

    check(_resample(dh, n_in, r).cpu().numpy(), "offline")
    pool = Pool(r, 16, 4, "3of8", 200)                               # a ring that holds every output: no wrap
    for i in range(0, n_in, 7):
        pool.push({1: dh[i:i + 7]})
    torch.cuda.synchronize()
    check(pool.ring(1)[:want.shape[0]], "live")
    assert np.all(pool.mem[1].cpu().numpy()[want.shape[0] * 64:] == 0x5A)


def test_skip_gives_the_bits_of_a_push_of_missing_rows():
    """C ABI: a call without a staging buffer leaves the ring and the tail of a call whose staging rows are all NaN.  LiveMonitor:
    skip(sid, n) and push(sid, n NaN rows) give the same timeline, ring and tail."""
    from multimodalsignal_amd.reference import Gaps
    T, S = 256, 64
    r = FirResampler(700, 64, DEV)
    sig, dev = _raw(16, 175, T, S, 0)
    nan_rows = torch.full((9000, 8), float("nan"), dtype=torch.float64, device=DEV)
    pa, pb = Pool(r, T, S, "8of8", _ring(T, S)), Pool(r, T, S, "8of8", _ring(T, S))
    for lo, hi, missing in [(0, 4000, False), (4000, 4100, True), (4100, 4500, False), (4500, 7000, True), (7000, 7001, True), (7001, 9000, False)]:
        pa.push({3: dev[lo:hi]}, missing=missing)
        pb.push({3: nan_rows[:hi - lo] if missing else dev[lo:hi]})
    torch.cuda.synchronize()
    assert np.array_equal(pa.ring(3).view(np.uint64), pb.ring(3).view(np.uint64))
    assert np.array_equal(pa.tail(3).view(np.uint64), pb.tail(3).view(np.uint64))
    t = np.arange(9000 - r.tail_rows, 9000)
    assert np.array_equal(pa.tail(3)[t % r.tail_rows].view(np.uint64), sig[t].view(np.uint64))
    gone = pa.ring(3)[np.arange(r.out_count(6000), r.out_count(7001)) % pa.R]      # outputs whose whole support was missing
    assert gone.shape[0] > 80 and np.all(np.isnan(gone))

    live, mon, _m = _monitors(r, T, S, 1, "expanding", Gaps(0.75, 2))
    live.open("skipped", NAMES8)
    live.open("pushed", NAMES8)
    hurt = sig.copy()
    for lo, hi, missing in [(0, 9000, False), (9000, 16000, True), (16000, 16003, True), (16003, sig.shape[0], False)]:
        if missing:
            hurt[lo:hi] = np.nan
            ua, ub = live.skip("skipped", hi - lo), live.push("pushed", nan_rows[:hi - lo])
            assert [(u.window, u.valid, u.smoothed) for u in ua] == [(u.window, u.valid, u.smoothed) for u in ub]
        else:
            live.push({"skipped": dev[lo:hi], "pushed": dev[lo:hi]})
    a, b = live.timeline("skipped"), live.timeline("pushed")
    _same(a, b, "skip against push")
    _same(a, mon.run(hurt, NAMES8), "skip against the offline run")
    assert (~a.valid).sum() >= 2 and a.lost.any() and a.valid[-1]
    sa, sb = live.sessions["skipped"].slot, live.sessions["pushed"].slot
    torch.cuda.synchronize()
    assert np.array_equal(live.pool[sa].cpu().numpy().view(np.uint64), live.pool[sb].cpu().numpy().view(np.uint64))
    assert np.array_equal(live.tails[sa].cpu().numpy().view(np.uint64), live.tails[sb].cpu().numpy().view(np.uint64))


def test_a_reused_slot_has_no_memory_of_the_closed_sessions_tail():
    T, S = 200, 37
    r = _rs(2, 3)
    recs = {k: _raw(2, 3, T, S, k)[1] for k in (0, 1, 3)}
    kw = dict(ring_s=_ring(T, S) / FS, max_sessions=2)

    def monitor():
        from multimodalsignal_amd.live import LiveMonitor
        models = R.models("cnn_gru_attention", 3, 2, 1, DEV)
        return LiveMonitor(models, FS, window_s=T / FS, stride_s=S / FS, reference=f"head:{K_HEAD}", eval_batch=16,
                           channels=[NAMES8[c] for c in COLS["3of8"]], halflife=2, on=0.55, off=0.45, min_on=2,
                           resampler=FirResampler(3 * 32, 2 * 32, DEV), **kw)

    alone = monitor()
    alone.open("solo", NAMES8)
    for i in range(0, recs[3].shape[0], 101):
        alone.push("solo", recs[3][i:i + 101])
    live = monitor()
    live.open("first", NAMES8)
    live.open("left", NAMES8)
    slot = live.sessions["left"].slot
    live.push({"first": recs[0][:1500], "left": recs[1][:1517]})       # left ends mid-support: its tail holds rows a successor must not see
    assert len(live.timeline("left").t_end) > 0 and live.sessions["left"].raw == 1517
    live.close("left")
    with pytest.raises(ValueError):
        live.push("left", recs[1][:5])
    live.open("new", NAMES8)
    assert live.sessions["new"].slot == slot and live.sessions["new"].raw == 0 and len(live.timeline("new").t_end) == 0
    assert not bool(live.tails[slot].any())
    for i in range(0, recs[3].shape[0], 101):
        live.push({"new": recs[3][i:i + 101], "first": recs[0][1500 + i:1500 + i + 50]})
    _same(live.timeline("new"), alone.timeline("solo"), "in a reused slot")
    assert live.timeline("new").meta["raw_samples"] == recs[3].shape[0]


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3


def test_live_call_refuses_before_any_launch():
    """Every check of msig_rs_lv_push; after each refused call the pool and the tails are what they were.  The rings and the tails lie
    8 bytes further apart than they are long: the padding is never written."""
    r = _rs(16, 175)
    Rn, tail_rows = 100, r.tail_rows
    pool = torch.full((POOL_SLOTS, Rn * 8 * 8 + 8), 0x5A, dtype=torch.uint8, device=DEV)
    tails = torch.full((POOL_SLOTS, tail_rows * 8 * 8 + 8), 0x5A, dtype=torch.uint8, device=DEV)
    staging = torch.zeros((4000, 8), dtype=torch.float64, device=DEV)
    bad_h = torch.zeros(2 * r.half + 2, dtype=torch.float64, device=DEV)
    i32, i64 = lambda *v: (C.c_int32 * len(v))(*v), lambda *v: (C.c_int64 * len(v))(*v)      # noqa: E731
    base = dict(pool=pool.data_ptr(), sessions=POOL_SLOTS, R=Rn, ring_bytes=Rn * 64 + 8, C_all=8, tails=tails.data_ptr(), tail_rows=tail_rows,
                tail_bytes=tail_rows * 64 + 8, h=r.h.data_ptr(), L=16, M=175, half=r.half, sess=i32(0, 3), raw=i64(0, 500), len=i64(300, 700), n=2,
                staging=staging.data_ptr())
    most = r.max_rows(r.out_count(500) + Rn) - 500                   # the longest chunk after 500 rows that yields R outputs
    cases = [("pool", None, E_NULL), ("tails", None, E_NULL), ("h", None, E_NULL), ("sess", None, E_NULL), ("raw", None, E_NULL), ("len", None, E_NULL),
             ("sessions", 0, E_SHAPE), ("sessions", L.LV_MAX_SESSIONS + 1, E_SHAPE), ("R", 0, E_SHAPE), ("R", 1 << 31, E_SHAPE), ("C_all", 0, E_SHAPE),
             ("ring_bytes", Rn * 64 - 8, E_SHAPE), ("L", 0, E_SHAPE), ("L", 4097, E_SHAPE), ("M", 0, E_SHAPE), ("M", 4097, E_SHAPE),
             ("L", 175, E_SHAPE), ("L", 35, E_SHAPE), ("half", 174, E_SHAPE), ("half", L.RS_MAX_HALF + 1, E_SHAPE),
             ("tail_rows", tail_rows - 1, E_SHAPE), ("tail_rows", 1 << 31, E_SHAPE), ("tail_bytes", tail_rows * 64 - 8, E_SHAPE),
             ("n", 0, E_SHAPE), ("n", POOL_SLOTS + 1, E_SHAPE), ("sess", i32(0, 4), E_SHAPE), ("sess", i32(-1, 3), E_SHAPE),
             ("sess", i32(3, 3), E_SHAPE), ("raw", i64(0, -1), E_SHAPE), ("len", i64(300, -1), E_SHAPE), ("len", i64(300, 1 << 31), E_SHAPE),
             ("raw", i64(0, 1 << 48), E_SHAPE), ("len", i64(300, most + 1), E_SHAPE),
             ("pool", pool.data_ptr() + 4, E_ALIGN), ("tails", tails.data_ptr() + 4, E_ALIGN), ("h", bad_h.data_ptr() + 4, E_ALIGN),
             ("staging", staging.data_ptr() + 4, E_ALIGN), ("ring_bytes", Rn * 64 + 12, E_ALIGN), ("tail_bytes", tail_rows * 64 + 12, E_ALIGN)]
    order = ("pool", "sessions", "R", "ring_bytes", "C_all", "tails", "tail_rows", "tail_bytes", "h", "L", "M", "half", "sess", "raw", "len", "n", "staging")
    for name, value, code in cases:
        a = dict(base, **{name: value})
        rc = L.lib().msig_rs_lv_push(*[a[k] for k in order], _stream())
        assert rc == code, (name, value, rc)
    torch.cuda.synchronize()
    assert bool((pool == 0x5A).all()) and bool((tails == 0x5A).all())
    ok = dict(base, len=i64(300, most))                              # the longest chunk is taken, and writes
    assert L.lib().msig_rs_lv_push(*[ok[k] for k in order], _stream()) == 0
    torch.cuda.synchronize()
    assert not bool((pool[3, :Rn * 64] == 0x5A).all()) and bool((pool[1:3] == 0x5A).all()) and bool((pool[:, Rn * 64:] == 0x5A).all())
    assert bool((tails[:, tail_rows * 64:] == 0x5A).all()) and bool((tails[1:3] == 0x5A).all())


def test_offline_call_and_the_python_layer_refuse():
    from multimodalsignal_amd.live import LiveMonitor
    from multimodalsignal_amd.monitor import Monitor
    r = _rs(16, 175)
    x = torch.zeros((5000, 3), dtype=torch.float64, device=DEV)
    y = torch.full((449, 3), -7.25, dtype=torch.float64, device=DEV)
    base = dict(x=x.data_ptr(), n_in=5000, C_all=3, h=r.h.data_ptr(), L=16, M=175, half=r.half, y=y.data_ptr(), n_out=448)
    order = ("x", "n_in", "C_all", "h", "L", "M", "half", "y", "n_out")
    cases = [("x", None, E_NULL), ("y", None, E_NULL), ("h", None, E_NULL), ("n_in", -1, E_SHAPE), ("C_all", 0, E_SHAPE), ("n_out", 447, E_SHAPE),
             ("n_out", 449, E_SHAPE), ("n_out", 458, E_SHAPE), ("L", 0, E_SHAPE), ("M", 4097, E_SHAPE), ("L", 175, E_SHAPE), ("L", 35, E_SHAPE),
             ("half", 174, E_SHAPE), ("x", x.data_ptr() + 4, E_ALIGN), ("y", y.data_ptr() + 4, E_ALIGN), ("h", r.h.data_ptr() + 4, E_ALIGN)]
    for name, value, code in cases:
        a = dict(base, **{name: value})
        assert L.lib().msig_rs_resample(*[a[k] for k in order], _stream()) == code, (name, value)
    torch.cuda.synchronize()
    assert bool((y == -7.25).all())
    assert L.lib().msig_rs_resample(None, 0, 3, r.h.data_ptr(), 16, 175, r.half, None, 0, _stream()) == 0      # nothing in, nothing out
    models = R.models("cnn_gru_attention", 3, 2, 1, DEV)
    kw = dict(window_s=200 / FS, stride_s=37 / FS, eval_batch=16, channels=[NAMES8[c] for c in COLS["3of8"]])
    for cls in (LiveMonitor, Monitor):
        with pytest.raises(ValueError):
            cls(models, FS, reference="expanding", resampler=FirResampler(700, 32, DEV), **kw)          # another output rate
        with pytest.raises(ValueError):
            cls(models, FS, reference="expanding", resampler="fir", **kw)
    with pytest.raises(ValueError):
        LiveMonitor(models, FS, reference="expanding", resampler=FirResampler(700, 64, "cpu"), **kw)     # taps on another device
    with pytest.raises(ValueError):
        LiveMonitor(models, 700.0, window_s=200 / 700, stride_s=37 / 700, eval_batch=16, channels=kw["channels"], reference="expanding",
                    ring_s=203 / 700, resampler=FirResampler(64, 700, DEV))                             # no room for one raw row's 11 outputs
    live = LiveMonitor(models, FS, reference="expanding", resampler=FirResampler(700, 64, DEV), **kw)
    live.open("a", NAMES8)
    with pytest.raises(ValueError):
        live.skip("a", 700)                                                                             # skip needs gaps, as ever
    with pytest.raises(ValueError):
        live.push("a", torch.zeros((10, 7), dtype=torch.float64, device=DEV))
    assert live.sessions["a"].raw == 0 and live.push("a", np.zeros((0, 8))) == []


# ---- 6. the command line -------------------------------------------------------------------------------------------------------------
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


def test_cli_replays_the_raw_rate_synthetic_recording(run_dir, tmp_path, capsys):
    import json
    from multimodalsignal_amd import live, monitor
    args = ["--run", str(run_dir), "--synthetic-recording", "--resample-from", "700", "--resampler", "fir", "--window-s", "8", "--stride-s", "8",
            "--reference", "expanding", "--gaps", "--synthetic-gaps", "drop=0.0002,all=900:70"]      # a missing raw sample costs the 20 outputs whose support holds it
    tl = live.main(args + ["--sessions", "2", "--chunk-s", "20", "--out", str(tmp_path / "live")])
    said = capsys.readouterr().out
    want = monitor.main(args + ["--out", str(tmp_path / "offline")])
    r = FirResampler(700, 64, "cpu")
    n = (r.out_count(40 * 60 * 700) - 512) // 512 + 1
    assert len(tl.t_end) == n == len(want.t_end)
    _same(tl, want, "cli")
    assert (tmp_path / "live" / "timeline.csv").read_text() == (tmp_path / "offline" / "timeline.csv").read_text()
    doc = json.loads((tmp_path / "live" / "timeline.json").read_text())
    assert doc == json.loads((tmp_path / "offline" / "timeline.json").read_text())
    assert doc["resampler"] == r.spelling and doc["resampler_latency_s"] == r.latency_s and doc["raw_samples"] == 40 * 60 * 700
    assert doc["samples"] == r.out_count(40 * 60 * 700) and doc["lost_windows"] > 0
    line = [ln for ln in said.splitlines() if "Monitor.run's" in ln]
    assert len(line) == 1 and line[0].endswith(": equal bit for bit") and "NOT" not in line[0]
    assert any("pushed at 700 Hz" in ln for ln in said.splitlines()) and any(f"{70 * 700} of session 0's" in ln for ln in said.splitlines())
    with pytest.raises(SystemExit):
        live.parse_args(["--run", str(run_dir), "--synthetic-recording", "--resample-from", "700", "--out", str(tmp_path / "x")])      # fft: as ever
    with pytest.raises(SystemExit):
        monitor.parse_args(["--run", str(run_dir), "--synthetic-recording", "--resampler", "fir", "--out", str(tmp_path / "x")])
