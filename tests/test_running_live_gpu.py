"""Causal running references, live equals offline (include/msig_rn.h, multimodalsignal_amd/live.py).

Kernel level: three sessions of a ring pool, out of phase, fed in chunks of 1, S and 3 S + 1 samples through rings of R = T and
R = T + 5 rows (every window wraps; R = T + 3 S + 1 lets one step take several windows of a session) — every statistics record
msig_rn_lv_step writes and every row msig_rn_lv_windows_multi writes equals, bit for bit, what msig_rn_sums, msig_rn_stats and
msig_rn_windows give for the session's linear recording, under expanding and trailing:2 / trailing:7, in mixed batches, and in a
slot that is closed and reopened without its state being cleared.  End to end: LiveMonitor's timelines, alarms and statistics
against Monitor.run on the same samples under "expanding" and "trailing:5:2", and "head:6" as before."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import lv_reference as LV
import rn_reference as R
from multimodalsignal_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MC = L.MAX_C
NAMES8, COLS = LV.NAMES8, LV.COLS
POOL_SLOTS = 4                                  # sessions live in slots 0, 1 and 3: ring and state 2 are never touched
FS = 64.0


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "the gpu tier needs an MI355X"


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


@functools.lru_cache(maxsize=None)
def _recording(T, S, N, seed):
    sig = LV.recording((N - 1) * S + T + 2, seed)
    return sig, torch.from_numpy(sig).to(DEV)


def _head(dev, cols, T, S):
    return dev.data_ptr(), dev.shape[0], dev.shape[1], (C.c_int32 * len(cols))(*cols), len(cols), LV.mask_of(cols), T, S


@functools.lru_cache(maxsize=None)
def _offline(T, S, N, seed, key, K):
    """The table and every row of the LINEAR recording: msig_rn_sums, msig_rn_stats, msig_rn_windows — computed once."""
    _sig, dev = _recording(T, S, N, seed)
    cols, lib = COLS[key], L.lib()
    sums = torch.zeros((N, 2 * MC), dtype=torch.float64, device=DEV)
    table = torch.zeros((N, 2 * MC + 1), dtype=torch.float64, device=DEV)
    out = torch.empty((N, len(cols), T), dtype=torch.float32, device=DEV)
    L.check(lib.msig_rn_sums(*_head(dev, cols, T, S), 0, N, sums.data_ptr(), _stream()), "msig_rn_sums")
    L.check(lib.msig_rn_stats(*_head(dev, cols, T, S), sums.data_ptr(), N, K, table.data_ptr(), _stream()), "msig_rn_stats")
    L.check(lib.msig_rn_windows(*_head(dev, cols, T, S), 0, N, table.data_ptr(), out.data_ptr(), _stream()), "msig_rn_windows")
    torch.cuda.synchronize()
    return table.cpu().numpy(), out.cpu().numpy()


def _selected(rec, Cn):
    return np.concatenate([rec[..., :Cn], rec[..., MC:MC + Cn], rec[..., 2 * MC:]], axis=-1)


class Pool:
    """A caller-owned pool of POOL_SLOTS rings filled with 0x5A and as many session states filled with NaN (the library needs no
    initialisation), and the host's side of every open session: samples written, next window, its ring's bookkeeping."""

    def __init__(self, T, S, Rn, key, K):
        from multimodalsignal_amd.live import RingBook
        self.T, self.S, self.R, self.K, self.cols, self.RingBook = T, S, Rn, K, COLS[key], RingBook
        self.mem = torch.full((POOL_SLOTS, Rn * 8 * 8), 0x5A, dtype=torch.uint8, device=DEV)
        self.state = torch.full((POOL_SLOTS, L.lib().msig_rn_state_bytes(K) // 8), float("nan"), dtype=torch.float64, device=DEV)
        self.book, self.next = {}, {}

    def open(self, k):
        self.book[k], self.next[k] = self.RingBook(self.R, self.T, self.S, 0), 0

    def args(self):
        return self.mem.data_ptr(), POOL_SLOTS, self.R, self.R * 8 * 8, 8

    def rows_args(self):
        return (C.c_int32 * len(self.cols))(*self.cols), len(self.cols), LV.mask_of(self.cols), self.T, self.S

    def push(self, chunks):
        ks = list(chunks)
        staging = torch.cat([chunks[k] for k in ks] + [torch.zeros((1, 8), dtype=torch.float64, device=DEV)]).contiguous()
        n = len(ks)
        L.check(L.lib().msig_lv_push(*self.args(), (C.c_int32 * n)(*ks), (C.c_int64 * n)(*[self.book[k].written for k in ks]),
                                     (C.c_int64 * n)(*[int(chunks[k].shape[0]) for k in ks]), n, staging.data_ptr(), _stream()), "msig_lv_push")

    def _rows(self, rows):
        B = len(rows)
        return ((C.c_int32 * B)(*[k for k, _n in rows]), (C.c_int64 * B)(*[n for _k, n in rows]),
                (C.c_int64 * B)(*[self.book[k].written for k, _n in rows]))

    def step(self, rows, nxt=None):
        """ONE msig_rn_lv_step for the mixed batch; returns its (B + 1, 33) table, the last record a canary."""
        B = len(rows)
        table = torch.full((B + 1, 2 * MC + 1), float("nan"), dtype=torch.float64, device=DEV)
        nxt = nxt if nxt is not None else [self.next[k] for k, _n in rows]
        rc = L.lib().msig_rn_lv_step(*self.args(), *self.rows_args(), self.K, self.state.data_ptr(), self.state.shape[1] * 8, *self._rows(rows),
                                     (C.c_int64 * B)(*nxt), B, table.data_ptr(), _stream())
        if rc == 0:
            for k, _n in rows:
                self.next[k] += 1
        return rc, table

    def windows(self, rows, table, arenas, slots):
        L.check(L.lib().msig_rn_lv_windows_multi(*self.args(), *self.rows_args(), *self._rows(rows), len(rows), table.data_ptr(), arenas.ptr("x"),
                                                 C.byref(arenas.multi(slots)), _stream()), "msig_rn_lv_windows_multi")


SHAPES = [(16, 4, "8of8"), (10, 3, "3of8")]
RINGS = ["t", "t+5", "t+3s+1"]


@pytest.mark.parametrize("K", [0, 2, 7], ids=["expanding", "trailing2", "trailing7"])
@pytest.mark.parametrize("ring", RINGS)
@pytest.mark.parametrize("T,S,key", SHAPES, ids=[f"t{T}-s{S}-{key}" for T, S, key in SHAPES])
def test_live_tables_and_rows_are_the_offline_ones(T, S, key, ring, K):
    from multimodalsignal_amd.runtime import Arenas
    Rn = {"t": T, "t+5": T + 5, "t+3s+1": T + 3 * S + 1}[ring]
    Cn = len(COLS[key])
    pool = Pool(T, S, Rn, key, K)
    # slot -> the recordings it takes one after the other (windows, seed): slot 1 is closed after its first and reopened
    plan = {0: [(19, 11)], 1: [(8, 12), (9, 14)], 3: [(15, 13)]}
    cycle = {0: [3 * S + 1, 1, S, 1], 1: [S, 3 * S + 1, 1], 3: [1, 1, S, 3 * S + 1, S]}
    late = {0: 0, 1: 2, 3: 5}                                   # ticks before the session starts: out of phase
    cur = {k: 0 for k in plan}                                  # which of its recordings the slot is on
    at = {k: 0 for k in plan}
    done = {k: 0 for k in plan}
    for k in plan:
        pool.open(k)
    arenas = Arenas(3, DEV, (("other", 1000), ("x", 24 * Cn * T * 4), ("tail", 256)))
    tick, mixed, longest, reopened, checked = 0, 0, 0, False, 0

    def rec(k):
        N, seed = plan[k][cur[k]]
        return N, seed, _recording(T, S, N, 100 * T + seed)[1]

    while True:
        chunks = {}
        for k in plan:
            if tick < late[k] or cur[k] >= len(plan[k]):
                continue
            _N, _seed, dev = rec(k)
            n = cycle[k][(tick - late[k]) % len(cycle[k])]
            chunks[k] = dev[at[k]:at[k] + n]
            at[k] += chunks[k].shape[0]
        if not chunks:
            break
        off = {k: 0 for k in chunks}
        while True:                                             # a push in segments, as live.py makes it
            seg = {k: pool.book[k].segment(chunks[k].shape[0] - off[k]) for k in chunks if chunks[k].shape[0] > off[k]}
            if not seg:
                break
            pool.push({k: chunks[k][off[k]:off[k] + a] for k, a in seg.items()})
            rows = []
            for k, a in seg.items():
                off[k] += a
                _due, wins = pool.book[k].advance(a)
                rows += [(k, w) for w in wins]
            if not rows:
                continue
            rc, table = pool.step(rows)
            assert rc == 0, rc
            arenas.mem.fill_(0x5A)
            pool.windows(rows, table, arenas, [2, 0])
            torch.cuda.synchronize()
            got = table.cpu().numpy()
            assert np.all(np.isnan(got[len(rows)])), "wrote past the table"
            want_rows = []
            for b, (k, w) in enumerate(rows):
                N, seed, _dev = rec(k)
                tab, out = _offline(T, S, N, 100 * T + seed, key, K)
                assert np.array_equal(_selected(got[b], Cn).view(np.uint64), _selected(tab[w], Cn).view(np.uint64)), (tick, k, w)
                assert np.all(np.isnan(got[b, Cn:MC])) and np.all(np.isnan(got[b, MC + Cn:2 * MC]))
                assert w == done[k]
                done[k] += 1
                want_rows.append(out[w].reshape(-1))
            ref, n = np.concatenate(want_rows).view(np.uint32), len(rows) * Cn * T
            for s in (0, 2):
                x = arenas.view(s, "x", torch.float32).cpu().numpy()
                assert np.array_equal(x[:n].view(np.uint32), ref), (tick, s, rows)
                assert np.all(x[n:].view(np.uint8) == 0x5A), "wrote past the batch"
                assert np.all(arenas.view(s, "other").cpu().numpy() == 0x5A) and np.all(arenas.view(s, "tail").cpu().numpy() == 0x5A)
            assert np.all(arenas.mem[1].cpu().numpy() == 0x5A) and np.all(pool.mem[2].cpu().numpy() == 0x5A)
            checked += len(rows)
            mixed += len({k for k, _w in rows}) > 1
            longest = max(longest, max(sum(1 for k2, _w in rows if k2 == k) for k, _w in rows))
        for k in list(chunks):                                  # a recording is through: close; slot 1 reopens with its next one
            N, _seed, dev = rec(k)
            if at[k] >= dev.shape[0]:
                assert done[k] == N
                st = pool.state[k].cpu().numpy()
                assert st[3 * MC] == N and st[3 * MC + 1] == K          # the state knows where it stands
                cur[k] += 1
                at[k], done[k] = 0, 0
                if cur[k] < len(plan[k]):
                    pool.open(k)                                # the same slot, its ring and its state as they were left
                    reopened = True
        tick += 1
    assert checked == 19 + 8 + 9 + 15 and mixed >= 3 and reopened
    assert longest >= (3 if ring == "t+3s+1" else 2 if ring == "t+5" else 1)
    assert torch.isnan(pool.state[2]).all()                     # nobody's state


def test_step_refuses_a_row_that_is_not_the_sessions_next_window():
    """Session 0 has taken windows 0 and 1 and the caller expects window 2 next: a row that disagrees with `next`, the same window
    twice and descending windows are refused before any launch, so the state stays where it stood — windows 2 and 3 then have their
    offline bits."""
    T, S, key, K = 16, 4, "3of8", 2
    pool = Pool(T, S, T + 3 * S + 1, key, K)
    pool.open(0)
    N, seed = 9, 21
    dev = _recording(T, S, N, seed)[1]
    pool.push({0: dev[:T + S]})
    pool.book[0].advance(T + S)
    rc, table = pool.step([(0, 0), (0, 1)])
    assert rc == 0
    pool.push({0: dev[T + S:T + 3 * S]})
    pool.book[0].advance(2 * S)
    for rows, nxt in (([(0, 3)], [2]), ([(0, 2)], [1]), ([(0, 2)], [3]), ([(0, 2), (0, 2)], [2, 2]), ([(0, 3), (0, 2)], [3, 3])):
        rc, _t = pool.step(rows, nxt)
        assert rc == -2, (rows, nxt)
    rc, table = pool.step([(0, 2), (0, 3)])
    torch.cuda.synchronize()
    assert rc == 0
    tab, _out = _offline(T, S, N, seed, key, K)
    Cn = len(COLS[key])
    assert np.array_equal(_selected(table.cpu().numpy()[:2], Cn).view(np.uint64), _selected(tab[2:4], Cn).view(np.uint64))


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
CHANNELS = ["chest_ECG", "chest_EDA", "chest_Resp", "wrist_BVP", "chest_ACC_x", "wrist_EDA"]
TL_FIELDS = ("t_end", "mean_p", "std_p", "pred", "entropy", "mutual_info", "votes", "score", "smoothed", "state", "warmup")


def _monitors(models, reference, **kw):
    from multimodalsignal_amd.live import LiveMonitor
    from multimodalsignal_amd.monitor import Monitor
    common = dict(window_s=64 / FS, stride_s=16 / FS, reference=reference, eval_batch=16, channels=CHANNELS, halflife=2, on=kw.pop("on", 0.55),
                  off=kw.pop("off", 0.45), min_on=2)
    live = LiveMonitor(models, FS, max_sessions=3, **common, **kw)
    assert (live.T, live.S) == (64, 16)
    return live, Monitor(models, FS, **common)


@pytest.mark.parametrize("reference, K, W", [("expanding", 0, 6), ("trailing:5:2", 5, 2)])
def test_live_timelines_alarms_and_statistics_are_the_offline_ones(reference, K, W):
    """Three sessions, out of phase, in chunks of 1, S and 3 S + 1 samples and one single push of a whole recording; a session closed
    and another opened in its slot: timelines_equal(LiveMonitor.timeline(sid), Monitor.run(the same samples)), the same meta (the
    reference string, warmup_windows, every window's reference-window count), one onset and one offset per offline event, no warm-up
    delay (a window is reported by the push that completes it, the first W flagged), session_stats = the offline table's last record."""
    from multimodalsignal_amd.live import alarms_of_events, timelines_equal
    T, S, M = 64, 16, 3
    models = LV.models("cnn_gru_attention", len(CHANNELS), 2, M, DEV)
    recs = {k: _recording(T, S, N, seed) for k, N, seed in (("a", 40, 501), ("b", 33, 502), ("c", 37, 503), ("d", 21, 504))}
    _live, mon = _monitors(models, reference)
    sm = mon.run(recs["a"][1], NAMES8).smoothed                 # thresholds these never-trained members cross
    off, on = float(np.percentile(sm, 40)), float(np.percentile(sm, 60))
    if not off < on:
        off, on = 0.45, 0.55
    live, mon = _monitors(models, reference, on=on, off=off)
    assert live.R == T + 8 * S                                  # no head span: one window and eight strides
    offline = {k: mon.run(recs[k][1], NAMES8) for k in recs}
    assert len(offline["a"].events) >= 1
    ups = {k: [] for k in recs}
    chunk = {"a": [1, S, 3 * S + 1], "b": [3 * S + 1, 1, S, S], "c": [10 ** 6]}          # c: the whole recording in one push
    late = {"a": 0, "b": 3, "c": 7}
    at = {k: 0 for k in chunk}
    for k in chunk:
        live.open(k, NAMES8)
    assert live.session_stats("a") is None
    tick = 0
    while any(at[k] < recs[k][1].shape[0] for k in chunk):
        push = {}
        for k in chunk:
            if tick >= late[k] and at[k] < recs[k][1].shape[0]:
                n = chunk[k][(tick - late[k]) % len(chunk[k])]
                push[k] = recs[k][0 if k == "b" else 1][at[k]:at[k] + n]      # b pushes numpy arrays
                at[k] += push[k].shape[0]
        for k, u in live.push(push).items():
            ups[k] += u
            assert len(ups[k]) == R.count(at[k], T, S), "a window is reported by the push that completes it"
        tick += 1
    assert timelines_equal(live.timeline("b"), offline["b"]) and live.timeline("b").meta == offline["b"].meta
    slot_b = live.sessions["b"].slot
    live.close("b")
    live.open("d", NAMES8)
    assert live.sessions["d"].slot == slot_b and live.session_stats("d") is None and len(live.timeline("d").t_end) == 0
    for i in range(0, recs["d"][1].shape[0], 2 * S + 3):
        ups["d"] += live.push("d", recs["d"][1][i:i + 2 * S + 3])
    from multimodalsignal_amd.monitor import RecordingWindows
    for k in ("a", "c", "d"):
        tl, want = live.timeline(k), offline[k]
        assert timelines_equal(tl, want), k
        for f in TL_FIELDS:
            x, y = getattr(tl, f), getattr(want, f)
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (k, f)
        assert tl.meta == want.meta
        N = len(want.t_end)
        assert want.meta["reference"] == reference and want.meta["warmup_windows"] == W
        assert want.meta["reference_window_counts"] == [n + 1 if K == 0 else min(n + 1, K) for n in range(N)]
        assert list(want.warmup) == [n < W for n in range(N)]
        assert [u.window for u in ups[k]] == list(range(N)) and [u.warmup for u in ups[k]] == [n < W for n in range(N)]
        implied = alarms_of_events(want.state, mon.min_on)
        assert implied == LV.alarms(want.smoothed, on, off, mon.min_on)
        assert [(a.kind, a.window, a.start_window) for a in live.alarms(k)] == implied
        assert sum(a.kind == "onset" for a in live.alarms(k)) == len(want.events)                  # one onset per offline event,
        ends_inside = sum(1 for _a, b, _p, _m in want.events if b < want.t_end[-1])
        assert sum(a.kind == "offset" for a in live.alarms(k)) == ends_inside                     # one offset per event that ends
        rw = RecordingWindows(recs[k][1], NAMES8, CHANNELS, T, S, reference)
        last = live.session_stats(k)
        torch.cuda.synchronize()
        Cn = len(CHANNELS)
        assert rw.stats.shape == (N, 2 * MC + 1) and rw.running == (K, W)
        assert np.array_equal(_selected(last.cpu().numpy(), Cn).view(np.uint64), _selected(rw.stats[N - 1].cpu().numpy(), Cn).view(np.uint64))
        whole = rw.materialise().cpu().numpy()                  # batch() with n0 > 0 takes the table from that row on
        part = rw.batch(5, 7).cpu().numpy()
        assert np.array_equal(part.view(np.uint32), whole[5:12].view(np.uint32))
    with pytest.raises(ValueError):
        live.open("e", NAMES8, stats=torch.zeros(2 * MC + 1, dtype=torch.float64, device=DEV))      # a running reference takes none
    with pytest.raises(ValueError):
        rw.batch(N - 1, 2)


def test_head_6_gives_the_timeline_it_gave():
    """The untouched path beside the new one: "head:6" live equals Monitor.run (which does not change) on the same data."""
    from multimodalsignal_amd.live import timelines_equal
    T, S = 64, 16
    models = LV.models("cnn_gru_attention", len(CHANNELS), 2, 3, DEV)
    _sig, dev = _recording(T, S, 40, 501)
    live, mon = _monitors(models, "head:6")
    assert live.running is None and live.warm == 6 and not hasattr(live, "rn_state")
    live.open("a", NAMES8)
    ups = []
    for i in range(0, dev.shape[0], 3 * S + 1):
        ups += live.push("a", dev[i:i + 3 * S + 1])
    want = mon.run(dev, NAMES8)
    assert timelines_equal(live.timeline("a"), want) and live.timeline("a").meta == want.meta
    assert "reference_window_counts" not in want.meta and want.meta["warmup_windows"] == 6
    assert [u.warmup for u in ups] == [n < 6 for n in range(40)]


# ---- the command line ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run_dir(tmp_path_factory):
    """A run directory of saved random state_dicts: folds S2 and S10."""
    from multimodalsignal_amd.synth import CHANNELS6
    root = tmp_path_factory.mktemp("run")
    for seed, sid in ((40, "S2"), (41, "S10")):
        d = root / f"fold_test_on_{sid}"
        d.mkdir(parents=True)
        torch.save(LV.models("cnn_gru_attention", 6, 2, 1, DEV, seed)[0].state_dict(), d / "best_model.pt")
    (root / "cv_summary.txt").write_text(f"实验配置:\nSEED: 42\nCHANNELS_TO_USE: {list(CHANNELS6)}\n", encoding="utf-8")
    return root


@pytest.mark.parametrize("reference, K, W", [("expanding:3", 0, 3), ("trailing:60", 60, 6)])
def test_both_command_lines_take_a_running_reference(run_dir, tmp_path, capsys, reference, K, W):
    """live replays the synthetic recording into two sessions and says that session 0 equals Monitor.run; monitor writes the same
    timeline.csv and timeline.json, whose meta carries the reference string, warmup_windows and every window's reference count."""
    import json
    from multimodalsignal_amd import live, monitor
    args = ["--run", str(run_dir), "--synthetic-recording", "--window-s", "8", "--stride-s", "8", "--reference", reference]
    tl = live.main(args + ["--sessions", "2", "--chunk-s", "3", "--out", str(tmp_path / "live")])
    said = capsys.readouterr().out
    want = monitor.main(args + ["--out", str(tmp_path / "offline")])
    n = (40 * 60 * 64 - 512) // 512 + 1
    rows = (tmp_path / "live" / "timeline.csv").read_text().splitlines()
    assert len(tl.t_end) == n and len(rows) == n + 1 and rows[0] == "window,t_end_s,score,std,smoothed,state,pred,entropy,mutual_info,warmup"
    assert rows == (tmp_path / "offline" / "timeline.csv").read_text().splitlines()
    doc = json.loads((tmp_path / "offline" / "timeline.json").read_text())
    assert json.loads((tmp_path / "live" / "timeline.json").read_text()) == doc
    assert doc["reference"] == reference and doc["warmup_windows"] == W
    assert doc["reference_window_counts"] == [k + 1 if K == 0 else min(k + 1, K) for k in range(n)]
    assert [r.rsplit(",", 1)[1] for r in rows[1:]] == ["1"] * W + ["0"] * (n - W)
    line = [ln for ln in said.splitlines() if "Monitor.run" in ln]
    assert len(line) == 1 and line[0].endswith(": equal bit for bit") and "NOT" not in line[0]
    assert want.meta["reference"] == reference
