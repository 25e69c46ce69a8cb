"""The decayed running reference, live equals offline (include/msig_rd.h, multimodalsignal_amd/live.py).

Kernel level — tests/test_running_live_gpu.py's scenario with msig_rd_lv_step in msig_rn_lv_step's place: three sessions of a ring
pool, out of phase, fed in chunks of 1, S and 3 S + 1 samples through rings of R = T, T + 5 and T + 3 S + 1 rows, a slot closed and
reopened with its state left as it was — every statistics record msig_rd_lv_step writes and every row msig_rn_lv_windows_multi then
writes equals, as uint64 / uint32, what msig_rn_sums, msig_rd_stats and msig_rn_windows give for the session's linear recording, under
lambda = exp2(-1/3) and lambda = 1.  End to end: LiveMonitor.timeline against Monitor.run at T = 64, S = 16 under "decayed:5:2"."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import lv_reference as LV
import rn_reference as R
import test_running_live_gpu as RL
from multimodalsignal_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = RL.DEV
MC = L.MAX_C
COLS, NAMES8 = LV.COLS, LV.NAMES8
DECAYS = {"h3": float(np.exp2(-1.0 / 3)), "one": 1.0}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "the gpu tier needs an MI355X"


@functools.lru_cache(maxsize=None)
def _offline(T, S, N, seed, key, lam):
    """The table and every row of the LINEAR recording: msig_rn_sums, msig_rd_stats, msig_rn_windows — computed once."""
    _sig, dev = RL._recording(T, S, N, seed)
    cols, lib = COLS[key], L.lib()
    sums = torch.zeros((N, 2 * MC), dtype=torch.float64, device=DEV)
    table = torch.zeros((N, 2 * MC + 1), dtype=torch.float64, device=DEV)
    out = torch.empty((N, len(cols), T), dtype=torch.float32, device=DEV)
    L.check(lib.msig_rn_sums(*RL._head(dev, cols, T, S), 0, N, sums.data_ptr(), RL._stream()), "msig_rn_sums")
    L.check(lib.msig_rd_stats(*RL._head(dev, cols, T, S), sums.data_ptr(), N, lam, table.data_ptr(), RL._stream()), "msig_rd_stats")
    L.check(lib.msig_rn_windows(*RL._head(dev, cols, T, S), 0, N, table.data_ptr(), out.data_ptr(), RL._stream()), "msig_rn_windows")
    torch.cuda.synchronize()
    return table.cpu().numpy(), out.cpu().numpy()


class Pool(RL.Pool):
    """test_running_live_gpu's pool — rings of 0x5A, states of NaN, msig_rn_state_bytes(0) each — stepped by msig_rd_lv_step."""

    def __init__(self, T, S, Rn, key, lam):
        super().__init__(T, S, Rn, key, 0)
        self.lam = lam

    def step(self, rows, nxt=None):
        B = len(rows)
        table = torch.full((B + 1, 2 * MC + 1), float("nan"), dtype=torch.float64, device=DEV)
        nxt = nxt if nxt is not None else [self.next[k] for k, _n in rows]
        rc = L.lib().msig_rd_lv_step(*self.args(), *self.rows_args(), self.lam, self.state.data_ptr(), self.state.shape[1] * 8, *self._rows(rows),
                                     (C.c_int64 * B)(*nxt), B, table.data_ptr(), RL._stream())
        if rc == 0:
            for k, _n in rows:
                self.next[k] += 1
        return rc, table


@pytest.mark.parametrize("decay", list(DECAYS))
@pytest.mark.parametrize("ring", RL.RINGS)
@pytest.mark.parametrize("T,S,key", RL.SHAPES, ids=[f"t{T}-s{S}-{key}" for T, S, key in RL.SHAPES])
def test_live_tables_and_rows_are_the_offline_ones(T, S, key, ring, decay):
    from multimodalsignal_amd.runtime import Arenas
    lam = DECAYS[decay]
    Rn = {"t": T, "t+5": T + 5, "t+3s+1": T + 3 * S + 1}[ring]
    Cn = len(COLS[key])
    pool = Pool(T, S, Rn, key, lam)
    assert pool.state.shape[1] * 8 == L.lib().msig_rn_state_bytes(0)
    # slot -> the recordings it takes one after the other (windows, seed): slot 1 is closed after its first and reopened
    plan = {0: [(19, 11)], 1: [(8, 12), (9, 14)], 3: [(15, 13)]}
    cycle = {0: [3 * S + 1, 1, S, 1], 1: [S, 3 * S + 1, 1], 3: [1, 1, S, 3 * S + 1, S]}
    late = {0: 0, 1: 2, 3: 5}                                   # ticks before the session starts: out of phase
    cur, at, done = {k: 0 for k in plan}, {k: 0 for k in plan}, {k: 0 for k in plan}
    for k in plan:
        pool.open(k)
    arenas = Arenas(3, DEV, (("other", 1000), ("x", 24 * Cn * T * 4), ("tail", 256)))
    tick, mixed, longest, reopened, checked = 0, 0, 0, False, 0

    def rec(k):
        N, seed = plan[k][cur[k]]
        return N, seed, RL._recording(T, S, N, 100 * T + seed)[1]

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
                tab, out = _offline(T, S, N, 100 * T + seed, key, lam)
                assert np.array_equal(RL._selected(got[b], Cn).view(np.uint64), RL._selected(tab[w], Cn).view(np.uint64)), (tick, k, w)
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
            N, seed, dev = rec(k)
            if at[k] >= dev.shape[0]:
                assert done[k] == N
                st = pool.state[k].cpu().numpy()
                tab, _out = _offline(T, S, N, 100 * T + seed, key, lam)
                assert st[3 * MC] == N and st[3 * MC + 1] == 0 and st[3 * MC + 3] == lam          # the state knows where it stands,
                assert st[3 * MC + 2] == tab[N - 1, 2 * MC] and (lam < 1 or st[3 * MC + 2] == N)     # and c lives where the header says
                assert np.all(np.isnan(st[3 * MC + 4:]))                                           # the rest of the head is nobody's
                cur[k] += 1
                at[k], done[k] = 0, 0
                if cur[k] < len(plan[k]):
                    pool.open(k)                                # the same slot, its ring and its state as they were left
                    reopened = True
        tick += 1
    assert checked == 19 + 8 + 9 + 15 and mixed >= 3 and reopened
    assert longest >= (3 if ring == "t+3s+1" else 2 if ring == "t+5" else 1)
    assert torch.isnan(pool.state[2]).all()                     # nobody's state


def test_live_with_decay_one_is_the_expanding_step():
    """lambda = 1 live: msig_rn_lv_step(K = 0)'s records bit for bit, two windows in one step and one more after it."""
    T, S, key = 16, 4, "3of8"
    N, seed = 9, 21
    dev = RL._recording(T, S, N, seed)[1]
    tabs = []
    for pool in (Pool(T, S, T + 3 * S + 1, key, 1.0), RL.Pool(T, S, T + 3 * S + 1, key, 0)):
        pool.open(0)
        pool.push({0: dev[:T + S]})
        pool.book[0].advance(T + S)
        rc, t0 = pool.step([(0, 0), (0, 1)])
        assert rc == 0
        pool.push({0: dev[T + S:T + 2 * S]})
        pool.book[0].advance(S)
        rc, t1 = pool.step([(0, 2)])
        assert rc == 0
        torch.cuda.synchronize()
        tabs.append(np.concatenate([t0.cpu().numpy()[:2], t1.cpu().numpy()[:1]]))
    Cn = len(COLS[key])
    assert np.array_equal(RL._selected(tabs[0], Cn).view(np.uint64), RL._selected(tabs[1], Cn).view(np.uint64))
    assert list(tabs[0][:, 2 * MC]) == [1.0, 2.0, 3.0]


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_live_timeline_is_monitor_run_under_decayed():
    """Three sessions out of phase in chunks of 1, S and 3 S + 1 samples, one of them a single push, a slot closed and reopened:
    timelines_equal(LiveMonitor.timeline(sid), Monitor.run(the same samples)) under "decayed:5:2", the same meta — the reference
    string, warmup_windows and every window's real c_n — and session_stats = the offline table's last record."""
    from multimodalsignal_amd.live import timelines_equal
    from multimodalsignal_amd.monitor import RecordingWindows
    reference, H, W = "decayed:5:2", 5, 2
    T, S, M = 64, 16, 3
    models = LV.models("cnn_gru_attention", len(RL.CHANNELS), 2, M, DEV)
    recs = {k: RL._recording(T, S, N, seed) for k, N, seed in (("a", 40, 501), ("b", 33, 502), ("c", 37, 503), ("d", 21, 504))}
    live, mon = RL._monitors(models, reference)
    assert live.R == T + 8 * S and live.running == (0, W) and live.running.H == H and live.rn_state.shape[1] * 8 == L.lib().msig_rn_state_bytes(0)
    offline = {k: mon.run(recs[k][1], NAMES8) for k in recs}
    ups = {k: [] for k in recs}
    chunk = {"a": [1, S, 3 * S + 1], "b": [3 * S + 1, 1, S, S], "c": [10 ** 6]}
    late = {"a": 0, "b": 3, "c": 7}
    at = {k: 0 for k in chunk}
    for k in chunk:
        live.open(k, NAMES8)
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
    assert live.sessions["d"].slot == slot_b and live.session_stats("d") is None
    for i in range(0, recs["d"][1].shape[0], 2 * S + 3):
        ups["d"] += live.push("d", recs["d"][1][i:i + 2 * S + 3])
    lam = float(np.exp2(-1.0 / H))
    for k in ("a", "c", "d"):
        tl, want = live.timeline(k), offline[k]
        assert timelines_equal(tl, want), k
        assert tl.meta == want.meta
        N = len(want.t_end)
        assert want.meta["reference"] == reference and want.meta["warmup_windows"] == W and "reference_requested" not in want.meta
        counts = want.meta["reference_window_counts"]
        assert all(isinstance(v, float) for v in counts) and counts[0] == 1.0 and counts[1] == 1.0 + lam and len(counts) == N
        assert all(a < b < 1 / (1 - lam) for a, b in zip(counts, counts[1:]))
        assert list(want.warmup) == [n < W for n in range(N)] and [u.warmup for u in ups[k]] == [n < W for n in range(N)]
        rw = RecordingWindows(recs[k][1], NAMES8, RL.CHANNELS, T, S, reference)
        last = live.session_stats(k)
        torch.cuda.synchronize()
        Cn = len(RL.CHANNELS)
        assert rw.stats.shape == (N, 2 * MC + 1) and rw.running == (0, W) and rw.running.kind == "decayed"
        assert np.array_equal(RL._selected(last.cpu().numpy(), Cn).view(np.uint64), RL._selected(rw.stats[N - 1].cpu().numpy(), Cn).view(np.uint64))
    with pytest.raises(ValueError):
        live.open("e", NAMES8, stats=torch.zeros(2 * MC + 1, dtype=torch.float64, device=DEV))      # a running reference takes none
