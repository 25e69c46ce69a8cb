"""The host side of live monitoring (multimodalsignal_amd/live.py), without a GPU: the incremental smoother against monitor.ema at
every prefix, the alarm state machine against find_events(hysteresis(...)) of the whole sequence and against the restatement in
tests/lv_reference.py, and the ring bookkeeping against a sample-by-sample restatement."""
import numpy as np
import pytest

import lv_reference as R
from multimodalsignal_amd.live import AlarmMachine, RingBook, Smoother, alarms_of_events, build_parser, parse_args
from multimodalsignal_amd.monitor import _runs, ema, find_events, hysteresis


# ---- 1. the smoother -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("halflife", [0, 2, 3])
def test_smoother_gives_emas_bits_at_every_prefix(halflife):
    x = np.random.RandomState(11 + halflife).rand(200)
    sm, got = Smoother(halflife), []
    for n, v in enumerate(x):
        got.append(sm.push(v))
        assert np.array(got, dtype=np.float64).tobytes() == ema(x[:n + 1], halflife).tobytes(), n
    assert any(g != v for g, v in zip(got, x)) == (halflife != 0)
    with pytest.raises(ValueError):
        Smoother(-1)


# ---- 2. the alarms -------------------------------------------------------------------------------------------------------------------
def _live(x, on, off, min_on):
    m, flags, out = AlarmMachine(on, off, min_on), [], []
    for n, v in enumerate(x):
        flag, alarm = m.step(v)
        flags.append(flag)
        if alarm is not None:
            assert alarm.window == n
            out.append((alarm.kind, alarm.window, alarm.start_window))
    return flags, out


def _check(x, on, off, min_on):
    """The alarms of the sequence x correspond one to one with the offline events."""
    x = np.asarray(x, dtype=np.float64)
    flags, got = _live(x, on, off, min_on)
    state = hysteresis(x, on, off, min_on)
    t_end = np.arange(len(x), dtype=np.float64) * 10 + 60
    events = find_events(state, x, t_end)
    runs = _runs(state)
    assert len(events) == len(runs)
    onsets, offsets = [g for g in got if g[0] == "onset"], [g for g in got if g[0] == "offset"]
    assert [(w, a) for _k, w, a in onsets] == [(a + min_on - 1, a) for a, _b in runs]                     # one onset per offline event
    assert [(w, a) for _k, w, a in offsets] == [(b, a) for a, b in runs if b < len(x)]                    # one offset per event that ended
    assert [w for _k, w, _a in got] == sorted(w for _k, w, _a in got)
    assert got == alarms_of_events(state, min_on) == R.alarms(x, on, off, min_on)
    # `on` is the state from the onset on: the min_on - 1 windows before it are what a live system cannot know yet
    want = state.copy()
    for a, _b in runs:
        want[a:a + min_on - 1] = False
    assert flags == want.tolist()
    return got


def test_alarms_of_random_scores():
    rs = np.random.RandomState(3)
    seen = set()
    for trial in range(400):
        n, min_on = rs.randint(1, 80), rs.randint(1, 6)
        x = np.clip(0.5 + rs.choice([0.1, 0.25, 0.4]) * rs.randn(n), 0, 1)
        if trial % 3 == 0:
            x = ema(x, 2)
        got = _check(x, 0.6, 0.4, min_on)
        seen.update(k for k, _w, _a in got)
    assert seen == {"onset", "offset"}


H, M, Lo = 0.9, 0.5, 0.1          # above `on`, between the thresholds (the state holds), below `off`


def test_alarms_of_hand_made_scores():
    on, off = 0.6, 0.4
    assert _check([Lo, H, H, Lo, Lo], on, off, 3) == []                                                 # a run of exactly min_on - 1 windows
    assert _check([Lo, H, M, H, Lo, Lo], on, off, 3) == [("onset", 3, 1), ("offset", 4, 1)]             # exactly min_on; M holds the state
    assert _check([Lo, Lo, H, H, H], on, off, 2) == [("onset", 3, 2)]                                   # in progress when the stream stops
    assert _check([Lo, H, H, H, Lo], on, off, 2) == [("onset", 2, 1), ("offset", 4, 1)]                 # ends at the last window
    assert _check([Lo, Lo, Lo, H, H], on, off, 2) == [("onset", 4, 3)]                                  # reaches min_on at the last window
    assert _check([Lo, Lo, Lo, Lo, H], on, off, 2) == []                                                # min_on - 1 windows, still running
    assert _check([H, Lo, H, Lo, H, H, Lo], on, off, 1) == [("onset", 0, 0), ("offset", 1, 0), ("onset", 2, 2), ("offset", 3, 2), ("onset", 4, 4),
                                                            ("offset", 6, 4)]
    assert _check([H, Lo, H, Lo, H, H, Lo], on, off, 2) == [("onset", 5, 4), ("offset", 6, 4)]          # the dropped runs yield nothing
    assert _check([0.6, 0.4, 0.6], on, off, 1) == [("onset", 0, 0), ("offset", 1, 0), ("onset", 2, 2)]  # the thresholds are inclusive
    assert _check([], on, off, 2) == []
    with pytest.raises(ValueError):
        AlarmMachine(0.4, 0.6, 1)
    with pytest.raises(ValueError):
        AlarmMachine(0.6, 0.4, 0)


# ---- 3. the ring bookkeeping ---------------------------------------------------------------------------------------------------------
T_, S_, K_ = 200, 37, 7
HEAD = (K_ - 1) * S_ + T_            # 422
RING = HEAD + 41                     # 463


def _norm(plan):
    return [(a, due, list(w)) for a, due, w in plan]


@pytest.mark.parametrize("warm", [K_, 0])
@pytest.mark.parametrize("chunk", [0, 1, S_, RING + 1, 3 * RING + 5])
def test_bookkeeping_against_the_sample_by_sample_restatement(chunk, warm):
    """Chunk lengths 0, 1, exactly one stride and more than R, pushed until the ring has wrapped several times: the segments, where
    the statistics are due and which windows each segment completes."""
    book = RingBook(RING, T_, S_, warm)
    state = (0, 0, warm > 0)
    handed, stats_at = [], []
    for _ in range(3 if chunk == 0 else max(4, 4 * RING // chunk)):
        want, *state = R.bookkeeping(chunk, *state, RING, T_, S_, warm)
        got = _norm(book.plan(chunk))
        assert got == want
        assert (book.written, book.next_window, book.pending) == tuple(state)
        assert sum(a for a, _d, _w in got) == chunk and all(1 <= a <= RING for a, _d, _w in got)
        for a, due, w in got:
            handed += w
            if due:
                stats_at.append(book.written)
        if chunk <= RING - T_:
            assert len(got) == (1 if chunk else 0)                                # a chunk the ring can take is ONE append
    assert handed == list(range(R.count(book.written, T_, S_))) or (warm and book.written < HEAD and handed == [])
    assert len(stats_at) == (1 if warm and book.written >= HEAD else 0)


def test_the_split_at_the_head_span_and_at_r():
    book = RingBook(RING, T_, S_, K_)
    # one push far past the head: the first segment fills the ring without wrapping (the head lies at its start), the statistics are
    # due right after it, before the segment that wraps; it hands out the K warm-up windows and window 7 (7 * 37 + 200 = 459 <= 463)
    plan = _norm(book.plan(2000))
    assert plan[0] == (RING, True, list(range(8)))
    assert all(not due for _a, due, _w in plan[1:])
    # every later segment stops where it would overwrite the next window's first sample: 8 * 37 + 463 - 463 = 296
    assert plan[1] == (296, False, list(range(8, 16)))
    assert sum(a for a, _d, _w in plan) == 2000 and [w for _a, _d, ws in plan for w in ws] == list(range(R.count(2000, T_, S_)))
    # window by window: nothing before the head is complete, then all K at once
    book = RingBook(RING, T_, S_, K_)
    assert _norm(book.plan(HEAD - 1)) == [(HEAD - 1, False, [])]
    assert _norm(book.plan(1)) == [(1, True, list(range(K_)))]
    assert _norm(book.plan(S_ - 1)) == [(S_ - 1, False, [])] and _norm(book.plan(1)) == [(1, False, [K_])]
    assert _norm(book.plan(0)) == []
    # given statistics: window 0 as soon as it is complete
    book = RingBook(RING, T_, S_, 0)
    assert _norm(book.plan(T_)) == [(T_, False, [0])]
    # S > T: samples between two windows are appended and never read
    book = RingBook(1000, 200, 300, 0)
    plan = _norm(book.plan(5000))
    assert [w for _a, _d, ws in plan for w in ws] == list(range(R.count(5000, 200, 300)))
    assert plan == R.bookkeeping(5000, 0, 0, False, 1000, 200, 300, 0)[0]
    book = RingBook(250, 200, 300, 0)                # ... and an append never takes more than R rows, though none of them is needed
    plan = _norm(book.plan(5000))
    assert max(a for a, _d, _w in plan) == 250 and plan == R.bookkeeping(5000, 0, 0, False, 250, 200, 300, 0)[0]
    assert [w for _a, _d, ws in plan for w in ws] == list(range(R.count(5000, 200, 300)))
    # the smallest ring there is: R = T
    book = RingBook(T_, T_, S_, 0)
    assert [w for _a, _d, ws in book.plan(1000) for w in ws] == list(range(R.count(1000, T_, S_)))


def test_bookkeeping_refusals():
    with pytest.raises(ValueError):
        RingBook(HEAD - 1, T_, S_, K_)              # shorter than the head span
    with pytest.raises(ValueError):
        RingBook(T_ - 1, T_, S_, 0)                 # shorter than a window
    with pytest.raises(ValueError):
        RingBook(RING, T_, 0, 0)
    book = RingBook(RING, T_, S_, 0)
    with pytest.raises(ValueError):
        book.advance(RING + 1)                      # would overwrite window 0 before it is handed out


def test_the_command_lines_arguments():
    a = parse_args(["--run", "r", "--synthetic-recording", "--out", "o"])
    assert (a.reference, a.sessions, a.chunk_s, a.window_s, a.stride_s) == ("head:6", 1, 2.5, 60.0, 10.0)
    for bad in (["--reference", "recording"], ["--sessions", "0"], ["--chunk-s", "0"], ["--reference", "head:0"], ["--names", "x"]):
        with pytest.raises(SystemExit):
            parse_args(["--run", "r", "--synthetic-recording", "--out", "o"] + bad)
    assert build_parser().prog.endswith("live")
