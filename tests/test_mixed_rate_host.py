"""Mixed-rate streams, the parts that need no GPU (multimodalsignal_amd/resample.py, live.py, monitor.py):
MixedResampler on "cpu" — the column order, the per-stream numbers, the refusals —, the round planner `MixedBook` on integers
against a row-by-row brute force with seeded random arrivals over 700, 4, 32 and 64 Hz, the two ring sizes of the real-time
simulation, and the command line's --streams."""
import math

import numpy as np
import pytest

from multimodalsignal_amd import _lib as L
from multimodalsignal_amd import live, monitor, synth
from multimodalsignal_amd.live import MixedBook, MixedStuck, RingBook
from multimodalsignal_amd.resample import FirResampler, MixedResampler, Stream, out_count, parse_streams

FS = 64.0
RATES = (700, 4, 32, 64)
SHAPES = [(256, 64, 7), (200, 37, 0), (256, 64, 0)]


def _four(device="cpu"):
    return MixedResampler([Stream("chest", 700, ["chest_ECG", "chest_EDA", "chest_Resp", "chest_EMG"]), Stream("eda", 4, ["wrist_EDA", "wrist_TEMP"]),
                           Stream("acc", 32, ["wrist_ACC"]), Stream("bvp", 64, ["wrist_BVP"])], FS, device=device)


# ---- MixedResampler on the host -------------------------------------------------------------------------------------------------------
def test_mixed_resampler_on_cpu_orders_columns_and_keeps_the_streams_apart():
    mx = _four()
    assert mx.names == ["chest_ECG", "chest_EDA", "chest_Resp", "chest_EMG", "wrist_EDA", "wrist_TEMP", "wrist_ACC", "wrist_BVP"] and mx.C_all == 8
    assert [g.name for g in mx.streams] == ["chest", "eda", "acc", "bvp"] and mx.stream["acc"] is mx.streams[2]
    assert [(g.col0, g.ncols) for g in mx.streams] == [(0, 4), (4, 2), (6, 1), (7, 1)]
    got = {g.name: (g.L, g.M, g.half, g.tail_rows, g.latency_s) for g in mx.streams}
    assert got == {"chest": (16, 175, 1750, 219, 110 / 700), "eda": (16, 1, 160, 21, 2.75), "acc": (2, 1, 20, 21, 0.34375), "bvp": (1, 1, 0, 0, 0)}
    assert abs(got["chest"][4] - 0.157) < 5e-4
    for g in mx.streams[:3]:                                          # a resampled stream is FirResampler's, number for number and tap for tap
        r = FirResampler(g.fs, FS, "cpu")
        assert (g.L, g.M, g.half, g.tail_rows, g.latency_s) == (r.L, r.M, r.half, r.tail_rows, r.latency_s)
        assert mx.taps[g.h_off:g.h_off + 2 * g.half + 1].tobytes() == r.taps.tobytes()
        assert [g.out_count(n) for n in (0, 1, 5, 219, 220, 5000)] == [r.out_count(n) for n in (0, 1, 5, 219, 220, 5000)]
        assert [g.max_rows(k) for k in (0, 1, 17, 400)] == [r.max_rows(k) for k in (0, 1, 17, 400)]
    same = mx.stream["bvp"]
    assert [same.out_count(n) for n in (0, 1, 2, 77)] == [0, 1, 2, 77] and [same.max_rows(k) for k in (0, 1, 77)] == [0, 1, 77]
    # the tap ranges and the tail ranges lie side by side: none overlaps another, the identity has neither
    taps = [(g.h_off, g.h_off + 2 * g.half + 1) for g in mx.streams[:3]]
    tails = [(g.tail_off, g.tail_off + g.tail_rows * g.ncols) for g in mx.streams[:3]]
    for spans, end in ((taps, len(mx.taps)), (tails, mx.tail_doubles)):
        assert spans[0][0] == 0 and all(a[1] == b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= end
    assert tails == [(0, 219 * 4), (876, 876 + 42), (918, 939)] and mx.tail_doubles == 939
    assert mx.latency_s == 2.75 and mx.latency_spread_rows == 176 == math.ceil((2.75 - 0.0) * 64)
    two = MixedResampler([Stream("chest", 700, ["a"]), Stream("acc", 32, ["b"])], FS, device="cpu")
    assert two.latency_spread_rows == math.ceil((0.34375 - 110 / 700) * 64) == 12 and two.latency_s == 0.34375
    n = {"chest": 7000, "eda": 40, "acc": 333, "bvp": 480}
    each = [out_count(7000, 16, 175, 1750), out_count(40, 16, 1, 160), out_count(333, 2, 1, 20), 480]
    assert mx.out_count(n) == min(each) == 480 and mx.out_count(dict(n, eda=20)) == out_count(20, 16, 1, 160) == 160
    assert all(g.name in mx.spelling for g in mx.streams) and "700" in mx.spelling and "16/175" in mx.spelling and "copy" in mx.spelling
    g = mx.streams[1].group()
    assert (g.L, g.M, g.half, g.col0, g.ncols, g.h_off, g.tail_rows, g.tail_off) == (16, 1, 160, 4, 2, 3501, 21, 876)
    table = mx.groups()
    assert len(table) == 4 and (table[3].L, table[3].M, table[3].half, table[3].tail_rows) == (1, 1, 0, 0)


def test_mixed_resampler_refuses():
    ok = [Stream("a", 700, ["x", "y"]), Stream("b", 4, ["z"])]
    MixedResampler(ok, FS, device="cpu")
    with pytest.raises(ValueError, match="more than once"):
        MixedResampler([Stream("a", 700, ["x", "y"]), Stream("b", 4, ["y"])], FS, device="cpu")          # a column in two streams
    with pytest.raises(ValueError, match="more than once"):
        MixedResampler([Stream("a", 700, ["x", "x"])], FS, device="cpu")
    with pytest.raises(ValueError, match="unique"):
        MixedResampler([Stream("a", 700, ["x"]), Stream("a", 4, ["z"])], FS, device="cpu")               # a stream name twice
    with pytest.raises(ValueError):
        MixedResampler([Stream(f"s{i}", 4, [f"c{i}"]) for i in range(9)], FS, device="cpu")              # nine streams
    MixedResampler([Stream(f"s{i}", 4, [f"c{i}"]) for i in range(8)], FS, device="cpu")
    with pytest.raises(ValueError):
        MixedResampler([], FS, device="cpu")
    with pytest.raises(ValueError, match=str(L.RS_MAX_RATIO)):
        MixedResampler([Stream("a", 700, ["x"]), Stream("b", 64.0 * 4097, ["z"])], FS, device="cpu")     # 1 / 4097
    with pytest.raises(ValueError):
        MixedResampler(ok, FS, device="cpu", half_width=0)
    for bad in (("", 4, ["x"]), ("a", 0, ["x"]), ("a", "fast", ["x"]), ("a", 4, []), ("a", 4, "x")):
        with pytest.raises(ValueError):
            Stream(*bad)
    mx = MixedResampler(ok, FS, device="cpu")
    with pytest.raises(ValueError):
        mx.out_count({"a": 5})                                        # every stream has a count
    with pytest.raises(ValueError):
        mx.apply({"a": np.zeros((5, 2)), "b": np.zeros(5)})           # no CPU fallback


# ---- the round planner ----------------------------------------------------------------------------------------------------------------
def _ratios():
    return [(g.L, g.M, g.half) for g in _four().streams]


def _brute(mb, waiting):
    """The call row by row, on plain integers: a stream takes one raw row whenever the outputs it then has stay at or below
    next_window * S + R — no ring slot that a window not yet handed out needs (or, while the statistics are pending, that the unwrapped
    head needs) is overwritten — and after every row the statistics and the complete windows are taken.  Returns (stuck, raw,
    written, next_window, pending, windows handed out): stuck = rows are left and no stream can take one."""
    b, ratios = mb.book, mb.ratios
    raw, left = list(mb.raw), list(waiting)
    written, nw, pending, handed = b.written, b.next_window, b.pending, []
    moved = True
    while moved:
        moved = False
        for g, (up, down, half) in enumerate(ratios):
            while left[g] and out_count(raw[g] + 1, up, down, half) <= nw * b.S + b.R:
                raw[g], left[g], moved = raw[g] + 1, left[g] - 1, True
                written = min(out_count(raw[k], *ratios[k]) for k in range(len(ratios)))
                if pending and written >= b.head:
                    pending = False
                while not pending and nw * b.S + b.T <= written:
                    handed.append(nw)
                    nw += 1
    return any(left), raw, written, nw, pending, handed


@pytest.mark.parametrize("T,S,warm", SHAPES, ids=[f"t{T}-s{S}-warm{w}" for T, S, w in SHAPES])
def test_planner_against_the_row_by_row_brute_force(T, S, warm):
    """Seeded random arrivals over 700, 4, 32 and 64 Hz into the default ring (head + 8 S + latency spread): each call delivers some
    streams a random stretch, so streams run ahead and fall behind by up to tens of seconds.  Per round: no stream's output count passes
    next_window * S + R, nothing wraps while the statistics are pending, a window is handed out once, in order, and only when every
    stream covers it.  Per call: the planner raises exactly when the brute force is stuck, and then nothing has changed; otherwise
    both end in the same state."""
    ratios = _ratios()
    head = (warm - 1) * S + T if warm else T
    R = head + 8 * S + 176
    mb = MixedBook(RingBook(R, T, S, warm), ratios)
    rs = np.random.RandomState(T + S + warm)
    sent = [0.0] * 4                                                  # seconds delivered per stream
    handed, raised, finished, due_seen = [], 0, 0, 0
    for call in range(400):
        waiting = [0] * 4
        lag = min(range(4), key=lambda g: sent[g])
        for g in range(4):
            if rs.rand() < (0.9 if g == lag else 0.5):
                sec = float(rs.choice([0.02, 0.25, 1.0, 2.5, 7.0]))
                waiting[g] = int(round((sent[g] + sec) * RATES[g])) - int(round(sent[g] * RATES[g]))
        stuck, raw, written, nw, pending, wins = _brute(mb, waiting)
        before = (list(mb.raw), mb.book.written, mb.book.next_window, mb.book.pending)
        if stuck:
            with pytest.raises(MixedStuck) as e:
                mb.plan(waiting)
            assert waiting[e.value.ahead] > 0 and e.value.lead_rows > 0 and e.value.need_rows > R
            with pytest.raises(ValueError):
                mb.push(waiting)
            assert (list(mb.raw), mb.book.written, mb.book.next_window, mb.book.pending) == before
            raised += 1
            continue
        rounds = mb.plan(waiting)
        assert (list(mb.raw), mb.book.written, mb.book.next_window, mb.book.pending) == before          # a plan changes nothing
        for take, due, windows in rounds:
            was_pending, bound = mb.book.pending, mb.book.next_window * S + R
            assert any(take) and all(0 <= a for a in take)
            assert mb.apply(take) == (due, windows)
            counts = mb.counts()
            assert max(counts) <= bound and mb.book.written == min(counts)
            if was_pending:
                assert max(counts) <= R                              # the head span lies unwrapped when the statistics are taken
            due_seen += due
            for w in windows:
                assert w * S + T <= min(counts)
            handed += list(windows)
        assert [mb.raw[g] - before[0][g] for g in range(4)] == waiting
        assert (list(mb.raw), mb.book.written, mb.book.next_window, mb.book.pending) == (raw, written, nw, pending)
        assert [w for _t, _d, ws in rounds for w in ws] == wins
        for g in range(4):
            sent[g] += waiting[g] / RATES[g]
        finished += 1
        if call % 16:
            continue
        room = [mb.room(g) for g in range(4)]                         # room: exactly what a stream can take alone
        for g in range(4):
            alone = [room[g] if k == g else 0 for k in range(4)]
            assert not _brute(mb, alone)[0]
            alone[g] += 1
            assert _brute(mb, alone)[0]
    assert handed == list(range(len(handed))) and len(handed) > 100
    assert raised > 10 and finished > 100 and due_seen == (1 if warm else 0)
    assert mb.book.written > 3 * R                                   # every ring wrapped several times


def _real_time(R, jitter_s, seconds, seed=0, T=256, S=64, warm=7):
    """Four devices sampled in real time and polled together: the calls come at random intervals of up to `jitter_s` seconds beyond
    0.25 s (jitter_s = 0: every 0.25 s), each delivering what every stream has sampled by then.  Returns the seconds after which a
    call was refused, or None."""
    mb = MixedBook(RingBook(R, T, S, warm), _ratios())
    rs = np.random.RandomState(seed)
    t, got = 0.0, [0] * 4
    while t < seconds:
        t += 0.25 + jitter_s * rs.rand()
        now = [int(t * f) for f in RATES]
        try:
            mb.push([n - g for n, g in zip(now, got)])
        except MixedStuck:
            return t
        got = now
    assert mb.book.next_window > 0
    return None


def test_ring_of_the_real_time_simulation():
    """head:7, T = 256, S = 64: the head span is 640 rows.  With the streams arriving in real time a ring of head + 41 rows gets stuck
    — the 4 Hz stream's outputs trail the others by its 2.75 s, 176 rows, so the 700 Hz stream fills the ring before the 4 Hz stream
    has completed the head — and the same ring plus latency_spread_rows does not, with up to 1 s of arrival jitter."""
    head = 6 * 64 + 256
    assert _four().latency_spread_rows == 176
    assert _real_time(head + 41, 0.0, 60.0) is not None
    for seed in range(5):
        assert _real_time(head + 41 + 176, 0.0 if seed == 0 else 1.0, 180.0, seed) is None


def test_mixed_book_with_one_stream_is_the_ring_book():
    """One stream: never stuck, and the windows are RingBook's own."""
    for ratio in ((16, 175, 1750), (1, 1, 0)):
        mb, rb = MixedBook(RingBook(700, 256, 64, 7), [ratio]), RingBook(700, 256, 64, 7)
        rs = np.random.RandomState(3)
        for _ in range(60):
            n = int(rs.choice([1, 50, 700, 9000]))
            wins = [w for _t, _d, ws in mb.push([n]) for w in ws]
            before = out_count(mb.raw[0] - n, *ratio)
            assert wins == [w for _a, _d, ws in rb.plan(out_count(mb.raw[0], *ratio) - before) for w in ws]
        assert mb.room(0) == (1 << 31) - 1 and mb.book.written == rb.written > 3 * 700
    with pytest.raises(ValueError):
        MixedBook(RingBook(700, 256, 64, 7), [])
    with pytest.raises(ValueError):
        MixedBook(RingBook(700, 256, 64, 7), _ratios()).plan([1, 2, 3])


# ---- the command line -----------------------------------------------------------------------------------------------------------------
SPEC = "chest=700:chest_ECG,chest_EDA,chest_Resp,chest_EMG;bvp=64:wrist_BVP;eda=4:wrist_EDA"


def test_parse_streams():
    got = parse_streams(SPEC)
    assert [(s.name, s.fs, s.columns) for s in got] == [("chest", 700.0, ["chest_ECG", "chest_EDA", "chest_Resp", "chest_EMG"]),
                                                        ("bvp", 64.0, ["wrist_BVP"]), ("eda", 4.0, ["wrist_EDA"])]
    assert [(s.name, s.fs, s.columns) for s in parse_streams(" a = 0.5 : x , y ")] == [("a", 0.5, ["x", "y"])]
    for bad in ("", "a", "a=4", "a=4:", "=4:x", "a=fast:x", "a=4:x;", "a=0:x", "a=4:x,,y"):
        with pytest.raises(ValueError):
            parse_streams(bad)


@pytest.mark.parametrize("mod", [monitor, live], ids=["monitor", "live"])
def test_cli_streams(mod, tmp_path, capsys):
    base = ["--run", str(tmp_path), "--out", str(tmp_path / "o")]
    a = mod.parse_args(base + ["--synthetic-recording", "--streams", SPEC])
    assert [s.name for s in a.streams] == ["chest", "bvp", "eda"] and a.resample_from is None
    assert mod.parse_args(base + ["--synthetic-recording"]).streams is None
    a = mod.parse_args(base + ["--recording", str(tmp_path / "x.npz"), "--streams", SPEC])      # the arrays are keyed by stream: no --names
    assert a.names is None and len(a.streams) == 3
    a = mod.parse_args(base + ["--synthetic-recording", "--streams", SPEC, "--reference", "expanding", "--gaps", "--synthetic-gaps",
                               "drop=0.001,stream=eda:100:9,stream=bvp:5:1"])
    assert a.gaps is not None
    refused = [["--synthetic-recording", "--streams", SPEC, "--resample-from", "700"],
               ["--synthetic-recording", "--streams", SPEC, "--resample-from", "700", "--resampler", "fir"],
               ["--recording", str(tmp_path / "x.npz"), "--streams", SPEC, "--names", str(tmp_path / "n.txt")],
               ["--synthetic-recording", "--streams", "chest=700:chest_ECG;bvp=64:chest_ECG"],          # a column twice
               ["--synthetic-recording", "--streams", "chest=700:chest_ECG;chest=64:wrist_BVP"],        # a name twice
               ["--synthetic-recording", "--streams", "chest=700:chest_ECG;bvp=64.0001:wrist_BVP"],     # no exact ratio within 4096
               ["--synthetic-recording", "--streams", "chest=700:chest_ECG,nothing"],                   # not a synthetic channel
               ["--synthetic-recording", "--streams", "chest=700"],
               ["--synthetic-recording", "--streams", SPEC, "--reference", "expanding", "--gaps", "--synthetic-gaps", "stream=wrist:100:9"],
               ["--synthetic-recording", "--reference", "expanding", "--gaps", "--synthetic-gaps", "stream=eda:100:9"]]      # no --streams
    for extra in refused:
        with pytest.raises(SystemExit):
            mod.parse_args(base + extra)
    capsys.readouterr()


def test_synthetic_streams_share_the_planted_effects():
    """The generator draws a recording's noise before its per-block levels, so those draws differ between rates too; what is planted
    per protocol phase — the stress terms — and the subject's gain and offset are the same at every rate."""
    phases = [(1, 60.0), (2, 60.0)]
    streams = parse_streams(SPEC)
    got, table = synth.make_synthetic_streams(phases, streams, seed=3)
    assert {k: v.shape for k, v in got.items()} == {"chest": (84000, 4), "bvp": (7680, 1), "eda": (480, 1)}
    assert [(r["label"], r["start"], r["end"], r["start_s"], r["end_s"]) for r in table] == [(1, 0, 3840, 0.0, 60.0), (2, 3840, 7680, 60.0, 120.0)]
    for st in streams:                                                # a stream is its columns of the recording at its rate
        whole, _t = synth.make_synthetic_recording(phases, fs=st.fs, seed=3)
        assert got[st.name].tobytes() == np.ascontiguousarray(whole[:, [synth.CHANNELS6.index(c) for c in st.columns]]).tobytes()
    # the planted stress effect on the EDA level (column 1 of the recording) is there at both rates: ten blocks a phase, so the blocks'
    # own draws (0.35 a block) average out against the planted 0.5 and the ramp
    long = [(1, 600.0), (2, 600.0)]
    other, _t = synth.make_synthetic_streams(long, [Stream("slow", 4, ["chest_EDA"]), Stream("fast", 64, ["chest_ECG"])], seed=3)
    again, _t = synth.make_synthetic_streams(long, [Stream("slow", 64, ["chest_EDA"])], seed=3)
    rise = lambda x: x[len(x) // 2:].mean() - x[:len(x) // 2].mean()      # noqa: E731
    slow, fast = rise(other["slow"][:, 0]), rise(again["slow"][:, 0])
    assert slow > 0.25 and fast > 0.25 and abs(slow - fast) < 0.5 * max(slow, fast)
    gapped, _t = synth.make_synthetic_streams(phases, streams, seed=3, gaps="stream=eda:10:9,all=100:2")
    assert np.isnan(gapped["eda"][40:76]).all() and np.isnan(gapped["eda"][400:408]).all() and np.isnan(gapped["eda"]).sum() == 36 + 8
    assert np.isnan(gapped["chest"]).sum() == 1400 * 4 and np.isnan(gapped["bvp"]).sum() == 128
    keep = ~np.isnan(gapped["eda"])
    assert np.array_equal(gapped["eda"][keep], got["eda"][keep])
    assert synth.gap_spans("stream=eda:10:9,all=100:2", 4.0, 480, stream="eda") == [(40, 76), (400, 408)]
    assert synth.gap_spans("stream=eda:10:9,all=100:2", 4.0, 480) == [(400, 408)] == synth.gap_spans("stream=eda:10:9,all=100:2", 4.0, 480, stream="bvp")
    with pytest.raises(ValueError):
        synth.make_synthetic_streams(phases, streams, gaps="stream=wrist:10:9")
    with pytest.raises(ValueError):
        synth.make_synthetic_recording(phases, fs=8.0, gaps="stream=eda:10:9")      # a single-rate recording has no streams
    with pytest.raises(ValueError):
        synth.make_synthetic_streams(phases, [Stream("a", 4, ["nothing"])])
