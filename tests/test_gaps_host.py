"""Gap-tolerant monitoring, the parts that need no GPU (multimodalsignal_amd/reference.py, monitor.py, live.py, synth.py; DESIGN.md
section 38): the Gaps policy and its parsing, the refusals, ema_gaps / hysteresis_gaps against tests/gp_reference.py's restatement,
the all-valid anchor as raw bits, the live smoother and alarm machine against the offline vectors, Timeline's files with and without
gaps, the planted gaps of the synthetic recording, and the restatement's own standing inside the statistics yardstick."""
import json

import numpy as np
import pytest

import gp_reference as G
from multimodalsignal_amd import live, monitor, synth
from multimodalsignal_amd.reference import Gaps, gp_mode_fields, parse_gaps, parse_running


# ---- the policy --------------------------------------------------------------------------------------------------------------------
def test_gaps_defaults_parsing_and_refusals():
    assert (Gaps().min_coverage, Gaps().lost_after) == (0.75, 6) and Gaps() == parse_gaps("") == parse_gaps(None) and monitor.Gaps is Gaps
    assert parse_gaps("0.5") == Gaps(0.5, 6) and parse_gaps("0.5:3") == Gaps(0.5, 3) and parse_gaps("0:1") == Gaps(0.0, 1) and parse_gaps("1") == Gaps(1.0)
    assert parse_gaps(Gaps(0.6, 4).spelling) == Gaps(0.6, 4)
    for bad in ("x", "0.5:", "0.5:0", "0.5:-1", "0.5:2.5", "1.5", "-0.1", "nan", "inf", "0.5:3:1", ":3"):
        with pytest.raises(ValueError):
            parse_gaps(bad)
    for args in ((-0.1, 6), (1.1, 6), (float("nan"), 6), ("0.5", 6), (True, 6), (0.5, 0), (0.5, 2.5), (0.5, True), (0.5, "3")):
        with pytest.raises(ValueError):
            Gaps(*args)
    cov = np.array([[1.0, 0.75], [1.0, 0.7499], [0.0, 0.0]])
    assert list(Gaps(0.75).valid(cov)) == [True, False, False] and list(Gaps(0.0).valid(cov)) == [True, True, True]      # 0 never invalidates
    assert gp_mode_fields(parse_running("expanding")) == (0, 0, 0.0) and gp_mode_fields(parse_running("trailing:7:2")) == (1, 7, 0.0)
    assert gp_mode_fields(parse_running("decayed:3")) == (2, 0, float(np.exp2(-1.0 / 3))) and gp_mode_fields(None) == (0, 0, 0.0)


@pytest.mark.parametrize("reference", ["recording", "head:6", (0, 3)])
def test_monitors_refuse_gaps_under_a_reference_without_a_per_channel_count(reference):
    """Refused with one sentence before any model or GPU is touched."""
    with pytest.raises(ValueError, match="gaps need a running reference"):
        monitor.Monitor([], 64.0, reference=reference, gaps=Gaps())
    if isinstance(reference, str) and reference != "recording":
        with pytest.raises(ValueError, match="a live monitor with gaps takes a running reference"):
            live.LiveMonitor([], 64.0, reference=reference, gaps=Gaps())
    with pytest.raises(ValueError, match="gaps is a Gaps"):
        monitor.Monitor([], 64.0, reference="expanding", gaps=(0.75, 6))
    with pytest.raises(ValueError, match="gaps is a Gaps"):
        live.LiveMonitor([], 64.0, reference="expanding", gaps="0.75")


def test_command_lines_check_gaps_before_the_gpu(capsys):
    base = ["--run", "nowhere", "--synthetic-recording", "--out", "o"]
    a = monitor.parse_args(base + ["--reference", "expanding", "--gaps"])
    assert a.gaps == Gaps() and a.synthetic_gaps is None
    a = monitor.parse_args(base + ["--reference", "decayed:60", "--gaps", "0.5:3", "--synthetic-gaps", "drop=0.05,all=100:70"])
    assert a.gaps == Gaps(0.5, 3) and a.synthetic_gaps == "drop=0.05,all=100:70"
    assert monitor.parse_args(base).gaps is None and live.parse_args(base).gaps is None
    assert live.parse_args(base + ["--reference", "trailing:9", "--gaps", "0.9"]).gaps == Gaps(0.9)
    assert live.parse_args(base + ["--reference", "auto", "--gaps"]).gaps == Gaps()
    for mod, extra in ((monitor, ["--gaps"]), (monitor, ["--reference", "head:6", "--gaps"]), (live, ["--gaps"]),
                       (monitor, ["--reference", "expanding", "--gaps", "2"]), (monitor, ["--reference", "expanding", "--synthetic-gaps", "drop=2"]),
                       (live, ["--reference", "expanding", "--gaps", "0.5:x"])):
        with pytest.raises(SystemExit):
            mod.parse_args(base + extra)
    with pytest.raises(SystemExit):
        monitor.parse_args(["--run", "nowhere", "--recording", "x.npy", "--names", "n", "--out", "o", "--synthetic-gaps", "drop=0.1"])
    assert "gaps need a running reference" in capsys.readouterr().err


# ---- the smoother and the state machine ----------------------------------------------------------------------------------------------
def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _random_case(rs):
    N = int(rs.randint(1, 60))
    score = rs.rand(N)
    p = rs.choice([0.0, 0.1, 0.4, 0.8])
    valid = rs.rand(N) >= p
    if rs.rand() < 0.3 and N > 8:                     # a long invalid stretch
        a = int(rs.randint(0, N - 4))
        valid[a:a + int(rs.randint(2, 12))] = False
    return score, valid, float(rs.choice([0, 0.5, 1, 3, 7.5])), int(rs.randint(1, 7)), int(rs.randint(1, 5))


def test_ema_gaps_and_hysteresis_gaps_against_the_restatement_on_400_random_sequences():
    rs = np.random.RandomState(38)
    for _ in range(400):
        score, valid, halflife, lost_after, min_on = _random_case(rs)
        sm = monitor.ema_gaps(score, valid, halflife, lost_after)
        assert np.array_equal(_bits(sm), _bits(G.ema_gaps(score, valid, halflife, lost_after)))
        st = monitor.hysteresis_gaps(sm, valid, 0.6, 0.4, min_on, lost_after)
        assert st.dtype == bool and np.array_equal(st, G.hysteresis_gaps(sm, valid, 0.6, 0.4, min_on, lost_after))
        assert np.array_equal(monitor.lost_windows(valid, lost_after), G.lost(valid, lost_after))
        assert not st[G.lost(valid, lost_after)].any()                    # a lost window is never on


def _hand(valid_runs, hi=0.9, lo=0.1):
    """valid flags from a run-length list [(valid?, length), ...]; the score is `hi` everywhere."""
    valid = np.concatenate([np.full(n, v, dtype=bool) for v, n in valid_runs])
    return np.full(valid.size, hi), valid


@pytest.mark.parametrize("lost_after", [1, 3, 6])
def test_hand_made_sequences(lost_after):
    K = lost_after
    # on, then an invalid run of K - 1: the state holds through it, nothing is lost, the smoother goes on where it stood
    score, valid = _hand([(True, 4), (False, K - 1), (True, 3)])
    score[4 + K - 1:] = 0.5
    sm = monitor.ema_gaps(score, valid, 2, K)
    st = monitor.hysteresis_gaps(sm, valid, 0.6, 0.4, 1, K)
    assert not monitor.lost_windows(valid, K).any() and st[:4 + K - 1].all()
    assert np.all(sm[4:4 + K - 1] == sm[3]) and sm[4 + K - 1] == sm[3] + (1.0 - 2.0 ** -0.5) * (0.5 - sm[3])
    # a run of exactly K: lost at its last window, the state forced off there, and the smoother restarts at the next valid window
    score, valid = _hand([(True, 4), (False, K), (True, 3)])
    score[4 + K:] = [0.5, 0.7, 0.7]
    sm = monitor.ema_gaps(score, valid, 2, K)
    st = monitor.hysteresis_gaps(sm, valid, 0.6, 0.4, 1, K)
    lost = monitor.lost_windows(valid, K)
    assert list(np.flatnonzero(lost)) == [4 + K - 1] and st[:4 + K - 1].all() and not st[4 + K - 1] and sm[4 + K] == 0.5 and not st[4 + K]
    assert sm[4 + K - 1] == sm[3]                                         # held, reported, and off
    # a run that ends at the last window
    score, valid = _hand([(True, 3), (False, K + 2)])
    sm, lost = monitor.ema_gaps(score, valid, 2, K), monitor.lost_windows(valid, K)
    st = monitor.hysteresis_gaps(sm, valid, 0.6, 0.4, 1, K)
    assert list(np.flatnonzero(lost)) == list(range(3 + K - 1, 3 + K + 2)) and st[:3 + K - 1].all() and not st[3 + K - 1:].any()
    # invalid from window 0: smoothed 0.0 and off before the first valid window, which starts the smoother as window 0 would
    score, valid = _hand([(False, K + 1), (True, 2)])
    sm = monitor.ema_gaps(score, valid, 2, K)
    st = monitor.hysteresis_gaps(sm, valid, 0.6, 0.4, 1, K)
    assert np.all(sm[:K + 1] == 0.0) and sm[K + 1] == 0.9 and not st[:K + 1].any() and st[K + 1:].all()
    assert list(np.flatnonzero(monitor.lost_windows(valid, K))) == list(range(K - 1, K + 1))
    # a run that starts while on, with min_on = 3: the episode counts its held windows, and is dropped when the loss cuts it short
    score, valid = _hand([(True, 1), (False, K + 1), (True, 1)])
    st = monitor.hysteresis_gaps(monitor.ema_gaps(score, valid, 0, K), valid, 0.6, 0.4, 3, K)
    assert list(st) == ([True] * K + [False] * 3 if K >= 3 else [False] * (K + 3))
    # and the restatement says the same of all five
    for runs in ([(True, 4), (False, K - 1), (True, 3)], [(True, 4), (False, K), (True, 3)], [(True, 3), (False, K + 2)], [(False, K + 1), (True, 2)],
                 [(True, 1), (False, K + 1), (True, 1)]):
        score, valid = _hand(runs)
        sm = monitor.ema_gaps(score, valid, 2, K)
        assert np.array_equal(_bits(sm), _bits(G.ema_gaps(score, valid, 2, K)))
        for min_on in (1, 3):
            assert np.array_equal(monitor.hysteresis_gaps(sm, valid, 0.6, 0.4, min_on, K), G.hysteresis_gaps(sm, valid, 0.6, 0.4, min_on, K))


def test_all_valid_is_ema_and_hysteresis_as_raw_bits():
    rs = np.random.RandomState(5)
    for N in (0, 1, 2, 37, 200):
        score, ok = rs.rand(N), np.ones(N, dtype=bool)
        for halflife in (0, 0.5, 3, 40):
            sm, want = monitor.ema_gaps(score, ok, halflife, 6), monitor.ema(score, halflife)
            assert sm.dtype == want.dtype and sm.tobytes() == want.tobytes()
            for min_on in (1, 2, 5):
                st, ws = monitor.hysteresis_gaps(sm, ok, 0.6, 0.4, min_on, 1), monitor.hysteresis(want, 0.6, 0.4, min_on)
                assert st.dtype == ws.dtype and st.tobytes() == ws.tobytes()
    with pytest.raises(ValueError):
        monitor.ema_gaps([0.1, 0.2], [True], 3, 6)
    with pytest.raises(ValueError):
        monitor.hysteresis_gaps([0.1], [True], 0.4, 0.6, 1, 6)
    with pytest.raises(ValueError):
        monitor.lost_windows([True], 0)


def test_live_smoother_and_alarms_against_the_offline_vectors():
    """GapSmoother and GapAlarmMachine, one window at a time, against ema_gaps / hysteresis_gaps of the whole vectors, against
    alarms_of_gaps and against the restatement's alarms: lost, back and the forced offset included."""
    rs = np.random.RandomState(77)
    kinds = set()
    for _ in range(400):
        score, valid, halflife, lost_after, min_on = _random_case(rs)
        smoother, machine = live.GapSmoother(halflife, lost_after), live.GapAlarmMachine(0.6, 0.4, min_on, lost_after)
        sm, on, raised = [], [], []
        for v, ok in zip(score, valid):
            sm.append(smoother.push(v, bool(ok)))
            o, al = machine.step(sm[-1], bool(ok))
            on.append(o)
            raised += [(a.kind, a.window, a.start_window) for a in al]
        want_sm = monitor.ema_gaps(score, valid, halflife, lost_after)
        assert np.array_equal(_bits(sm), _bits(want_sm))
        state = monitor.hysteresis_gaps(want_sm, valid, 0.6, 0.4, min_on, lost_after)
        assert raised == live.alarms_of_gaps(state, valid, lost_after, min_on) == G.alarms(want_sm, valid, 0.6, 0.4, min_on, lost_after)
        a = np.array(on, dtype=bool)                  # `on`: the offline state from the window of the onset on
        for s0, s1 in monitor._runs(state):
            assert a[s0 + min_on - 1:s1].all() and not a[s0:s0 + min_on - 1].any()
        assert not a[~state].any()
        kinds |= {k for k, _w, _s in raised}
    assert kinds == {"onset", "offset", "lost", "back"}
    # the forced offset: on for 4 windows, then lost — offset and lost at the same window, in that order; back with the next sample
    machine, got = live.GapAlarmMachine(0.6, 0.4, 2, 3), []
    for n, (v, ok) in enumerate([(0.9, True)] * 4 + [(0.9, False)] * 4 + [(0.9, True)] * 2):
        got += [(a.kind, a.window, a.start_window) for a in machine.step(v, ok)[1]]
    assert got == [("onset", 1, 0), ("offset", 6, 0), ("lost", 6, 4), ("back", 8, 4), ("onset", 9, 8)]


# ---- the timeline's files ------------------------------------------------------------------------------------------------------------
def _timeline(gaps):
    N, rs = 5, np.random.RandomState(1)
    z = dict(t_end=np.arange(N) + 1.0, mean_p=rs.rand(N, 2).astype(np.float32), std_p=rs.rand(N, 2).astype(np.float32), pred=np.zeros(N, dtype=np.int32),
             entropy=rs.rand(N).astype(np.float32), mutual_info=rs.rand(N).astype(np.float32), votes=np.zeros((N, 2), dtype=np.int32), score=rs.rand(N),
             smoothed=rs.rand(N), state=np.array([0, 1, 1, 0, 0], dtype=bool), warmup=np.arange(N) < 2, events=[(2.0, 3.0, 0.9, 0.8)],
             meta=dict(positive=1, reference="expanding"))
    if gaps:
        cov = np.array([[1, 1], [1, 0.5], [0, 0.25], [0, 0], [1, 1]], dtype=np.float64)
        valid = Gaps(0.5, 2).valid(cov)
        z.update(coverage=cov, valid=valid, lost=monitor.lost_windows(valid, 2))
        z["meta"].update(gaps=Gaps(0.5, 2).spelling, invalid_windows=2, lost_windows=1)
    return monitor.Timeline(**z)


def test_timeline_files_with_and_without_gaps(tmp_path):
    plain, gapped = _timeline(False), _timeline(True)
    assert plain.coverage is None and plain.valid is None and plain.lost is None          # the new fields have defaults
    a = plain.to_csv(tmp_path / "a.csv").read_text().splitlines()
    b = gapped.to_csv(tmp_path / "b.csv").read_text().splitlines()
    assert a[0] == "window,t_end_s,score,std,smoothed,state,pred,entropy,mutual_info,warmup" and b[0] == a[0] + ",valid,coverage_min,lost"
    assert [r.rsplit(",", 3)[0] for r in b[1:]] == a[1:]                                 # the old columns as they were
    assert [r.split(",")[-3:] for r in b[1:]] == [["1", "1", "0"], ["1", "0.5", "0"], ["0", "0", "0"], ["0", "0", "1"], ["1", "1", "0"]]
    da = json.loads(plain.to_json(tmp_path / "a.json").read_text())
    db = json.loads(gapped.to_json(tmp_path / "b.json").read_text())
    assert not {"gaps", "invalid_windows", "lost_windows"} & set(da) and (db["gaps"], db["invalid_windows"], db["lost_windows"]) == ("0.5:2", 2, 1)
    assert {k: v for k, v in db.items() if k not in ("gaps", "invalid_windows", "lost_windows")} == da
    assert live.timelines_equal(plain, plain) and live.timelines_equal(gapped, gapped) and not live.timelines_equal(plain, gapped)
    other = _timeline(True)
    other.coverage[1, 1] = 0.75
    assert not live.timelines_equal(gapped, other)


# ---- the synthetic recording's planted gaps ------------------------------------------------------------------------------------------
def test_synthetic_gaps_are_seeded_off_by_default_and_leave_the_recording_alone():
    phases = [(1, 60.0), (2, 60.0)]
    plain, table = synth.make_synthetic_recording(phases, fs=8.0, seed=3)
    again, _t = synth.make_synthetic_recording(phases, fs=8.0, seed=3, gaps=None)
    assert plain.tobytes() == again.tobytes() and np.isfinite(plain).all()
    spec = "drop=0.05,channel=2:10:20,all=70:15,all=80:10"
    x, table2 = synth.make_synthetic_recording(phases, fs=8.0, seed=3, gaps=spec)
    y, _t = synth.make_synthetic_recording(phases, fs=8.0, seed=3, gaps=spec)
    assert x.tobytes() == y.tobytes() and table2 == table
    gone = np.isnan(x)
    assert np.array_equal(x[~gone], plain[~gone])                                        # what is left is the recording's
    assert gone[80:240, 2].all() and gone[560:720, :].all() and not gone[:, 2].all()
    assert 0.03 < gone[:80].mean() < 0.07
    assert synth.gap_spans(spec, 8.0, x.shape[0]) == [(560, 720)] and synth.gap_spans("drop=0.1", 8.0, 100) == []
    assert synth.gap_spans("all=5:10,all=100:50", 8.0, 900) == [(40, 120), (800, 900)]
    for bad in ("drop=1", "drop=-0.1", "channel=1:2", "channel=1.5:2:3", "all=5", "all=5:0", "gone=1", "drop", ""):
        with pytest.raises(ValueError):
            synth.parse_synthetic_gaps(bad)
    with pytest.raises(ValueError):
        synth.make_synthetic_recording(phases, fs=8.0, seed=3, gaps="channel=6:1:1")
    assert live.replay_pieces(0, 100, [(10, 20), (90, 200)]) == [(0, 10, False), (10, 20, True), (20, 90, False), (90, 100, True)]
    assert live.replay_pieces(20, 60, [(10, 20), (90, 200)]) == [(20, 60, False)] and live.replay_pieces(12, 18, [(10, 20)]) == [(12, 18, True)]


# ---- the restatement itself ----------------------------------------------------------------------------------------------------------
def test_missing_is_the_bit_pattern_and_the_restatement_anchors_on_rn_reference():
    import rn_reference as R
    v = np.array([0.0, -0.0, 1e308, 5e-324, np.nan, -np.nan, np.inf, -np.inf, G.QNAN])
    assert list(G.missing(v)) == [False] * 4 + [True] * 5
    sig = G.case_recording(200, 37, "3of8", "log1p_m1")
    _v, ok = G.transformed(sig, G.COLS["3of8"], G.mask_of(G.COLS["3of8"]))
    assert (~ok[:, 1]).sum() == (sig[:, 1] == -1.0).sum() > 0 and ok[:, [0, 2]].all()          # log1p(-1) = -inf is missing, nothing else
    sig = G.case_recording(200, 37, "3of8", "none")
    cols = G.COLS["3of8"]
    v, ok = G.transformed(sig, cols, G.mask_of(cols))
    assert ok.all() and np.array_equal(v, R.transformed(sig, cols, G.mask_of(cols)))
    for name, K in (("expanding", 0), ("trailing2", 2), ("trailing13", 13)):
        m, i, n_ref, cov, W, has = G.stats_table(v, ok, 200, 37, G.N_WINDOWS, G.MODES[name])
        wm, wi, wc = R.stats_table(v, 200, 37, K)
        assert np.array_equal(_bits(m), _bits(wm)) and np.array_equal(_bits(i), _bits(wi)) and list(n_ref) == list(wc) and np.all(cov == 1.0) and has.all()
        assert np.array_equal(_bits(W[:, :2]), _bits(R.window_sums(v, 200, 37))) and np.all(W[:, 2] == 200)


@pytest.mark.parametrize("kind", G.INPUTS)
def test_the_float64_restatement_stays_inside_the_yardstick(kind):
    """The statistics criterion of the GPU tests, applied to the float64 restatement itself on one shape per input (the whole grid of
    tests/test_gaps_gpu.py was swept the same way before it was fixed): its bounds are finite, the flat and the empty entries meet
    their absolute conditions, and no input leaves a non-finite value in any record."""
    T, S, key = G.SHAPES[1]
    sig, cols = G.case_recording(T, S, key, kind), G.COLS[key]
    v, ok = G.transformed(sig, cols, G.mask_of(cols))
    for name in ("expanding", "trailing2", "decayed3"):
        m, i, n_ref, cov, W, _has = G.stats_table(v, ok, T, S, G.N_WINDOWS, G.MODES[name])
        y = G.yardstick(m, i, T, S, key, kind, G.MODES[name])
        assert y["flat_ok"] and y["none_ok"], name
        assert np.all(np.isfinite(y["bound_mean"].astype(np.float64))) and np.all(np.isfinite(y["bound_inv"].astype(np.float64)))
        assert np.all(y["r_mean"] <= y["bound_mean"]) and np.all(y["r_inv"] <= y["bound_inv"])
        for a in (m, i, n_ref, cov, W):
            assert np.all(np.isfinite(a))
        assert np.all((cov >= 0) & (cov <= 1)) and (kind == "none") == bool(np.all(cov == 1.0))
