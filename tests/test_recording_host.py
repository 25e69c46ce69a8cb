"""The host side of the recording monitor (multimodalsignal_amd/monitor.py, synth.make_synthetic_recording) and the numpy
restatement the GPU tests compare against (tests/rec_reference.py).  No GPU."""
import hashlib
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import rec_reference as R  # noqa: E402

from multimodalsignal_amd import monitor as M  # noqa: E402
from multimodalsignal_amd.dataset import normalise_subject  # noqa: E402
from multimodalsignal_amd.synth import CHANNELS6, make_synthetic_recording, make_synthetic_wesad  # noqa: E402


# ---- the window count and the multiplicities -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("L, T, S, n", [(255, 256, 64, 0), (256, 256, 64, 1), (256 + 63, 256, 64, 1), (256 + 64, 256, 64, 2),
                                        (256 + 5 * 64 + 17, 256, 64, 6), (1000, 100, 300, 4), (300, 256, 1, 45)])
def test_window_count(L, T, S, n):
    assert M.count_windows(L, T, S) == R.count(L, T, S) == n
    assert R.materialise(np.zeros((L, 2)), T, S).shape[0] == n


def test_window_count_refuses_nonsense():
    for T, S in ((0, 1), (10, 0), (-1, 5)):
        with pytest.raises(ValueError):
            M.count_windows(100, T, S)


def test_multiplicities_at_the_head_the_tail_and_between_windows():
    T, S = 10, 3
    L = 4 * S + T + 2                                        # 5 windows, two samples of tail no window covers
    m = R.multiplicity(L, T, S, 0, R.count(L, T, S))
    assert m.tolist() == [1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 3, 3, 4, 3, 3, 3, 2, 2, 2, 1, 1, 1, 0, 0]
    assert m.sum() == 5 * T
    assert R.multiplicity(L, T, S, 1, 3).tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    g = R.multiplicity(30, 4, 10, 0, 3)                     # S > T: gaps between the windows
    assert g.tolist() == [1] * 4 + [0] * 6 + [1] * 4 + [0] * 6 + [1] * 4 + [0] * 6
    for i, mi in enumerate(m):                               # the closed form the kernels use: ceil((i - T + 1) / S) .. floor(i / S)
        lo, hi = max(0, -(-(i - T + 1) // S)), min(4, i // S)
        assert max(0, hi - lo + 1) == mi


@pytest.mark.parametrize("T, S, w", [(64, 16, (0, None)), (64, 16, (3, 11)), (50, 50, (0, None)), (40, 70, (1, 4)), (64, 1, (5, 15))])
def test_reference_statistics_are_normalise_subjects_on_the_materialised_windows(T, S, w):
    rs = np.random.RandomState(3)
    L = 12 * S + T + 5
    names = ["a", "chest_EDA", "c", "d"]
    sig = rs.randn(L, 4) * np.array([1.0, 0.3, 20.0, 0.05]) + np.array([0.0, 0.0, -7.0, 33.0])
    sig[:, 1] = np.abs(sig[:, 1]) + 0.05
    N = R.count(L, T, S)
    w0, w1 = w[0], N if w[1] is None else w[1]
    cols, mask = [3, 1, 0], 0b010
    sel = [names[c] for c in cols]
    win = R.materialise(sig, T, S)[:, :, cols].copy()
    ref = np.zeros(N, dtype=bool)
    ref[w0:w1] = True
    base = win[ref].copy()
    base[:, :, 1] = np.log1p(base[:, :, 1])
    mean_np, std_np = base.mean(axis=(0, 1)), base.std(axis=(0, 1))
    for fn in (R.stats_longdouble, R.stats_weighted_longdouble):
        mean, std = fn(sig, cols, mask, T, S, w0, w1)
        scale = np.abs(mean_np) + std_np
        assert np.all(np.abs(mean.astype(np.float64) - mean_np) <= 64 * np.finfo(np.float64).eps * scale)       # numpy's pairwise fp64 sums
        assert np.all(np.abs(std.astype(np.float64) - std_np) <= 64 * np.finfo(np.float64).eps * scale)
    # ... and the normalised batch is normalise_subject's output, cast and transposed, to float32 rounding of fp64-close values
    mean, std = R.stats_longdouble(sig, cols, mask, T, S, w0, w1)
    out = R.batch(sig, cols, mask, T, S, 0, N, mean.astype(np.float64), 1.0 / (std.astype(np.float64) + 1e-8))
    want = normalise_subject(win.copy(), sel, ref if not ref.all() else None).transpose(0, 2, 1)
    assert out.shape == (N, 3, T) and out.dtype == np.float32
    np.testing.assert_allclose(out, want, rtol=0, atol=2e-6 * max(1.0, np.abs(want).max()))


# ---- the reference argument ------------------------------------------------------------------------------------------------------------
def test_parse_recording_reference():
    assert M.parse_recording_reference("recording", 37) == (0, 37, 0)
    assert M.parse_recording_reference("head:7", 37) == (0, 7, 7)
    assert M.parse_recording_reference((3, 9), 37) == (3, 9, 0)
    for bad in ("head:0", "head:", "head:-1", "head:x", "baseline", "subject", (3, 3), (5, 2), (-1, 4), (0, 38), (0.0, 3), None, "head:38"):
        with pytest.raises(ValueError):
            M.parse_recording_reference(bad, 37)


# ---- smoothing, state machine, events --------------------------------------------------------------------------------------------------
def test_ema_is_the_recursion_and_halves_a_step_in_halflife_windows():
    s = M.ema([0, 0, 1, 1, 1, 1, 1], 3)
    assert s[0] == 0 and s[1] == 0
    assert abs((1 - s[4]) - 0.5) < 1e-15                        # three windows after the step
    x = np.random.RandomState(0).rand(50)
    np.testing.assert_array_equal(M.ema(x, 2.5), R.ema(x, 2.5))
    np.testing.assert_array_equal(M.ema(x, 0), x)
    assert M.ema([], 3).shape == (0,)
    with pytest.raises(ValueError):
        M.ema(x, -1)


def _check(score, on=0.6, off=0.4, min_on=2):
    sm = np.asarray(score, dtype=np.float64)
    t = (np.arange(len(sm)) * 10 + 60).astype(np.float64)
    state = M.hysteresis(sm, on, off, min_on)
    events = M.find_events(state, sm, t)
    rstate, revents = R.state_and_events(sm, t, on, off, min_on)
    np.testing.assert_array_equal(state, rstate)
    assert len(events) == len(revents) and np.allclose(np.array(events).reshape(-1, 4), np.array(revents).reshape(-1, 4), rtol=1e-13, atol=0)
    return state.astype(int).tolist(), events


def test_an_episode_shorter_than_min_on_is_dropped():
    state, events = _check([0.1, 0.7, 0.2, 0.1, 0.9, 0.8, 0.3, 0.1])
    assert state == [0, 0, 0, 0, 1, 1, 0, 0]
    assert events == [(100.0, 110.0, 0.9, pytest.approx(0.85))]
    assert _check([0.1, 0.7, 0.2, 0.1], min_on=1)[0] == [0, 1, 0, 0]


def test_an_episode_that_touches_the_end():
    state, events = _check([0.1, 0.2, 0.65, 0.7, 0.8])
    assert state == [0, 0, 1, 1, 1]
    assert events == [(80.0, 100.0, 0.8, pytest.approx((0.65 + 0.7 + 0.8) / 3))]
    assert _check([0.1, 0.2, 0.3, 0.9])[0] == [0, 0, 0, 0]       # one window at the end: shorter than min_on


def test_flapping_between_off_and_on_holds_the_state():
    state, events = _check([0.5, 0.59, 0.6, 0.41, 0.59, 0.45, 0.4, 0.59, 0.5, 0.6, 0.6])
    assert state == [0, 0, 1, 1, 1, 1, 0, 0, 0, 1, 1]           # on at >= 0.6, off only at <= 0.4; 0.59 alone never turns it on
    assert [e[:2] for e in events] == [(80.0, 110.0), (150.0, 160.0)]


def test_the_thresholds_are_inclusive_and_ordered():
    assert _check([0.6, 0.6, 0.4, 0.4])[0] == [1, 1, 0, 0]
    for on, off in ((0.4, 0.4), (0.3, 0.6)):
        with pytest.raises(ValueError):
            M.hysteresis([0.5], on, off, 1)
    with pytest.raises(ValueError):
        M.hysteresis([0.5], 0.6, 0.4, 0)


# ---- the synthetic recording ---------------------------------------------------------------------------------------------------------
def _dir_hash(d):
    h = hashlib.sha256()
    for f in sorted(Path(d).iterdir()):
        h.update(f.name.encode())
        h.update(f.read_bytes())
    return h.hexdigest()


def test_synthetic_recording_is_seeded_and_leaves_make_synthetic_wesad_alone(tmp_path):
    kw = dict(subjects=["S2", "S3"], windows_per_subject=5, T=64, seed=11)
    before = _dir_hash(make_synthetic_wesad(tmp_path / "a", **kw))
    phases = [(1, 30.0), (2, 20.5), (4, 10.0)]
    sig, table = make_synthetic_recording(phases, fs=32.0, seed=5, difficulty=2.0)
    assert sig.shape == (int(30 * 32) + int(20.5 * 32) + 320, len(CHANNELS6)) and sig.dtype == np.float64 and sig.flags.c_contiguous
    assert [(r["label"], r["start"], r["end"]) for r in table] == [(1, 0, 960), (2, 960, 1616), (4, 1616, 1936)]
    assert table[1]["start_s"] == 30.0 and table[2]["end_s"] == 60.5
    again, _ = make_synthetic_recording(phases, fs=32.0, seed=5, difficulty=2.0)
    np.testing.assert_array_equal(sig, again)
    other, _ = make_synthetic_recording(phases, fs=32.0, seed=6, difficulty=2.0)
    assert not np.array_equal(sig, other)
    assert np.isfinite(sig).all() and (sig[:, 1] > 0).all()                            # chest_EDA stays log1p-safe
    assert sig[960:1616, 1].mean() > sig[:960, 1].mean() - 3 * sig[:960, 1].std()       # a level, not a discontinuity in scale
    two, _ = make_synthetic_recording(phases, fs=32.0, channels=CHANNELS6[:2], seed=5)
    assert two.shape == (1936, 2)
    assert _dir_hash(make_synthetic_wesad(tmp_path / "b", **kw)) == before             # the same files after the new function ran
    for bad in ([], [(5, 10.0)], [(1, 0.0)], [(2, -3.0)]):
        with pytest.raises(ValueError):
            make_synthetic_recording(bad)


def test_the_planted_rhythms_are_phase_continuous():
    sig, table = make_synthetic_recording([(1, 60.0), (2, 60.0)], fs=64.0, seed=1, channels=["only"])
    edge = table[1]["start"]
    jump = np.abs(np.diff(sig[:, 0]))
    assert jump[edge - 1] <= np.percentile(jump, 99.9)          # no step where the phase changes: noise-sized like everywhere


# ---- the CLI's argument errors -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv", [
    ["--out", "o"],                                                                      # no --run
    ["--run", "r"],                                                                      # no --out
    ["--run", "r", "--out", "o"],                                                        # neither a recording nor the synthetic one
    ["--run", "r", "--out", "o", "--recording", "x.npy", "--names", "n", "--synthetic-recording"],
    ["--run", "r", "--out", "o", "--recording", "x.npy"],                                # no --names
    ["--run", "r", "--out", "o", "--synthetic-recording", "--resample-from", "700"],
    ["--run", "r", "--out", "o", "--synthetic-recording", "--reference", "baseline"],
    ["--run", "r", "--out", "o", "--synthetic-recording", "--reference", "head:0"],
    ["--run", "r", "--out", "o", "--synthetic-recording", "--fs", "0"],
    ["--run", "r", "--out", "o", "--synthetic-recording", "--stride-s", "0"],
    ["--run", "r", "--out", "o", "--synthetic-recording", "--window-s", "-60"],
    ["--run", "r", "--out", "o", "--recording", "x.npy", "--names", "n", "--resample-from", "-1"],
], ids=lambda a: " ".join(a[4:]) or " ".join(a))
def test_cli_argument_errors(argv, capsys):
    with pytest.raises(SystemExit) as e:
        M.parse_args(argv)
    assert e.value.code == 2
    assert "error" in capsys.readouterr().err


def test_cli_accepts_the_documented_forms():
    a = M.parse_args(["--run", "r", "--subject", "S5", "--config", "cnn_gru", "--recording", "x.npy", "--names", "n.txt", "--fs", "64",
                      "--resample-from", "700", "--reference", "head:6", "--stride-s", "5", "--out", "o"])
    assert (a.subject, a.config, a.fs, a.resample_from, a.reference, a.stride_s) == ("S5", "cnn_gru", 64.0, 700.0, "head:6", 5.0)
    assert M.parse_args(["--run", "r", "--synthetic-recording", "--out", "o"]).reference == "recording"


def test_run_files_rules(tmp_path):
    for sub in ("fold_test_on_S10", "fold_test_on_S2", "seed_1/fold_test_on_S2", "seed_1/fold_test_on_S10", "seed_2/fold_test_on_S2"):
        (tmp_path / sub).mkdir(parents=True)
        (tmp_path / sub / "best_model.pt").write_bytes(b"")
    (tmp_path / "fold_test_on_S3").mkdir()                                                # a fold without a checkpoint is not a member
    rel = lambda fs: [str(f.relative_to(tmp_path)) for f in fs]      # noqa: E731
    assert rel(M.Monitor.run_files(tmp_path, "S2")) == ["fold_test_on_S2/best_model.pt", "seed_1/fold_test_on_S2/best_model.pt",
                                                        "seed_2/fold_test_on_S2/best_model.pt"]
    assert rel(M.Monitor.run_files(tmp_path, "S10")) == ["fold_test_on_S10/best_model.pt", "seed_1/fold_test_on_S10/best_model.pt"]
    assert rel(M.Monitor.run_files(tmp_path)) == ["fold_test_on_S2/best_model.pt", "fold_test_on_S10/best_model.pt"]
    with pytest.raises(FileNotFoundError):
        M.Monitor.run_files(tmp_path, "S3")
    with pytest.raises(FileNotFoundError):
        M.Monitor.run_files(tmp_path / "seed_2" / "fold_test_on_S2")
    (tmp_path / "cv_summary.txt").write_text("实验配置:\nSEED: 42\nCHANNELS_TO_USE: ['chest_ECG', 'chest_EDA']\n", encoding="utf-8")
    assert M.Monitor.run_channels(tmp_path) == ["chest_ECG", "chest_EDA"]
    assert M.Monitor.run_channels(tmp_path / "seed_1") is None
