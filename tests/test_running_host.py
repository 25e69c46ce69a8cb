"""Causal running references without a GPU (multimodalsignal_amd/monitor.py, live.py): the spellings the
parsers take and refuse, with "head:K" and the others unchanged, and the restatement (tests/rn_reference.py) against itself and
against tests/rec_reference.py — trailing:K with K >= N is expanding bit for bit, the last window's expanding statistics are the
"recording" reference's, and the host model of the live state machine reproduces the offline table bit for bit."""
import numpy as np
import pytest

import lv_reference as LV
import rec_reference as REC
import rn_reference as R
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd import live, monitor

EPS = float(np.finfo(np.float64).eps)


def _bits(a, b):
    """The same values bit for bit (np.longdouble's bytes carry padding, so: equal, and the same signs of zero)."""
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


# ---- parsing -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref, want, running", [
    ("expanding", (0, 50, 6), (0, 6)), ("expanding:0", (0, 50, 0), (0, 0)), ("expanding:9", (0, 50, 9), (0, 9)),
    ("trailing:1", (0, 50, 6), (1, 6)), ("trailing:180", (0, 50, 6), (180, 6)), ("trailing:5:2", (0, 50, 2), (5, 2)),
    ("trailing:4096:0", (0, 50, 0), (4096, 0)), ("expanding:77", (0, 50, 77), (0, 77)),
    ("recording", (0, 50, 0), None), ("head:1", (0, 1, 1), None), ("head:6", (0, 6, 6), None), ("head:50", (0, 50, 50), None),
    ((3, 11), (3, 11, 0), None), ([0, 50], (0, 50, 0), None)], ids=str)
def test_accepted_references(ref, want, running):
    assert monitor.parse_recording_reference(ref, 50) == want
    assert monitor.running_reference(ref) == running


@pytest.mark.parametrize("ref", ["expanding:", "expanding:-1", "expanding:x", "expanding:1:2", "expanding:1.5", "trailing", "trailing:", "trailing:0",
                                 "trailing:4097", "trailing:-3", "trailing:x", "trailing:3:", "trailing:3:-1", "trailing:3:1:1", "trailing:٣",
                                 "Expanding", "expanding ", "trail:3", "head:0", "head:", "head:51", "head:x", "tail:3", "", None, 7, (3, 3), (0, 51),
                                 (1.0, 2), (True, 2)], ids=repr)
def test_refused_references(ref):
    with pytest.raises(ValueError):
        monitor.parse_recording_reference(ref, 50)


def test_the_error_text_lists_the_new_forms_and_the_limits_agree():
    with pytest.raises(ValueError) as e:
        monitor.parse_recording_reference("nothing", 50)
    for form in ("'recording'", "'head:K'", "'expanding[:W]'", "'trailing:K[:W]'", str(L.RN_MAX_K)):
        assert form in str(e.value)
    assert L.RN_MAX_K == R.MAX_K >= 4096 and monitor.RUNNING_WARMUP == 6
    assert monitor.running_reference((0, 5)) is None and monitor.running_reference("head:6") is None


BASE = ["--run", "r", "--synthetic-recording", "--out", "o"]


@pytest.mark.parametrize("ref", ["expanding", "expanding:3", "trailing:180", "trailing:60:0", "head:6"])
def test_both_command_lines_take_the_causal_references(ref):
    assert monitor.parse_args(BASE + ["--reference", ref]).reference == ref
    assert live.parse_args(BASE + ["--reference", ref]).reference == ref


@pytest.mark.parametrize("ref", ["recording", "trailing:0", "trailing", "expanding:x", "head:0"])
def test_the_live_command_line_refuses_the_rest(ref, capsys):
    with pytest.raises(SystemExit):
        live.parse_args(BASE + ["--reference", ref])
    if ref == "recording":
        assert "expanding" in capsys.readouterr().err
    assert monitor.parse_args(BASE + ["--reference", "recording"]).reference == "recording"
    assert live.parse_args(BASE).reference == "head:6"


def test_live_monitor_refuses_recording_and_points_to_expanding():
    """The reference is checked before the members are looked at: no GPU is needed to be refused."""
    for ref in ("recording", (0, 7), "trailing:0", "expanding:x"):
        with pytest.raises(ValueError) as e:
            live.LiveMonitor([], 64.0, reference=ref)
        if ref == "recording":
            assert "'expanding' is the causal counterpart of 'recording'" in str(e.value) and "trailing:K" in str(e.value)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
CASES = [(16, 4, "8of8"), (10, 3, "3of8"), (4, 7, "3of8"), (257, 5, "1of8")]


def _v(T, S, key, N, dtype=np.float64):
    sig = LV.recording((N - 1) * S + T + 2, 100 * T + S)
    return sig, R.transformed(sig, LV.COLS[key], LV.mask_of(LV.COLS[key]), dtype)


@pytest.mark.parametrize("T,S,key", CASES)
def test_trailing_with_k_at_least_n_is_expanding_bit_for_bit(T, S, key):
    N = 23
    for dtype in (np.float64, np.longdouble):
        _sig, v = _v(T, S, key, N, dtype)
        W = R.window_sums(v, T, S)
        assert W.shape == (N, 2, v.shape[1])
        ex = R.reference_sums(W, 0)
        for K in (N, N + 1, R.MAX_K):
            assert _bits(R.reference_sums(W, K), ex)
        m0, i0, c0 = R.stats_table(v, T, S, 0)
        mK, iK, cK = R.stats_table(v, T, S, N + 3)
        assert _bits(m0, mK) and _bits(i0, iK) and list(c0) == list(cK) == list(range(1, N + 1))
        # and below N it is another reference: the counts saturate at K and the leading K windows still agree
        m7, i7, c7 = R.stats_table(v, T, S, 7)
        assert list(c7) == [min(n + 1, 7) for n in range(N)]
        assert _bits(m7[:7], m0[:7]) and _bits(i7[:7], i0[:7]) and not np.array_equal(m7[7:], m0[7:])


@pytest.mark.parametrize("T,S,key", CASES)
def test_the_last_expanding_window_has_the_recording_reference(T, S, key):
    """Expanding at window N - 1 is the "recording" reference in value: against rec_reference's two-pass np.longdouble statistics
    of all materialised windows.  In np.longdouble the two agree to 4 float64 ulps of |mean| + std (test_recording_gpu's bound for
    its two restatements); the float64 restatement's N T terms may each contribute half an ulp of the spread, so N T eps."""
    N = 23
    cols = LV.COLS[key]
    sig, v = _v(T, S, key, N)
    _sig, vl = _v(T, S, key, N, np.longdouble)
    assert R.count(sig.shape[0], T, S) == N == REC.count(sig.shape[0], T, S)
    mean, std = REC.stats_longdouble(sig, cols, LV.mask_of(cols), T, S, 0, N)
    scale = np.abs(mean) + std
    ml, il, _c = R.stats_table(vl, T, S, 0)
    sl = 1 / il[-1] - np.longdouble(1e-8)
    assert np.all(np.abs(ml[-1] - mean) <= 4 * EPS * scale) and np.all(np.abs(sl - std) <= 4 * EPS * scale + 1e-6 * (std == 0))
    m, i, c = R.stats_table(v, T, S, 0)
    s = 1 / i[-1] - 1e-8
    assert c[-1] == N
    assert np.all(np.abs(m[-1] - mean) <= N * T * EPS * scale) and np.all(np.abs(s - std) <= N * T * EPS * scale + 1e-6 * (std == 0))
    assert np.all(np.abs(R.std_longdouble(vl, T, S, 0)[-1] - std) <= 4 * EPS * scale)


@pytest.mark.parametrize("K", [0, 1, 2, 7, 40])
@pytest.mark.parametrize("T,S,key", CASES[:3])
def test_the_live_state_model_reproduces_the_offline_table(T, S, key, K):
    N = 23
    _sig, v = _v(T, S, key, N)
    mean, inv, cnt = R.stats_table(v, T, S, K)
    st = R.LiveState(K)
    for n in range(N):
        m, i, c = st.step(n, v[n * S:n * S + T])
        assert m.tobytes() == mean[n].tobytes() and i.tobytes() == inv[n].tobytes() and c == cnt[n]
    with pytest.raises(AssertionError):
        st.step(N + 1, v[:T])                       # not the next window


def test_rows_take_each_rows_own_record():
    T, S, key, N = 10, 3, "3of8", 9
    _sig, v = _v(T, S, key, N)
    mean, inv, _c = R.stats_table(v, T, S, 2)
    out = R.rows(v, T, S, 2, mean[2:6], inv[2:6])
    assert out.shape == (4, 3, T) and out.dtype == np.float32
    for b in range(4):
        want = LV.normalised(_sig[(2 + b) * S:(2 + b) * S + T], LV.COLS[key], LV.mask_of(LV.COLS[key]), mean[2 + b], inv[2 + b])
        assert out[b].tobytes() == want.tobytes()
