"""The decayed:H running reference and training under the causal references, without a GPU (include/msig_rd.h,
multimodalsignal_amd/reference.py, dataset.py, monitor.py, live.py): the spellings both grammars take and
refuse, --reference auto's whole table from a temporary cv_summary.txt, the restatement (tests/rd_reference.py) at its two exact
anchors and against its own live state model, and the float64 host normalisation of WesadDataset and the host stores."""
import numpy as np
import pytest

import lv_reference as LV
import rd_reference as RD
import rn_reference as R
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd import dataset, live, monitor
from multimodalsignal_amd.reference import Running, parse_running

EPS = float(np.finfo(np.float64).eps)


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


# ---- the two grammars ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref, K, W, H", [("decayed:1", 0, 6, 1), ("decayed:60", 0, 6, 60), ("decayed:5:2", 0, 2, 5), ("decayed:3:0", 0, 0, 3),
                                          (f"decayed:{1 << 20}", 0, 6, 1 << 20), ("expanding", 0, 6, 0), ("expanding:3", 0, 3, 0),
                                          ("trailing:5", 5, 6, 0), ("trailing:5:2", 5, 2, 0)])
def test_the_monitors_grammar_accepts(ref, K, W, H):
    run = monitor.running_reference(ref)
    assert isinstance(run, Running) and run == (K, W) and run.H == H and run.kind == ref.split(":")[0]
    assert (run.decay == float(np.exp2(-1.0 / H))) if H else run.decay is None
    assert monitor.parse_recording_reference(ref, 50) == (0, 50, W)
    base = ["--run", "r", "--synthetic-recording", "--out", "o", "--reference", ref]
    assert monitor.parse_args(base).reference == ref and live.parse_args(base).reference == ref


@pytest.mark.parametrize("ref, kind, K, H", [("expanding", "expanding", 0, 0), ("trailing:1", "trailing", 1, 0), ("trailing:4096", "trailing", 4096, 0),
                                             ("decayed:1", "decayed", 0, 1), ("decayed:60", "decayed", 0, 60), (f"decayed:{1 << 20}", "decayed", 0, 1 << 20)])
def test_the_training_grammar_accepts(ref, kind, K, H):
    run = dataset.parse_reference(ref)
    assert isinstance(run, Running) and (run.kind, run.K, run.H) == (kind, K, H) and run.spelling == ref
    assert dataset.running_norm_reference(ref) is run or dataset.running_norm_reference(ref) == run
    assert dataset.reference_mask(np.array([1, 2, 3]), ref).all() and dataset.subject_reference(np.array([2, 2]), ref, "S2") is None


def test_the_training_grammar_keeps_its_present_values():
    assert dataset.parse_reference("subject") is None and dataset.parse_reference("baseline") == 0 and dataset.parse_reference("baseline:7") == 7
    assert not isinstance(dataset.parse_reference("baseline"), Running) and dataset.running_norm_reference("baseline:7") is None
    for ref in ("baseline:0", "baseline:", "Subject", "head:6", "recording", None, 3):
        with pytest.raises(ValueError):
            dataset.parse_reference(ref)


REFUSED_EVERYWHERE = ["decayed", "decayed:", "decayed:0", "decayed:1.5", "decayed:x", "decayed:3:-1", "decayed:-2", f"decayed:{(1 << 20) + 1}",
                      "decayed:3:1:1", "Decayed:3", "decayed :3", "decayed:٣", "trailing:0", "trailing:4097", "trailing", "expanding:x"]


@pytest.mark.parametrize("ref", REFUSED_EVERYWHERE, ids=repr)
def test_refused_in_both_grammars_and_on_both_command_lines(ref):
    with pytest.raises(ValueError):
        monitor.parse_recording_reference(ref, 50)
    if ref.split(":")[0] in ("expanding", "trailing", "decayed"):          # spelled as a running reference, and wrongly
        with pytest.raises(ValueError):
            monitor.running_reference(ref)
    else:
        assert monitor.running_reference(ref) is None
    with pytest.raises(ValueError):
        dataset.parse_reference(ref)
    with pytest.raises(ValueError):
        live.LiveMonitor([], 64.0, reference=ref)
    base = ["--run", "r", "--synthetic-recording", "--out", "o", "--reference", ref]
    for mod in (monitor, live):
        with pytest.raises(SystemExit):
            mod.parse_args(base)


@pytest.mark.parametrize("ref", ["expanding:3", "expanding:0", "trailing:5:2", "decayed:3:2", "decayed:60:6"])
def test_a_warmup_count_is_a_monitor_flag(ref):
    """--reference takes ':W'; --norm-reference refuses it, and the error says whose flag it is."""
    assert monitor.running_reference(ref) is not None
    with pytest.raises(ValueError) as e:
        dataset.parse_reference(ref)
    assert "monitor" in str(e.value) and "':W'" in str(e.value)
    from multimodalsignal_amd import main
    with pytest.raises(SystemExit):
        main.parse_args(main.build_parser(), ["--synthetic", "x", "--norm-reference", ref])


def test_the_train_command_line_takes_the_new_values_and_keeps_its_refusals(capsys):
    from multimodalsignal_amd import main
    a = main.parse_args(main.build_parser(), ["--synthetic", "x", "--norm-reference", "expanding"])
    assert a.norm_reference == ["expanding"]
    a = main.parse_args(main.build_parser(), ["--synthetic", "x", "--norm-reference", "subject", "expanding", "trailing:60", "decayed:60"])
    assert a.norm_reference == ["subject", "expanding", "trailing:60", "decayed:60"]
    for extra in (["--hierarchical"], ["--calibrate"], ["--seeds", "2"]):
        with pytest.raises(SystemExit):
            main.parse_args(main.build_parser(), ["--synthetic", "x", "--norm-reference", "expanding", "decayed:60"] + extra)
    with pytest.raises(SystemExit):
        main.parse_args(main.build_parser(), ["--synthetic", "x", "--norm-reference", "decayed:60", "decayed:60"])
    for ref in ("decayed", "decayed:0", "decayed:1.5", "decayed:x", "decayed:3:-1"):
        with pytest.raises(SystemExit):
            main.parse_args(main.build_parser(), ["--synthetic", "x", "--norm-reference", ref])
    capsys.readouterr()


def test_the_error_texts_name_the_new_form_and_the_limits_agree():
    with pytest.raises(ValueError) as e:
        monitor.parse_recording_reference("nothing", 50)
    for form in ("'recording'", "'head:K'", "'expanding[:W]'", "'trailing:K[:W]'", "'decayed:H[:W]'", str(L.RN_MAX_K), str(L.RD_MAX_H)):
        assert form in str(e.value)
    with pytest.raises(ValueError) as e:
        dataset.parse_reference("nothing")
    for form in ("'subject'", "'baseline:K'", "'expanding'", "'trailing:K'", "'decayed:H'"):
        assert form in str(e.value)
    assert L.RD_MAX_H == RD.MAX_H == 1 << 20 and monitor.RUNNING_WARMUP == 6
    assert monitor.running_reference("decayed:60") == parse_running("decayed:60")          # one grammar, not two


# ---- --reference auto ----------------------------------------------------------------------------------------------------------------
def _run(tmp_path, line):
    (tmp_path / "cv_summary.txt").write_text("实验配置:\nSEED: 42\nCHANNELS_TO_USE: ['a', 'b']\n" + (f"NORM_REFERENCE: {line}\n" if line else "")
                                             + "NUM_EPOCHS: 3\n", encoding="utf-8")
    return tmp_path


@pytest.mark.parametrize("trained, offline, online", [(None, "recording", None), ("subject", "recording", None), ("baseline:6", "head:6", "head:6"),
                                                      ("baseline:30", "head:30", "head:30"), ("baseline", None, None),
                                                      ("expanding", "expanding:6", "expanding:6"), ("trailing:60", "trailing:60:6", "trailing:60:6"),
                                                      ("decayed:60", "decayed:60:6", "decayed:60:6")])
def test_auto_resolves_the_runs_reference(tmp_path, trained, offline, online):
    run = _run(tmp_path, trained)
    got = monitor.run_norm_reference(run)
    assert got == (trained or "subject")
    for is_live, want in ((False, offline), (True, online)):
        if want is not None:
            assert monitor.resolve_reference(got, live=is_live) == want
            monitor.parse_recording_reference(want, 1 << 62)          # what it resolves to is a reference the monitors take
            continue
        with pytest.raises(ValueError) as e:
            monitor.resolve_reference(got, live=is_live)
        assert ("head:K" if trained == "baseline" else "expanding") in str(e.value)
    # from_run resolves before it looks for a checkpoint: a refusal needs no model, a resolution fails only at the missing folds
    for cls, want in ((monitor.Monitor, offline), (live.LiveMonitor, online)):
        with pytest.raises(ValueError if want is None else FileNotFoundError):
            cls.from_run(run, reference="auto")


def test_auto_reads_a_configurations_own_summary_and_the_command_lines_take_it(tmp_path):
    (tmp_path / "decayed_60").mkdir()
    _run(tmp_path / "decayed_60", "decayed:60")
    _run(tmp_path, "baseline:6")
    assert monitor.run_norm_reference(tmp_path, "decayed_60") == "decayed:60" and monitor.run_norm_reference(tmp_path) == "baseline:6"
    assert monitor.run_norm_reference(tmp_path / "nowhere") == "subject"
    base = ["--run", "r", "--synthetic-recording", "--out", "o"]
    assert monitor.parse_args(base + ["--reference", "auto"]).reference == "auto" and live.parse_args(base + ["--reference", "auto"]).reference == "auto"
    assert monitor.parse_args(base).reference == "recording" and live.parse_args(base).reference == "head:6"      # the defaults stay
    with pytest.raises(ValueError):
        monitor.resolve_reference("something else")


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
CASES = [(16, 4, "8of8"), (10, 3, "3of8"), (257, 5, "1of8")]


def _v(T, S, key, N, dtype=np.float64):
    sig = LV.recording((N - 1) * S + T + 2, 100 * T + S)
    return sig, R.transformed(sig, LV.COLS[key], LV.mask_of(LV.COLS[key]), dtype)


@pytest.mark.parametrize("T,S,key", CASES)
def test_the_two_anchors_bit_for_bit(T, S, key):
    """lambda = 1 is expanding (c_n = n + 1), lambda = 0 is trailing:1 (c_n = 1): sums, means, reciprocals and counts."""
    N = 23
    for dtype in (np.float64, np.longdouble):
        _sig, v = _v(T, S, key, N, dtype)
        W = R.window_sums(v, T, S)
        for lam, K in ((1.0, 0), (0.0, 1)):
            A, c = RD.reference_sums(W, lam)
            assert _bits(A, R.reference_sums(W, K))
            m, i, c2 = RD.stats_table(v, T, S, lam)
            mk, ik, ck = R.stats_table(v, T, S, K)
            assert _bits(m, mk) and _bits(i, ik) and list(c) == list(c2) == [float(x) for x in ck]
        m, i, c = RD.stats_table(v, T, S, RD.decay_of(3))                 # in between it is another reference
        assert not np.array_equal(m[5:], R.stats_table(v, T, S, 0)[0][5:]) and 1 < c[-1] < 1 / (1 - RD.decay_of(3)) + 1e-9


def test_the_float64_fma_is_one_rounding():
    rs = np.random.RandomState(5)
    a, x, y = rs.rand(), rs.randn(4000) * 1e3, rs.randn(4000)
    want = (np.longdouble(a) * x.astype(np.longdouble) + y.astype(np.longdouble))
    got = RD.fma64(a, x, y)
    assert np.all(np.abs(got.astype(np.longdouble) - want) <= 0.5 * np.spacing(np.abs(got)) * (1 + 2.0 ** -9))
    assert np.array_equal(RD.fma64(1.0, x, y), x + y) and np.array_equal(RD.fma64(0.0, x, y), y)
    c = 1.0
    for _ in range(500):
        c = float(RD.fma64(0.5, np.array([c]), np.ones(1))[0])
    assert c == 2.0                                                        # c_n -> 1 / (1 - lambda)


@pytest.mark.parametrize("T,S,key", CASES)
@pytest.mark.parametrize("lam", [1.0, float(np.exp2(-1.0 / 3))], ids=["one", "h3"])
def test_the_live_state_model_reproduces_the_offline_table(T, S, key, lam):
    N = 17
    for dtype in (np.float64, np.longdouble):
        _sig, v = _v(T, S, key, N, dtype)
        m, i, c = RD.stats_table(v, T, S, lam)
        st = RD.LiveState(lam)
        for n in range(N):
            mn, inn, cn = st.step(n, v[n * S:n * S + T])
            assert _bits(mn, m[n]) and _bits(inn, i[n]) and cn == c[n]
        with pytest.raises(AssertionError):
            st.step(N + 1, v[:T])


# ---- host normalisation --------------------------------------------------------------------------------------------------------------
NAMES = ["chest_ECG", "chest_EDA", "chest_Temp", "wrist_BVP"]
USE = ["chest_Temp", "chest_EDA", "chest_ECG"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Two subjects' window files cut from a recording each: (N, T, 4) float64, raw labels that run through the protocol."""
    root = tmp_path_factory.mktemp("windows")
    out = {}
    for sid, N, seed in (("S2", 14, 1), ("S3", 9, 2)):
        rs = np.random.RandomState(seed)
        T = 32
        rec = rs.randn(N * T, 4) * [1.0, 0.3, 0.05, 2.0] + [0.2, 0.0, 33.0, -1.0] + 0.5 * np.sin(np.arange(N * T) / 40.0)[:, None]
        rec[:, 1] = np.exp(0.5 * rs.randn(N * T)) + 0.1
        x = np.ascontiguousarray(rec.reshape(N, T, 4))
        y = np.array(([1] * 4 + [2] * 3 + [3] * 3 + [4] * 2 + [1] * 2)[:N])
        np.save(root / f"{sid}_X.npy", x)
        np.save(root / f"{sid}_y.npy", y)
        out[sid] = (x, y)
    return root, out


def _ds(root, sids, ref, mode="stress_binary", cache=None):
    return dataset.WesadDataset(root, sids, USE, NAMES, classification_mode=mode, cache=cache, reference=ref)


def test_trailing_with_k_at_least_n_is_expanding_in_the_dataset(files):
    root, raw = files
    ex = _ds(root, ["S2", "S3"], "expanding")
    assert ex.data.shape == (23, 32, 3) and np.all(np.isfinite(ex.data))
    for K in (14, 15, 4096):
        assert _bits(_ds(root, ["S2", "S3"], f"trailing:{K}").data, ex.data)
    assert not np.array_equal(_ds(root, ["S2"], "trailing:3").data[3:], ex.data[3:14])
    assert _bits(_ds(root, ["S2"], "trailing:3").data[:3], ex.data[:3])
    assert not np.array_equal(_ds(root, ["S2"], "decayed:3").data[1:], ex.data[1:14])
    assert not np.array_equal(ex.data, _ds(root, ["S2", "S3"], "subject").data)


def test_the_definition_is_the_headers(files):
    """dataset.running_statistics against the restatement in np.longdouble (its window sums in the device's order, numpy's in its
    own: the float64 results agree to rounding, scaled as in test_running_host), and every row is (v - mean[n]) * inv[n]."""
    root, raw = files
    x = raw["S2"][0][:, :, [NAMES.index(c) for c in USE]].copy()
    x[:, :, 1] = np.log1p(x[:, :, 1])
    N, T, Cn = x.shape
    flat = x.reshape(N * T, Cn)
    for ref, rest in (("expanding", lambda v: R.stats_table(v, T, T, 0)), ("trailing:5", lambda v: R.stats_table(v, T, T, 5)),
                      ("decayed:3", lambda v: RD.stats_table(v, T, T, RD.decay_of(3)))):
        run = dataset.parse_reference(ref)
        mean, inv, c = dataset.running_statistics(x, run)
        ml, il, cl = rest(flat.astype(np.longdouble))
        std = 1 / il
        assert np.all(np.abs(mean - ml) <= 8 * N * T * EPS * std) and np.all(np.abs(inv - il) <= 8 * N * T * EPS * il)
        assert np.all(np.abs(c - cl.astype(np.float64)) <= 4 * EPS * c)
        got = _ds(root, ["S2"], ref).data
        assert _bits(got, (x - mean[:, None, :]) * inv[:, None, :])


def test_the_last_expanding_window_has_the_subject_rules_statistics(files):
    """Window N - 1 under expanding draws on every window: its mean and std are normalise_subject's ("subject") to float64
    rounding — N T terms of at most half an ulp of the spread each — so its rows agree with the subject rule's rows that closely."""
    root, raw = files
    x = raw["S2"][0][:, :, [NAMES.index(c) for c in USE]].copy()
    x[:, :, 1] = np.log1p(x[:, :, 1])
    N, T, _Cn = x.shape
    mean, inv, c = dataset.running_statistics(x, dataset.parse_reference("expanding"))
    mu, sd = x.mean(axis=(0, 1)), x.std(axis=(0, 1))
    assert c[-1] == N and np.all(np.abs(mean[-1] - mu) <= N * T * EPS * (np.abs(mu) + sd))
    assert np.all(np.abs(inv[-1] - 1 / (sd + 1e-8)) <= N * T * EPS / sd)
    ex, sub = _ds(root, ["S2"], "expanding").data, _ds(root, ["S2"], "subject").data
    assert np.max(np.abs(ex[-1] - sub[-1])) <= 64 * N * T * EPS * (1 + np.max(np.abs(sub[-1])))
    assert np.max(np.abs(ex[0] - sub[0])) > 1e-3                          # and window 0 draws on itself alone


def test_amusement_binary_keeps_the_statistics_of_the_undropped_file(files):
    root, raw = files
    for ref in ("expanding", "trailing:4", "decayed:3"):
        full = _ds(root, ["S2"], ref, "stress_binary")
        am = _ds(root, ["S2"], ref, "amusement_binary")
        keep = np.isin(raw["S2"][1], (1, 3))
        assert len(am) == int(keep.sum()) < len(full) and _bits(am.data, full.data[keep])
        assert list(am.labels) == [0 if v == 1 else 1 for v in raw["S2"][1][keep]]


def test_host_stores_hold_the_datasets_bits(files):
    root, raw = files
    for ref in ("expanding", "trailing:4", "decayed:3"):
        ds = _ds(root, ["S2", "S3"], ref)
        want = np.ascontiguousarray(ds.data.transpose(0, 2, 1), dtype=np.float32)
        host = dataset.SubjectStore(root, ["S2", "S3"], USE, NAMES, device="cpu", normalise="host", reference=ref)
        wes = dataset.SubjectStore.from_wesad(root, ["S2", "S3"], USE, NAMES, device="cpu", cache={}, reference=ref)
        for st in (host, wes):
            assert np.array_equal(st.x.numpy().view(np.uint32), want.view(np.uint32)) and st.ranges == {"S2": (0, 14), "S3": (14, 23)}
        assert host.reference_windows == {"S2": ("per window", False), "S3": ("per window", False)}
    assert dataset.SubjectStore(root, ["S2"], USE, NAMES, device="cpu", normalise="host").reference_windows == {}


def test_the_normalisation_table_says_per_window(files, tmp_path):
    from multimodalsignal_amd import main
    root, raw = files
    refs = ["subject", "baseline:2", "expanding", "decayed:3"]
    fold = lambda sid, a: {"subject": sid, "accuracy": a, "f1_score": a}      # noqa: E731
    res = {"": {r: [fold("S2", 0.5 + 0.1 * i), fold("S3", 0.6)] for i, r in enumerate(refs)}}
    table = main.normalisation(res, refs, root, ["S2", "S3"])
    assert table["reference_windows"]["expanding"]["S2"] == {"n_windows": 14, "reference_windows": "per window", "fallback": False}
    assert table["reference_windows"]["baseline:2"]["S2"]["reference_windows"] == 2 and table["reference_windows"]["subject"]["S3"]["reference_windows"] == 9
    text = main.write_normalisation(tmp_path, table).read_text()
    assert "  expanding: S2 per window, S3 per window" in text and "  decayed:3: S2 per window, S3 per window" in text
    assert "  baseline:2: S2 2/14, S3 2/9" in text
    assert main.reference_dir("decayed:3") == "decayed_3"
