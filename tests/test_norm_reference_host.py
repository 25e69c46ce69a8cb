"""Baseline-referenced per-subject normalisation, everything that needs no GPU: the host rule against the
reference's own baseline-normalising dataset (tests/golden/norm_reference.npz, written by make_norm_reference_golden.py), the
three forms of a reference, the fallback of a subject without a baseline window, the cache key, and the --norm-reference flag."""
import numpy as np
import pytest

from multimodalsignal_amd import main as M
from multimodalsignal_amd.dataset import (WesadDataset, map_labels, normalise_subject, parse_reference, reference_mask,
                                          subject_reference)

PATTERN = [1, 1, 2, 3, 4, 1, 2]          # baseline windows 0, 1 and 5: not contiguous in file order


@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(golden_dir / "norm_reference.npz", allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.fixture()
def golden_files(golden, tmp_path):
    """The fixture's raw subjects as the files a data directory holds."""
    for sid in golden["subjects"]:
        np.save(tmp_path / f"{sid}_X.npy", golden[f"X_{sid}"])
        np.save(tmp_path / f"{sid}_y.npy", golden[f"y_{sid}"])
    return tmp_path


def _dataset(path, golden, mode, **kw):
    return WesadDataset(path, [str(s) for s in golden["subjects"]], [str(c) for c in golden["channels_to_use"]],
                        [str(c) for c in golden["all_channel_names"]], classification_mode=mode, **kw)


def _restated(x, names, ref):
    """The rule in five lines: statistics of the reference windows, applied to all windows."""
    v = np.stack([np.log1p(x[:, :, c]) if n == "chest_EDA" else x[:, :, c] for c, n in enumerate(names)], axis=2)
    m = np.stack([v[ref][:, :, c].mean() for c in range(len(names))])
    s = np.stack([v[ref][:, :, c].std() for c in range(len(names))])
    return (v - m) / (s + 1e-8)


def test_fixture_is_the_set_the_tests_rely_on(golden):
    names, sel = [str(c) for c in golden["all_channel_names"]], [str(c) for c in golden["channels_to_use"]]
    cols = [names.index(c) for c in sel]
    assert sorted(cols) == list(range(5)) and cols != sorted(cols) and 0 < sel.index("chest_EDA") < 4
    assert golden["y_S2"].tolist() == PATTERN and golden["X_S2"].shape == (7, 64, 5)
    for sid in golden["subjects"]:
        x, y = golden[f"X_{sid}"], golden[f"y_{sid}"]
        assert (y == 1).any() and not (y == 1).all()
        assert (x[:, :, names.index("chest_EDA")] > 0).all() and np.ptp(x[:, :, names.index("chest_EMG")]) == 0
        assert abs(x[:, :, names.index("chest_Temp")].mean() - 33) < 0.2 and x[:, :, names.index("chest_Temp")].std() < 0.1


@pytest.mark.parametrize("mode,ref_mode", [("stress_binary", "binary"), ("ternary", "ternary")])
def test_baseline_reference_is_the_references_dataset_bit_for_bit(golden, golden_files, mode, ref_mode):
    ds = _dataset(golden_files, golden, mode, reference="baseline")
    assert ds.data.dtype == np.float64 and ds.data.shape == golden[f"data_{ref_mode}"].shape
    assert np.array_equal(ds.data, golden[f"data_{ref_mode}"])            # bit for bit, channel order as selected
    assert np.array_equal(ds.labels, golden[f"labels_{ref_mode}"])
    sel = [str(c) for c in golden["channels_to_use"]]
    assert np.all(ds.data[:, :, sel.index("chest_EMG")] == 0)             # the constant channel
    # and it is not the whole-recording rule
    assert not np.array_equal(ds.data, _dataset(golden_files, golden, mode).data)


def test_subject_reference_and_absent_keyword_are_todays_rule(golden, golden_files):
    names, sel = [str(c) for c in golden["all_channel_names"]], [str(c) for c in golden["channels_to_use"]]
    cols = [names.index(c) for c in sel]
    want = np.concatenate([normalise_subject(golden[f"X_{sid}"][:, :, cols], sel) for sid in golden["subjects"]])
    a, b = _dataset(golden_files, golden, "stress_binary"), _dataset(golden_files, golden, "stress_binary", reference="subject")
    assert np.array_equal(a.data, want) and np.array_equal(b.data, want) and np.array_equal(a.labels, b.labels)


def test_reference_forms():
    y = np.array(PATTERN)
    assert reference_mask(y, "subject").tolist() == [True] * 7
    assert np.flatnonzero(reference_mask(y, "baseline")).tolist() == [0, 1, 5]
    assert np.flatnonzero(reference_mask(y, "baseline:1")).tolist() == [0]
    assert np.flatnonzero(reference_mask(y, "baseline:2")).tolist() == [0, 1]
    assert np.flatnonzero(reference_mask(y, "baseline:3")).tolist() == [0, 1, 5]
    assert np.flatnonzero(reference_mask(y, "baseline:99")).tolist() == [0, 1, 5]
    assert reference_mask(y, "baseline").dtype == bool and not reference_mask(np.array([2, 3]), "baseline:4").any()
    assert (parse_reference("subject"), parse_reference("baseline"), parse_reference("baseline:7")) == (None, 0, 7)
    for bad in ("baseline:0", "baseline:-1", "baseline:", "baseline:1.5", "baseline:x", "Baseline", "", "rest", None, 3, "baseline: 2",
                "baseline:+2"):
        with pytest.raises(ValueError):
            reference_mask(y, bad)
        with pytest.raises(ValueError):
            WesadDataset(".", ["S2"], ["a"], ["a"], reference=bad)


@pytest.mark.parametrize("K,windows", [(2, [0, 1]), (3, [0, 1, 5]), (99, [0, 1, 5])])
def test_first_k_baseline_windows(golden, golden_files, K, windows):
    names, sel = [str(c) for c in golden["all_channel_names"]], [str(c) for c in golden["channels_to_use"]]
    cols = [names.index(c) for c in sel]
    ds = WesadDataset(golden_files, ["S2"], sel, names, reference=f"baseline:{K}")
    ref = np.zeros(7, dtype=bool)
    ref[windows] = True
    want = _restated(golden["X_S2"][:, :, cols], sel, ref)
    scale = np.maximum(1.0, np.abs(want))
    assert np.max(np.abs(ds.data - want) / scale) < 1e-12        # float64 against float64: rounding of two equivalent expressions
    assert np.array_equal(ds.data, normalise_subject(golden["X_S2"][:, :, cols], sel, ref))
    full = WesadDataset(golden_files, ["S2"], sel, names, reference="baseline")
    assert np.array_equal(ds.data, full.data) == (K >= 3)


def test_subject_without_baseline_falls_back_to_the_subject_rule_with_one_warning(golden, tmp_path, capsys):
    names, sel = [str(c) for c in golden["all_channel_names"]], [str(c) for c in golden["channels_to_use"]]
    x = golden["X_S3"][:5].copy()
    np.save(tmp_path / "S9_X.npy", x)
    np.save(tmp_path / "S9_y.npy", np.array([2, 3, 4, 2, 3]))
    capsys.readouterr()
    for ref in ("baseline", "baseline:2"):
        got = WesadDataset(tmp_path, ["S9"], sel, names, reference=ref)
        out = capsys.readouterr().out
        assert out.count("S9") == 1 and len(out.strip().splitlines()) == 1 and "no baseline window" in out
        want = WesadDataset(tmp_path, ["S9"], sel, names)
        assert capsys.readouterr().out == ""
        assert np.array_equal(got.data, want.data) and np.array_equal(got.labels, want.labels)
        assert not np.array_equal(got.data, x[:, :, [names.index(c) for c in sel]])          # normalised, unlike the reference's fallback
    assert subject_reference(np.array([2, 3]), "subject", "S9") is None and capsys.readouterr().out == ""


def test_amusement_binary_takes_the_mask_before_rows_are_dropped(golden, golden_files):
    names, sel = [str(c) for c in golden["all_channel_names"]], [str(c) for c in golden["channels_to_use"]]
    cols = [names.index(c) for c in sel]
    y_raw = golden["y_S2"]
    y = map_labels(y_raw, "amusement_binary")
    for ref in ("baseline", "baseline:2"):
        ds = WesadDataset(golden_files, ["S2"], sel, names, classification_mode="amusement_binary", reference=ref)
        full = normalise_subject(golden["X_S2"][:, :, cols], sel, reference_mask(y_raw, ref))
        assert len(ds) == 4 and np.array_equal(ds.labels, y[y >= 0]) and np.array_equal(ds.data, full[y >= 0])
    # "baseline:2" is windows 0 and 1 of the FILE; the kept rows' first two baseline windows would be the same here, the third not
    a = WesadDataset(golden_files, ["S2"], sel, names, classification_mode="amusement_binary", reference="baseline:3")
    b = WesadDataset(golden_files, ["S2"], sel, names, classification_mode="stress_binary", reference="baseline:3")
    assert np.array_equal(a.data, b.data[y >= 0])


def test_cache_key_separates_references(golden, golden_files):
    cache = {}
    a = _dataset(golden_files, golden, "stress_binary", cache=cache)
    n = len(cache)
    b = _dataset(golden_files, golden, "stress_binary", cache=cache, reference="baseline")
    assert len(cache) == 2 * n and not np.array_equal(a.data, b.data)
    c = _dataset(golden_files, golden, "stress_binary", cache=cache, reference="baseline:1")
    assert len(cache) == 3 * n and not np.array_equal(b.data, c.data)
    again = _dataset(golden_files, golden, "stress_binary", cache=cache, reference="baseline")
    assert len(cache) == 3 * n and np.array_equal(again.data, b.data)
    assert np.array_equal(_dataset(golden_files, golden, "stress_binary", cache=cache).data, a.data)


# ---- the flag ----------------------------------------------------------------------------------------------------------

def _cfg(argv):
    ap = M.build_parser()
    args = M.parse_args(ap, argv)
    return M.build_cfg(args, [k for k in M.MODEL_PARAMS if k in args.model])


def test_key_exists_only_with_the_flag():
    assert "norm_reference" not in _cfg([]) and M.norm_reference(_cfg([])) == "subject"
    assert "norm_reference" not in _cfg(["--hierarchical"]) and "norm_reference" not in _cfg(["--ablation", "--seeds", "2"])
    assert _cfg(["--norm-reference", "baseline"])["norm_reference"] == "baseline"
    assert _cfg(["--norm-reference", "subject"])["norm_reference"] == "subject"
    assert _cfg(["--norm-reference", "baseline:30", "--hierarchical"])["norm_reference"] == "baseline:30"
    assert _cfg(["--norm-reference", "subject", "baseline", "baseline:6"])["norm_reference"] == ["subject", "baseline", "baseline:6"]
    # one value goes with everything
    for extra in (["--calibrate", "4"], ["--adapt-bn"], ["--attribute"], ["--mc-dropout"], ["--seeds", "2"], ["--weight-average", "ema"],
                  ["--model", "cnn_gru_attention", "cnn_gru"], ["--ablation"], ["--subject-adversarial"]):
        assert _cfg(["--norm-reference", "baseline"] + extra)["norm_reference"] == "baseline"
    assert _cfg(["--norm-reference", "subject", "baseline", "--ablation"])["norm_reference"] == ["subject", "baseline"]


@pytest.mark.parametrize("argv", [
    ["--norm-reference", "baseline:0"], ["--norm-reference", "rest"], ["--norm-reference", "subject", "baseline:x"],
    ["--norm-reference", "baseline", "baseline"], ["--norm-reference"],
    ["--norm-reference", "subject", "baseline", "--model", "cnn_gru_attention", "cnn_gru"],
    ["--norm-reference", "subject", "baseline", "--hierarchical"],
    ["--norm-reference", "subject", "baseline", "--calibrate", "4"],
    ["--norm-reference", "subject", "baseline", "--adapt-bn"],
    ["--norm-reference", "subject", "baseline", "--attribute"],
    ["--norm-reference", "subject", "baseline", "--mc-dropout"],
    ["--norm-reference", "subject", "baseline", "--seeds", "2"],
    ["--norm-reference", "subject", "baseline", "--weight-average", "ema"],
], ids=lambda a: " ".join(a))
def test_refused_combinations_error_before_any_gpu_work(argv, capsys):
    with pytest.raises(SystemExit) as e:
        _cfg(argv)
    assert e.value.code == 2
    assert "--norm-reference" in capsys.readouterr().err


def test_summary_echoes_the_reference_only_with_the_flag(tmp_path):
    results = [{"subject": "S2", "accuracy": 0.5, "f1_score": 0.4}]
    text = M.write_summary(tmp_path, results, _cfg([]), 1.0, 1).read_text(encoding="utf-8")
    assert "NORM_REFERENCE" not in text
    with_flag = M.write_summary(tmp_path, results, _cfg(["--norm-reference", "baseline:3"]), 1.0, 1).read_text(encoding="utf-8")
    assert with_flag.replace("NORM_REFERENCE: baseline:3\n", "") == text and with_flag != text


def test_normalisation_table(tmp_path):
    subjects = ["S2", "S3", "S4"]
    for sid, y in zip(subjects, ([1, 1, 2, 3, 4, 1, 2], [2, 3, 4, 2, 3], [1, 2, 1, 2])):
        np.save(tmp_path / f"{sid}_y.npy", np.array(y))
    acc = {"subject": [0.9, 0.8, 0.7], "baseline": [0.8, 0.8, 0.9], "baseline:2": [0.9, 0.7, 0.7]}
    per_ref = {r: [{"subject": s, "accuracy": a, "f1_score": a / 2} for s, a in zip(subjects, v)] for r, v in acc.items()}
    t = M.normalisation({"": per_ref}, list(acc), tmp_path, subjects)
    assert t["anchor"] == "subject" and t["references"] == list(acc)
    st = t["sets"][""]["references"]
    assert st["subject"]["difference"]["accuracy"] == {"mean": 0.0, "std": 0.0, "wins": 0, "ties": 3, "losses": 0}
    d = st["baseline"]["difference"]["accuracy"]
    assert (d["wins"], d["ties"], d["losses"]) == (1, 1, 1) and abs(d["mean"] - np.mean([-0.1, 0.0, 0.2])) < 1e-12
    assert abs(st["baseline"]["summary"]["accuracy"]["mean"] - np.mean(acc["baseline"])) < 1e-12
    assert abs(st["baseline"]["summary"]["f1_score"]["std"] - np.std(np.array(acc["baseline"]) / 2)) < 1e-12
    assert [f["subject"] for f in st["baseline:2"]["folds"]] == subjects
    assert abs(st["baseline:2"]["folds"][1]["difference"]["accuracy"] + 0.1) < 1e-12
    w = t["reference_windows"]
    assert w["baseline"]["S2"] == {"n_windows": 7, "reference_windows": 3, "fallback": False}
    assert w["baseline:2"]["S2"]["reference_windows"] == 2 and w["baseline:2"]["S4"]["reference_windows"] == 2
    assert w["baseline"]["S3"] == {"n_windows": 5, "reference_windows": 5, "fallback": True}
    assert w["subject"]["S3"] == {"n_windows": 5, "reference_windows": 5, "fallback": False}
    # without "subject" the first reference is the anchor
    t2 = M.normalisation({"": {r: per_ref[r] for r in ("baseline:2", "baseline")}}, ["baseline:2", "baseline"], tmp_path, subjects)
    assert t2["anchor"] == "baseline:2" and t2["sets"][""]["references"]["baseline"]["difference"]["accuracy"]["wins"] == 2
    path = M.write_normalisation(tmp_path, t, synthetic=True)
    text = path.read_text(encoding="utf-8")
    assert path.name == "normalisation.txt" and (tmp_path / "normalisation.json").exists()
    assert "not what a reference costs or gains on WESAD" in text and "S3 5/5 fallback" in text
