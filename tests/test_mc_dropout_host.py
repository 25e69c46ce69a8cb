"""Monte-Carlo dropout, the parts that need no GPU (multimodalsignal_amd/uncertainty.py): the chunk plan and its keys, the host
metrics against sklearn and against the slow restatement (tests/mc_reference.py), the restatement of the reduction against
vectorised numpy, the tables' round trip and the command line."""
import json

import numpy as np
import pytest
import torch

import mc_reference as R
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd import uncertainty as U
from oracle import cnn_gru_oracle as O


def test_chunk_plan_and_keys():
    assert U.chunk_plan(5, 3, 2) == [(0, 0, 2), (1, 2, 2), (2, 4, 1)]
    assert [U.chunk_keys(9, j) for j, _, _ in U.chunk_plan(5, 3, 2)] == [(L.dropout_key(9, j, 1), L.dropout_key(9, j, 2)) for j in (0, 1, 2)]
    assert U.chunk_keys(9, 1) == (O.dropout_key(9, 1, O.STREAM_GRU), O.dropout_key(9, 1, O.STREAM_HEAD))
    assert len({U.chunk_keys(9, j) for j in range(3)} | {U.chunk_keys(10, 0)}) == 4
    # the default: the most windows with chunk * S <= 2048 rows, at least one
    assert U.default_chunk(32) == 64 and U.default_chunk(1) == 2048 and U.default_chunk(256) == 8 and U.default_chunk(7) == 292
    assert U.chunk_plan(64, 32) == [(0, 0, 64)] and U.chunk_plan(65, 32) == [(0, 0, 64), (1, 64, 1)]
    assert U.chunk_plan(3, 5, 100) == [(0, 0, 3)]
    with pytest.raises(ValueError):
        U.chunk_plan(0, 3, 2)


def test_argument_errors_are_raised_before_anything_is_launched():
    from multimodalsignal_amd.models import CnnGruAttentionModel
    m = CnnGruAttentionModel(6, 3)          # on the CPU: anything that reached the engine would raise RuntimeError, not ValueError
    for kw in (dict(samples=0), dict(samples=257), dict(samples=2.0), dict(samples=True), dict(seed=-1), dict(seed=1 << 64), dict(seed=0.5),
               dict(chunk=0), dict(chunk=-1), dict(chunk=1.5)):
        with pytest.raises(ValueError):
            m.predict_mc(torch.zeros(2, 6, 256), **kw)
    with pytest.raises(ValueError, match="GPU tensor"):
        m.predict_mc(torch.zeros(2, 6, 256))
    mc = U.McDropout(m, samples=7)
    assert (mc.S, mc.seed, mc.chunk, mc.thr) == (7, 0, 292, 128)


def test_auroc_against_sklearn_with_ties():
    from sklearn.metrics import roc_auc_score
    rs = np.random.RandomState(0)
    for n, levels in ((40, None), (60, 5), (25, 2), (7, 1)):
        score = rs.rand(n) if levels is None else rs.randint(0, levels, size=n).astype(np.float64)          # few levels: many ties
        pos = rs.rand(n) < 0.3
        pos[0], pos[1] = True, False
        got = U.auroc(score, pos)
        assert got == pytest.approx(roc_auc_score(pos, score), abs=1e-12)
        assert got == pytest.approx(R.auroc_pairs(score.tolist(), pos.tolist()), abs=1e-12)
    assert U.auroc([0.1, 0.1, 0.1], [True, False, False]) == 0.5          # all tied
    assert U.auroc([0.3, 0.2, 0.1], [True, False, False]) == 1.0 and U.auroc([0.1, 0.2, 0.3], [True, False, False]) == 0.0


def test_auroc_is_none_without_errors_or_without_correct_windows():
    assert U.auroc([0.1, 0.2], [False, False]) is None and U.auroc([0.1, 0.2], [True, True]) is None
    w = dict(correct_eval=[True, True], correct_mc=[True, True], conf_eval=[0.9, 0.8], conf_mc=[0.9, 0.8], entropy=[0.1, 0.2],
             mutual_information=[0.0, 0.01])
    r = U.window_metrics(w)
    assert r["auroc_entropy"] is None and r["entropy_wrong"] is None and r["mutual_information_wrong"] is None and r["accuracy_mc"] == 1.0
    assert json.loads(json.dumps(r))["auroc_entropy"] is None             # null in the files
    r = U.window_metrics(dict(w, correct_mc=[False, False]))
    assert r["auroc_entropy"] is None and r["entropy_correct"] is None and r["accuracy_mc"] == 0.0


def test_selective_accuracy_on_hand_built_arrays():
    #            window   0     1     2     3     4     5     6     7     8     9
    correct = [True, False, True, True, False, True, True, True, False, True]
    unc = [0.1, 0.9, 0.2, 0.5, 0.5, 0.5, 0.0, 0.3, 0.8, 0.4]
    got = U.selective_accuracy(correct, unc)
    # 90 %: window 1 goes; 80 %: 1 and 8; 50 %: kept are 6, 0, 2, 7, 9 — of the three tied at 0.5 the higher indices go first
    assert got == {"100": 0.7, "90": 7 / 9, "80": 7 / 8, "50": 1.0}
    assert U.selective_accuracy(correct, unc, (70, 60)) == {"70": 6 / 7, "60": 1.0}          # 70 %: windows 3 and 4 of the tie stay: 3 is right, 4 wrong
    for cov in (100, 90, 80, 70, 60, 50, 33):
        assert U.selective_accuracy(correct, unc, (cov,))[str(cov)] == pytest.approx(R.selective(correct, unc, cov))
    assert U.selective_accuracy([True, False, True], [0.3, 0.2, 0.1], (50,)) == {"50": 0.5}   # ceil(1.5) = 2 kept


def test_ece_on_hand_built_arrays():
    # two bins of 15: (0.6, 0.6667] holds 0.62, 0.64 (one right), (0.9333, 1] holds 0.95, 0.97, 0.99, 1.0 (three right)
    conf, ok = [0.62, 0.64, 0.95, 0.97, 0.99, 1.0], [True, False, True, True, False, True]
    want = (abs(0.5 - 0.63) * 2 + abs(0.75 - 0.9775) * 4) / 6
    assert U.expected_calibration_error(conf, ok) == pytest.approx(want, abs=1e-12) == pytest.approx(R.ece(conf, ok), abs=1e-12)
    assert U.expected_calibration_error([1.0, 1.0], [True, True]) == 0.0
    assert U.expected_calibration_error([0.5, 0.5], [True, False]) == 0.0
    rs = np.random.RandomState(1)
    conf, ok = (0.34 + 0.66 * rs.rand(200)).tolist(), (rs.rand(200) < 0.7).tolist()
    assert U.expected_calibration_error(conf, ok) == pytest.approx(R.ece(conf, ok), abs=1e-12)


def test_restatement_of_the_reduction():
    """The explicit loops against vectorised numpy (another order of summation: to 1e-12), and the edge cases by hand."""
    rs = np.random.RandomState(2)
    N, S, K = 4, 7, 3
    lg = (3 * rs.randn(N * S, K)).astype(np.float32)
    lg[0:S] = lg[0]                                       # window 0: all samples equal
    lg[S, :] = [60.0, 0.0, 0.0]                           # window 1: one saturated row
    r = R.reduce(lg, N, S, K)
    x = lg.astype(np.float64).reshape(N, S, K)
    p = np.exp(x - x.max(axis=2, keepdims=True))
    p /= p.sum(axis=2, keepdims=True)
    m = p.mean(axis=1)
    H = lambda q: -(np.where(q > 0, q * np.log(np.where(q > 0, q, 1.0)), 0.0)).sum(axis=-1)
    assert np.allclose(r["mean_p"], m, atol=1e-12, rtol=0) and np.allclose(r["std_p"], p.std(axis=1), atol=1e-12, rtol=0)
    assert np.allclose(r["entropy"], H(m), atol=1e-12, rtol=0) and np.allclose(r["expected_entropy"], H(p).mean(axis=1), atol=1e-12, rtol=0)
    assert np.array_equal(r["mutual_info"], r["entropy"] - r["expected_entropy"])
    assert np.array_equal(r["pred"], m.argmax(axis=1)) and np.array_equal(r["votes"].sum(axis=1), np.full(N, S))
    assert np.array_equal(r["votes"], np.stack([np.bincount(x[n].argmax(axis=1), minlength=K) for n in range(N)]))
    assert np.all(r["std_p"][0] <= 1e-12)                 # (7 p) / 7 is p only to a rounding
    assert abs(r["mutual_info"][0]) <= 1e-12 and r["votes"][0].max() == S
    # an exact two-way tie: the first maximum wins, in the votes and in the prediction
    t = R.reduce(np.array([[1.0, 1.0, 0.0], [2.0, 2.0, -1.0]], dtype=np.float32), 1, 2, 3)
    assert t["votes"].tolist() == [[2, 0, 0]] and t["pred"].tolist() == [0] and t["mean_p"][0, 0] == t["mean_p"][0, 1]
    # 0 ln 0 = 0: a gap wide enough for exp to underflow
    z = R.reduce(np.array([[0.0, -800.0]], dtype=np.float32), 1, 1, 2)
    assert z["mean_p"].tolist() == [[1.0, 0.0]] and z["entropy"][0] == 0.0 and z["expected_entropy"][0] == 0.0
    assert np.array_equal(R.expand(np.arange(6).reshape(2, 3), 2), [[0, 1, 2], [0, 1, 2], [3, 4, 5], [3, 4, 5]])


def _fold(subject, seed, n=12, all_right=False):
    rs = np.random.RandomState(seed)
    ok = np.ones(n, dtype=bool) if all_right else rs.rand(n) < 0.7
    w = dict(correct_eval=ok.tolist(), correct_mc=ok.tolist(), conf_eval=(0.5 + 0.5 * rs.rand(n)).tolist(), conf_mc=(0.5 + 0.5 * rs.rand(n)).tolist(),
             entropy=rs.rand(n).tolist(), mutual_information=(0.1 * rs.rand(n)).tolist())
    return dict(U.window_metrics(w), subject=subject, samples=4, seed=0, chunk=512, dropout=0.5, windows=w)


def test_summary_and_formatting_round_trip(tmp_path):
    folds = [_fold("S2", 1), _fold("S3", 2), _fold("S4", 3, all_right=True)]
    path = U.write_uncertainty(tmp_path, folds, {"samples": 4, "seed": 0, "dropout": 0.5}, synthetic=True)
    doc = json.loads((tmp_path / "uncertainty.json").read_text())
    assert doc["n_folds"] == 3 and [f["subject"] for f in doc["folds"]] == ["S2", "S3", "S4"] and doc["note"] == U.SYNTHETIC_NOTE
    assert doc["settings"] == {"samples": 4, "seed": 0, "dropout": 0.5}
    keys = {"n", "accuracy_eval", "accuracy_mc", "entropy_correct", "entropy_wrong", "mutual_information_correct", "mutual_information_wrong",
            "auroc_entropy", "selective_accuracy", "ece_eval", "ece_mc"}
    for f, src in zip(doc["folds"], folds):
        assert keys <= set(f) and "windows" not in f and f == {k: v for k, v in json.loads(json.dumps(src)).items() if k != "windows"}
        assert set(f["selective_accuracy"]) == {"100", "90", "80", "50"}
    assert doc["folds"][2]["auroc_entropy"] is None and doc["folds"][2]["entropy_wrong"] is None
    # the pooled row is the metrics of all windows together, not a mean of the folds' rows
    pooled = U.window_metrics({k: sum((f["windows"][k] for f in folds), []) for k in U.WINDOW_KEYS})
    assert set(doc["pooled"]) == keys and doc["pooled"] == json.loads(json.dumps(pooled)) and doc["pooled"]["n"] == 36
    assert doc["pooled"]["auroc_entropy"] == pytest.approx(R.auroc_pairs(sum((f["windows"]["entropy"] for f in folds), []),
                                                                         [not c for f in folds for c in f["windows"]["correct_mc"]]), abs=1e-12)
    txt = path.read_text(encoding="utf-8")
    assert path.name == "uncertainty.txt" and U.SYNTHETIC_NOTE in txt and all(s in txt for s in ("S2", "S3", "S4", "pooled", "n/a", "sel@90"))
    assert "machinery works" in U.SYNTHETIC_NOTE and "not what abstention is worth on WESAD" in U.SYNTHETIC_NOTE
    assert U.format_uncertainty(U.summarise_uncertainty(folds), {"samples": 4, "seed": 0, "dropout": 0.5}, True) == txt
    assert U.SYNTHETIC_NOTE not in U.format_uncertainty(U.summarise_uncertainty(folds))


def test_cli_flag():
    from multimodalsignal_amd import main as M
    ap = M.build_parser()
    base = ["--synthetic", "/tmp/x"]
    a = M.parse_args(ap, base)
    cfg = M.build_cfg(a, ["cnn_gru_attention"])
    assert a.mc_dropout is None and "mc_dropout" not in cfg and "mc_seed" not in cfg           # without the flag: no such key
    a = M.parse_args(ap, base + ["--mc-dropout"])
    cfg = M.build_cfg(a, ["cnn_gru_attention"])
    assert a.mc_dropout == 32 and cfg["mc_dropout"] == 32 and cfg["mc_seed"] == 0 and cfg["synthetic"] is True
    assert M.uncertainty_settings(cfg) == {"samples": 32, "seed": 0, "dropout": 0.5}
    a = M.parse_args(ap, base + ["--mc-dropout", "4", "--mc-seed", "11", "--model", "cnn_gru", "cnn_gru_attention"])
    cfg = M.build_cfg(a, ["cnn_gru_attention", "cnn_gru"])
    assert cfg["mc_dropout"] == 4 and cfg["mc_seed"] == 11
    a = M.parse_args(ap, base + ["--mc-dropout", "--attribute", "--adapt-bn", "--calibrate", "8"])          # may be combined
    cfg = M.build_cfg(a, ["cnn_gru_attention"])
    assert cfg["mc_dropout"] == 32 and cfg["attribute"] == 32 and cfg["adapt_bn"] == 1.0 and cfg["calibrate"] == 8
    for bad in (["--mc-dropout", "0"], ["--mc-dropout", "257"], ["--mc-dropout", "-3"], ["--mc-seed", "3"], ["--mc-dropout", "4", "--mc-seed", "-1"],
                ["--mc-dropout", "--hierarchical"], ["--mc-dropout", "--ablation"], ["--mc-dropout", "--sweep"]):
        with pytest.raises(SystemExit):
            M.parse_args(ap, base + bad)


def test_rejection_wording_is_the_other_stages(capsys):
    from multimodalsignal_amd import main as M
    ap = M.build_parser()
    msgs = []
    for flag in (["--mc-dropout"], ["--attribute"]):
        with pytest.raises(SystemExit):
            M.parse_args(ap, ["--synthetic", "/tmp/x", "--hierarchical"] + flag)
        msgs.append(capsys.readouterr().err.strip().splitlines()[-1].split("error: ")[1])
    assert msgs[0] == msgs[1].replace("--attribute", "--mc-dropout")
