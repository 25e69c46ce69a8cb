"""Seed replicas and deep ensembles (multimodalsignal_amd/ensemble.py): everything that needs no GPU — the seed
rule, the dealing of replicas, the tables over seeds, the ensemble's metrics, the command line, and the fp64 restatement
(tests/en_reference.py) against the Monte-Carlo one on the transposed stack."""
import math

import numpy as np
import pytest

import en_reference as E
import mc_reference as R
from multimodalsignal_amd import ensemble as EN
from multimodalsignal_amd import main as M
from multimodalsignal_amd.loso import split_train_val


def test_replica_seed_rule():
    for k in (0, 3, 14):
        assert EN.replica_seed(42, k, 0) == 42 + k == EN.replica_seed(42, k)          # replica 0 is today's unit
        assert EN.replica_seed(42, k, 2) == 42 + k + 2 * 1_000_003
    seeds = {EN.replica_seed(42, k, r) for r in range(64) for k in range(64)}
    assert len(seeds) == 64 * 64
    # the split is seeded by the run's seed, never by a replica's: prepare_fold passes the replica seed to the unit alone
    subs = [f"S{i}" for i in range(2, 18) if i != 12]
    assert split_train_val(subs, "S5", 42) == split_train_val(subs, "S5", M.default_cfg()["seed"])
    assert EN.replica_name("", 0) == "" and EN.replica_name("", 2) == "seed_2" and EN.replica_name("cnn_gru", 1) == "cnn_gru/seed_1"
    for bad in (0, 65, -1, 2.0, True, "3"):
        with pytest.raises(ValueError):
            EN.check_seeds(bad)
    assert EN.check_seeds(1) == 1 and EN.check_seeds(64) == 64


def _cfgs(names, n_subjects=15):
    return {n: dict(subjects=[f"S{i}" for i in range(n_subjects)]) for n in names}


@pytest.mark.parametrize("world", [1, 2, 4])
@pytest.mark.parametrize("names", [[""], ["cnn_gru_attention", "cnn_gru"]])
def test_one_seed_deals_as_today(world, names):
    cfgs = _cfgs(names)
    for rank in range(world):
        units, mine, groups = M.rank_units(cfgs, world, rank)
        assert EN.deal_replicas(units, mine, 1) == (units, mine, groups)


@pytest.mark.parametrize("names", [[""], ["a", "b"]])
def test_three_seeds_on_two_ranks(names):
    cfgs, S, world = _cfgs(names, 5), 3, 2
    seen, owner = [], {}
    for rank in range(world):
        base_units, base_mine, _ = M.rank_units(cfgs, world, rank)
        units, mine, groups = EN.deal_replicas(base_units, base_mine, S)
        assert len(units) == S * len(base_units) and sorted(u for g in groups for u in g) == sorted(mine)
        for g in groups:
            assert len({units[u][0] for u in g}) == 1                              # a group is one replica of one configuration
        for u in mine:
            seen.append(u)
            base_name, r = base_units[u // S][0], u % S
            assert units[u] == (EN.replica_name(base_name, r), base_units[u // S][1])
            owner.setdefault((base_name, units[u][1]), set()).add(rank)
    assert sorted(seen) == list(range(S * 5 * len(names)))                         # every unit exactly once
    assert all(len(r) == 1 for r in owner.values()) and len(owner) == 5 * len(names)   # all replicas of a (configuration, fold) on one rank


def test_seed_table_by_hand():
    v = [[0.5, 1.0, 0.75, 0.75], [1.0, 1.0, 0.5, 0.5], [0.75, 0.25, 0.5, 0.5]]          # 3 seeds x 4 folds
    t = EN.seed_table(v)
    assert t["seeds"] == 3 and t["folds"] == 4 and t["per_seed"] == [0.75, 0.75, 0.5]
    assert t["mean"] == pytest.approx(2.0 / 3.0) and t["std"] == pytest.approx(math.sqrt(((1 / 12) ** 2 * 2 + (1 / 6) ** 2) / 2))
    assert t["per_fold"][0]["members"] == [0.5, 1.0, 0.75] and t["per_fold"][0]["mean"] == 0.75
    assert t["per_fold"][0]["std"] == pytest.approx(0.25) and t["per_fold"][3]["std"] == pytest.approx(math.sqrt((2 * (1 / 12) ** 2 + (1 / 6) ** 2) / 2))
    one = EN.seed_table([v[0]])
    assert one["std"] is None and one["mean"] == 0.75 and all(f["std"] is None for f in one["per_fold"])
    with pytest.raises(ValueError):
        EN.seed_table([0.5, 0.5])


def test_pair_table_by_hand():
    p = EN.pair_table([0.75, 0.5, 0.5], [0.5, 0.5, 0.75], 0.875, 0.75)
    assert p["per_seed_difference"] == [0.25, 0.0, -0.25] and p["mean"] == 0.0 and p["std"] == pytest.approx(0.25)
    assert (p["wins"], p["losses"], p["ties"], p["seeds"]) == (1, 1, 1, 3) and p["ensemble_difference"] == 0.125
    assert EN.pair_table([0.5], [0.25])["std"] is None and EN.pair_table([0.5], [0.25])["ensemble_difference"] is None
    with pytest.raises(ValueError):
        EN.pair_table([0.5, 0.5], [0.5])


def test_ensemble_metrics_by_hand():
    p = np.array([[0.75, 0.25], [0.5, 0.5], [0.25, 0.75], [0.125, 0.875]])
    y = np.array([0, 1, 1, 0])                  # predictions 0, 0 (the tie: first), 1, 1 -> correct, wrong, correct, wrong
    ent = [0.5, 0.7, 0.5, 0.3]
    mi = [0.0, 0.1, 0.0, 0.2]
    r = EN.ensemble_metrics(p, y, ent, mi, disagreement=[0.0, 1.0, 0.0, 0.5])
    assert r["n"] == 4 and r["accuracy"] == 0.5
    assert r["nll"] == pytest.approx(-(math.log(0.75) + math.log(0.5) + math.log(0.75) + math.log(0.125)) / 4)
    assert r["brier"] == pytest.approx((2 * 0.25 ** 2 + 2 * 0.5 ** 2 + 2 * 0.25 ** 2 + 2 * 0.875 ** 2) / 4)
    assert r["ece"] == pytest.approx(R.ece([0.75, 0.5, 0.75, 0.875], [True, False, True, False]))
    assert r["mean_disagreement"] == 0.375 and r["entropy_correct"] == 0.5 and r["entropy_wrong"] == 0.5
    assert r["mutual_information_wrong"] == pytest.approx(0.15) and r["mutual_information_correct"] == 0.0
    assert r["auroc_entropy"] == pytest.approx(R.auroc_pairs(ent, [False, True, False, True]))
    assert set(r["selective_accuracy"]) == {"100", "90", "80", "50"} and r["selective_accuracy"]["100"] == 0.5
    assert r["selective_accuracy"]["50"] == pytest.approx(R.selective([True, False, True, False], ent, 50))
    assert r["f1_score"] == pytest.approx(0.5)              # per class: tp 1, fp 1, fn 1 -> F1 1/2, supports 2 and 2
    assert EN.ensemble_metrics(p, y, ent, mi)["mean_disagreement"] is None
    # a probability of exactly 0 on the true class: a finite NLL
    assert math.isfinite(EN.ensemble_metrics(np.array([[1.0, 0.0]]), [1], [0.0], [0.0])["nll"])


def test_seeds_document_and_text():
    """summarise_seeds / write_seeds on hand-made fold records: two configurations, two seeds, two folds of three windows."""
    def fold(subject, shift):
        win = {"y": [0, 1, 1], "mean_p": [[0.75, 0.25], [0.25 + shift, 0.75 - shift], [0.5, 0.5]], "entropy": [0.5, 0.5, 0.69],
               "mutual_info": [0.0, 0.01, 0.02], "disagreement": [0.0, 0.0, 1.0]}
        mem = [{k: win[k] for k in ("mean_p", "entropy", "mutual_info")} for _ in range(2)]
        return dict(subject=subject, n=3, member_accuracy=[2 / 3, 1 / 3], member_f1=[0.6, 0.3], epochs=[2, 2],
                    ensemble=EN.ensemble_metrics(win["mean_p"], win["y"], win["entropy"], win["mutual_info"], win["disagreement"]),
                    windows=win, member_windows=mem)
    per = {"accuracy": [[2 / 3, 2 / 3], [1 / 3, 1 / 3]], "f1_score": [[0.6, 0.6], [0.3, 0.3]]}
    a, b = EN.summarise_seeds([fold("S2", 0.0), fold("S3", 0.0)], per), EN.summarise_seeds([fold("S2", 0.5), fold("S3", 0.5)], per)
    assert a["seeds"] == 2 and a["n_folds"] == 2 and a["ensemble"]["pooled"]["n"] == 6 and len(a["accuracy"]["per_seed"]) == 2
    assert a["folds"][0]["member_accuracy"] == [2 / 3, 1 / 3] and a["folds"][0]["member_accuracy_mean"] == pytest.approx(0.5)
    assert a["mean_member"]["loso_mean"]["accuracy"] == pytest.approx(0.5) and a["mean_member"]["pooled"]["mean_disagreement"] is None
    assert a["ensemble"]["loso_mean"]["accuracy"] == pytest.approx(2 / 3) and b["ensemble"]["loso_mean"]["accuracy"] == pytest.approx(1 / 3)
    import json, tempfile
    from pathlib import Path
    with tempfile.TemporaryDirectory() as d:
        path = EN.write_seeds(d, {"cnn_gru_attention": a, "cnn_gru": b}, 2, synthetic=True)
        doc, txt = json.loads((Path(d) / "seeds.json").read_text()), path.read_text(encoding="utf-8")
    assert doc["settings"] == {"seeds": 2, "stride": 1_000_003} and doc["note"] == EN.SYNTHETIC_NOTE and len(doc["pairs"]) == 1
    pair = doc["pairs"][0]
    assert (pair["a"], pair["b"]) == ("cnn_gru_attention", "cnn_gru") and pair["accuracy"]["per_seed_difference"] == [0.0, 0.0]
    assert pair["accuracy"]["ensemble_difference"] == pytest.approx(1 / 3) and pair["accuracy"]["ties"] == 2
    assert EN.format_seeds(doc) == txt and EN.SYNTHETIC_NOTE in txt
    for word in ("ensemble", "mean member", "per seed", "S2", "S3", "pairs of configurations", "cnn_gru_attention - cnn_gru"):
        assert word in txt, word


def test_command_line():
    ap = M.build_parser()
    base = ["--synthetic", "/tmp/x"]
    cfg = M.build_cfg(M.parse_args(ap, base), ["cnn_gru_attention"])
    assert "seeds" not in cfg
    assert M.build_cfg(M.parse_args(ap, base + ["--seeds", "1"]), ["cnn_gru_attention"]) == cfg          # --seeds 1 is the run without it
    cfg3 = M.build_cfg(M.parse_args(ap, base + ["--seeds", "3", "--mixup", "0.2", "--weight-average", "ema"]), ["cnn_gru_attention"])
    assert cfg3["seeds"] == 3 and cfg3["synthetic"] is True
    assert M.parse_args(ap, base + ["--seeds", "2", "--ablation"]).seeds == 2 and M.parse_args(ap, base + ["--seeds", "2", "--sweep", "a=chest_ECG"]).seeds == 2
    assert M.parse_args(ap, base + ["--seeds", "64", "--model", "cnn_gru", "cnn_gru_attention", "--mc-dropout"]).seeds == 64
    for bad in (["--seeds", "0"], ["--seeds", "65"], ["--seeds", "-2"], ["--seeds", "x"], ["--seeds", "2", "--hierarchical"]):
        with pytest.raises(SystemExit):
            M.parse_args(ap, base + bad)
    assert M.parse_args(ap, base + ["--seeds", "1", "--hierarchical"]).seeds == 1


@pytest.mark.parametrize("M_,K", [(1, 2), (4, 3), (7, 16)])
def test_restatement_agrees_with_the_monte_carlo_one_on_the_transpose(M_, K):
    N = 5
    lg = E.crafted_logits(M_, N, K, 10 * M_ + K)
    mine, theirs = E.reduce(lg), R.reduce(np.ascontiguousarray(lg.transpose(1, 0, 2)).reshape(N * M_, K), N, M_, K)
    for name in E.COMMON:
        assert np.array_equal(mine[name], theirs[name]), name          # the same sums in the same order: equal in fp64
    assert np.array_equal(mine["member_pred"], lg.argmax(axis=2).T)
    assert mine["votes"][1, 0] == M_ and mine["disagreement"][1] == 0.0 and mine["disagreement"][2] == 0.0
    if M_ == 1:
        assert np.all(mine["disagreement"] == 0.0)


def test_disagreement_by_hand():
    assert E.disagreement_from_votes([2, 2], 4) == pytest.approx(4 / 6)          # 6 pairs, 2 of them agree
    assert E.disagreement_from_votes([4, 0], 4) == 0.0 and E.disagreement_from_votes([1, 1, 1], 3) == 1.0
    assert E.disagreement_from_votes([1, 0], 1) == 0.0
    lg = np.zeros((4, 1, 2), dtype=np.float32)
    lg[:2, 0, 0], lg[2:, 0, 1] = 1.0, 1.0                                        # members 0, 1 say class 0; members 2, 3 class 1
    r = E.reduce(lg)
    assert r["votes"].tolist() == [[2, 2]] and r["member_pred"].tolist() == [[0, 0, 1, 1]] and r["disagreement"][0] == pytest.approx(4 / 6)
    assert r["pred"][0] == 0 and r["mean_p"][0, 0] == r["mean_p"][0, 1] == 0.5
