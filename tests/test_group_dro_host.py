"""Group-DRO (include/msig_dro.h) on the host: the numpy restatement (tests/dro_reference.py) against torch
autograd of the robust loss, the group tables, the settings and the command line's refusals, and the report writer."""
import json
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dro_reference as R
from multimodalsignal_amd import dro as D


def _case(B, K, G, seed, weights, absent=(), ungrouped=0):
    rs = np.random.RandomState(seed)
    z = (2.0 * rs.randn(B, K)).astype(np.float32)
    y = rs.randint(0, K, size=B).astype(np.int64)
    pool = [g for g in range(G) if g not in absent]
    grp = np.array([pool[i % len(pool)] for i in rs.permutation(B)], dtype=np.int32)
    grp[:ungrouped] = [-1, G, -7, G + 5][:ungrouped]
    q = rs.rand(G) + 0.1
    q = (q / q.sum()).astype(np.float32)
    w = (0.25 + rs.rand(K)).astype(np.float32) if weights else None
    return z, y, grp, q, w


@pytest.mark.parametrize("weights,eps", [(False, 0.0), (True, 0.1)], ids=["plain", "weighted-smoothed"])
@pytest.mark.parametrize("G", [1, 3, 33])
@pytest.mark.parametrize("K", [2, 3, 16])
def test_restatement_is_the_gradient_of_the_robust_loss(K, G, weights, eps):
    """dlogits of the restatement = d/dz sum_{g present} q_g F.cross_entropy(z[g], y[g], weight, label_smoothing) with the updated q
    held constant, in fp64 to 1e-12; absent groups and rows in no group (which get exactly zero) included."""
    B = 140                                      # every pooled group keeps rows after four of them leave their groups
    absent = () if G == 1 else (1,) if G == 3 else (0, 7, 32)
    z, y, grp, q, w = _case(B, K, G, 100 * K + G, weights, absent, ungrouped=0 if G == 1 else 4)
    out = R.apply(z, y, grp, q, 0.3, G, w, eps, dlogits=R.criterion_dlogits(z, y, w, eps))
    assert out["wrote"] and [p for p in range(G) if not out["present"][p]] == list(absent)
    assert abs(out["q"].sum() - 1.0) < 1e-6 and np.array_equal(out["q"], out["q"].astype(np.float32).astype(np.float64))
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    yt = torch.tensor(y)
    wt = None if w is None else torch.tensor(w, dtype=torch.float64)
    groups = np.array(out["groups"])
    loss, robust = 0.0, 0.0
    for g in range(G):
        rows = torch.tensor(np.nonzero(groups == g)[0])
        if len(rows):
            Lg = F.cross_entropy(zt[rows], yt[rows], weight=wt, label_smoothing=float(np.float32(eps)))
            loss = loss + float(out["q"][g]) * Lg
            assert abs(float(Lg.detach()) - out["T"][g] / out["W_g"][g]) < 1e-12
    loss.backward()
    assert float(np.abs(out["dlogits"] - zt.grad.numpy()).max()) <= 1e-12
    assert abs(out["robust"] - float(loss.detach())) < 1e-12
    assert not out["dlogits"][groups < 0].any()
    # the weights moved towards the groups with the larger loss, by exp(eta L_g) before normalisation
    Lg = np.array([out["T"][g] / out["W_g"][g] if out["present"][g] else 0.0 for g in range(G)])
    want = q.astype(np.float64) * np.exp(float(np.float32(0.3)) * Lg)
    assert np.allclose(out["q"], want / want.sum(), rtol=0, atol=1e-7)


def test_restatement_boundary_cases():
    z, y, grp, q, w = _case(17, 3, 2, 5, True)
    dl = R.criterion_dlogits(z, y, w, 0.1)
    none = R.apply(z, y, np.full(17, -1, np.int32), q, 0.5, 2, w, 0.1, dlogits=dl, stats=np.ones(R.STATS))
    assert not none["wrote"] and np.array_equal(none["q"], q.astype(np.float64)) and np.array_equal(none["stats"], np.ones(R.STATS))
    one = R.apply(z, y, np.zeros(17, np.int32), [1.0], 0.5, 1, w, 0.1, dlogits=dl)
    assert np.array_equal(one["r"], np.ones(17)) and np.array_equal(one["dlogits"], dl) and one["q"][0] == 1.0
    upd = R.apply(z, y, grp, q, 0.5, 2, w, 0.1, dlogits=dl, stats=np.zeros(R.STATS))
    frz = R.apply(z, y, grp, upd["q"], 0.5, 2, w, 0.1, dlogits=dl, frozen=True, stats=np.zeros(R.STATS))
    assert np.array_equal(frz["dlogits"], upd["dlogits"]) and np.array_equal(frz["q"], upd["q"]) and not frz["stats"].any()
    st = upd["stats"]
    assert st[R.STATS - 1] == 1.0 and st[128:130].sum() == 17 and abs(st[64:66].sum() - upd["Wall"]) < 1e-12
    idx = np.random.RandomState(1).permutation(40)[:17]
    table = np.full(40, -1, np.int32)
    table[idx] = grp
    assert np.array_equal(R.apply(z, y, table, q, 0.5, 2, w, 0.1, dlogits=dl, idx=idx)["dlogits"], upd["dlogits"])
    zero_w = R.apply(z, y, grp, q, 0.5, 2, np.zeros(3, np.float32), 0.0, dlogits=dl)         # W_g = 0 everywhere: no group is present
    assert not zero_w["wrote"]


def _dataset(ordinals, labels, positions=None, store_rows=None):
    ds = types.SimpleNamespace(subject_ordinals=np.asarray(ordinals, np.int32), labels=np.asarray(labels, np.int64))
    if positions is not None:
        ds.index_host = np.asarray(positions, np.int64)
        ds.store = types.SimpleNamespace(x=np.zeros((store_rows, 1, 1)))
    return ds


def test_group_table_for_both_modes():
    ords, labels = [0, 0, 1, 1, 1, 2], [1, 0, 0, 2, 1, 2]
    own = _dataset(ords, labels)
    assert D.group_table(own, "subject", 3).tolist() == ords and D.group_table(own, "subject", 3).dtype == np.int32
    assert D.group_table(own, "subject-class", 3).tolist() == [1, 0, 3, 5, 4, 8]
    assert (D.group_count(own, "subject", 3), D.group_count(own, "subject-class", 3)) == (3, 9)
    view = _dataset(ords, labels, positions=[9, 2, 4, 5, 0, 7], store_rows=11)
    assert D.group_table(view, "subject", 3).tolist() == [1, -1, 0, -1, 1, 1, -1, 2, -1, 0, -1]
    assert D.group_table(view, "subject-class", 3).tolist() == [4, -1, 0, -1, 3, 5, -1, 8, -1, 1, -1]
    with pytest.raises(ValueError, match="1..64 groups"):
        D.group_table(_dataset(list(range(33)), [0] * 33), "subject-class", 2)
    with pytest.raises(ValueError, match="outside"):
        D.group_table(_dataset([0, 0], [0, 3]), "subject-class", 3)
    with pytest.raises(ValueError, match="one of"):
        D.group_table(own, "class", 3)


def test_settings_and_state():
    assert D.settings(None) is None
    assert D.settings(0.5) == dict(eta=0.5, groups="subject") and D.settings(dict(groups="subject-class")) == dict(eta=0.01, groups="subject-class")
    assert D.parse(None) == dict(eta=0.01, groups="subject") and D.parse(0, "subject-class") == dict(eta=0.0, groups="subject-class")
    for bad in (-1, float("nan"), float("inf"), "0.1", True, dict(eta=0.1, lam=1), dict(groups="class")):
        with pytest.raises(ValueError):
            D.settings(bad)
    with pytest.raises(ValueError, match="at most 2048"):
        D.check_batch_size(2049)
    D.check_batch_size(2048)
    d = D.GroupDro(0.1, "subject-class").set_groups([0, 1, 2, 5, -1], 6, 3)
    assert d.q.tolist() == [np.float32(1 / 6)] * 6 and d.q.dtype == torch.float32 and d.grp.dtype == torch.int32 and d.K == 3
    with pytest.raises(ValueError, match="names group"):
        D.GroupDro().set_groups([0, 4], 4)
    with pytest.raises(RuntimeError, match="not bound"):
        d.descriptor()
    stats = np.zeros(D.STATS)
    stats[:6], stats[64:70], stats[128:134] = [3, 1, 0, 8, 2, 0], [2, 1, 0, 2, 2, 0], [2, 1, 0, 2, 2, 0]
    stats[192], stats[193] = 5.0, 4.0
    s = d.epoch_summary(stats, [0.1, 0.1, 0.1, 0.5, 0.1, 0.1])
    assert s["dro_robust_loss"] == 1.25 and s["dro_worst_group_loss"] == 4.0 and (s["dro_worst_group"], s["dro_worst_subject"]) == (3, 1)
    assert s["dro_q_max"] == 0.5 and abs(s["dro_q_entropy"] + 5 * 0.1 * np.log(0.1) + 0.5 * np.log(0.5)) < 1e-12
    assert s["dro_subject_loss"] == [4.0 / 3.0, 2.5] and np.allclose(s["dro_subject_q"], [0.3, 0.7])
    assert D.worst_subject_accuracy([1, 1, 0, 0, 1], [1, 0, 0, 0, 0], [0, 0, 1, 1, 2]) == (2, 0.0)


def test_flag_parsing_and_the_two_refusals():
    from multimodalsignal_amd import main as M
    ap = M.build_parser()
    base = ["--synthetic", "x"]
    assert M.parse_args(ap, base).group_dro is None and "group_dro" not in M.build_cfg(M.parse_args(ap, base), ["cnn_gru_attention"])
    a = M.parse_args(ap, base + ["--group-dro"])
    assert a.group_dro == dict(eta=0.01, groups="subject")
    a = M.parse_args(ap, base + ["--group-dro", "0.5", "--dro-groups", "subject-class", "--batch-size", "2048"])
    cfg = M.build_cfg(a, ["cnn_gru_attention"])
    assert cfg["group_dro"] == dict(eta=0.5, groups="subject-class") and cfg["synthetic"] is True
    assert M.trainer_config(cfg, 0)["trainer"]["group_dro"] == cfg["group_dro"]
    assert "group_dro" not in M.trainer_config(M.default_cfg(), 0)["trainer"]
    for bad in (["--group-dro", "--mixup", "0.2"], ["--group-dro", "--batch-size", "2049"], ["--dro-groups", "subject"],
                ["--group-dro", "-0.1"], ["--group-dro", "nan"], ["--group-dro", "--dro-groups", "class"]):
        with pytest.raises(SystemExit):
            M.parse_args(ap, base + bad)
    # every option it composes with parses beside it
    M.parse_args(ap, base + ["--group-dro", "--subject-adversarial", "--label-smoothing", "0.1", "--max-grad-norm", "1", "--augment", "scale=0.1",
                             "--class-weights", "balanced", "--seeds", "2", "--distill"])
    M.parse_args(ap, base + ["--group-dro", "--sam", "0.05", "--weight-average", "ema"])
    M.parse_args(ap, base + ["--group-dro", "--hierarchical"])


def _info(subject, names, q, losses, acc):
    hist = [dict(epoch=1, train_loss=0.7, dro_q=[1 / len(q)] * len(q), dro_subject_loss=[0.7] * len(names), dro_robust_loss=0.7,
                 val_worst_subject="S9", val_worst_subject_acc=0.5),
            dict(epoch=2, train_loss=0.6, dro_q=q, dro_subject_loss=losses, dro_robust_loss=0.65, val_worst_subject="S8", val_worst_subject_acc=0.25)]
    return dict(subject=subject, accuracy=acc, history=hist,
                group_dro=dict(eta=0.1, groups="subject", G=len(q), K=len(q) // len(names), subjects=names, q=q))


def test_write_dro_on_hand_made_fold_records(tmp_path):
    assert D.fold_record(dict(subject="S2", history=[dict(epoch=1, train_loss=0.5)])) is None
    folds = [D.fold_record(_info("S2", ["S3", "S4", "S5"], [0.2, 0.5, 0.3], [0.5, 0.9, 0.6], 0.75)),
             D.fold_record(_info("S3", ["S2", "S4"], [0.1, 0.2, 0.3, 0.4], [0.4, None], None))]
    assert [s["subject"] for s in folds[0]["subjects"]] == ["S4", "S5", "S3"] and folds[0]["heaviest"] == "S4"
    assert folds[0]["subjects"][0] == dict(subject="S4", q=0.5, loss=0.9)
    assert (folds[0]["robust_loss"], folds[0]["mean_loss"], folds[0]["worst_val_subject"], folds[0]["worst_val_acc"]) == (0.65, 0.6, "S8", 0.25)
    assert [round(s["q"], 6) for s in folds[1]["subjects"]] == [0.7, 0.3] and folds[1]["heaviest"] == "S4"      # (subject, class) weights pooled
    path = D.write_dro(tmp_path, folds, dict(eta=0.1, groups="subject"), synthetic=True)
    doc = json.loads((tmp_path / "dro.json").read_text())
    assert doc["settings"] == dict(eta=0.1, groups="subject") and doc["probe"] is False and doc["synthetic"] is True
    assert doc["folds"] == json.loads(json.dumps(folds)) and doc["pooled"]["heaviest"] == [dict(subject="S4", folds=2)]
    txt = path.read_text(encoding="utf-8")
    assert path.name == "dro.txt" and txt.startswith("GROUP DRO: eta=0.1 groups=subject\n") and "say nothing about WESAD accuracy" in txt
    assert "fold S2: G=3" in txt and "heaviest subject over folds: S4=2" in txt and "n/a" in txt
    D.write_dro(tmp_path, folds[:1], 0.0, stem="dro_m1")
    assert json.loads((tmp_path / "dro_m1.json").read_text())["probe"] is True and "probe" in (tmp_path / "dro_m1.txt").read_text()
