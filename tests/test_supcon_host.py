"""The supervised contrastive term without a GPU: the restatement of tests/sc_reference.py against autograd of the loss written from
its definition, its boundary cases, the settings and flags, the two refusals and the report."""
import json

import numpy as np
import pytest
import torch

import sc_reference as R
from multimodalsignal_amd import supcon as SC

MODES = ("class", "cross-subject")


@pytest.mark.parametrize("tau", [0.1, 0.5])
@pytest.mark.parametrize("B", [2, 5, 33])
@pytest.mark.parametrize("positives", MODES)
def test_restatement_equals_autograd_of_the_definition(positives, B, tau):
    """fp64, with labels outside [0, K) and groups < 0 present: the closed-form gradient is autograd's to rounding."""
    K = 3
    for seed in range(4):
        f, y, table, idx = R.make_case(B, K, 100 * B + seed, invalid=0.2)
        g = table[idx]
        if B == 2 and seed == 0:                       # a pair that is an anchor pair in both modes
            y[:], g = 1, np.array([0, 1], dtype=np.int32)
        ft = torch.tensor(f, dtype=torch.float64, requires_grad=True)
        direct = R.loss_direct(ft, y, g, K, tau, positives)
        L, df, stats, na, _ = R.restatement(f, y, g, K, tau, positives)
        if direct is None:
            assert L is None and na == 0 and not df.any()
            continue
        direct.backward()
        assert abs(float(direct.detach()) - L) <= 1e-12 * max(1.0, abs(L))
        assert float((ft.grad - df).abs().max()) <= 1e-12 * float(df.abs().max())
        _, A, P = R.sets(y, g, K, positives)
        assert na == int(P.any(dim=1).sum()) and stats[1] == na and 0 <= stats[2] <= na
        assert not bool((P & ~A).any())                                                  # positives are a subset of A
        invalid = (y < 0) | (y >= K) | ((g < 0) if positives == "cross-subject" else False)
        assert not df[torch.as_tensor(invalid)].any()                                    # a row in no set gets no gradient


def test_cross_subject_mode_drops_same_subject_same_class_rows_from_both_sets():
    y, g = np.array([0, 0, 0, 1, 1]), np.array([0, 0, 1, 0, 1])
    _, A, P = R.sets(y, g, 2, "cross-subject")
    assert not A[0, 1] and not P[0, 1] and P[0, 2] and A[0, 3] and not P[0, 3]
    _, A, P = R.sets(y, g, 2, "class")
    assert A[0, 1] and P[0, 1]


def test_boundary_cases():
    rs = np.random.RandomState(0)
    f = rs.randn(6, 128).astype(np.float32)
    one = np.zeros(6, dtype=np.int64)
    # no anchor: every row a class of its own; no valid row; (cross-subject) one class and one subject
    for y, g, mode in ((np.arange(6), np.zeros(6), "class"), (np.full(6, -1), np.zeros(6), "class"), (one, np.zeros(6), "cross-subject"),
                       (one, np.full(6, -1), "cross-subject")):
        L, df, stats, na, _ = R.restatement(f, y, g, 8, 0.1, mode)
        assert L is None and na == 0 and stats == [0.0, 0, 0] and not df.any()
    # one class only (class mode): every row is an anchor, A(i) = P(i): the positives' mean log-probability, and top-1 everywhere
    L, df, stats, na, _ = R.restatement(f, one, np.zeros(6), 2, 0.1, "class")
    assert na == 6 and stats[2] == 6 and L > 0 and float(df.abs().max()) > 0
    # a zero-norm row: z = 0, finite everywhere (the clamp's gradient, scaled by 1 / 1e-12, is what autograd gives too)
    f0 = f.copy()
    f0[2] = 0.0
    ft = torch.tensor(f0, dtype=torch.float64, requires_grad=True)
    y = np.array([0, 1, 0, 1, 0, 1])
    R.loss_direct(ft, y, np.zeros(6), 2, 0.5, "class").backward()
    L, df, _, na, _ = R.restatement(f0, y, np.zeros(6), 2, 0.5, "class")
    assert na == 6 and np.isfinite(L) and bool(torch.isfinite(df).all())
    assert float((ft.grad - df).abs().max()) <= 1e-12 * float(df.abs().max())


def test_zero_padding_columns_change_nothing_and_get_no_gradient():
    """The embedded model's layout: 64 real columns at 0..31 and 64..95 of 128, exact zeros elsewhere."""
    f, y, table, idx = R.make_case(17, 2, 3)
    real = np.r_[0:32, 64:96]
    padded = np.zeros_like(f)
    padded[:, real] = f[:, real]
    La, dfa, sa, _, _ = R.restatement(padded, y, table[idx], 2, 0.1, "cross-subject")
    Lb, dfb, sb, _, _ = R.restatement(f[:, real], y, table[idx], 2, 0.1, "cross-subject")
    assert abs(La - Lb) < 1e-12 and sa[1:] == sb[1:] and float((dfa[:, real] - dfb).abs().max()) < 1e-12
    assert not dfa[:, np.r_[32:64, 96:128]].any()


def test_settings_and_flags():
    assert SC.settings(None) is None
    assert SC.settings(0.3) == dict(weight=0.3, tau=0.1, positives="class")
    assert SC.settings(dict(tau=0.5, positives="cross-subject")) == dict(weight=0.1, tau=0.5, positives="cross-subject")
    assert SC.parse(None) == SC.parse("") == dict(weight=0.1, tau=0.1, positives="class")
    assert SC.parse("0.2") == dict(weight=0.2, tau=0.1, positives="class")
    assert SC.parse("0:0.5", "cross-subject") == dict(weight=0.0, tau=0.5, positives="cross-subject")
    assert SC.settings_line(SC.parse("0.2:0.05")) == "SUPCON: weight=0.2 tau=0.05 positives=class"
    for bad in (dict(weight=-0.1), dict(weight=float("nan")), dict(weight="0.1"), dict(weight=True), dict(tau=0.0), dict(tau=1e-4), dict(tau=2e3),
                dict(tau=float("inf")), dict(positives="subject"), dict(temperature=0.1)):
        with pytest.raises(ValueError):
            SC.settings(bad)
    for bad in ("a", "0.1:b", "0.1:0.2:0.3", "-1", "0.1:0"):
        with pytest.raises(ValueError):
            SC.parse(bad)
    sc = SC.SupCon()
    assert (sc.weight, sc.tau, sc.positives, sc.cross_subject) == (0.1, 0.1, "class", False)
    with pytest.raises(RuntimeError):
        SC.SupCon(positives="cross-subject").bind("cpu")            # no subject table
    with pytest.raises(RuntimeError):
        sc.descriptor()                                             # not bound


def test_command_line_flags_and_the_two_refusals(tmp_path):
    from multimodalsignal_amd import main as M
    base = ["--synthetic", str(tmp_path / "w"), "--out", str(tmp_path / "o")]
    with pytest.raises(ValueError, match="mixup"):
        M.main(base + ["--supcon", "--mixup", "0.2"])
    with pytest.raises(ValueError, match="at most 2048"):
        M.main(base + ["--supcon", "0.1:0.2", "--batch-size", "2049"])
    for bad in (["--supcon", "x"], ["--supcon", "0.1:0"], ["--supcon-positives", "class"], ["--supcon", "--supcon-positives", "subject"]):
        with pytest.raises(SystemExit):
            M.main(base + bad)
    assert not (tmp_path / "o").exists() and not (tmp_path / "w").exists()      # refused before any data is made


def test_the_trainer_configuration_carries_the_setting_and_refuses_mixup_and_large_batches():
    from multimodalsignal_amd import main as M
    cfg = dict(epochs=1, lr=1e-3, patience=3, weight_decay=0.0, supcon=dict(weight=0.2, positives="cross-subject"))
    tc = M.trainer_config(cfg, 0)
    assert tc["trainer"]["supcon"] == dict(weight=0.2, tau=0.1, positives="cross-subject")
    assert "supcon" not in M.trainer_config(dict(cfg, supcon=None), 0)["trainer"]
    with pytest.raises(ValueError, match="at most 2048"):
        SC.check_batch_size(2049)
    SC.check_batch_size(2048)


def test_epoch_summary_and_the_report(tmp_path):
    s = SC.SupCon.epoch_summary([30.0, 12.0, 9.0, 4.0])
    assert s == dict(supcon_loss=2.5, supcon_top1=0.75, supcon_anchors=3.0)
    assert SC.SupCon.epoch_summary([0.0, 0.0, 0.0, 0.0]) == dict(supcon_loss=None, supcon_top1=None, supcon_anchors=None)
    hist = [dict(epoch=1, train_loss=0.7, supcon_loss=3.0, supcon_top1=0.5, supcon_anchors=14.0),
            dict(epoch=2, train_loss=0.6, supcon_loss=2.5, supcon_top1=0.75, supcon_anchors=15.0)]
    info = dict(subject="S2", history=hist, accuracy=0.8, supcon=dict(weight=0.1, tau=0.1, positives="class"))
    rec = SC.fold_record(info)
    assert rec == dict(subject="S2", weight=0.1, tau=0.1, positives="class", supcon_loss=2.5, supcon_top1=0.75, supcon_anchors=15.0,
                       train_loss=0.6, epochs=2, test_accuracy=0.8)
    assert SC.fold_record(dict(subject="S3", history=hist)) is None and SC.fold_record(dict(info, history=[])) is None
    rec2 = dict(rec, subject="S3", supcon_loss=3.5, supcon_top1=0.25, test_accuracy=None)
    path = SC.write_supcon(tmp_path, [rec, rec2], dict(weight=0.1), synthetic=True)
    txt = path.read_text(encoding="utf-8")
    assert path.name == "supcon.txt" and txt.startswith("SUPCON: weight=0.1 tau=0.1 positives=class\n")
    assert "say nothing about WESAD accuracy" in txt and "S2" in txt and "S3" in txt and "n/a" in txt
    doc = json.loads((tmp_path / "supcon.json").read_text())
    assert doc["folds"] == [rec, rec2] and doc["synthetic"] is True and doc["probe"] is False
    assert doc["pooled"] == dict(supcon_loss=3.0, supcon_top1=0.5, supcon_anchors=15.0, test_accuracy=0.8)
    path = SC.write_supcon(tmp_path, [rec], dict(weight=0.0, tau=0.5), stem="supcon_m1")
    assert path.name == "supcon_m1.txt" and "probe" in path.read_text(encoding="utf-8") and "WESAD" not in path.read_text(encoding="utf-8")
    assert json.loads((tmp_path / "supcon_m1.json").read_text())["probe"] is True
