"""Distillation, the host side checked without a GPU: the numpy restatement the GPU tests compare against (tests/kd_reference.py)
agrees with torch's kl_div / cross_entropy autograd in fp64, a teacher row with an exact zero included; at T = 1 the restated
teacher is en_reference's mean; Distillation.parse, the student's name, and the report on hand-made rows."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import en_reference as E
import kd_reference as R
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd import distill as D
from multimodalsignal_amd import ensemble as ensemble_mod


def _soft_loss(z, y, w, eps, lam):
    return lam * F.cross_entropy(z, y, weight=w, label_smoothing=eps) + (1.0 - lam) * F.cross_entropy(z, y.flip(0), weight=w, label_smoothing=eps)


@pytest.mark.parametrize("lam", [1.0, 0.3])
@pytest.mark.parametrize("alpha,T", [(0.5, 2.0), (1.0, 0.5), (0.25, 4.0)])
def test_reference_gradient_and_loss_agree_with_autograd(alpha, T, lam):
    """B = 7 (a self-paired middle row), K = 3, class weights, eps = 0.1, one saturated teacher row (1, 0, 0).  dL/dz as the header
    states it, alpha (T / B) (s - qm), is the gradient of the KL term exactly when qm sums to 1; the fp32 rows sum to 1 within an
    ulp or two, so the restatement may differ from autograd by kappa * |sum qm - 1| per entry and no more.  With dyadic teacher
    rows and lam = 1 the sums are exact and so is the agreement."""
    B, K = 7, 3
    rs = np.random.RandomState(3)
    z = (2.0 * rs.randn(B, K)).astype(np.float32)
    y = torch.as_tensor(rs.randint(0, K, size=B).astype(np.int64))
    w = torch.tensor([0.3, 2.5, 1.0], dtype=torch.float64)
    e = np.exp(rs.randn(B, K))
    for rows in ((e / e.sum(axis=1, keepdims=True)).astype(np.float32),
                 np.array([[0.5, 0.25, 0.25], [0.125, 0.75, 0.125], [0.0, 1.0, 0.0]] * 3, dtype=np.float32)[:B]):
        rows = rows.copy()
        rows[2] = (1.0, 0.0, 0.0)
        qm = R.blend(rows, lam)
        zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
        hard = _soft_loss(zt, y, w, 0.1, lam)
        dl_hard = torch.autograd.grad(hard, zt)[0].numpy()
        zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
        kd = T * T * F.kl_div(F.log_softmax(zt / T, dim=1), torch.tensor(qm, dtype=torch.float64), reduction="batchmean")
        total = (1.0 - alpha) * _soft_loss(zt, y, w, 0.1, lam) + alpha * kd
        total.backward()
        r = R.apply(z, dl_hard.astype(np.float32), qm, alpha, T)
        # the restatement takes dlogits as the fp32 values the launch finds; feed it the fp64 hard gradient's own rounding error too
        want = zt.grad.numpy() - (1.0 - alpha) * (dl_hard - dl_hard.astype(np.float32).astype(np.float64))
        slack = alpha * T / B * float(np.abs(qm.astype(np.float64).sum(axis=1) - 1.0).max())
        assert np.abs(r["dlogits"] - want).max() <= slack + 1e-15
        assert abs(r["L_kd"] - float(kd.detach())) <= 1e-14 * max(1.0, float(kd.detach()))
        assert r["stats"][2] == B and r["stats"][0] == B * r["L_kd"]
        if lam == 1.0 and rows[0, 0] == 0.5:
            assert slack == 0.0
    assert (qm == 0).any() or lam != 1.0


def test_fp32_restatement_is_close_to_the_fp64_one_and_counts_first_argmax():
    rs = np.random.RandomState(1)
    z = (2.0 * rs.randn(17, 4)).astype(np.float32)
    e = np.exp(rs.randn(17, 4))
    qm = R.blend((e / e.sum(axis=1, keepdims=True)).astype(np.float32), 0.3)
    dl = (rs.randn(17, 4) / 17).astype(np.float32)
    a, b = R.apply(z, dl, qm, 0.3, 2.0), R.apply(z, dl, qm, 0.3, 2.0, dtype=np.float32)
    assert b["dlogits"].dtype == np.float32 and 0 < np.abs(b["dlogits"] - a["dlogits"]).max() < 1e-7
    assert a["stats"][1] == b["stats"][1] == float((z.argmax(axis=1) == qm.argmax(axis=1)).sum())
    tie_z, tie_q = np.array([[1.0, 1.0, 0.0]], dtype=np.float32), np.array([[0.4, 0.4, 0.2]], dtype=np.float32)
    assert R.apply(tie_z, np.zeros((1, 3), np.float32), tie_q, 1.0, 1.0)["stats"][1] == 1.0          # both first argmax = 0


@pytest.mark.parametrize("M,K", [(1, 2), (3, 3), (7, 16)])
def test_restated_teacher_is_the_ensemble_mean_at_T_1(M, K):
    lg = R.crafted_logits(M, 5, K, seed=M + K)
    assert np.array_equal(R.teacher(lg, 1.0), E.reduce(lg)["mean_p"])
    t = R.teacher(lg, 4.0)
    assert np.allclose(t.sum(axis=1), 1.0, atol=1e-14) and not np.array_equal(t, R.teacher(lg, 1.0))
    want = torch.softmax(torch.as_tensor(lg, dtype=torch.float64) / 4.0, dim=2).mean(dim=0).numpy()
    assert np.abs(t - want).max() < 1e-15


# ---- the setting ----------------------------------------------------------------------------------------------------------------
def test_parse():
    d = D.Distillation.parse("0.25:4")
    assert (d.alpha, d.temperature) == (0.25, 4.0) and d.spec() == "0.25:4"
    assert (D.Distillation.parse("0.7").alpha, D.Distillation.parse("0.7").temperature) == (float(np.float32(0.7)), 2.0)
    for empty in (None, "", True):
        d = D.Distillation.parse(empty)
        assert (d.alpha, d.temperature) == (0.5, 2.0)
    assert D.Distillation.parse("0").alpha == 0.0 and D.Distillation.parse("1:0.015625").temperature == 1.0 / 64.0
    for bad in ("x", "0.5:", "0.5:2:3", "1.5", "-0.1", "0.5:0", "0.5:65", "nan", "0.5:nan"):
        with pytest.raises(ValueError):
            D.Distillation.parse(bad)


def test_check_distill_returns_the_fp32_values_and_refuses_what_the_library_refuses():
    assert L.check_distill(0.3, 2) == (float(np.float32(0.3)), 2.0)
    for a, t in ((True, 2.0), ("0.5", 2.0), (0.5, None), (float("nan"), 2.0), (0.5, float("inf")), (0.5, 1.0 / 128.0), (-1e-9, 2.0)):
        with pytest.raises(ValueError):
            L.check_distill(a, t)


def test_student_name_and_teacher_table_checks():
    assert D.student_name(ensemble_mod.replica_name("", 0)) == ensemble_mod.replica_name("", 0) + "/distilled"
    assert D.student_name(ensemble_mod.replica_name("cnn_gru", 0)).endswith("/distilled")
    d = D.Distillation(0.5, 2.0)
    with pytest.raises(RuntimeError):
        d.descriptor()
    for bad in (np.zeros((4, 3)), np.zeros((4,), np.float32), np.zeros((4, 1), np.float32), np.zeros((4, L.MAX_K + 1), np.float32)):
        with pytest.raises(ValueError):
            d.set_teacher(bad)
    d.set_teacher(np.full((4, 3), 1.0 / 3.0, dtype=np.float32))
    k = d.descriptor(idx=None)
    assert (k.alpha, k.temperature, k.idx, k.stride_bytes) == (0.5, 2.0, None, 0) and k.q == d.q.data_ptr() and k.stats == d.stats.data_ptr()
    assert D.Distillation.epoch_summary([6.0, 3.0, 12.0]) == dict(kd_loss=0.5, kd_agreement=0.25)
    assert D.Distillation.epoch_summary([0.0, 0.0, 0.0]) == dict(kd_loss=None, kd_agreement=None)


# ---- the report -----------------------------------------------------------------------------------------------------------------
def _row(acc, f1, nll, brier, ece, fid):
    return dict(accuracy=acc, f1=f1, nll=nll, brier=brier, ece=ece, fidelity=fid)


def test_fidelity_and_paired():
    assert D.fidelity([0, 1, 1, 0], [0, 1, 0, 0]) == 0.75 and D.fidelity([1], [1]) == 1.0
    with pytest.raises(ValueError):
        D.fidelity([0, 1], [0])
    p = D.paired([0.9, 0.5, 0.7], [0.8, 0.5, 0.75])
    assert (p["wins"], p["ties"], p["losses"]) == (1, 1, 1) and abs(p["mean_difference"] - (0.1 + 0.0 - 0.05) / 3) < 1e-15


def test_table_on_hand_made_rows(tmp_path):
    folds = [dict(subject="S2", ensemble=_row(0.9, 0.9, 0.3, 0.1, 0.05, 1.0), mean_member=_row(0.85, 0.84, 0.4, 0.15, 0.07, None),
                  replica0=_row(0.8, 0.8, 0.5, 0.2, 0.1, 0.9), student=_row(0.9, 0.88, 0.35, 0.12, 0.06, 0.95), kd_loss=0.02, kd_agreement=0.97),
             dict(subject="S3", ensemble=_row(0.7, 0.7, 0.6, 0.3, 0.1, 1.0), mean_member=_row(0.65, 0.6, 0.7, 0.35, 0.12, None),
                  replica0=_row(0.7, 0.7, 0.6, 0.3, 0.1, 0.8), student=_row(0.6, 0.7, 0.7, 0.3, 0.2, 0.85), kd_loss=0.04, kd_agreement=0.9)]
    pooled = dict(ensemble=_row(0.8, 0.8, 0.45, 0.2, 0.07, 1.0), student=_row(0.75, 0.79, 0.5, 0.21, 0.1, 0.9))
    path = D.write_distillation(tmp_path, folds, D.Distillation(0.5, 2.0), members=3, pooled=pooled, synthetic=True)
    doc = json.loads((tmp_path / "distillation.json").read_text())
    assert (doc["alpha"], doc["temperature"], doc["members"], doc["synthetic"]) == (0.5, 2.0, 3, True)
    assert [f["subject"] for f in doc["folds"]] == ["S2", "S3"] and doc["pooled"]["student"]["fidelity"] == 0.9
    pa = doc["paired"]
    assert (pa["accuracy"]["wins"], pa["accuracy"]["ties"], pa["accuracy"]["losses"]) == (1, 0, 1) and abs(pa["accuracy"]["mean_difference"]) < 1e-15
    assert (pa["f1"]["wins"], pa["f1"]["ties"], pa["f1"]["losses"]) == (1, 1, 0)
    assert (pa["nll"]["wins"], pa["nll"]["losses"]) == (1, 1) and abs(pa["nll"]["mean_difference"] - (-0.15 + 0.1) / 2) < 1e-12      # lower wins
    assert (pa["ece"]["wins"], pa["ece"]["losses"]) == (1, 1) and pa["brier"]["ties"] == 1
    txt = path.read_text(encoding="utf-8")
    assert txt.startswith("DISTILLATION: alpha=0.5 T=2 members=3") and "shows the machinery, not what WESAD would give" in txt
    for needle in ("S2       student", "S3       replica0", "pooled   ensemble", "kd_loss=0.0200 kd_agreement=0.9700", "wins/ties/losses 1/0/1"):
        assert needle in txt, needle
    assert "n/a" in txt                                            # the mean member has no fidelity
    assert "NOTE" not in D.format_table(dict(doc, synthetic=False))


# ---- the driver's arguments and dealing -----------------------------------------------------------------------------------------
def _args(*extra):
    from multimodalsignal_amd import main as M
    return M.parse_args(M.build_parser(), ["--synthetic", "/nonexistent", *extra])


def test_the_flag():
    assert _args().distill is None
    assert _args("--distill").distill == "0.5:2" and _args("--seeds", "3", "--distill", "0.25:4").distill == "0.25:4"
    assert _args("--distill", "0").distill == "0:2"
    for bad in (["--distill", "1.5"], ["--distill", "0.5:100"], ["--distill", "x"], ["--hierarchical", "--distill"],
                ["--hierarchical", "--seeds", "2", "--distill", "0.3"]):
        with pytest.raises(SystemExit):
            _args(*bad)


@pytest.mark.parametrize("world", [1, 2])
def test_every_student_is_on_the_rank_of_its_folds_replicas_and_every_unit_is_dealt_once(world):
    """The students of a rank are the base units it holds (main.distill_units takes them from the replicas the rank trained): over
    one and two ranks every (configuration, fold) has exactly one student, on the rank of all its replicas, and waves.deal puts each
    student into exactly one fold batch, one batch group per configuration."""
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd import waves
    S = 3
    subjects = [f"S{i}" for i in range(2, 9)]
    base = {"": dict(subjects=subjects), "cnn_gru": dict(subjects=subjects)}
    seen = {}
    for rank in range(world):
        units, mine, _ = M.rank_units(base, world, rank)
        xunits, xmine, _ = ensemble_mod.deal_replicas(units, mine, S)
        students = sorted(u for u in xmine if u % S == 0)
        groups = {}
        for u0 in students:
            n, k = xunits[u0]
            assert all(u0 + r in xmine and xunits[u0 + r] == (ensemble_mod.replica_name(n, r), k) for r in range(S))
            assert (D.student_name(n), k) not in seen
            seen[D.student_name(n), k] = rank
            groups.setdefault(D.student_name(n), []).append(u0)
        dealt = [u for wave in waves.deal(list(groups.values()), students, 15, 4, sweep=len(groups) > 1) for batch in wave for u in batch]
        assert sorted(dealt) == students
    assert sorted(seen) == sorted((D.student_name(n), k) for n in base for k in range(len(subjects)))
    assert ensemble_mod.replica_seed(42, 3, 0) == 45                       # the student's unit seed: replica 0's, the plain fold's
