"""Label-free BatchNorm adaptation, the parts that need no GPU: the float64 restatement (tests/ab_reference.py) pinned to torch's
BatchNorm1d, its independence of the batching, the order of the stages, the batch-grouping plan of adapt.BnAdapter, the driver's
--adapt-bn handling and the adaptation table."""
import json

import numpy as np
import pytest
import torch

import ab_reference as R
from oracle import cnn_gru_oracle as O
from multimodalsignal_amd import adapt as A

C_, K, T, N = 6, 2, 256, 37


def _x(n=N, c=C_, t=T, seed=3):
    rs = np.random.RandomState(seed)
    return torch.as_tensor(rs.randn(n, c, t) * (1.5 + 1.5 * rs.rand(1, c, 1)) + 2.0 * rs.rand(1, c, 1) - 1.0, dtype=torch.float64)


def _case(seed=11):
    return O.init_params(C_, K, seed=seed), O.init_buffers(), _x()


def test_stage_one_is_what_torch_batchnorm_leaves_as_running_statistics():
    """One batch, alpha = 1: BatchNorm1d(momentum = 1.0) after ONE training forward on y1 holds the batch mean and the UNBIASED
    batch variance in its running statistics — the definition the adaptation uses."""
    params, buffers, x = _case()
    got = R.adapt(params, buffers, x, alpha=1.0)
    y1 = R.conv1_out(R._cast(params, torch.float64), x)
    bn = torch.nn.BatchNorm1d(16, momentum=1.0).double().train()
    bn(y1)
    assert float((got[R.KEYS[0]] - bn.running_mean).abs().max()) < 1e-12
    assert float((got[R.KEYS[1]] - bn.running_var).abs().max() / bn.running_var.abs().max()) < 1e-12
    biased = R.adapt(params, buffers, x, alpha=1.0, wrong="biased")
    n1 = N * y1.shape[2]
    assert float((biased[R.KEYS[1]] * n1 / (n1 - 1) - bn.running_var).abs().max() / bn.running_var.abs().max()) < 1e-12
    assert float((biased[R.KEYS[1]] - bn.running_var).abs().max() / bn.running_var.abs().max()) > 0.5 / n1
    # and a blend is the momentum update from the source state
    half = R.adapt(params, buffers, x, alpha=0.25)
    bn = torch.nn.BatchNorm1d(16, momentum=0.25).double().train()
    bn(y1)
    assert float((half[R.KEYS[0]] - bn.running_mean).abs().max()) < 1e-12 and float((half[R.KEYS[1]] - bn.running_var).abs().max()) < 1e-11


@pytest.mark.parametrize("kind", ["cnn_gru_attention", "cnn_gru"])
def test_reference_does_not_depend_on_the_batching(kind):
    params, buffers, x = _case()
    whole = R.adapt(params, buffers, x, kind=kind)
    for batch in (16, 32, 5, 1):
        cut = R.adapt(params, buffers, x, batch=batch, kind=kind)
        for k in R.KEYS:
            assert float((cut[k] - whole[k]).abs().max() / whole[k].abs().max()) < 1e-12, (batch, k)
    # the whole-set statistic is NOT the moving average over batches
    p = R._cast(params, torch.float64)
    bn = torch.nn.BatchNorm1d(16, momentum=1.0).double().train()
    for i in range(0, N, 16):
        bn(R.conv1_out(p, x[i:i + 16], kind))
    assert float((bn.running_var - whole[R.KEYS[1]]).abs().max() / whole[R.KEYS[1]].abs().max()) > 1e-3
    # alpha = 0 is the source, the float32 mode is close to the float64 one
    same = R.adapt(params, buffers, x, alpha=0.0, batch=16, kind=kind)
    own = R.adapt(params, buffers, x, batch=16, kind=kind, dtype=torch.float32)
    for k in R.KEYS:
        assert torch.equal(same[k], buffers[k].double())
        assert own[k].dtype == torch.float32 and float((own[k].double() - whole[k]).abs().max() / whole[k].abs().max()) < 1e-5


def test_the_order_of_the_stages_matters():
    """Stage 2 under the SOURCE BatchNorm-1 statistics is a different quantity: stage 1 agrees, stage 2 does not."""
    params, buffers, x = _case()
    good, bad = R.adapt(params, buffers, x), R.adapt(params, buffers, x, wrong="source_bn1")
    for k in R.KEYS[:2]:
        assert torch.equal(good[k], bad[k])
    for k in R.KEYS[2:]:
        assert float((good[k] - bad[k]).abs().max() / good[k].abs().max()) > 1e-2, k


def test_batch_plan_groups_folds_of_equal_batch_size():
    assert A.batch_plan([37], 16) == [(0, 16, [0]), (16, 16, [0]), (32, 5, [0])]
    assert A.batch_plan([37, 37, 37], 16) == [(0, 16, [0, 1, 2]), (16, 16, [0, 1, 2]), (32, 5, [0, 1, 2])]
    # unequal N, any order: full batches together, ragged last batches by size, shorter sets leave
    plan = A.batch_plan([20, 37, 36, 37, 16], 16)
    assert plan == [(0, 16, [1, 3, 2, 0, 4]), (16, 16, [1, 3, 2]), (16, 4, [0]), (32, 5, [1, 3]), (32, 4, [2])]
    for sizes, bs in (([20, 37, 36, 37, 16], 16), ([5, 1, 9], 4), ([3, 3], 8), ([1024, 1000, 7], 256)):
        seen = {j: [] for j in range(len(sizes))}
        for i, b, jobs in A.batch_plan(sizes, bs):
            assert 1 <= b <= bs and len(set(jobs)) == len(jobs)
            for j in jobs:
                assert b == min(bs, sizes[j] - i)
                seen[j].append((i, b))
        for j, n in enumerate(sizes):            # every window exactly once, in order
            assert [i for i, _ in seen[j]] == list(range(0, n, bs)) and sum(b for _, b in seen[j]) == n
    with pytest.raises(ValueError):
        A.batch_plan([4, 0], 2)
    with pytest.raises(ValueError):
        A.batch_plan([4], 0)


def test_alpha_check():
    assert A.check_alpha(0) == 0.0 and A.check_alpha(1) == 1.0 and A.check_alpha("0.25") == 0.25
    for bad in (-0.1, 1.0001, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError):
            A.check_alpha(bad)


def test_cli_flag():
    from multimodalsignal_amd import main as M
    ap = M.build_parser()
    base = ["--synthetic", "/tmp/x"]
    a = M.parse_args(ap, base)
    assert a.adapt_bn is None and "adapt_bn" not in M.build_cfg(a, ["cnn_gru_attention"])       # without the flag: no such key
    a = M.parse_args(ap, base + ["--adapt-bn"])
    cfg = M.build_cfg(a, ["cnn_gru_attention"])
    assert a.adapt_bn == 1.0 and cfg["adapt_bn"] == 1.0 and cfg["adapt_bn_batched"] is True and cfg["synthetic"] is True
    a = M.parse_args(ap, base + ["--adapt-bn", "0.3", "--adapt-bn-sequential", "--model", "cnn_gru", "cnn_gru_attention"])
    cfg = M.build_cfg(a, ["cnn_gru_attention", "cnn_gru"])
    assert cfg["adapt_bn"] == 0.3 and cfg["adapt_bn_batched"] is False and "calibrate" not in cfg
    assert M.adaptation_settings(cfg) == {"alpha": 0.3}
    a = M.parse_args(ap, base + ["--adapt-bn", "--calibrate", "8"])                               # the two may be combined
    cfg = M.build_cfg(a, ["cnn_gru_attention"])
    assert cfg["adapt_bn"] == 1.0 and cfg["calibrate"] == 8
    for bad in (["--adapt-bn", "1.5"], ["--adapt-bn", "-0.1"], ["--adapt-bn", "nan"], ["--adapt-bn-sequential"],
                ["--adapt-bn", "--hierarchical"], ["--adapt-bn", "--ablation"], ["--adapt-bn", "0.5", "--sweep", "a=chest_ECG"]):
        with pytest.raises(SystemExit):
            M.parse_args(ap, base + bad)


def test_rejection_wording_is_the_calibrations(capsys):
    from multimodalsignal_amd import main as M
    ap = M.build_parser()
    msgs = []
    for flag in (["--adapt-bn"], ["--calibrate", "8"]):
        with pytest.raises(SystemExit):
            M.parse_args(ap, ["--synthetic", "/tmp/x", "--hierarchical"] + flag)
        msgs.append(capsys.readouterr().err.strip().splitlines()[-1].split("error: ")[1])
    assert msgs[0] == msgs[1].replace("--calibrate", "--adapt-bn")


def test_adaptation_table_from_canned_numbers(tmp_path):
    folds = [{"subject": "S2", "n": 270, "before": {"accuracy": 0.80, "f1_score": 0.75}, "after": {"accuracy": 0.90, "f1_score": 0.85}},
             {"subject": "S3", "n": 260, "before": {"accuracy": 0.70, "f1_score": 0.65}, "after": {"accuracy": 0.70, "f1_score": 0.60}},
             {"subject": "S4", "n": 275, "before": {"accuracy": 0.60, "f1_score": 0.55}, "after": {"accuracy": 0.50, "f1_score": 0.55}}]
    path = A.write_adaptation(tmp_path, folds, {"alpha": 1.0}, synthetic=True)
    doc = json.loads((tmp_path / "adaptation.json").read_text())
    assert doc["n_folds"] == 3 and [f["subject"] for f in doc["folds"]] == ["S2", "S3", "S4"] and doc["settings"] == {"alpha": 1.0}
    assert doc["note"] == A.SYNTHETIC_NOTE and "synthetic" in doc["note"]
    sm = doc["summary"]["accuracy"]
    assert sm["before"]["mean"] == pytest.approx(0.7) and sm["after"]["mean"] == pytest.approx(0.7)
    assert sm["before"]["std"] == pytest.approx(np.std([0.8, 0.7, 0.6])) and sm["after"]["std"] == pytest.approx(np.std([0.9, 0.7, 0.5]))
    assert sm["difference"]["mean"] == pytest.approx(0.0) and sm["difference"]["std"] == pytest.approx(np.std([0.1, 0.0, -0.1]))
    assert (doc["wins"]["accuracy"], doc["ties"]["accuracy"], doc["losses"]["accuracy"]) == (1, 1, 1)
    assert (doc["wins"]["f1_score"], doc["ties"]["f1_score"], doc["losses"]["f1_score"]) == (1, 1, 1)
    txt = path.read_text(encoding="utf-8")
    assert path.name == "adaptation.txt" and A.SYNTHETIC_NOTE in txt and "alpha = 1.0" in txt
    assert all(s in txt for s in ("S2", "S3", "S4", "270", "mean paired difference", "adapted wins 1 of 3 folds, ties 1, losses 1"))
    assert "+0.1000" in txt and "-0.1000" in txt and "0.7000 ± " in txt
    A.write_adaptation(tmp_path, folds, {"alpha": 0.5})                    # a real data set: no note
    assert "note" not in json.loads((tmp_path / "adaptation.json").read_text()) and "NOTE" not in (tmp_path / "adaptation.txt").read_text(encoding="utf-8")
