"""Integrated-gradients attribution, the parts that need no GPU: the midpoint table, the target vectors, the path-batch plan, the
argument errors (raised before anything is launched), the restatement tests/at_reference.py against the module's tables, the
driver's --attribute handling and the attribution tables."""
import json

import numpy as np
import pytest
import torch

import at_reference as R
from multimodalsignal_amd import attribute as AT


def test_midpoint_table():
    for P in (1, 2, 5, 32, 256):
        alpha, w = AT.midpoint_table(P)
        assert alpha.dtype == w.dtype == np.float64 and alpha.shape == w.shape == (P,)
        assert abs(w.sum() - 1.0) < 1e-14 and np.all(w == 1.0 / P)
        assert np.allclose(alpha + alpha[::-1], 1.0, rtol=0, atol=1e-15)          # symmetric about 1/2
        assert alpha[0] == 0.5 / P and 0.0 < alpha.min() and alpha.max() < 1.0        # never the baseline, never the window
        ra, rw = R.midpoint(P)
        assert np.array_equal(alpha, ra) and np.array_equal(w, rw)
    # the midpoint rule is exact for a quadratic f along the path: IG total = f(x) - f(x0) with one point
    x, b = np.array([[1.0, -2.0, 0.5]]), np.array([[0.25, 0.5, -1.0]])
    m, _ = R.integrated_gradients(lambda z: 2.0 * z, x, b, 1)
    assert abs(m.sum() - ((x ** 2).sum() - (b ** 2).sum())) < 1e-12
    for bad in (0, 257, -1, 2.5, "8", None, True):
        with pytest.raises(ValueError):
            AT.midpoint_table(bad)


def test_occlusion_table():
    t = AT.occlusion_table(4)
    assert t.shape == (5, 4) and np.array_equal(t, R.occlusion_coef(4))
    assert np.array_equal(t[4], np.ones(4)) and np.array_equal(t[:4], 1.0 - np.eye(4))


def test_target_vectors():
    assert AT.class_target(1, 2).tolist() == [-1.0, 1.0] and AT.class_target(0, 2).tolist() == [1.0, -1.0]        # the log-odds
    for K in (2, 3, 16):
        for k in range(K):
            v = AT.class_target(k, K)
            assert v.dtype == torch.float32 and v[k] == 1.0 and abs(float(v.double().sum())) < 1e-6
            assert np.allclose(v.numpy(), R.class_target(k, K))
    v = AT.target_vectors(2, 3, 4)
    assert v.shape == (4, 3) and v.is_contiguous() and torch.equal(v, AT.class_target(2, 3).expand(4, 3))
    logits = torch.tensor([[0.1, 0.9, 0.0], [2.0, -1.0, 2.0], [-3.0, -2.0, -1.0]])
    v = AT.target_vectors("predicted", 3, 3, logits)
    assert torch.equal(v, torch.stack([AT.class_target(k, 3) for k in (1, 0, 2)]))            # a tie: the first maximum
    one, per = torch.tensor([0.5, -1.5, 1.0], dtype=torch.float64), torch.arange(12, dtype=torch.float32).view(4, 3)
    assert torch.equal(AT.target_vectors(one, 3, 4), one.float().expand(4, 3)) and AT.target_vectors(one, 3, 4).dtype == torch.float32
    assert torch.equal(AT.target_vectors(per, 3, 4), per)                                       # an explicit tensor passes through
    for bad in (3, -1, 1.0, True, None, "top", torch.zeros(4), torch.zeros(3, 3), torch.zeros(3, dtype=torch.int64)):
        with pytest.raises(ValueError):
            AT.target_vectors(bad, 3, 4, torch.zeros(4, 3))
    with pytest.raises(ValueError):
        AT.target_vectors("predicted", 3, 4)                                                    # needs the logits
    # target_dot adds in class order
    lg, vv = torch.tensor([[1e8, 1.0, -1e8]]), torch.ones(1, 3)
    assert float(AT.target_dot(lg, vv)) == float((torch.tensor(1e8) + torch.tensor(1.0)) - torch.tensor(1e8))


def test_path_plan():
    assert AT.path_plan(9, 8, 16) == [(0, 2), (2, 2), (4, 2), (6, 2), (8, 1)]
    assert AT.path_plan(9, 8, 72) == [(0, 9)] and AT.path_plan(9, 8, 2048) == [(0, 9)]
    assert AT.path_plan(5, 32, 63) == [(i, 1) for i in range(5)]
    for N, P, pb in ((270, 32, 2048), (7, 3, 10), (1, 256, 256), (100, 1, 7), (9, 8, 23)):
        plan = AT.path_plan(N, P, pb)
        assert plan == R.path_plan(N, P, pb)
        assert all(1 <= n and n * P <= pb for _, n in plan)                        # whole windows only
        assert [i for i, _ in plan] == list(np.cumsum([0] + [n for _, n in plan])[:-1]) and sum(n for _, n in plan) == N
        assert all(n == pb // P for _, n in plan[:-1])                             # only the last one is ragged
    for bad in ((0, 4, 8), (3, 8, 7), (3, 0, 8)):
        with pytest.raises(ValueError):
            AT.path_plan(*bad)


def test_restatement_of_the_kernels():
    rs = np.random.RandomState(0)
    N, P, C, T = 2, 3, 4, 21
    x, b = rs.randn(N, C, T).astype(np.float32), rs.randn(N, C, T).astype(np.float32)
    coef = rs.rand(P, C)
    xp = R.path(x, b, R.BASE_OWN, coef)
    assert xp.dtype == np.float32 and xp.shape == (N * P, C, T)
    want = b[:, None] + coef.astype(np.float32)[None, :, :, None].astype(np.float64) * (x.astype(np.float64) - b)[:, None]
    assert np.abs(xp.reshape(N, P, C, T) - want).max() < 1e-6
    assert np.array_equal(R.path(x, None, R.BASE_ZERO, np.ones((1, C))), x)                     # coef 1 from zero: the window itself
    assert np.array_equal(R.path(x, b[0, :, 0], R.BASE_CHANNEL, np.zeros((1, C))), R.broadcast_base(b[0, :, 0], R.BASE_CHANNEL, N, C, T, np.float32))
    occ = R.path(x, b[0], R.BASE_SHARED, R.occlusion_coef(C)).reshape(N, C + 1, C, T)
    assert np.array_equal(occ[:, C], x) and np.array_equal(occ[1, 2, 2], b[0, 2]) and np.array_equal(occ[1, 2, 3], x[1, 3])
    v = rs.randn(N, 3).astype(np.float32)
    assert np.array_equal(R.path_dlogits(v, P)[P:2 * P], np.repeat(v[1:2], P, axis=0))
    dx, w = rs.randn(N * P, C, T).astype(np.float32), rs.rand(P).astype(np.float32)
    m, bound = R.reduce_map(dx, x, b, R.BASE_OWN, w)
    direct = (x.astype(np.float64) - b) * sum(float(w[p]) * dx.reshape(N, P, C, T)[:, p].astype(np.float64) for p in range(P))
    assert np.allclose(m, direct, rtol=1e-13, atol=0) and np.all(bound >= 0) and bound.max() < 1e-5
    for bin_, nb in ((8, 3), (21, 1), (1, 21), (64, 1)):
        bins, chan, total = R.sums_of_map(m.astype(np.float32), bin_)
        assert bins.shape == (N, C, nb) and chan.shape == (N, C) and total.shape == (N,)
        assert np.allclose(bins.sum(axis=2), chan, rtol=1e-5, atol=1e-6) and np.allclose(chan.sum(axis=1), total, rtol=1e-5, atol=1e-6)
    assert R.within_ulps(np.float32(1.0) + np.spacing(np.float32(1.0)), np.float32(1.0)) and not R.within_ulps(np.float32(1.0) + 3 * np.spacing(np.float32(1.0)), np.float32(1.0))


def _cpu_model(C=6, K=3):
    from multimodalsignal_amd.models import CnnGruAttentionModel
    return CnnGruAttentionModel(C, K)


def test_argument_errors_are_raised_before_anything_is_launched():
    m = _cpu_model()                     # on the CPU: anything that reached the engine would raise RuntimeError, not ValueError
    for kw in (dict(steps=0), dict(steps=257), dict(steps=2.0), dict(bin=0), dict(bin=-3), dict(bin=1.5), dict(steps=32, path_batch=31),
               dict(path_batch=0), dict(baseline=torch.zeros(5)), dict(baseline=torch.zeros(7, 256)), dict(baseline=torch.zeros(2, 5, 256)),
               dict(baseline=torch.zeros(1, 2, 6, 256)), dict(baseline=torch.zeros(6, dtype=torch.int64)), dict(baseline=[0.0] * 6)):
        with pytest.raises(ValueError):
            AT.Attributor(m, **kw)
    at = AT.Attributor(m, steps=8, path_batch=8, bin=4, baseline=torch.zeros(6))
    assert (at.P, at.bin, at.path_batch) == (8, 4, 8)
    for call in (at.attribute, at.channel_occlusion, at.gate):
        for bad in (torch.zeros(2, 6, 256), np.zeros((2, 6, 256), dtype=np.float32)):          # a CPU tensor, not a tensor
            with pytest.raises(ValueError):
                call(bad)
    with pytest.raises(ValueError):
        m.attribute(torch.zeros(2, 6, 256))
    with pytest.raises(ValueError):
        m.attribute(torch.zeros(2, 6, 256), steps=300)
    with pytest.raises(ValueError):
        m.channel_occlusion(torch.zeros(2, 6, 256))
    # shapes of a baseline against the input, the four kinds
    assert AT.baseline_kind(None, 6) == 0 and AT.baseline_kind(torch.zeros(6), 6, 4, 256) == 1
    assert AT.baseline_kind(torch.zeros(6, 256), 6, 4, 256) == 2 and AT.baseline_kind(torch.zeros(4, 6, 256), 6, 4, 256) == 3
    for bad in (torch.zeros(6, 255), torch.zeros(3, 6, 256), torch.zeros(4, 6, 255), torch.zeros(4, 5, 256)):
        with pytest.raises(ValueError):
            AT.baseline_kind(bad, 6, 4, 256)
    assert AT.default_bin(3840) == 64 and AT.default_bin(256) == 4 and AT.default_bin(30) == 1


def test_cli_flag():
    from multimodalsignal_amd import main as M
    ap = M.build_parser()
    base = ["--synthetic", "/tmp/x"]
    a = M.parse_args(ap, base)
    cfg = M.build_cfg(a, ["cnn_gru_attention"])
    assert a.attribute is None and "attribute" not in cfg and "attribute_bin" not in cfg           # without the flag: no such key
    a = M.parse_args(ap, base + ["--attribute"])
    cfg = M.build_cfg(a, ["cnn_gru_attention"])
    assert a.attribute == 32 and cfg["attribute"] == 32 and "attribute_bin" not in cfg and cfg["synthetic"] is True
    assert M.attribution_settings(cfg) == {"steps": 32, "baseline": "zero", "target": "predicted"}
    a = M.parse_args(ap, base + ["--attribute", "4", "--attribute-bin", "16", "--model", "cnn_gru", "cnn_gru_attention"])
    cfg = M.build_cfg(a, ["cnn_gru_attention", "cnn_gru"])
    assert cfg["attribute"] == 4 and cfg["attribute_bin"] == 16 and M.attribution_settings(cfg)["bin"] == 16
    a = M.parse_args(ap, base + ["--attribute", "--adapt-bn", "--calibrate", "8"])                  # may be combined
    cfg = M.build_cfg(a, ["cnn_gru_attention"])
    assert cfg["attribute"] == 32 and cfg["adapt_bn"] == 1.0 and cfg["calibrate"] == 8
    for bad in (["--attribute", "0"], ["--attribute", "257"], ["--attribute", "x"], ["--attribute-bin", "8"], ["--attribute", "--attribute-bin", "0"],
                ["--attribute", "--hierarchical"], ["--attribute", "--ablation"], ["--attribute", "8", "--sweep", "a=chest_ECG"]):
        with pytest.raises(SystemExit):
            M.parse_args(ap, base + bad)


def test_rejection_wording_is_the_other_stages(capsys):
    from multimodalsignal_amd import main as M
    ap = M.build_parser()
    msgs = []
    for flag in (["--attribute"], ["--adapt-bn"]):
        with pytest.raises(SystemExit):
            M.parse_args(ap, ["--synthetic", "/tmp/x", "--hierarchical"] + flag)
        msgs.append(capsys.readouterr().err.strip().splitlines()[-1].split("error: ")[1])
    assert msgs[0] == msgs[1].replace("--adapt-bn", "--attribute")


def _fold(subject, share_raw, gate=(0.4, 0.5, 0.6), zero=False):
    chan = np.asarray(share_raw, dtype=np.float64)
    den = np.abs(chan).sum()
    share = (np.abs(chan) / den).tolist() if den > 0 else [0.0] * len(chan)
    return {"subject": subject, "n": 12, "steps": 4, "bin": 4, "channels": ["chest_ECG", "chest_EDA", "chest_Resp"], "share": share,
            "signed": chan.tolist(), "signed_by_class": {"0": (-chan).tolist(), "1": None}, "occlusion": (2 * chan).tolist(),
            "time_profile": [0.0] * 4 if zero else [0.1, 0.4, 0.2, 0.1], "gap_rel_mean": 0.0 if zero else 1e-3, "gap_rel_max": 0.0 if zero else 5e-3,
            "gate": None if gate is None else list(gate)}


def test_attribution_tables_from_canned_numbers(tmp_path):
    folds = [_fold("S2", [3.0, -1.0, 1.0]), _fold("S3", [1.0, 1.0, -2.0]), _fold("S4", [0.0, 0.0, 0.0], zero=True)]
    path = AT.write_attribution(tmp_path, folds, {"steps": 4, "baseline": "zero"}, synthetic=True)
    doc = json.loads((tmp_path / "attribution.json").read_text())
    assert doc["n_folds"] == 3 and [f["subject"] for f in doc["folds"]] == ["S2", "S3", "S4"] and doc["settings"] == {"steps": 4, "baseline": "zero"}
    assert doc["note"] == AT.SYNTHETIC_NOTE and "synthetic" in doc["note"]
    for f in doc["folds"][:2]:
        assert sum(f["share"]) == pytest.approx(1.0)                                  # shares sum to 1 per fold
    assert doc["folds"][2]["share"] == [0.0, 0.0, 0.0]                                # an all-zero attribution: no division by zero
    sm = doc["summary"]
    assert sm["share"]["mean"] == pytest.approx(np.mean([[0.6, 0.2, 0.2], [0.25, 0.25, 0.5], [0, 0, 0]], axis=0).tolist())
    assert sm["share"]["std"] == pytest.approx(np.std([[0.6, 0.2, 0.2], [0.25, 0.25, 0.5], [0, 0, 0]], axis=0).tolist())       # population std
    assert sm["signed"]["mean"] == pytest.approx([4 / 3, 0.0, -1 / 3]) and sm["occlusion"]["mean"] == pytest.approx([8 / 3, 0.0, -2 / 3])
    assert sm["gate"]["mean"] == pytest.approx([0.4, 0.5, 0.6]) and doc["ranking"] == ["chest_ECG", "chest_Resp", "chest_EDA"]
    assert doc["gap_rel_max"] == pytest.approx(5e-3) and all(np.isfinite(v) for v in sm["share"]["mean"] + sm["share"]["std"])
    txt = path.read_text(encoding="utf-8")
    assert path.name == "attribution.txt" and AT.SYNTHETIC_NOTE in txt and "steps = 4" in txt and "nan" not in txt.lower()
    assert all(s in txt for s in ("S2", "S3", "S4", "chest_ECG", "share", "occlusion", "gate", "signed|y=0", "0.6000", "channel ranking by mean share",
                                  "chest_ECG > chest_Resp > chest_EDA", "completeness gap"))
    assert "signed|y=1" not in txt                                                     # a class the subject has no window of
    # a baseline model: no gate column, a note instead; a real data set: no synthetic note
    nog = [dict(_fold("S2", [1.0, 1.0, 2.0], gate=None), gate_note="cnn_gru has no gate")]
    AT.write_attribution(tmp_path, nog, {"steps": 4})
    doc = json.loads((tmp_path / "attribution.json").read_text())
    txt = (tmp_path / "attribution.txt").read_text(encoding="utf-8")
    assert "note" not in doc and "NOTE" not in txt and doc["summary"]["gate"] is None and "cnn_gru has no gate" in txt
