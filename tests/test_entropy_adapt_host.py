"""Entropy-minimisation adaptation (include/msig_tt.h, tta.py, --adapt-entropy), what needs no GPU: the fp64 restatement's gradient
against torch autograd, flag parsing and its refusals, the determinism of the epoch order and the launch plan, the table."""
import json

import numpy as np
import pytest
import torch

import tt_reference as TR
from multimodalsignal_amd import main as M
from multimodalsignal_amd import tta
from multimodalsignal_amd.adapt import SYNTHETIC_NOTE, batch_plan


@pytest.mark.parametrize("regime", TR.REGIMES)
@pytest.mark.parametrize("div", TR.DIVERSITIES)
@pytest.mark.parametrize("K", TR.CLASSES)
def test_reference_gradient_is_autograds(K, div, regime):
    """dlogits of the restatement against torch autograd of L in fp64: within 1e-12 (absolute; every element is below 1 / B)."""
    for B in (1, 3, 65):
        z = TR.logits_case(B, K, regime)
        ref = TR.objective(z, div)
        zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
        loss = TR.loss_torch(zt, div)
        loss.backward()
        assert abs(float(loss.detach()) - ref["L"]) <= 1e-12
        assert np.abs(ref["dlogits"] - zt.grad.numpy()).max() <= 1e-12
        assert np.abs(ref["dlogits"].sum(axis=1)).max() <= 1e-15            # a softmax gradient: every row sums to zero
        if regime == "equal" and div == 0.0:
            assert np.abs(ref["dlogits"]).max() <= 1e-15                    # lp + H cancels to rounding at a uniform row
            assert np.allclose(ref["H"], np.log(K), rtol=0, atol=1e-15)


def test_reference_statistics():
    z = TR.logits_case(65, 3, "saturated")
    r = TR.objective(z, 0.5)
    s = r["stats"]
    assert s[TR.S_ROWS] == 65 and s[TR.S_STEPS] == 1 and s[TR.S_PRED:TR.S_PRED + 3].sum() == 65
    assert abs(s[TR.S_P:TR.S_P + 3].sum() - 65) <= 1e-12 and (s[TR.S_P + 3:TR.S_PRED] == 0).all()
    assert abs(TR.mean_objective(s, 0.5) - r["L"]) <= 1e-15
    one_hot = np.array([[80.0, -80.0]] * 4, dtype=np.float32)
    assert TR.objective(one_hot, 1.0)["Hq"] < 1e-60 and np.isfinite(TR.objective(one_hot, 1.0)["dlogits"]).all()


def test_mirrored_constants_match_the_header():
    import re
    from pathlib import Path
    H = (Path(__file__).resolve().parent.parent / "include" / "msig_tt.h").read_text()
    val = lambda name: int(re.search(rf"#define {name}\s+(\d+)", H).group(1))
    assert (val("MSIG_TT_ABI_VERSION"), val("MSIG_TT_MAX_BATCH"), val("MSIG_TT_STATS")) == (tta.TT_ABI_VERSION, tta.TT_MAX_BATCH, tta.TT_STATS)
    assert [val(f"MSIG_TT_S_{n}") for n in ("ENT", "ROWS", "HQ", "STEPS", "P", "PRED")] == [
        tta.TT_S_ENT, tta.TT_S_ROWS, tta.TT_S_HQ, tta.TT_S_STEPS, tta.TT_S_P, tta.TT_S_PRED] == [
        TR.S_ENT, TR.S_ROWS, TR.S_HQ, TR.S_STEPS, TR.S_P, TR.S_PRED]
    assert tta.TT_STATS == TR.TT_STATS == tta.TT_S_PRED + 16 and tta.TT_S_PRED == tta.TT_S_P + 16
    from multimodalsignal_amd import _lib as L
    keys = dict(L.param_keys("cnn_gru_attention"))
    assert [keys[i] for i in (tta.P_BN1_G, tta.P_BN1_B, tta.P_BN2_G, tta.P_BN2_B)] == [
        "cnn_encoder.1.weight", "cnn_encoder.1.bias", "cnn_encoder.5.weight", "cnn_encoder.5.bias"]
    assert [keys[i] for i in (tta.P_GATE_W1, tta.P_GATE_W2)] == list(L.GATE_KEYS)
    assert tta.NPARAM == max(keys) + 1 and tta.SELECT["all"] == (1 << tta.NPARAM) - 1
    assert bin(tta.SELECT["bn"]).count("1") == 4 and tta.SELECT["bn+gate"] == tta.SELECT["bn"] | 0b11


# ---- flags ---------------------------------------------------------------------------------------------------------------------------
def test_flag_values():
    assert tta.parse_flag(None) == tta.parse_flag("") == dict(lr=1e-3, epochs=1, diversity=0.0)
    assert tta.parse_flag("3e-4") == dict(lr=3e-4, epochs=1, diversity=0.0)
    assert tta.parse_flag("0.01:3") == dict(lr=0.01, epochs=3, diversity=0.0)
    assert tta.parse_flag("0:2:0.5") == dict(lr=0.0, epochs=2, diversity=0.5)
    for bad in ("x", "1e-3:", ":2", "1e-3:1.5", "1e-3:0", "-1e-3", "nan", "inf", "1e-3:2:-0.1", "1e-3:2:nan", "1e-3:2:1:4", "1e-3::1"):
        with pytest.raises(ValueError):
            tta.parse_flag(bad)


def test_settings_refusals():
    assert tta.check_settings() == dict(lr=1e-3, epochs=1, diversity=0.0, batch=64, params="bn", seed=0, order="shuffled")
    for kw in (dict(lr=-1.0), dict(lr=float("nan")), dict(lr="a"), dict(epochs=0), dict(epochs=1.5), dict(epochs=True), dict(diversity=-0.1),
               dict(diversity=float("inf")), dict(batch=0), dict(batch=2049), dict(params="head"), dict(order="sorted"), dict(seed=-1)):
        with pytest.raises(ValueError):
            tta.check_settings(**kw)
    assert tta.check_settings(batch=2048, params="all", order="recorded")["batch"] == 2048


def _parse(argv):
    return M.parse_args(M.build_parser(), argv)


def test_driver_flags_parse_into_the_configuration():
    base = ["--synthetic", "x"]
    args = _parse(base)
    assert args.adapt_entropy is None
    cfg = M.build_cfg(args, ["cnn_gru_attention"])
    assert not any(k.startswith("adapt_entropy") for k in cfg)                # without the flag there is no such key
    args = _parse(base + ["--adapt-entropy"])
    assert args.adapt_entropy == dict(lr=1e-3, epochs=1, diversity=0.0)
    cfg = M.build_cfg(args, ["cnn_gru_attention"])
    assert cfg["adapt_entropy"] == dict(lr=1e-3, epochs=1, diversity=0.0) and cfg["adapt_entropy_batched"] is True and cfg["synthetic"] is True
    assert "adapt_entropy_params" not in cfg and "adapt_entropy_batch" not in cfg
    assert tta.settings_of(cfg) == dict(lr=1e-3, epochs=1, diversity=0.0, params="bn", batch=64, order="shuffled", seed=0)
    args = _parse(base + ["--adapt-entropy", "1e-2:2:0.5", "--adapt-entropy-params", "bn+gate", "--adapt-entropy-batch", "32",
                          "--adapt-entropy-sequential", "--adapt-bn", "0.5"])
    cfg = M.build_cfg(args, ["cnn_gru_attention"])
    assert cfg["adapt_entropy"] == dict(lr=1e-2, epochs=2, diversity=0.5) and cfg["adapt_entropy_batched"] is False
    assert tta.settings_of(cfg) == dict(lr=1e-2, epochs=2, diversity=0.5, params="bn+gate", batch=32, order="shuffled", seed=0, adabn_alpha=0.5)
    json.dumps(cfg["adapt_entropy"])


@pytest.mark.parametrize("argv", [["--adapt-entropy", "abc"], ["--adapt-entropy", "1e-3:0"], ["--adapt-entropy", "-1"],
                                  ["--adapt-entropy", "1e-3:1:-1"], ["--adapt-entropy", "1e-3:1:1:1"],
                                  ["--adapt-entropy", "--adapt-entropy-batch", "0"], ["--adapt-entropy", "--adapt-entropy-batch", "2049"],
                                  ["--adapt-entropy", "--adapt-entropy-params", "head"],
                                  ["--adapt-entropy-params", "bn"], ["--adapt-entropy-batch", "8"], ["--adapt-entropy-sequential"],
                                  ["--adapt-entropy", "--hierarchical"], ["--adapt-entropy", "--ablation"]])
def test_malformed_values_are_refused_before_any_training(argv, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(["--synthetic", "x"] + argv)
    assert e.value.code == 2
    assert "adapt-entropy" in capsys.readouterr().err


# ---- order and plan --------------------------------------------------------------------------------------------------------------------
def test_epoch_order_is_a_deterministic_permutation():
    for n in (1, 2, 37, 150):
        a, b = tta.epoch_order(n, 0, 0), tta.epoch_order(n, 0, 0)
        assert a.dtype == np.int64 and (a == b).all() and sorted(a) == list(range(n))
        assert (tta.epoch_order(n, 0, 0, "recorded") == np.arange(n)).all()
    assert (tta.epoch_order(150, 0, 0) != tta.epoch_order(150, 0, 1)).any()             # a new order per epoch
    assert (tta.epoch_order(150, 0, 0) != tta.epoch_order(150, 1, 0)).any()             # and per seed
    assert list(tta.epoch_order(8, 3, 2)) == list(np.random.default_rng([3, 2]).permutation(8))


def test_plan_is_deterministic_and_covers_every_window_once():
    sizes = [37, 21, 37, 64, 5]
    plan = batch_plan(sizes, 16)
    assert plan == batch_plan(list(sizes), 16)
    seen = {j: [] for j in range(len(sizes))}
    for first, b, jobs in plan:
        assert 1 <= b <= 16 and len(set(jobs)) == len(jobs)
        for j in jobs:
            seen[j].extend(range(first, first + b))
    assert all(seen[j] == list(range(n)) for j, n in enumerate(sizes))
    steps = {j: sum(j in jobs for _, _, jobs in plan) for j in seen}
    assert steps == {j: -(-n // 16) for j, n in enumerate(sizes)}                       # folds of a batch take different step counts


# ---- the table -------------------------------------------------------------------------------------------------------------------------
def _fold(s, acc0, acc1, start=None):
    f = dict(subject=s, n=150, before=dict(accuracy=acc0, f1_score=acc0 - 0.01), after=dict(accuracy=acc1, f1_score=acc1 - 0.02),
             entropy=dict(before=0.41, after=0.12), shares=dict(before=[0.6, 0.4], after=[0.9, 0.1]), flipped=7, objective=[0.4, 0.2])
    if start is not None:
        f["start"] = dict(accuracy=start, f1_score=start - 0.01, entropy=0.3, shares=[0.5, 0.5])
    return f


def test_table_has_both_columns_the_collapse_indicator_and_the_note(tmp_path):
    folds = [_fold("S2", 0.8, 0.9), _fold("S3", 0.7, 0.6), _fold("S4", 0.5, 0.5)]
    st = dict(lr=1e-3, epochs=1, diversity=0.0, params="bn", batch=64, order="shuffled", seed=0)
    path = tta.write_entropy_adaptation(tmp_path, folds, st, synthetic=True)
    assert path.name == "entropy_adaptation.txt"
    doc = json.loads((tmp_path / "entropy_adaptation.json").read_text())
    assert doc["n_folds"] == 3 and doc["settings"] == st and doc["note"] == SYNTHETIC_NOTE
    assert (doc["wins"]["accuracy"], doc["ties"]["accuracy"], doc["losses"]["accuracy"]) == (1, 1, 1)
    assert abs(doc["summary"]["accuracy"]["difference"]["mean"]) < 1e-12
    assert doc["folds"][0]["shares"] == dict(before=[0.6, 0.4], after=[0.9, 0.1]) and doc["folds"][0]["flipped"] == 7
    txt = path.read_text(encoding="utf-8")
    assert SYNTHETIC_NOTE in txt and "not known" in txt and "mean paired difference" in txt and "AdaBN" not in txt
    row = next(l for l in txt.splitlines() if l.lstrip().startswith("S2"))
    assert "0.8000" in row and "0.9000" in row and "+0.1000" in row and "0.4100" in row and "0.1200" in row
    assert "[0.60 0.40] -> [0.90 0.10]" in row and " 7 " in row
    head = next(l for l in txt.splitlines() if "LOSO acc" in l)
    assert head.index("LOSO acc") < head.index("adapt acc") and "predicted-class shares" in head
    assert "NOTE" not in tta.format_entropy(doc, st, synthetic=False)


def test_table_with_adabn_has_three_columns(tmp_path):
    folds = [_fold("S2", 0.8, 0.9, 0.85), _fold("S3", 0.7, 0.6, 0.75)]
    st = dict(lr=1e-3, epochs=1, diversity=0.0, params="bn", batch=64, order="shuffled", seed=0, adabn_alpha=1.0)
    txt = tta.write_entropy_adaptation(tmp_path, folds, st).read_text(encoding="utf-8")
    head = next(l for l in txt.splitlines() if "LOSO acc" in l)
    assert head.index("LOSO acc") < head.index("AdaBN acc") < head.index("adapt acc")
    row = next(l for l in txt.splitlines() if l.lstrip().startswith("S2"))
    assert row.index("0.8000") < row.index("0.8500") < row.index("0.9000")
    assert "AdaBN 0.8000" in txt and "LOSO, AdaBN, AdaBN + entropy" in txt
    assert json.loads((tmp_path / "entropy_adaptation.json").read_text())["folds"][0]["start"]["accuracy"] == 0.85
