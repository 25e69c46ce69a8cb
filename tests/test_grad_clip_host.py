"""Gradient-norm clipping, the host side checked without a GPU: the trainer's setting, the key's way from the command line into
every Trainer's configuration, and the summary line that appears only when the option is set."""
import pytest

from multimodalsignal_amd import _lib as L
from multimodalsignal_amd import main as M
from multimodalsignal_amd.trainer import grad_clip_setting, grad_norm_summary


def test_setting_accepts_none_and_positive_finite_numbers():
    assert grad_clip_setting(None) is None
    for v in (1, 1.0, 0.25, 1e-6, 1e30):
        got = grad_clip_setting(v)
        assert isinstance(got, float) and got == float(v)
    import numpy as np
    assert grad_clip_setting(np.float32(2.0)) == 2.0


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan"), float("inf"), -float("inf"), "1.0", "none", True, [1.0], (2.0,)])
def test_setting_rejects_everything_else(bad):
    with pytest.raises(ValueError):
        grad_clip_setting(bad)


def test_binding_check_allows_infinity_only_upwards():
    assert L.check_max_grad_norm(float("inf")) == float("inf") and L.check_max_grad_norm(3) == 3.0
    for bad in (0.0, -2.0, float("nan"), -float("inf"), "x", "1", b"1", None, True):
        with pytest.raises(ValueError):
            L.check_max_grad_norm(bad)


def test_summary_of_an_epoch():
    assert grad_norm_summary(dict(sum=6.0, max=3.5, clipped=2.0, last=1.0), 4) == dict(grad_norm_mean=1.5, grad_norm_max=3.5, clipped_steps=2)


def test_trainer_config_carries_the_key_only_when_set():
    base = M.default_cfg()
    assert "max_grad_norm" not in base
    for fold in (0, 3):
        assert "max_grad_norm" not in M.trainer_config(base, fold)["trainer"]
        tc = M.trainer_config(dict(base, max_grad_norm=0.5), fold)["trainer"]
        assert tc["max_grad_norm"] == 0.5
        assert {k: v for k, v in tc.items() if k != "max_grad_norm"} == M.trainer_config(base, fold)["trainer"]
    assert M.trainer_config(dict(base, max_grad_norm=None), 0) == M.trainer_config(base, 0)
    with pytest.raises(ValueError):
        M.trainer_config(dict(base, max_grad_norm=-1.0), 0)
    both = M.trainer_config(dict(base, max_grad_norm=2, class_weights="balanced"), 1)["trainer"]
    assert both["max_grad_norm"] == 2.0 and both["class_weights"] == "balanced"


@pytest.mark.parametrize("mode", [[], ["--ablation"], ["--hierarchical"], ["--model", "cnn_gru", "cnn_gru_attention"], ["--concurrent-folds", "1"],
                                  ["--no-lockstep"]])
def test_cli_parses_in_every_mode(mode):
    ap = M.build_parser()
    args = M.parse_args(ap, ["--synthetic", "x", "--max-grad-norm", "1.5", *mode])
    assert args.max_grad_norm == 1.5
    assert M.parse_args(M.build_parser(), ["--synthetic", "x", *mode]).max_grad_norm is None


@pytest.mark.parametrize("bad", ["0", "-1", "nan", "inf", "abc"])
def test_cli_rejects_bad_values(bad, capsys):
    with pytest.raises(SystemExit):
        M.parse_args(M.build_parser(), ["--max-grad-norm", bad])
    assert "max-grad-norm" in capsys.readouterr().err


def test_summaries_name_the_setting_only_when_set(tmp_path):
    res = [{"subject": "S2", "accuracy": 0.5, "f1_score": 0.5}]
    base = M.default_cfg()
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    ta = M.write_summary(tmp_path / "a", res, base, 1.0, 1).read_text(encoding="utf-8")
    tb = M.write_summary(tmp_path / "b", res, dict(base, max_grad_norm=1.0), 1.0, 1).read_text(encoding="utf-8")
    assert "MAX_GRAD_NORM" not in ta
    assert "MAX_GRAD_NORM: 1\n" in tb and tb.replace("MAX_GRAD_NORM: 1\n", "") == ta
