"""Sharpness-aware minimisation, the host layers checked without a GPU: the setting and its parser, the configuration keys, the
refused combination, the summary of an epoch's statistics."""
import pytest

from multimodalsignal_amd import _lib as L
from multimodalsignal_amd import main as M
from multimodalsignal_amd import sam as S
from multimodalsignal_amd.sam import Sam


def _cfg(argv):
    ap = M.build_parser()
    args = M.parse_args(ap, argv)
    return M.build_cfg(args, [k for k in M.MODEL_PARAMS if k in args.model])


def test_setting_holds_the_fp32_values_the_calls_see():
    s = Sam(0.05)
    assert (s.rho, s.adaptive, s.eta, s.on) == (L.C.c_float(0.05).value, False, L.C.c_float(0.01).value, True)
    a = Sam(0.5, adaptive=True, eta=0.0)
    assert (a.adaptive, a.eta, a.spec()) == (True, 0.0, "0.5:adaptive:0")
    assert not Sam(0).on and Sam(0.05) == Sam(0.05) and Sam(0.05) != Sam(0.05, True) and len({Sam(0.1), Sam(0.1)}) == 1
    d = a.descriptor("cnn_gru", 4096, 123456)
    assert (d.kind, d.adaptive, d.rho, d.eta, d.state, d.state_bytes) == (1, 1, 0.5, 0.0, 4096, 123456)
    assert Sam(0.05).descriptor("cnn_gru_attention", 8, 16).kind == 0


@pytest.mark.parametrize("kw", [dict(rho=-0.1), dict(rho=float("nan")), dict(rho=float("inf")), dict(rho="0.05"), dict(rho=None), dict(rho=True),
                                dict(rho=0.05, eta=-1.0), dict(rho=0.05, eta=float("nan")), dict(rho=0.05, eta="x"),
                                dict(rho=0.05, adaptive="yes"), dict(rho=0.05, adaptive=2)])
def test_bad_arguments_are_value_errors(kw):
    with pytest.raises(ValueError):
        Sam(**kw)
    with pytest.raises(ValueError):
        Sam(0.05).descriptor("transformer", 8, 16)


def test_parser_accepts():
    assert Sam.parse("0.05") == Sam(0.05) and Sam.parse("0.05").spec() == "0.05"
    assert Sam.parse("2:adaptive") == Sam(2.0, True, 0.01) and Sam.parse("2:adaptive").spec() == "2:adaptive:0.01"
    assert Sam.parse("0.5:adaptive:0.1") == Sam(0.5, True, 0.1)
    assert Sam.parse("1e-2") == Sam(0.01) and Sam.parse(0.05) == Sam(0.05) and Sam.parse("0") == Sam(0.0)
    s = Sam(0.3, True)
    assert Sam.parse(s) is s and Sam.parse(s.spec()) == s
    assert S.setting(None) is None and S.setting("0.05") == Sam(0.05)


@pytest.mark.parametrize("text", ["", "x", "0.05:", "0.05:sam", "0.05:adaptive:", "0.05:adaptive:x", "0.05:adaptive:0.01:1", "-0.05", "nan", "inf",
                                  "0.05:adaptive:-1", ":adaptive", None, True, [0.05]])
def test_parser_rejects(text):
    with pytest.raises(ValueError):
        Sam.parse(text)


def test_key_exists_only_with_the_flag_and_reaches_every_trainer_config():
    assert "sam" not in _cfg([]) and "sam" not in M.trainer_config(_cfg([]), 0)["trainer"]
    assert "sam" not in _cfg(["--sam", "0"])                                        # --sam 0 is the run without the flag
    assert _cfg(["--sam", "0.05"])["sam"] == "0.05"
    assert _cfg(["--sam", "0.05:adaptive"])["sam"] == "0.05:adaptive:0.01"
    for extra in ([], ["--hierarchical"], ["--ablation"], ["--model", "cnn_gru_attention", "cnn_gru"], ["--seeds", "2"], ["--seeds", "2", "--distill"],
                  ["--max-grad-norm", "1"], ["--label-smoothing", "0.1", "--mixup", "0.2"], ["--weight-average", "ema"], ["--no-lockstep"]):
        cfg = _cfg(["--sam", "0.1:adaptive:0.02"] + extra)
        assert cfg["sam"] == "0.1:adaptive:0.02", extra
        assert M.trainer_config(cfg, 3)["trainer"]["sam"] == "0.1:adaptive:0.02", extra
        assert S.setting(M.trainer_config(cfg, 3)["trainer"]["sam"]) == Sam(0.1, True, 0.02)


@pytest.mark.parametrize("argv", [["--sam", "0.05", "--subject-adversarial"], ["--sam", "0.05:adaptive", "--subject-adversarial", "0.5"],
                                  ["--sam", "-1"], ["--sam", "0.05:adapt"], ["--sam", "x"], ["--sam"], ["--sam", "0.05:adaptive:-0.1"]])
def test_refused_combinations_error_before_any_gpu_work(argv, capsys):
    with pytest.raises(SystemExit) as e:
        _cfg(argv)
    assert e.value.code == 2
    assert "--sam" in capsys.readouterr().err


def test_summary_echoes_the_setting_only_with_the_flag(tmp_path):
    results = [{"subject": "S2", "accuracy": 0.5, "f1_score": 0.4}]
    text = M.write_summary(tmp_path, results, _cfg([]), 1.0, 1).read_text(encoding="utf-8")
    assert "SAM" not in text
    with_flag = M.write_summary(tmp_path, results, _cfg(["--sam", "0.05"]), 1.0, 1).read_text(encoding="utf-8")
    assert with_flag.replace("SAM: 0.05\n", "") == text and with_flag != text


def test_epoch_summary():
    st = [0.0] * L.SAM_NSTAT
    st[L.SAM_NORM_SUM], st[L.SAM_NORM_MAX], st[L.SAM_SHARP_SUM], st[L.SAM_STEPS] = 6.0, 2.5, 0.3, 4.0
    assert S.summary(st, 4) == dict(sam_grad_norm=1.5, sam_grad_norm_max=2.5, sam_sharpness=0.3 / 4)
    assert S.summary([0.0] * L.SAM_NSTAT, 0) == dict(sam_grad_norm=0.0, sam_grad_norm_max=0.0, sam_sharpness=0.0)
