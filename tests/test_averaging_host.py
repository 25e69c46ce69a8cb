"""Weight averaging, the host side without a GPU: averaging.settings, the two coefficient schedules against tests/wa_reference.py and
the issue's spot values, the reference replay, WeightAverager's counters, and the command line."""
import numpy as np
import pytest

import wa_reference as R
from multimodalsignal_amd import averaging as AV


# ---- settings ----------------------------------------------------------------------------------------------------------------------
def test_settings_defaults():
    assert AV.settings(None) is None
    assert AV.settings({"mode": "ema"}) == dict(mode="ema", decay=0.99, warmup=10, start_epoch=10, bn="average", validate=False)
    assert AV.settings({"mode": "swa"}) == dict(mode="swa", decay=0.99, warmup=10, start_epoch=10, bn="recompute", validate=False)
    got = AV.settings({"mode": "swa", "start_epoch": 3, "bn": "average", "validate": True, "decay": 0, "warmup": 0})
    assert got == dict(mode="swa", decay=0.0, warmup=0, start_epoch=3, bn="average", validate=True)
    assert AV.settings(AV.settings({"mode": "ema", "decay": 0.9})) == AV.settings({"mode": "ema", "decay": 0.9})      # idempotent


@pytest.mark.parametrize("bad", [
    "ema", 5, {}, {"mode": "avg"}, {"mode": None}, {"mode": "ema", "decay": 1.0}, {"mode": "ema", "decay": -0.1},
    {"mode": "ema", "decay": float("nan")}, {"mode": "ema", "decay": "0.9"}, {"mode": "ema", "decay": True},
    {"mode": "ema", "decay": 1.0 - 1e-12},                                             # 1.0 as the fp32 number the library would see
    {"mode": "ema", "warmup": -1}, {"mode": "ema", "warmup": 2.5}, {"mode": "ema", "warmup": True},
    {"mode": "swa", "start_epoch": 0}, {"mode": "swa", "start_epoch": 1.0}, {"mode": "swa", "bn": "keep"},
    {"mode": "ema", "validate": 1}, {"mode": "ema", "horizon": 100}])
def test_settings_reject_bad_values(bad):
    with pytest.raises(ValueError):
        AV.settings(bad)


def test_trainer_config_checks_before_any_training():
    from multimodalsignal_amd import main as M
    cfg = dict(M.default_cfg(), averaging={"mode": "ema", "decay": 2.0})
    with pytest.raises(ValueError):
        M.trainer_config(cfg, 0)
    assert M.trainer_config(dict(cfg, averaging={"mode": "swa"}), 0)["averaging"]["bn"] == "recompute"
    assert "averaging" not in M.trainer_config(M.default_cfg(), 0)


# ---- schedules ---------------------------------------------------------------------------------------------------------------------
def test_ema_spot_values():
    assert AV.ema_coef(0, 0.99, 10) == np.float32(0.9)
    assert AV.ema_coef(90, 0.99, 10) == np.float32(0.09)
    for t in (990, 991, 5000, 10 ** 6):
        assert AV.ema_coef(t, 0.99, 10) == np.float32(0.01)
    assert AV.ema_coef(889, 0.99, 10) > np.float32(0.01) == AV.ema_coef(890, 0.99, 10)      # (1 + t) / (10 + t) reaches 0.99 at t = 890
    for decay in (0.0, 0.5, 0.99, 0.999):
        for t in (0, 1, 7, 10 ** 4):
            assert AV.ema_coef(t, decay, 0) == np.float32(1.0 - decay)


def test_swa_spot_values():
    assert [AV.swa_coef(k) for k in range(5)] == [np.float32(1.0), np.float32(0.5), np.float32(1.0 / 3.0), np.float32(0.25), np.float32(0.2)]


def test_schedules_equal_the_reference_and_are_fp32_numbers():
    for decay, warmup in ((0.99, 10), (0.9, 0), (0.999, 100), (0.0, 3)):
        for t in list(range(0, 40)) + [89, 90, 91, 989, 990, 12345]:
            a = AV.ema_coef(t, decay, warmup)
            assert a == R.ema_coef(t, decay, warmup) and np.float32(a) == a and 0.0 <= a <= 1.0
    for k in range(200):
        a = AV.swa_coef(k)
        assert a == R.swa_coef(k) and np.float32(a) == a and 0.0 < a <= 1.0


# ---- the reference itself ----------------------------------------------------------------------------------------------------------
def test_reference_update_cases():
    s = np.array([1.0, -2.0, 0.0, np.inf], np.float32)
    p = np.array([3.0, 0.5, -0.0, 1.0], np.float32)
    assert R.update(s, p, 0.0).tobytes() == s.tobytes()
    assert R.update(s, p, 1.0).tobytes() == p.tobytes()
    got = R.update(s[:2], p[:2], 0.25)
    assert got.dtype == np.float32 and got.tolist() == [1.5, -1.375]
    # three roundings, not a fused multiply-add: a value where the two differ
    s1, p1, a = np.float32(1.0), np.float32(1.0 + 2.0 ** -12), np.float32(0.1)
    want = np.float32(s1 + np.float32(a * np.float32(p1 - s1)))
    assert R.update([s1], [p1], a)[0] == want


def test_reference_replay_of_a_constant_sequence_returns_it_exactly():
    rs = np.random.RandomState(0)
    w = np.concatenate([rs.randn(64).astype(np.float32) * 3, np.array([0.0, 1e-30, 1e-42, -7.25e10, 3.0e38], np.float32)])
    assert R.replay_ema(w, [w] * 25).tobytes() == w.tobytes()
    assert R.replay_ema(w, [w] * 7, decay=0.5, warmup=0).tobytes() == w.tobytes()
    assert R.replay_swa([w] * 9).tobytes() == w.tobytes()
    # the one value the formula does not keep bit for bit: s + a * (p - s) of two negative zeros is +0.0 (equal as a number)
    z = np.array([-0.0], np.float32)
    assert R.replay_ema(z, [z]).tobytes() == np.array([0.0], np.float32).tobytes() and R.replay_ema(z, []).tobytes() == z.tobytes()


def test_reference_swa_is_the_running_mean():
    rs = np.random.RandomState(1)
    its = [rs.randn(32).astype(np.float32) for _ in range(6)]
    np.testing.assert_allclose(R.replay_swa(its), np.mean(np.stack(its).astype(np.float64), axis=0), rtol=0, atol=1e-6)
    assert R.replay_swa(its[:1]).tobytes() == its[0].tobytes()


# ---- the averager's counters -------------------------------------------------------------------------------------------------------
def test_ema_averager_counts_updates():
    av = AV.WeightAverager({"mode": "ema"})
    assert not av.ready and av.start_coef() == 1.0 and av.ready and av.start_coef() == 0.0
    assert av.peek_step_coefs(3) == [AV.ema_coef(t) for t in range(3)] and av.updates == 0
    assert [av.step_coef() for _ in range(3)] == [AV.ema_coef(t) for t in range(3)] and av.updates == 3
    av.advance(4)
    assert av.updates == 7 and av.step_coef() == AV.ema_coef(7)
    assert av.epoch_coef(50) == 0.0 and av.final_coef() == 0.0 and av.finished
    assert av.summary() == dict(mode="ema", updates=8, iterates=0, bn="average")
    with pytest.raises(RuntimeError):
        av.state_dict()                                  # no engine bound


def test_swa_averager_counts_iterates_and_falls_back_to_the_final_weights():
    av = AV.WeightAverager({"mode": "swa", "start_epoch": 3})
    assert av.start_coef() == 0.0 and av.step_coef() == 0.0 and av.peek_step_coefs(2) == [0.0, 0.0] and not av.ready
    assert [av.epoch_coef(e) for e in (1, 2, 3, 4, 5)] == [0.0, 0.0, 1.0, 0.5, AV.swa_coef(2)]
    assert av.iterates == 3 and av.ready and av.final_coef() == 0.0
    early = AV.WeightAverager({"mode": "swa", "start_epoch": 3})
    assert early.epoch_coef(1) == 0.0 and early.epoch_coef(2) == 0.0
    assert early.final_coef() == 1.0 and early.iterates == 0 and early.ready
    with pytest.raises(ValueError):
        AV.WeightAverager(None)


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def test_fold_record_and_table(tmp_path):
    infos = [dict(subject=f"S{i}", accuracy=(0.5, 0.75, 0.875)[i], f1_score=0.5, history=[],
                  averaging=dict(mode="ema", updates=20 + i, iterates=0, bn="average", val_loss=0.4, val_acc=0.9, val_f1=0.9, loso_val_loss=0.5,
                                 test_loss=0.3, accuracy=0.75, f1_score=(0.5, 0.75, 0.25)[i])) for i in range(3)]
    folds = [AV.fold_record(i) for i in infos]
    assert AV.fold_record(dict(subject="S9", accuracy=0.5, f1_score=0.5)) is None
    assert folds[1] == dict(subject="S1", updates=21, iterates=0, before={"accuracy": 0.75, "f1_score": 0.5},
                            after={"accuracy": 0.75, "f1_score": 0.75}, val_loss=0.5, val_loss_avg=0.4)
    path = AV.write_averaging(tmp_path, folds, {"mode": "ema"}, synthetic=True)
    import json
    doc = json.loads((tmp_path / "averaging.json").read_text())
    assert doc["n_folds"] == 3 and doc["settings"] == AV.settings({"mode": "ema"}) and doc["note"] == AV.SYNTHETIC_NOTE
    assert (doc["wins"], doc["ties"], doc["losses"]) == ({"accuracy": 1, "f1_score": 1},) * 3
    assert doc["summary"]["accuracy"]["difference"]["mean"] == pytest.approx((0.25 + 0.0 - 0.125) / 3)
    txt = path.read_text(encoding="utf-8")
    assert "WEIGHT AVERAGING: mode=ema decay=0.99 warmup=10 bn=average" in txt and AV.SYNTHETIC_NOTE in txt and "not known" in txt
    assert all(f"S{i}" in txt for i in range(3)) and "mean paired difference" in txt


# ---- the command line --------------------------------------------------------------------------------------------------------------
def _parse(*argv):
    from multimodalsignal_amd import main as M
    ap = M.build_parser()
    args = M.parse_args(ap, list(argv))
    return args, M.build_cfg(args, [k for k in M.MODEL_PARAMS if k in args.model])


def test_cli_maps_to_the_configuration():
    args, cfg = _parse()
    assert args.weight_average is None and "averaging" not in cfg
    _, cfg = _parse("--weight-average", "ema")
    assert cfg["averaging"] == AV.settings({"mode": "ema"})
    _, cfg = _parse("--weight-average", "ema:0.9", "--average-bn", "recompute", "--average-validate")
    assert cfg["averaging"] == dict(mode="ema", decay=0.9, warmup=10, start_epoch=10, bn="recompute", validate=True)
    _, cfg = _parse("--weight-average", "swa:4")
    assert cfg["averaging"] == dict(mode="swa", decay=0.99, warmup=10, start_epoch=4, bn="recompute", validate=False)
    _, cfg = _parse("--weight-average", "swa", "--average-bn", "average", "--model", "cnn_gru_attention", "cnn_gru", "--adapt-bn",
                    "--calibrate", "4", "--attribute", "--mc-dropout", "--subject-adversarial", "--mixup", "0.2", "--max-grad-norm", "1")
    assert cfg["averaging"]["bn"] == "average" and cfg["adapt_bn"] == 1.0 and cfg["calibrate"] == 4


@pytest.mark.parametrize("argv", [
    ["--weight-average", "sma"], ["--weight-average", "ema:"], ["--weight-average", "ema:1.0"], ["--weight-average", "ema:x"],
    ["--weight-average", "swa:0"], ["--weight-average", "swa:2.5"], ["--weight-average", "ema", "--hierarchical"],
    ["--weight-average", "ema", "--ablation"], ["--weight-average", "swa", "--sweep", "a=chest_ECG"], ["--average-bn", "average"],
    ["--average-validate"], ["--weight-average", "ema", "--average-bn", "keep"]])
def test_cli_errors(argv, capsys):
    with pytest.raises(SystemExit):
        _parse(*argv)
    assert "--weight-average" in capsys.readouterr().err or "--average-bn" in " ".join(argv)
