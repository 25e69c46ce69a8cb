"""The cnn_gru baseline (include/msig_cg.h, models.CnnGruModel), checked without a GPU: the new header's calls are exported beside
unchanged msig.h / msig_cw.h, every rejection happens before the first launch (descriptors with fake, aligned, never dereferenced
pointers, as in test_class_weights_host.py), the parameter layout and state_dict are the attention model's minus the gate, the
initial weights are a stock torch.nn graph's, fold batches refuse mixed kinds, and the driver's --model flag and comparison writer."""
import ctypes as C
import json
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

from multimodalsignal_amd import _lib as L
from multimodalsignal_amd import main as M
from multimodalsignal_amd.models import CnnGruAttentionModel, CnnGruModel
from multimodalsignal_amd.multifold import lockstep_compatible

ROOT = Path(__file__).resolve().parent.parent
CG_HEADER = (ROOT / "include" / "msig_cg.h").read_text()
E_NULL, E_SHAPE, E_ALIGN, E_WORKSPACE, E_FORM = -1, -2, -3, -4, -5
B, CH, T, K = 8, 6, 512, 2
f = C.c_float


def test_msig_cg_header_calls_are_exported_and_the_other_headers_are_unchanged():
    names = sorted(set(re.findall(r"\b(msig_cg_\w+)\(", CG_HEADER)))
    assert names == ["msig_cg_abi_version", "msig_cg_backward", "msig_cg_forward", "msig_cg_forward_multi", "msig_cg_param_layout",
                     "msig_cg_train_step", "msig_cg_train_step_multi"]
    lib = L.lib()
    for n in names:
        assert getattr(lib, n) is not None
    assert lib.msig_cg_abi_version() == int(re.search(r"#define MSIG_CG_ABI_VERSION (\d+)", CG_HEADER).group(1)) == L.CG_ABI_VERSION
    msig_h = (ROOT / "include" / "msig.h").read_text()
    assert len(set(re.findall(r"\b(msig_\w+)\(", msig_h))) == 26
    assert "msig_cg" not in msig_h
    assert lib.msig_abi_version() == L.ABI_VERSION == 5
    cw_h = (ROOT / "include" / "msig_cw.h").read_text()
    assert sorted(set(re.findall(r"\b(msig_cw_\w+)\(", cw_h))) == ["msig_cw_abi_version", "msig_cw_forward", "msig_cw_forward_multi",
                                                                  "msig_cw_train_step", "msig_cw_train_step_multi"]
    assert "msig_cg" not in cw_h and lib.msig_cw_abi_version() == 1


def _batch(training, ws_bytes, C_=CH, **kw):
    keep_alive = (C.c_char * 8192)()
    addr = (C.addressof(keep_alive) + 255) // 256 * 256
    b = L.Batch()
    b.shape = L.Shape(kw.get("B", B), C_, T, kw.get("K", K))
    b.training = training
    for name in ("x", "labels", "params", "grads", "bn_state", "bn_count", "ws"):
        setattr(b, name, addr)
    b.ws_bytes = ws_bytes
    b.gru_layers = 2
    return b, keep_alive, addr


def _multi(n=2):
    m = L.Multi()
    m.n, m.stride_bytes = n, 1 << 20
    for i in range(n):
        m.slot[i] = i
    return m


def _calls(b, m, cw, addr):
    """Every msig_cg.h launcher on one descriptor (the backward takes no weight)."""
    lib = L.lib()
    return [lib.msig_cg_forward(C.byref(b), cw, None),
            lib.msig_cg_train_step(C.byref(b), cw, addr, addr, f(1e-3), f(0.9), f(0.999), f(1e-8), f(0.0), 1, None),
            lib.msig_cg_forward_multi(C.byref(b), C.byref(m), cw, None),
            lib.msig_cg_train_step_multi(C.byref(b), C.byref(m), cw, addr, addr, f(0.9), f(0.999), f(1e-8), f(0.0), 1, None)]


def test_misaligned_weight_pointer_is_rejected_first():
    small = L.workspace_layout(B, CH, T, K, True)[-1] - 1
    b, _k, addr = _batch(1, small)
    m = _multi()
    assert _calls(b, m, addr + 2, addr) == [E_ALIGN] * 4
    assert _calls(b, m, addr + 4, addr) == [E_WORKSPACE] * 4
    assert _calls(b, m, None, addr) == [E_WORKSPACE] * 4
    assert L.lib().msig_cg_backward(C.byref(b), None, None) == E_WORKSPACE


def test_counterpart_checks_hold():
    """msig.h's checks, code for code: NULL descriptor, bad shape, misaligned buffers, bad kernel form, no labels in a train step, an
    eval descriptor in a backward, dx in the fused and fold-batch calls, a bad fold batch — nothing launched."""
    lib = L.lib()
    full = L.workspace_layout(B, CH, T, K, True)[-1]
    small = full - 1
    _, _k0, addr0 = _batch(1, small)
    assert lib.msig_cg_forward(None, None, None) == E_NULL
    assert lib.msig_cg_backward(None, None, None) == E_NULL
    assert lib.msig_cg_train_step(None, None, addr0, addr0, f(1e-3), f(0.9), f(0.999), f(1e-8), f(0.0), 1, None) == E_NULL
    assert lib.msig_cg_forward_multi(None, C.byref(_multi()), None, None) == E_NULL
    assert lib.msig_cg_train_step_multi(None, C.byref(_multi()), None, addr0, addr0, f(0.9), f(0.999), f(1e-8), f(0.0), 1, None) == E_NULL
    b, _k, addr = _batch(1, small)
    assert lib.msig_cg_forward_multi(C.byref(b), None, None, None) == E_NULL
    for kw in (dict(K=1), dict(K=L.MAX_K + 1), dict(B=0)):
        b, _k, addr = _batch(1, 1, **kw)
        assert _calls(b, _multi(), None, addr) == [E_SHAPE] * 4, kw
        assert lib.msig_cg_backward(C.byref(b), None, None) == E_SHAPE
    for C_ in (0, L.MAX_C + 1):
        b, _k, addr = _batch(1, 1 << 40, C_=C_)
        assert _calls(b, _multi(), None, addr) == [E_SHAPE] * 4, C_
    b, _k, addr = _batch(1, small)
    b.x = addr + 4                                                       # 16-byte alignment of the input
    assert _calls(b, _multi(), None, addr) == [E_ALIGN] * 4
    assert lib.msig_cg_backward(C.byref(b), None, None) == E_ALIGN
    b, _k, addr = _batch(1, small)
    b.fwd_form = 99
    assert _calls(b, _multi(), None, addr) == [E_FORM] * 4
    b, _k, addr = _batch(1, small)
    b.labels = None
    assert lib.msig_cg_train_step(C.byref(b), None, addr, addr, f(1e-3), f(0.9), f(0.999), f(1e-8), f(0.0), 1, None) == E_NULL
    b, _k, addr = _batch(0, L.workspace_layout(B, CH, T, K, False)[-1] + 4096)
    assert lib.msig_cg_backward(C.byref(b), None, None) == E_SHAPE            # an eval forward that kept nothing
    assert lib.msig_cg_train_step(C.byref(b), None, addr, addr, f(1e-3), f(0.9), f(0.999), f(1e-8), f(0.0), 1, None) == E_SHAPE
    # dx: only the single-model forward / backward take it; the fused step and the fold batches refuse it before anything runs
    b, _k, addr = _batch(1, small)
    b.dx = addr
    assert _calls(b, _multi(), None, addr) == [E_WORKSPACE, E_SHAPE, E_SHAPE, E_SHAPE]
    assert lib.msig_cg_backward(C.byref(b), None, None) == E_WORKSPACE
    b.dx = addr + 4
    assert lib.msig_cg_forward(C.byref(b), None, None) == E_ALIGN
    b, _k, addr = _batch(0, full)
    b.dx = addr                                                          # dx without a forward kept for a backward
    assert lib.msig_cg_forward(C.byref(b), None, None) == E_SHAPE
    b, _k, addr = _batch(1, small)
    bad = _multi(1)
    bad.n = 0
    assert _calls(b, bad, None, addr)[2:] == [E_SHAPE] * 2
    bad = _multi(2)
    bad.slot[1] = 0
    assert _calls(b, bad, None, addr)[2:] == [E_SHAPE] * 2
    bad = _multi(2)
    bad.stride_bytes = 100
    assert _calls(b, bad, None, addr)[2:] == [E_ALIGN] * 2


def _sizes(layout):
    return [layout[i + 1] - layout[i] for i in range(L.NPARAM)]


@pytest.mark.parametrize("C_", list(range(1, 17)))
@pytest.mark.parametrize("K_", [2, 3, 16])
def test_param_layout_is_the_attention_layout_without_the_gate(C_, K_):
    att, cg = L.param_layout(C_, K_), L.param_layout(C_, K_, "cnn_gru")
    sa, sc = _sizes(att), _sizes(cg)
    assert sc[L.P_GATE_W1] == sc[L.P_GATE_W2] == 0
    assert sc[L.P_CONV1_W:] == sa[L.P_CONV1_W:]
    gate = sa[L.P_GATE_W1] + sa[L.P_GATE_W2]
    assert all(cg[i] == att[i] - gate for i in range(L.P_CONV1_W, L.NPARAM + 1))
    if C_ < 4:
        assert cg == att
    bad = (C.c_int64 * (L.NPARAM + 1))()
    assert L.lib().msig_cg_param_layout(0, K_, bad) == E_SHAPE
    assert L.lib().msig_cg_param_layout(C_, K_, None) == E_NULL


@pytest.mark.parametrize("C_,cfg", [(3, (32, 64, 2)), (6, (32, 64, 2)), (12, (32, 32, 1)), (6, (32, 32, 1))])
def test_state_dict_is_the_attention_models_without_the_gate(C_, cfg):
    kw = dict(cnn_out_channels=cfg[0], gru_hidden_size=cfg[1], gru_num_layers=cfg[2])
    att = CnnGruAttentionModel(C_, 3, **kw).state_dict()
    cg = CnnGruModel(C_, 3, **kw).state_dict()
    expect = [(k, tuple(v.shape), v.dtype) for k, v in att.items() if k not in L.GATE_KEYS]
    assert [(k, tuple(v.shape), v.dtype) for k, v in cg.items()] == expect
    assert [k for _, k in L.param_keys("cnn_gru")] == [k for k in L.PARAM_KEYS if k not in L.GATE_KEYS]
    shapes = L.param_shapes(C_, 3, "cnn_gru")
    assert shapes[L.P_GATE_W1] == (0, C_) and shapes[L.P_GATE_W2] == (C_, 0)
    assert CnnGruModel.kind == "cnn_gru" and not hasattr(CnnGruModel(C_, 3, **kw), "channel_attention")


def test_other_configurations_raise():
    with pytest.raises(NotImplementedError):
        CnnGruModel(6, 2, gru_hidden_size=128)
    with pytest.raises(ValueError):
        CnnGruModel(17, 2)


def _stock(C_, K_, H, layers, dropout=0.5):
    """The baseline as a stock torch.nn graph, built in the attention model's order minus ChannelAttention."""
    cnn = nn.Sequential(nn.Conv1d(C_, 16, kernel_size=7, stride=2, padding=3, bias=False), nn.BatchNorm1d(16), nn.ReLU(),
                        nn.MaxPool1d(kernel_size=3, stride=2, padding=1),
                        nn.Conv1d(16, 32, kernel_size=5, stride=2, padding=2, bias=False), nn.BatchNorm1d(32), nn.ReLU(),
                        nn.MaxPool1d(kernel_size=3, stride=2, padding=1))
    gru = nn.GRU(32, H, layers, batch_first=True, bidirectional=True, dropout=dropout if layers > 1 else 0.0)
    cls = nn.Sequential(nn.Linear(2 * H, 64), nn.ReLU(), nn.Dropout(dropout), nn.Linear(64, K_))
    return {**{f"cnn_encoder.{k}": v for k, v in cnn.state_dict().items()}, **{f"gru.{k}": v for k, v in gru.state_dict().items()},
            **{f"classifier.{k}": v for k, v in cls.state_dict().items()}}


@pytest.mark.parametrize("C_,K_,H,layers", [(6, 2, 64, 2), (3, 3, 64, 2), (12, 2, 32, 1)])
def test_initial_weights_equal_a_stock_graph(C_, K_, H, layers):
    torch.manual_seed(1234)
    model = CnnGruModel(C_, K_, gru_hidden_size=H, gru_num_layers=layers).state_dict()
    torch.manual_seed(1234)
    ref = _stock(C_, K_, H, layers)
    assert list(model) == list(ref)
    for k in ref:
        assert torch.equal(model[k], ref[k]), k


def _prep(model, store, bs=64):
    ld = lambda b: SimpleNamespace(batch_size=b, store=store)
    return {"model": model, "loaders": (ld(bs), ld(bs), ld(bs)),
            "config": {"trainer": {"epochs": 10, "early_stopping": {"patience": 5}}}}


def test_lockstep_compatible_rejects_mixed_kinds():
    store = torch.zeros(4, 6, 8)
    att, cg = CnnGruAttentionModel(6, 2), [CnnGruModel(6, 2) for _ in range(2)]
    assert lockstep_compatible([_prep(m, store) for m in cg])
    assert not lockstep_compatible([_prep(cg[0], store), _prep(att, store)])
    assert not lockstep_compatible([_prep(att, store), _prep(cg[1], store)])
    e1, e2 = CnnGruModel(6, 2, gru_hidden_size=32, gru_num_layers=1), CnnGruAttentionModel(6, 2, gru_hidden_size=32, gru_num_layers=1)
    assert lockstep_compatible([_prep(e1, store)])
    assert not lockstep_compatible([_prep(e1, store), _prep(e2, store)])


def test_model_flag_parsing():
    with pytest.raises(SystemExit):
        M.main(["--model", "resnet", "--synthetic", "/nonexistent"])
    with pytest.raises(SystemExit):
        M.main(["--model", "cnn_gru_attention", "cnn_gru", "--hierarchical", "--synthetic", "/nonexistent"])
    assert M.MODEL_PARAMS["cnn_gru"] == M.MODEL_PARAMS["cnn_gru_attention"]
    assert M.MODEL_CLASSES["cnn_gru"] is CnnGruModel and M.MODEL_CLASSES["cnn_gru_attention"] is CnnGruAttentionModel
    assert M.model_kind({}) == "cnn_gru_attention" and M.model_kind({"model": "cnn_gru"}) == "cnn_gru"
    m = M.make_model({"model": "cnn_gru"}, 4, 2, M.MODEL_PARAMS["cnn_gru"])
    assert isinstance(m, CnnGruModel)


def test_two_kinds_with_hierarchical_is_rejected_with_a_message(capsys):
    with pytest.raises(SystemExit):
        M.main(["--model", "cnn_gru", "cnn_gru_attention", "--hierarchical"])
    assert "--hierarchical takes one --model kind" in capsys.readouterr().err


def test_summary_names_the_kind(tmp_path):
    cfg = dict(M.default_cfg(), model="cnn_gru", model_params=dict(M.MODEL_PARAMS["cnn_gru"]))
    res = [{"subject": "S2", "accuracy": 0.5, "f1_score": 0.4}]
    text = M.write_summary(tmp_path, res, cfg, 1.0, 1).read_text(encoding="utf-8")
    assert "MODEL_TO_USE: cnn_gru\n" in text and "MODEL_PARAMS: {'cnn_gru': {" in text
    text = M.write_summary(tmp_path, res, M.default_cfg(), 1.0, 1).read_text(encoding="utf-8")
    assert "MODEL_TO_USE: cnn_gru_attention\n" in text and "MODEL_PARAMS: {'cnn_gru_attention': {" in text


def test_comparison_writer_numbers(tmp_path):
    a = [{"subject": "S2", "accuracy": 0.9, "f1_score": 0.8}, {"subject": "S3", "accuracy": 0.6, "f1_score": 0.7},
         {"subject": "S4", "accuracy": 0.5, "f1_score": 0.5}]
    b = [{"subject": "S3", "accuracy": 0.7, "f1_score": 0.6}, {"subject": "S2", "accuracy": 0.8, "f1_score": 0.8},
         {"subject": "S4", "accuracy": 0.5, "f1_score": 0.25}]
    kinds = ["cnn_gru_attention", "cnn_gru"]
    cmp = M.comparison({"": {"cnn_gru_attention": a, "cnn_gru": b}, "ecg_only": {"cnn_gru_attention": a[:1], "cnn_gru": b[1:2]}},
                       kinds, {"": ["c1", "c2", "c3"], "ecg_only": ["c1"] * 5})
    st = cmp["sets"][""]
    assert st["gate_hidden_width"] == 0 and cmp["sets"]["ecg_only"]["gate_hidden_width"] == 1
    assert [f["subject"] for f in st["folds"]] == ["S2", "S3", "S4"]
    np.testing.assert_allclose([f["difference"]["accuracy"] for f in st["folds"]], [0.1, -0.1, 0.0], atol=1e-12)
    np.testing.assert_allclose([f["difference"]["f1_score"] for f in st["folds"]], [0.0, 0.1, 0.25], atol=1e-12)
    sm = st["summary"]
    np.testing.assert_allclose(sm["cnn_gru_attention"]["accuracy"]["mean"], np.mean([0.9, 0.6, 0.5]))
    np.testing.assert_allclose(sm["cnn_gru"]["accuracy"]["std"], np.std([0.8, 0.7, 0.5]))
    np.testing.assert_allclose(sm["difference"]["f1_score"]["mean"], np.mean([0.0, 0.1, 0.25]))
    np.testing.assert_allclose(sm["difference"]["accuracy"]["std"], np.std([0.1, -0.1, 0.0]), atol=1e-12)
    assert st["attention_wins"] == {"accuracy": 1, "f1_score": 2} and st["n_folds"] == 3
    assert st["baseline_wins"] == {"accuracy": 1, "f1_score": 0} and st["ties"] == {"accuracy": 1, "f1_score": 1}
    assert cmp["sets"]["ecg_only"]["n_folds"] == 1
    path = M.write_comparison(tmp_path, cmp)
    assert json.loads((tmp_path / "comparison.json").read_text()) == json.loads(json.dumps(cmp))
    text = path.read_text(encoding="utf-8")
    assert "gate hidden width C // 4 = 0" in text and "the gate is the constant 0.5" in text
    assert "accuracy: cnn_gru_attention wins 1 of 3 folds, cnn_gru wins 1, ties 1" in text
    assert "weighted F1: cnn_gru_attention wins 2 of 3 folds, cnn_gru wins 0, ties 1" in text


def test_comparison_is_attention_minus_baseline_whatever_the_order_of_kinds():
    """--model cnn_gru cnn_gru_attention: the difference, the win counts and the order of the kinds stay the attention model's."""
    a = [{"subject": "S2", "accuracy": 0.9, "f1_score": 0.8}, {"subject": "S3", "accuracy": 0.9, "f1_score": 0.7}]
    b = [{"subject": "S2", "accuracy": 0.5, "f1_score": 0.8}, {"subject": "S3", "accuracy": 0.5, "f1_score": 0.9}]
    res = {"": {"cnn_gru_attention": a, "cnn_gru": b}}
    fwd = M.comparison(res, ["cnn_gru_attention", "cnn_gru"], {"": ["c1"] * 6})
    rev = M.comparison(res, ["cnn_gru", "cnn_gru_attention"], {"": ["c1"] * 6})
    assert fwd == rev
    st = rev["sets"][""]
    assert rev["kinds"] == ["cnn_gru_attention", "cnn_gru"] and rev["difference"] == "cnn_gru_attention - cnn_gru"
    assert st["attention_wins"] == {"accuracy": 2, "f1_score": 0} and st["baseline_wins"] == {"accuracy": 0, "f1_score": 1}
    assert st["ties"] == {"accuracy": 0, "f1_score": 1}
    np.testing.assert_allclose([f["difference"]["accuracy"] for f in st["folds"]], [0.4, 0.4], atol=1e-12)


def test_the_shared_base_class_is_not_a_model():
    from multimodalsignal_amd.models import _MsigModel
    with pytest.raises(TypeError):
        _MsigModel(6, 2)
