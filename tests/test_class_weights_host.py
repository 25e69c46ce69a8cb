"""Class-weighted CrossEntropy (include/msig_cw.h), checked without a GPU: the new header's calls are exported beside an unchanged
msig.h, every rejection happens before the first launch (descriptors with fake, aligned, never dereferenced pointers, as in
test_input_grad_cabi.py), the binding refuses bad vectors on the host, and 'balanced' is sklearn's compute_class_weight."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from multimodalsignal_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
CW_HEADER = (ROOT / "include" / "msig_cw.h").read_text()
E_NULL, E_SHAPE, E_ALIGN, E_WORKSPACE, E_FORM = -1, -2, -3, -4, -5
B, CH, T, K = 8, 6, 512, 2
f = C.c_float


def test_msig_cw_header_calls_are_exported_and_msig_h_is_unchanged():
    names = sorted(set(re.findall(r"\b(msig_cw_\w+)\(", CW_HEADER)))
    assert names == ["msig_cw_abi_version", "msig_cw_forward", "msig_cw_forward_multi", "msig_cw_train_step", "msig_cw_train_step_multi"]
    lib = L.lib()
    for n in names:
        assert getattr(lib, n) is not None
    assert lib.msig_cw_abi_version() == int(re.search(r"#define MSIG_CW_ABI_VERSION (\d+)", CW_HEADER).group(1)) == L.CW_ABI_VERSION
    header = (ROOT / "include" / "msig.h").read_text()
    assert len(set(re.findall(r"\b(msig_\w+)\(", header))) == 26
    assert lib.msig_abi_version() == L.ABI_VERSION == 5


def _batch(training, ws_bytes, **kw):
    keep_alive = (C.c_char * 8192)()
    addr = (C.addressof(keep_alive) + 255) // 256 * 256
    b = L.Batch()
    b.shape = L.Shape(kw.get("B", B), CH, T, kw.get("K", K))
    b.training = training
    for name in ("x", "labels", "params", "grads", "bn_state", "bn_count", "ws"):
        setattr(b, name, addr)
    b.ws_bytes = ws_bytes
    b.gru_layers = 2
    return b, keep_alive, addr


def _calls(b, m, cw, addr):
    """Every msig_cw.h launcher on one descriptor."""
    lib = L.lib()
    return [lib.msig_cw_forward(C.byref(b), cw, None),
            lib.msig_cw_train_step(C.byref(b), cw, addr, addr, f(1e-3), f(0.9), f(0.999), f(1e-8), f(0.0), 1, None),
            lib.msig_cw_forward_multi(C.byref(b), C.byref(m), cw, None),
            lib.msig_cw_train_step_multi(C.byref(b), C.byref(m), cw, addr, addr, f(0.9), f(0.999), f(1e-8), f(0.0), 1, None)]


def _multi(n=2):
    m = L.Multi()
    m.n, m.stride_bytes = n, 1 << 20
    for i in range(n):
        m.slot[i] = i
    return m


def test_misaligned_weight_pointer_is_rejected_first():
    """A weight pointer that is not 4-byte aligned: MSIG_E_ALIGN from every call.  The descriptor's workspace is one byte short, so
    with an aligned (or NULL) pointer the same calls stop at MSIG_E_WORKSPACE: the rejection is the weight's, before any launch."""
    small = L.workspace_layout(B, CH, T, K, True)[-1] - 1
    b, _k, addr = _batch(1, small)
    m = _multi()
    assert _calls(b, m, addr + 2, addr) == [E_ALIGN] * 4
    assert _calls(b, m, addr + 4, addr) == [E_WORKSPACE] * 4          # 4-byte alignment is enough
    assert _calls(b, m, None, addr) == [E_WORKSPACE] * 4


def test_counterpart_checks_hold_with_weights():
    """The msig.h counterparts' checks, with a valid weight pointer: NULL descriptor, bad shape, bad kernel form, no labels in a
    train step, a bad fold batch — each rejected with the counterpart's code, nothing launched."""
    lib = L.lib()
    small = L.workspace_layout(B, CH, T, K, True)[-1] - 1
    _, _k0, addr0 = _batch(1, small)
    assert lib.msig_cw_forward(None, addr0, None) == E_NULL
    assert lib.msig_cw_train_step(None, addr0, addr0, addr0, f(1e-3), f(0.9), f(0.999), f(1e-8), f(0.0), 1, None) == E_NULL
    assert lib.msig_cw_forward_multi(None, C.byref(_multi()), addr0, None) == E_NULL
    for kw in (dict(K=1), dict(K=L.MAX_K + 1), dict(B=0)):
        b, _k, addr = _batch(1, 1, **kw)
        assert _calls(b, _multi(), addr, addr) == [E_SHAPE] * 4, kw
    b, _k, addr = _batch(1, small)                                       # (the form check comes before the workspace check)
    b.fwd_form = 99
    assert _calls(b, _multi(), addr, addr) == [E_FORM] * 4
    b, _k, addr = _batch(1, small)
    b.labels = None
    assert lib.msig_cw_train_step(C.byref(b), addr, addr, addr, f(1e-3), f(0.9), f(0.999), f(1e-8), f(0.0), 1, None) == E_NULL
    b, _k, addr = _batch(1, small)
    bad = _multi(1)
    bad.n = 0
    assert _calls(b, bad, addr, addr)[2:] == [E_SHAPE] * 2
    bad = _multi(2)
    bad.slot[1] = 0                                                      # two folds in one arena
    assert _calls(b, bad, addr, addr)[2:] == [E_SHAPE] * 2
    bad = _multi(2)
    bad.stride_bytes = 100
    assert _calls(b, bad, addr, addr)[2:] == [E_ALIGN] * 2


@pytest.mark.parametrize("bad", [[1.0], [1.0, 2.0, 3.0], [1.0, -0.5], [1.0, float("nan")], [float("inf"), 1.0], "balanced", [[1.0, 2.0]]])
def test_binding_rejects_bad_vectors_on_the_host(bad):
    with pytest.raises(ValueError):
        L.check_class_weight(bad, 2)


def test_binding_accepts_k_non_negative_values():
    np.testing.assert_array_equal(L.check_class_weight([0.0, 2.5, 1], 3), [0.0, 2.5, 1.0])


def test_balanced_equals_sklearn():
    from sklearn.utils.class_weight import compute_class_weight
    from multimodalsignal_amd.trainer import balanced_class_weights
    rs = np.random.RandomState(0)
    for trial in range(40):
        K_ = int(rs.randint(2, 7))
        n = int(rs.randint(K_, 400))
        y = np.concatenate([np.arange(K_), rs.choice(K_, size=n - K_, p=rs.dirichlet(np.ones(K_)))])
        rs.shuffle(y)
        want = compute_class_weight("balanced", classes=np.arange(K_), y=y)
        np.testing.assert_allclose(balanced_class_weights(y, K_), want, rtol=1e-15, atol=0)
        # the reference's own call (trainer.py:85-89: classes = np.unique(y)) gives the same vector when every class occurs
        np.testing.assert_allclose(balanced_class_weights(y, K_), compute_class_weight("balanced", classes=np.unique(y), y=y), rtol=1e-15)


def test_balanced_names_a_missing_class():
    from multimodalsignal_amd.trainer import balanced_class_weights
    with pytest.raises(ValueError, match=r"\[1\]"):
        balanced_class_weights(np.array([0, 0, 2, 2]), 3)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        balanced_class_weights(np.array([2, 2]), 3)


def test_trainer_setting_is_checked():
    from multimodalsignal_amd.trainer import class_weight_setting
    assert class_weight_setting(None, 2) is None and class_weight_setting("balanced", 2) == "balanced"
    np.testing.assert_array_equal(class_weight_setting((0.3, 2.5), 2), [0.3, 2.5])
    for bad in ("uniform", "none", [1.0], [-1.0, 1.0]):
        with pytest.raises(ValueError):
            class_weight_setting(bad, 2)


def test_cv_summary_names_the_setting_only_when_set(tmp_path):
    from multimodalsignal_amd import main as M
    res = [{"subject": "S2", "accuracy": 0.5, "f1_score": 0.5}]
    base = M.default_cfg()
    assert base["class_weights"] == M.CLASS_WEIGHTS == "none"
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    ta = M.write_summary(tmp_path / "a", res, base, 1.0, 1).read_text(encoding="utf-8")
    tb = M.write_summary(tmp_path / "b", res, dict(base, class_weights="balanced"), 1.0, 1).read_text(encoding="utf-8")
    assert "CLASS_WEIGHTS" not in ta
    assert "CLASS_WEIGHTS: balanced\n" in tb and tb.replace("CLASS_WEIGHTS: balanced\n", "") == ta
    assert M.trainer_class_weights(base) is None and M.trainer_class_weights(dict(base, class_weights="balanced")) == "balanced"
