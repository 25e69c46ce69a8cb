"""Subject-adversarial training (include/msig_da.h), the C ABI checked without a GPU: every call of the header is exported beside
the unchanged headers, the binding's mirror matches the build, msig_da_param_floats, and each rejection happens before the first
launch (descriptors with fake, aligned, never dereferenced pointers, as in test_grad_clip_cabi.py)."""
import ctypes as C
import re
from pathlib import Path

import pytest

from multimodalsignal_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
DA_HEADER = (ROOT / "include" / "msig_da.h").read_text()
E_NULL, E_SHAPE, E_ALIGN, E_WORKSPACE, E_FORM = -1, -2, -3, -4, -5
B, CH, T, K = 8, 6, 512, 2
f = C.c_float


def test_msig_da_header_calls_are_exported_and_the_other_headers_are_unchanged():
    names = sorted(set(re.findall(r"\b(msig_da_\w+)\(", DA_HEADER)))
    assert names == ["msig_da_abi_version", "msig_da_param_floats", "msig_da_step", "msig_da_step_multi", "msig_da_struct_bytes",
                     "msig_da_train_step", "msig_da_train_step_multi"]
    lib = L.lib()
    for n in names:
        assert getattr(lib, n) is not None
    assert lib.msig_da_abi_version() == int(re.search(r"#define MSIG_DA_ABI_VERSION (\d+)", DA_HEADER).group(1)) == L.DA_ABI_VERSION
    assert int(re.search(r"#define MSIG_DA_MAX_BATCH (\d+)", DA_HEADER).group(1)) == L.DA_MAX_BATCH == 256
    assert len(set(re.findall(r"\b(msig_\w+)\(", (ROOT / "include" / "msig.h").read_text()))) == 26
    assert (lib.msig_abi_version(), lib.msig_cw_abi_version(), lib.msig_cg_abi_version(), lib.msig_ft_abi_version(), lib.msig_gc_abi_version(),
            lib.msig_aug_abi_version(), lib.msig_st_abi_version(), lib.msig_ab_abi_version(), lib.msig_at_abi_version(),
            lib.msig_mc_abi_version()) == (5, 1, 1, 1, 1, 1, 1, 1, 1, 1)


def test_mirror_matches_the_header():
    body = re.search(r"typedef struct msig_da \{(.*?)\} msig_da;", DA_HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n for decl in body.split(";") for n in re.findall(r"[\s*,](\w+)(?:\[\w+\])?\s*(?=,|$)", decl.strip())]
    assert fields == [n for n, _ in L.Da._fields_]
    assert L.lib().msig_da_struct_bytes() == C.sizeof(L.Da)


@pytest.mark.parametrize("S", range(2, L.MAX_K + 1))
def test_param_floats(S):
    assert L.da_param_floats(S) == 64 * 128 + 64 + S * 64 + (S + 3) // 4 * 4


def test_param_floats_rejects_a_bad_domain_count():
    for S in (-1, 0, 1, L.MAX_K + 1):
        assert L.lib().msig_da_param_floats(S) == E_SHAPE


def _addr():
    keep_alive = (C.c_char * 8192)()
    return keep_alive, (C.addressof(keep_alive) + 255) // 256 * 256


def _da(addr, n=2, **kw):
    a = L.Da()
    a.S, a.weight_decay, a.beta1, a.beta2, a.eps = kw.get("S", 4), 0.0, 0.9, 0.999, 1e-8
    for name in ("dom", "idx", "params", "exp_avg", "exp_avg_sq", "stats"):
        setattr(a, name, kw.get(name, addr))
    a.idx_row_stride, a.stride_bytes = kw.get("idx_row_stride", 64), kw.get("stride_bytes", 1 << 16)
    for i in range(n):
        getattr(a, "lambda")[i] = kw.get("lam_rev", (0.5, 0.5))[i]
        a.lr[i] = kw.get("lr", (1e-3, 1e-3))[i]
        a.step[i] = kw.get("step", (1, 1))[i]
    return a


def _multi(n=2):
    m = L.Multi()
    m.n, m.stride_bytes = n, 1 << 20
    for i in range(n):
        m.slot[i] = i
    return m


def _batch(ws_bytes, addr, **kw):
    b = L.Batch()
    b.shape = L.Shape(kw.get("B", B), CH, T, K)
    b.training = 1
    for name in ("x", "labels", "params", "grads", "bn_state", "bn_count", "ws"):
        setattr(b, name, addr)
    b.ws_bytes = ws_bytes
    b.gru_layers = 2
    return b


def _small(Bv=B):
    """A workspace one byte short: with valid arguments the train steps stop at MSIG_E_WORKSPACE, the last check before a launch."""
    return L.workspace_layout(Bv, CH, T, K, True)[-1] - 1


def _train_calls(a, addr, Bv=B, lams=(1.0, 1.0)):
    lib = L.lib()
    b, m = _batch(_small(Bv), addr, B=Bv), _multi()
    s = L.make_st("cnn_gru_attention", 0.0, None, None, list(lams))
    ap = C.byref(a) if a is not None else None
    return [lib.msig_da_train_step(C.byref(b), C.byref(s), ap, addr, addr, f(1e-3), f(0.9), f(0.999), f(1e-8), f(0.0), 1, None),
            lib.msig_da_train_step_multi(C.byref(b), C.byref(m), C.byref(s), ap, addr, addr, f(0.9), f(0.999), f(1e-8), f(0.0), 1, None)]


def _step_calls(a, addr, Bv=B, feat="addr", dfeat="addr", lam=1.0, single=True):
    """The discriminator's step alone: [single, fold batch].  It has no later check to stop at — valid arguments would launch on the
    fake pointers — so every call made here carries a defect; single=False leaves out the single call where the defect is the fold
    batch's alone."""
    lib = L.lib()
    ap = C.byref(a) if a is not None else None
    ft, dft = (addr if feat == "addr" else feat), (addr if dfeat == "addr" else dfeat)
    return ([lib.msig_da_step(ap, ft, dft, Bv, f(lam), None)] if single else []) + [
        lib.msig_da_step_multi(ap, C.byref(_multi()), ft, dft, Bv, (C.c_float * L.MAX_FOLDS)(lam, lam), None)]


def _all(a, addr):
    return _train_calls(a, addr) + _step_calls(a, addr)


def test_valid_arguments_reach_the_counterparts_checks_and_a_null_adversary_is_the_counterpart():
    _k, addr = _addr()
    assert _train_calls(_da(addr), addr) == [E_WORKSPACE] * 2
    assert _train_calls(_da(addr, idx=None, stats=None), addr) == [E_WORKSPACE] * 2          # both optional
    assert _train_calls(_da(addr, S=2), addr) == [E_WORKSPACE] * 2
    assert _train_calls(_da(addr, S=L.MAX_K, lam_rev=(0.0, 7.0), lr=(0.0, 1.0)), addr) == [E_WORKSPACE] * 2
    assert _train_calls(_da(addr, stats=addr + 8, idx=addr + 8, dom=addr + 4), addr) == [E_WORKSPACE] * 2
    assert _train_calls(_da(addr, idx_row_stride=256), addr, Bv=256) == [E_WORKSPACE] * 2
    assert _train_calls(None, addr) == [E_WORKSPACE] * 2                                       # NULL msig_da: msig_st_train_step[_multi] itself
    assert _train_calls(None, addr, Bv=4096) == [E_WORKSPACE] * 2                              # ... whose batch size has no such limit


def test_null_pointers():
    _k, addr = _addr()
    assert _step_calls(None, addr) == [E_NULL] * 2
    for name in ("dom", "params", "exp_avg", "exp_avg_sq"):
        assert _all(_da(addr, **{name: None}), addr) == [E_NULL] * 4, name
    assert _step_calls(_da(addr), addr, feat=None) == [E_NULL] * 2
    assert _step_calls(_da(addr), addr, dfeat=None) == [E_NULL] * 2
    lib = L.lib()
    assert lib.msig_da_step_multi(C.byref(_da(addr)), None, addr, addr, B, (C.c_float * L.MAX_FOLDS)(1.0, 1.0), None) == E_NULL
    assert lib.msig_da_step_multi(C.byref(_da(addr)), C.byref(_multi()), addr, addr, B, None, None) == E_NULL
    b, s = _batch(_small(), addr), L.make_st("cnn_gru_attention", 0.0, None, None, [1.0])
    assert lib.msig_da_train_step(C.byref(b), None, C.byref(_da(addr)), addr, addr, f(1e-3), f(0.9), f(0.999), f(1e-8), f(0.0), 1, None) == E_NULL
    assert lib.msig_da_train_step(None, C.byref(s), C.byref(_da(addr)), addr, addr, f(1e-3), f(0.9), f(0.999), f(1e-8), f(0.0), 1, None) == E_NULL


@pytest.mark.parametrize("S", [-1, 0, 1, L.MAX_K + 1])
def test_bad_domain_count_is_a_shape_error(S):
    _k, addr = _addr()
    assert _all(_da(addr, S=S), addr) == [E_SHAPE] * 4


def test_bad_batch_size_is_a_shape_error():
    _k, addr = _addr()
    assert _train_calls(_da(addr), addr, Bv=257) == [E_SHAPE] * 2
    for Bv in (0, -3, 257):
        assert _step_calls(_da(addr), addr, Bv=Bv) == [E_SHAPE] * 2
    assert _step_calls(_da(addr, idx_row_stride=B - 1), addr, single=False) == [E_SHAPE]       # the folds' rows of idx would overlap


@pytest.mark.parametrize("field,bad", [("step", 0), ("step", -4), ("lam_rev", float("nan")), ("lam_rev", -0.5), ("lr", float("nan")),
                                       ("lr", -1e-3)])
def test_bad_per_fold_values_are_shape_errors(field, bad):
    _k, addr = _addr()
    assert _all(_da(addr, **{field: (bad, bad)}), addr) == [E_SHAPE] * 4
    # the second fold's value counts in the fold batch only
    a = _da(addr, **{field: ({"step": 1, "lam_rev": 0.5, "lr": 1e-3}[field], bad)})
    assert _train_calls(a, addr) == [E_WORKSPACE, E_SHAPE] and _step_calls(a, addr, single=False) == [E_SHAPE]


@pytest.mark.parametrize("lam", [float("nan"), -0.1, 1.5])
def test_bad_mixup_weight_is_a_shape_error(lam):
    _k, addr = _addr()
    assert _step_calls(_da(addr), addr, lam=lam) == [E_SHAPE] * 2


def test_misalignment():
    _k, addr = _addr()
    for name in ("params", "exp_avg", "exp_avg_sq"):
        assert _all(_da(addr, **{name: addr + 8}), addr) == [E_ALIGN] * 4, name
    for name in ("stats", "idx"):
        assert _all(_da(addr, **{name: addr + 4}), addr) == [E_ALIGN] * 4, name
    assert _all(_da(addr, dom=addr + 2), addr) == [E_ALIGN] * 4
    assert _step_calls(_da(addr), addr, feat=addr + 8) == [E_ALIGN] * 2
    assert _step_calls(_da(addr), addr, dfeat=addr + 4) == [E_ALIGN] * 2
    for stride in (0, -256, 100, 257):
        a = _da(addr, stride_bytes=stride)                                                     # the stride counts in fold batches only
        assert _train_calls(a, addr) == [E_WORKSPACE, E_ALIGN] and _step_calls(a, addr, single=False) == [E_ALIGN], stride
