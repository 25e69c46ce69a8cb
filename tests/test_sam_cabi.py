"""Sharpness-aware minimisation (include/msig_sam.h), the C ABI checked without a GPU: every call of the header is exported, the
binding's mirror matches the build, the state has a size for every supported shape, and each rejection happens before the first
launch (descriptors with fake, aligned, never dereferenced pointers, as in test_grad_clip_cabi.py)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import sam_reference as R
from multimodalsignal_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "msig_sam.h").read_text()
E_NULL, E_SHAPE, E_ALIGN, E_WORKSPACE, E_FORM = -1, -2, -3, -4, -5
B, CH, T, K = 8, 6, 512, 2
f = C.c_float


def test_header_calls_are_exported_and_the_mirror_matches():
    names = sorted(set(re.findall(r"\b(msig_sam_\w+)\(", HEADER)))
    assert names == ["msig_sam_abi_version", "msig_sam_perturb", "msig_sam_restore", "msig_sam_state_bytes", "msig_sam_struct_bytes",
                     "msig_sam_train_step", "msig_sam_train_step_multi"]
    lib = L.lib()
    for n in names:
        assert getattr(lib, n) is not None
    assert lib.msig_sam_abi_version() == int(re.search(r"#define MSIG_SAM_ABI_VERSION (\d+)", HEADER).group(1)) == L.SAM_ABI_VERSION
    assert lib.msig_sam_struct_bytes() == C.sizeof(L.Sam)
    body = re.search(r"typedef struct msig_sam \{(.*?)\} msig_sam;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+);", body) == [n for n, _ in L.Sam._fields_]
    enum = re.sub(r"/\*.*?\*/", "", re.search(r"enum \{ (MSIG_SAM_NORM_SUM.*?) \};", HEADER, re.S).group(1), flags=re.S)
    vals, at = {}, 0
    for item in (i.strip() for i in enum.split(",")):
        name, _, v = (s.strip() for s in item.partition("="))
        at = int(v) if v else at
        vals[name], at = at, at + 1
    assert vals == {"MSIG_SAM_NORM_SUM": L.SAM_NORM_SUM, "MSIG_SAM_NORM_MAX": L.SAM_NORM_MAX, "MSIG_SAM_NORM_LAST": L.SAM_NORM_LAST,
                    "MSIG_SAM_SHARP_SUM": L.SAM_SHARP_SUM, "MSIG_SAM_SHARP_LAST": L.SAM_SHARP_LAST, "MSIG_SAM_STEPS": L.SAM_STEPS,
                    "MSIG_SAM_NSTAT": L.SAM_NSTAT}
    # the headers beside it are what they were
    assert (lib.msig_abi_version(), lib.msig_gc_abi_version(), lib.msig_st_abi_version(), lib.msig_kd_abi_version()) == (5, 1, 1, 1)


@pytest.mark.parametrize("kind", list(L.GC_KINDS))
def test_state_size_is_a_multiple_of_8_monotone_and_holds_what_the_header_lists(kind):
    sizes = np.array([[L.sam_state_bytes(c, k, kind) for k in range(2, L.MAX_K + 1)] for c in range(1, L.MAX_C + 1)])
    assert (sizes > 0).all() and (sizes % 8 == 0).all()
    assert (np.diff(sizes, axis=0) > 0).all() and (np.diff(sizes, axis=1) >= 0).all() and (sizes[:, -1] > sizes[:, 0]).all()
    for c, k in ((2, 2), (6, 3), (16, 16)):
        n_flat = L.param_layout(c, k, kind)[-1]
        # statistics, at least one partial sum, the parameter backup, 96 BatchNorm floats, two counters, three loss floats
        assert L.sam_state_bytes(c, k, kind) >= 8 * L.SAM_NSTAT + 8 + 4 * n_flat + 4 * 96 + 16 + 12


def test_state_size_rejects_bad_arguments():
    lib = L.lib()
    assert lib.msig_sam_state_bytes(6, 2, 2) == E_SHAPE and lib.msig_sam_state_bytes(6, 2, -1) == E_SHAPE
    assert lib.msig_sam_state_bytes(0, 2, 0) == E_SHAPE and lib.msig_sam_state_bytes(6, 1, 0) == E_SHAPE
    assert lib.msig_sam_state_bytes(L.MAX_C + 1, 2, 1) == E_SHAPE and lib.msig_sam_state_bytes(6, L.MAX_K + 1, 1) == E_SHAPE


def _batch(ws_bytes, **kw):
    keep_alive = (C.c_char * 8192)()
    addr = (C.addressof(keep_alive) + 255) // 256 * 256
    b = L.Batch()
    b.shape = L.Shape(kw.get("B", B), CH, T, kw.get("K", K))
    b.training = kw.get("training", 1)
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


def _sam(addr, kind=0, adaptive=0, rho=0.05, eta=0.01, state="addr", state_bytes=None):
    s = L.Sam()
    s.kind, s.adaptive, s.rho, s.eta = kind, adaptive, rho, eta
    s.state = addr if state == "addr" else state
    s.state_bytes = L.sam_state_bytes(CH, K, "cnn_gru_attention") if state_bytes is None else state_bytes
    return s


def _calls(b, m, s, addr, st_kind=0, with_st=True):
    lib = L.lib()
    sp = C.byref(s) if s is not None else None
    sd = L.make_st("cnn_gru_attention" if st_kind == 0 else "cnn_gru", 0.0)
    stp = C.byref(sd) if with_st else None
    return [lib.msig_sam_train_step(C.byref(b), stp, None, sp, addr, addr, f(1e-3), f(0.9), f(0.999), f(1e-8), f(0.0), 1, None),
            lib.msig_sam_train_step_multi(C.byref(b), C.byref(m), stp, None, sp, addr, addr, f(0.9), f(0.999), f(1e-8), f(0.0), 1, None)]


def _small():
    """A workspace one byte short: with valid SAM arguments every train-step call stops at MSIG_E_WORKSPACE — the last check before a
    launch — so any other code seen below is the SAM arguments' own, returned before anything could have been launched."""
    return L.workspace_layout(B, CH, T, K, True)[-1] - 1


def test_valid_arguments_reach_the_counterparts_checks():
    b, _k, addr = _batch(_small())
    for s in (_sam(addr), _sam(addr, adaptive=1, eta=0.0), _sam(addr, rho=0.0), _sam(addr, state=addr + 8), None):
        assert _calls(b, _multi(), s, addr) == [E_WORKSPACE] * 2           # NULL and rho = 0: msig_kd_train_step[_multi] and its checks
    assert _calls(b, _multi(), _sam(addr, kind=1, state_bytes=L.sam_state_bytes(CH, K, "cnn_gru")), addr, st_kind=1) == [E_WORKSPACE] * 2


@pytest.mark.parametrize("kw", [dict(kind=2), dict(kind=-1), dict(kind=1), dict(adaptive=2), dict(adaptive=-1), dict(rho=float("nan")),
                                dict(rho=-0.05), dict(rho=-float("inf")), dict(eta=float("nan")), dict(eta=-1e-3)])
def test_shape_errors(kw):
    """kind=1 against an msig_st of kind 0: the kinds differ."""
    b, _k, addr = _batch(_small())
    assert _calls(b, _multi(), _sam(addr, **kw), addr) == [E_SHAPE] * 2
    if "kind" not in kw or kw["kind"] != 1:
        lib, s = L.lib(), _sam(addr, **kw)
        assert lib.msig_sam_perturb(addr, addr, addr, addr, addr, CH, K, C.byref(s), None) == E_SHAPE
        assert lib.msig_sam_restore(addr, addr, addr, addr, B, CH, K, C.byref(s), None) == E_SHAPE


def test_null_misaligned_and_small_state():
    b, _k, addr = _batch(_small())
    m, lib = _multi(), L.lib()
    need = L.sam_state_bytes(CH, K, "cnn_gru_attention")
    assert _calls(b, m, _sam(addr), addr, with_st=False) == [E_NULL] * 2               # a msig_sam needs its msig_st
    for s, want in ((_sam(addr, state=None), E_NULL), (_sam(addr, state=addr + 4), E_ALIGN), (_sam(addr, state_bytes=need - 8), E_WORKSPACE),
                    (_sam(addr, state_bytes=0), E_WORKSPACE)):
        assert _calls(b, m, s, addr) == [want] * 2
        assert lib.msig_sam_perturb(addr, addr, addr, addr, addr, CH, K, C.byref(s), None) == want
        assert lib.msig_sam_restore(addr, addr, addr, addr, B, CH, K, C.byref(s), None) == want
    big = L.workspace_layout(B, CH, T, K, True)[-1]
    b2, _k2, addr2 = _batch(big)                       # a sufficient workspace and state: the call goes on to the form check
    b2.fwd_form = 99
    assert _calls(b2, m, _sam(addr2, state_bytes=need), addr2) == [E_FORM] * 2
    # msig_multi's own checks come first
    bad = _multi(2)
    bad.slot[1] = 0
    assert _calls(b, bad, _sam(addr, kind=2), addr)[1] == E_SHAPE
    bad = _multi(2)
    bad.stride_bytes = 100
    assert _calls(b, bad, _sam(addr, kind=2), addr)[1] == E_ALIGN


def test_stand_alone_calls_check_their_own_pointers_and_shapes():
    _b, _k, addr = _batch(1)
    lib, s = L.lib(), _sam(addr)
    sp = C.byref(s)
    assert lib.msig_sam_perturb(addr, addr, addr, addr, addr, CH, K, None, None) == E_NULL
    assert lib.msig_sam_restore(addr, addr, addr, addr, B, CH, K, None, None) == E_NULL
    for i in range(5):
        args = [addr] * 5
        args[i] = None
        assert lib.msig_sam_perturb(*args, CH, K, sp, None) == E_NULL, i
    for i in range(4):
        args = [addr] * 4
        args[i] = None
        assert lib.msig_sam_restore(*args, B, CH, K, sp, None) == E_NULL, i
    for c, k in ((0, 2), (L.MAX_C + 1, 2), (6, 1), (6, L.MAX_K + 1)):
        assert lib.msig_sam_perturb(addr, addr, addr, addr, addr, c, k, sp, None) == E_SHAPE
        assert lib.msig_sam_restore(addr, addr, addr, addr, B, c, k, sp, None) == E_SHAPE
    assert lib.msig_sam_restore(addr, addr, addr, addr, 0, CH, K, sp, None) == E_SHAPE
    assert lib.msig_sam_perturb(addr + 8, addr, addr, addr, addr, CH, K, sp, None) == E_ALIGN
    assert lib.msig_sam_perturb(addr, addr + 4, addr, addr, addr, CH, K, sp, None) == E_ALIGN
    assert lib.msig_sam_perturb(addr, addr, addr + 2, addr, addr, CH, K, sp, None) == E_ALIGN
    assert lib.msig_sam_perturb(addr, addr, addr, addr + 4, addr, CH, K, sp, None) == E_ALIGN
    assert lib.msig_sam_perturb(addr, addr, addr, addr, addr + 1, CH, K, sp, None) == E_ALIGN
    assert lib.msig_sam_restore(addr + 4, addr, addr, addr, B, CH, K, sp, None) == E_ALIGN
    assert lib.msig_sam_restore(addr, addr, addr + 4, addr, B, CH, K, sp, None) == E_ALIGN


# ---- the restatement itself (tests/sam_reference.py): its rounding chain against fp64, on the CPU ------------------------------------
@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("kind,c,k", [("cnn_gru_attention", 6, 2), ("cnn_gru_attention", 2, 3), ("cnn_gru", 6, 3)])
def test_reference_perturbation_has_length_rho_and_leaves_the_padding(kind, c, k, adaptive):
    table, n_flat = R.tensor_table(c, k, kind)
    mask = R.element_mask(table, n_flat)
    assert n_flat % 4 == 0 and int(mask.sum()) == sum(n for _, n in table) and not mask.all()
    rs = np.random.RandomState(c * 10 + k)
    p = np.where(mask, rs.randn(n_flat) * 0.1, 0.0).astype(np.float32)
    g = (rs.randn(n_flat) * 1e-2).astype(np.float32)
    g[~mask] = np.nan                                   # nobody writes the gradient's padding: it must not be read
    N = R.norm(p, g, mask, adaptive, 0.01)
    assert np.isfinite(N) and N > 0
    q = R.perturb(p, g, mask, N, 0.05, adaptive, 0.01)
    assert q.dtype == np.float32 and np.array_equal(q[~mask], p[~mask]) and np.isfinite(q).all()
    e = q.astype(np.float64) - p
    if adaptive:                                        # ||T^-1 e|| = rho
        e = e / (np.abs(p).astype(np.float64) + 0.01)
    assert abs(np.sqrt(np.sum(e[mask] ** 2)) - 0.05) < 1e-5
    assert np.array_equal(R.perturb(p, np.zeros_like(g), mask, 0.0, 0.05, adaptive, 0.01), p)          # a zero gradient moves nothing
    assert R.sharpness(np.float32(12.5), np.float32(12.0), 8) == 0.0625
