"""Soft targets (include/msig_st.h), checked without a GPU: the header's calls are exported and the binding's mirror matches the build,
every rejection happens before a launch (fake, aligned, never dereferenced pointers), `Mixup`, the configuration keys and the
command line follow the same rules, tests/st_reference.py agrees with torch's cross_entropy(label_smoothing=, weight=) in fp64, and the
lam draw is deterministic, distinct, in (0, 1] and has Beta(alpha, alpha)'s first two moments within derived bounds."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import st_reference as S
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd.mixup import Mixup

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "msig_st.h").read_text()
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
B, CH, T = 8, 6, 512
NAN = float("nan")


# ---- header, exports, mirror ------------------------------------------------------------------------------------------------
def test_header_calls_are_exported():
    names = sorted(set(re.findall(r"\b(msig_st_\w+)\(", HEADER)))
    assert names == ["msig_st_abi_version", "msig_st_forward", "msig_st_forward_multi", "msig_st_gather_windows",
                     "msig_st_gather_windows_multi", "msig_st_struct_bytes", "msig_st_train_step", "msig_st_train_step_multi"]
    lib = L.lib()
    for n in names:
        assert getattr(lib, n) is not None
    assert lib.msig_st_abi_version() == int(re.search(r"#define MSIG_ST_ABI_VERSION (\d+)", HEADER).group(1)) == L.ST_ABI_VERSION
    assert lib.msig_st_struct_bytes() == C.sizeof(L.St)
    assert int(re.search(r"#define MSIG_ST_STREAM_ID (\d+)", HEADER).group(1)) == L.ST_STREAM_ID == 4
    assert (lib.msig_abi_version(), lib.msig_cw_abi_version(), lib.msig_cg_abi_version(), lib.msig_ft_abi_version(),
            lib.msig_gc_abi_version(), lib.msig_aug_abi_version()) == (5, 1, 1, 1, 1, 1)


def test_mirror_matches_the_header():
    body = re.search(r"typedef struct msig_st \{(.*?)\} msig_st;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.findall(r"(\w+)(?:\[\w+\])?\s*$", decl.strip())[0] for decl in body.split(";") if decl.strip()]
    assert fields == [n for n, _ in L.St._fields_]
    s = L.make_st("cnn_gru", 0.1, None, None, [0.25, 1.0])
    assert (s.kind, s.smoothing, s.clip, s.lam[0], s.lam[1], s.lam[15]) == (1, np.float32(0.1), None, 0.25, 1.0, 1.0)
    g = L.GcClip()
    assert L.make_st("cnn_gru_attention", 0.0, None, g).clip == C.addressof(g)


# ---- rejections, all before a launch ----------------------------------------------------------------------------------------
def _addr():
    keep_alive = (C.c_char * 8192)()
    return keep_alive, (C.addressof(keep_alive) + 255) // 256 * 256


def _multi(n=2):
    m = L.Multi()
    m.n, m.stride_bytes = n, 1 << 20
    for i in range(n):
        m.slot[i] = i
    return m


def _step_calls(s, b=None, m="default"):
    """The four criterion calls; b = None: a NULL msig_batch, which is what they answer (MSIG_E_NULL) once msig_st's own checks pass."""
    lib = L.lib()
    sp = C.byref(s) if s is not None else None
    bp = C.byref(b) if b is not None else None
    mm = _multi() if m == "default" else m
    dummy = L.Batch()                    # the multi calls read msig_multi first, which needs a batch pointer to be non-NULL
    return [lib.msig_st_forward(bp, sp, None),
            lib.msig_st_train_step(bp, sp, None, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None),
            lib.msig_st_forward_multi(C.byref(dummy) if b is None else bp, C.byref(mm), sp, None),
            lib.msig_st_train_step_multi(C.byref(dummy) if b is None else bp, C.byref(mm), sp, None, None, 0.9, 0.999, 1e-8, 0.0, 1, None)]


def test_null_descriptor():
    assert _step_calls(None) == [E_NULL] * 4
    ok = L.make_st("cnn_gru_attention", 0.1, None, None, [0.5, 0.5])
    assert _step_calls(ok)[:2] == [E_NULL] * 2                      # its own checks pass: the counterpart's NULL msig_batch


@pytest.mark.parametrize("eps", [-0.1, 1.0, 1.5, NAN, float("inf")])
def test_bad_smoothing_is_a_shape_error(eps):
    s = L.make_st("cnn_gru_attention", 0.0, None, None, [0.5, 0.5])
    s.smoothing = eps
    assert _step_calls(s) == [E_SHAPE] * 4


@pytest.mark.parametrize("lam", [-0.1, 1.0001, NAN, float("inf")])
def test_bad_lambda_of_a_fold_of_the_launch_is_a_shape_error(lam):
    s = L.make_st("cnn_gru", 0.1, None, None, [0.5, 0.5])
    s.lam[1] = lam
    got = _step_calls(s)
    assert got[2:] == [E_SHAPE] * 2                                  # fold 1 is a fold of the two-fold launch
    assert got[:2] == [E_NULL] * 2                                   # a single model reads lam[0] alone
    s.lam[0], s.lam[1] = lam, 0.5
    assert _step_calls(s) == [E_SHAPE] * 4
    s.lam[0], s.lam[5] = 0.5, lam
    assert _step_calls(s)[:2] == [E_NULL] * 2                        # beyond the launch: not read


def test_bad_kind_and_misaligned_weights():
    s = L.make_st("cnn_gru", 0.1, None, None, [0.5, 0.5])
    for kind in (2, -1):
        s.kind = kind
        assert _step_calls(s) == [E_SHAPE] * 4
    _k, addr = _addr()
    s = L.make_st("cnn_gru", 0.1, addr + 2, None, [0.5, 0.5])
    assert _step_calls(s) == [E_ALIGN] * 4


def test_msig_multis_own_checks_come_first():
    s = L.make_st("cnn_gru", 2.0, None, None, [0.5, 0.5])
    bad = _multi(2)
    bad.slot[1] = 0
    assert _step_calls(s, m=bad)[2:] == [E_SHAPE] * 2
    bad = _multi(2)
    bad.stride_bytes = 100
    assert _step_calls(s, m=bad)[2:] == [E_ALIGN] * 2


def test_clip_checks_follow_the_soft_target_checks():
    g = L.GcClip()
    g.kind, g.max_norm[0], g.max_norm[1] = 0, 1.0, 1.0
    s = L.make_st("cnn_gru", 0.1, None, g, [0.5, 0.5])
    b = L.Batch()
    lib = L.lib()
    call = lambda: lib.msig_st_train_step(C.byref(b), C.byref(s), None, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None)
    assert call() == E_SHAPE                                         # a clip of another kind
    g.kind = 1
    assert call() == E_NULL                                          # msig_gc.h's own: no state
    g.max_norm[0] = -1.0
    assert call() == E_SHAPE
    s.smoothing = 1.0
    g.max_norm[0] = 1.0
    assert call() == E_SHAPE                                         # the soft-target checks come before the clip's


def _gather_calls(lam, addr, a=None, B_=B, C_=CH, T_=T, store="addr", idx="addr", out="addr", m="default", stride=None, n=2):
    lib = L.lib()
    pick = lambda v: addr if v == "addr" else v
    mm = _multi(n) if m == "default" else m
    lp = (C.c_float * L.MAX_FOLDS)(*lam) if lam is not None else None
    ap = C.byref(a) if a is not None else None
    return [lib.msig_st_gather_windows(pick(store), addr, pick(idx), B_, C_, T_, pick(out), addr, ap, lp, None),
            lib.msig_st_gather_windows_multi(pick(store), addr, pick(idx), B_ if stride is None else stride, B_, C_, T_, pick(out), addr,
                                             C.byref(mm) if mm is not None else None, ap, lp, None)]


def test_gather_rejections():
    _k, addr = _addr()
    assert _gather_calls(None, addr) == [E_NULL] * 2
    for which in ("store", "idx", "out"):
        assert _gather_calls([0.5, 0.5], addr, **{which: None}) == [E_NULL] * 2, which
    assert _gather_calls([0.5, 0.5], addr, m=None)[1] == E_NULL
    for lam in (-0.5, 1.5, NAN):
        assert _gather_calls([lam, 0.5], addr + 4) == [E_SHAPE] * 2          # misaligned too: lam is checked first
        assert _gather_calls([0.5, lam], addr + 4) == [E_ALIGN, E_SHAPE]     # the single call reads lam[0] alone
    for kw in (dict(T_=510), dict(T_=0), dict(C_=0), dict(C_=L.MAX_C + 1), dict(B_=0), dict(B_=65536)):
        assert _gather_calls([0.5, 0.5], addr + 4, **kw) == [E_SHAPE] * 2, kw
    assert _gather_calls([0.5, 0.5], addr, stride=B - 1)[1] == E_SHAPE
    assert _gather_calls([0.5, 0.5], addr, store=addr + 8) == [E_ALIGN] * 2
    assert _gather_calls([1.0, 1.0], addr, out=addr + 4) == [E_ALIGN] * 2     # all lam at 1: the plain gather's launch, after the same checks
    bad_aug = L.Aug()
    bad_aug.scale_sigma = -1.0
    assert _gather_calls([0.5, 0.5], addr, a=bad_aug) == [E_SHAPE] * 2
    bad = _multi(2)
    bad.slot[1] = 0
    assert _gather_calls([NAN, 0.5], addr, m=bad)[1] == E_SHAPE
    bad.slot[1], bad.stride_bytes = 1, 100
    assert _gather_calls([NAN, 0.5], addr, m=bad)[1] == E_ALIGN              # msig_multi's own checks come first


# ---- Mixup, configuration keys, command line -----------------------------------------------------------------------------------
def test_mixup_value_object():
    m = Mixup(0.2)
    assert m.alpha == 0.2 and m == Mixup(0.2) and m != Mixup(0.4) and hash(m) == hash(Mixup(0.2)) and repr(m) == "Mixup(0.2)"
    assert Mixup.coerce(None) is None and Mixup.coerce(m) is m and Mixup.coerce(1) == Mixup(1.0)
    with pytest.raises(AttributeError):
        m.alpha = 1.0
    for bad in (0, 0.0, -0.2, NAN, float("inf"), "0.2", None, True):
        with pytest.raises(ValueError):
            Mixup(bad)


def test_host_checks_of_smoothing_and_lambda():
    assert L.check_label_smoothing(None) == 0.0 and L.check_label_smoothing(0) == 0.0 and L.check_label_smoothing(0.1) == 0.1
    for bad in (-0.1, 1.0, 1.0 - 1e-12, NAN, "0.1", True):
        with pytest.raises(ValueError):
            L.check_label_smoothing(bad)
    assert L.check_mix_lambda(None) == 1.0 and L.check_mix_lambda(1) == 1.0 and L.check_mix_lambda(0.0) == 0.0
    assert L.check_mix_lambda(0.3) == float(np.float32(0.3))
    for bad in (-0.1, 1.1, NAN, "0.5", False):
        with pytest.raises(ValueError):
            L.check_mix_lambda(bad)


def test_trainer_setting_and_configuration_keys():
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.trainer import label_smoothing_setting
    assert label_smoothing_setting(None) is None and label_smoothing_setting(0.1) == 0.1 and label_smoothing_setting(0) == 0.0
    with pytest.raises(ValueError):
        label_smoothing_setting(1.0)
    cfg = M.default_cfg()
    assert "label_smoothing" not in M.trainer_config(cfg, 0)["trainer"] and M.soft_targets_line(cfg) is None
    cfg.update(label_smoothing=0.1, mixup=0.2)
    assert M.trainer_config(cfg, 0)["trainer"]["label_smoothing"] == 0.1
    assert M.soft_targets_line(cfg) == "SOFT TARGETS: label_smoothing=0.1 mixup_alpha=0.2\n"
    assert M.soft_targets_line(dict(mixup=Mixup(1.0))) == "SOFT TARGETS: mixup_alpha=1\n"
    with pytest.raises(ValueError):
        M.trainer_config(dict(cfg, label_smoothing=-1.0), 0)


def test_flags_become_configuration_keys():
    from multimodalsignal_amd import main as M
    ap = M.build_parser()
    cfg = M.build_cfg(M.parse_args(ap, ["--synthetic", "x"]), ["cnn_gru_attention"])
    assert "label_smoothing" not in cfg and "mixup" not in cfg
    cfg = M.build_cfg(M.parse_args(ap, ["--synthetic", "x", "--label-smoothing", "0.1", "--mixup", "0.2"]), ["cnn_gru_attention"])
    assert cfg["label_smoothing"] == 0.1 and cfg["mixup"] == Mixup(0.2)
    for bad in (["--label-smoothing", "1.0"], ["--label-smoothing", "-0.5"], ["--mixup", "0"], ["--mixup", "-1"],
                ["--mixup", "0.2", "--samples", "510"]):
        with pytest.raises(SystemExit):
            M.parse_args(ap, ["--synthetic", "x", *bad])


# ---- the formulas against torch, fp64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("lam", [1.0, 0.3, 0.0])
@pytest.mark.parametrize("eps", [0.0, 0.1, 0.5])
def test_reference_formulas_equal_torch(eps, lam, K, weighted):
    rs = np.random.RandomState(K + int(10 * eps) + int(100 * lam))
    for Bn in (1, 5, 64):
        z = torch.tensor(rs.randn(Bn, K) * 2.0, dtype=torch.float64, requires_grad=True)
        y = torch.tensor(rs.randint(0, K, size=Bn), dtype=torch.int64)
        w = torch.tensor(rs.rand(K) * 3.0 + 0.1, dtype=torch.float64) if weighted else None
        want = lam * F.cross_entropy(z, y, weight=w, label_smoothing=eps) + (1.0 - lam) * F.cross_entropy(z, y.flip(0), weight=w, label_smoothing=eps)
        want.backward()
        got_l, got_d = S.loss_and_dlogits(z.detach().numpy(), y.numpy(), eps, lam, None if w is None else w.numpy())
        assert abs(got_l - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
        assert np.abs(got_d - z.grad.numpy()).max() <= 1e-12


def test_mix_restatement_basics():
    rs = np.random.RandomState(0)
    store = rs.randn(7, 2, 8).astype(np.float32)
    idx = np.array([3, 0, 6, 6, 1])
    a = store[idx]
    assert S.mix(store, idx, 1.0) is not None and np.array_equal(S.mix(store, idx, 1.0).view(np.int32), a.view(np.int32))
    got = S.mix(store, idx, 0.25)
    want = np.float32(0.25) * a + np.float32(0.75) * a[::-1]
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.array_equal(got[2], np.float32(0.25) * a[2] + np.float32(0.75) * a[2])        # the middle row pairs with itself


# ---- the lam draw ----------------------------------------------------------------------------------------------------------------
def test_lambda_draw_is_a_pure_function_in_the_half_open_interval():
    m = Mixup(0.2)
    a = [m.lam(7, s) for s in range(1, 200)]
    assert a == [m.lam(7, s) for s in range(1, 200)] == m.lams(7, range(1, 200))
    assert len(set(a)) > 190                                                  # distinct across steps (fp32 values; ties only at the ends)
    assert len({m.lam(seed, 1) for seed in range(100)}) > 95                  # and across seeds
    assert a != [Mixup(0.4).lam(7, s) for s in range(1, 200)]
    assert all(0.0 < v <= 1.0 and float(np.float32(v)) == v for v in a)
    assert m.lam(2 ** 63 + 5, 2 ** 40) == m.lam(2 ** 63 + 5, 2 ** 40)


@pytest.mark.parametrize("alpha", [0.2, 1.0])
def test_lambda_draw_has_betas_moments(alpha):
    """N = 20 000 draws of Beta(a, a): mean 1/2, variance v = 1 / (4 (2a + 1)).  The standard error of the sample mean is sqrt(v / N);
    that of the sample variance is sqrt((m4 - v^2) / N) with the fourth central moment m4 = v^2 * 3 (2a + 1) / (2a + 3) (Beta's
    kurtosis, symmetric case).  Both must lie within 6 standard errors (DESIGN.md section 17 records the observed values)."""
    N = 20000
    x = np.array(Mixup(alpha).lams(12345, range(1, N + 1)), dtype=np.float64)
    assert x.min() > 0.0 and x.max() <= 1.0
    v = 1.0 / (4.0 * (2.0 * alpha + 1.0))
    m4 = v * v * 3.0 * (2.0 * alpha + 1.0) / (2.0 * alpha + 3.0)
    se_mean, se_var = math.sqrt(v / N), math.sqrt((m4 - v * v) / N)
    mean, var = x.mean(), x.var()
    print(f"alpha={alpha}: mean {mean:.5f} (0.5 +- {6 * se_mean:.5f}), var {var:.5f} ({v:.5f} +- {6 * se_var:.5f})")
    assert abs(mean - 0.5) <= 6.0 * se_mean
    assert abs(var - v) <= 6.0 * se_var
