"""Gradient-norm clipping (include/msig_gc.h), the C ABI checked without a GPU: every call of the header is exported beside the
unchanged headers, the binding's mirror matches the build, the clip state has a size for every supported shape, and each rejection
happens before the first launch (descriptors with fake, aligned, never dereferenced pointers, as in test_class_weights_host.py)."""
import ctypes as C
import math
import re
from pathlib import Path

import pytest

from multimodalsignal_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
GC_HEADER = (ROOT / "include" / "msig_gc.h").read_text()
E_NULL, E_SHAPE, E_ALIGN, E_WORKSPACE, E_FORM = -1, -2, -3, -4, -5
B, CH, T, K = 8, 6, 512, 2
f = C.c_float


def test_msig_gc_header_calls_are_exported_and_the_other_headers_are_unchanged():
    names = sorted(set(re.findall(r"\b(msig_gc_\w+)\(", GC_HEADER)))
    assert names == ["msig_gc_abi_version", "msig_gc_state_bytes", "msig_gc_struct_bytes", "msig_gc_train_step", "msig_gc_train_step_multi"]
    lib = L.lib()
    for n in names:
        assert getattr(lib, n) is not None
    assert lib.msig_gc_abi_version() == int(re.search(r"#define MSIG_GC_ABI_VERSION (\d+)", GC_HEADER).group(1)) == L.GC_ABI_VERSION
    assert lib.msig_gc_struct_bytes() == C.sizeof(L.GcClip)
    assert len(set(re.findall(r"\b(msig_\w+)\(", (ROOT / "include" / "msig.h").read_text()))) == 26
    assert (lib.msig_abi_version(), lib.msig_cw_abi_version(), lib.msig_cg_abi_version(), lib.msig_ft_abi_version()) == (5, 1, 1, 1)


def test_mirror_matches_the_header():
    body = re.search(r"typedef struct msig_gc_clip \{(.*?)\} msig_gc_clip;", GC_HEADER, re.S).group(1)
    fields = re.findall(r"(\w+)(?:\[\w+\])?;", body)
    assert fields == [n for n, _ in L.GcClip._fields_]
    enum = re.search(r"enum \{ (MSIG_GC_SUM.*?) \};", GC_HEADER).group(1)
    vals = {k.strip(): int(v) for k, v in (item.split("=") for item in enum.split(","))}
    assert vals == {"MSIG_GC_SUM": L.GC_SUM, "MSIG_GC_MAX": L.GC_MAX, "MSIG_GC_CLIPPED": L.GC_CLIPPED, "MSIG_GC_LAST": L.GC_LAST,
                    "MSIG_GC_NSTAT": L.GC_NSTAT}
    for name, kind in L.GC_KINDS.items():
        tag = "ATTENTION" if name == "cnn_gru_attention" else "CNN_GRU"
        assert int(re.search(rf"#define MSIG_GC_KIND_{tag} (\d+)", GC_HEADER).group(1)) == kind


@pytest.mark.parametrize("kind", list(L.GC_KINDS))
@pytest.mark.parametrize("K_", [2, 3])
@pytest.mark.parametrize("C_", [1, 3, 6, 16])
def test_state_size(C_, K_, kind):
    """Positive, 8-byte aligned, and room for the statistics plus one partial per 32-column block of every parameter tensor."""
    n = L.gc_state_bytes(C_, K_, kind)
    assert n > 0 and n % 8 == 0
    layout, shapes = L.param_layout(C_, K_, kind), L.param_shapes(C_, K_, kind)
    blocks = sum(-(-math.prod(sh) // 32) for sh in shapes if math.prod(sh))
    assert n >= 8 * (L.GC_NSTAT + blocks + 1)          # + 1: gru.bias_hh is reduced as two jobs
    assert n < 8 * (L.GC_NSTAT + layout[-1] // 32 + 64)


def test_state_size_rejects_bad_arguments():
    lib = L.lib()
    assert lib.msig_gc_state_bytes(6, 2, 2) == E_SHAPE and lib.msig_gc_state_bytes(6, 2, -1) == E_SHAPE
    assert lib.msig_gc_state_bytes(0, 2, 0) == E_SHAPE and lib.msig_gc_state_bytes(6, 1, 0) == E_SHAPE
    assert lib.msig_gc_state_bytes(L.MAX_C + 1, 2, 1) == E_SHAPE


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


def _clip(addr, kind=0, max_norm=(1.0, 2.0), state="addr", state_bytes=None, cw=None):
    g = L.GcClip()
    g.kind, g.class_weight = kind, cw
    g.state = addr if state == "addr" else state
    g.state_bytes = L.gc_state_bytes(CH, K, "cnn_gru_attention") if state_bytes is None else state_bytes
    for i, v in enumerate(max_norm):
        g.max_norm[i] = v
    return g


def _calls(b, m, g, addr):
    lib = L.lib()
    gp = C.byref(g) if g is not None else None
    return [lib.msig_gc_train_step(C.byref(b), gp, addr, addr, f(1e-3), f(0.9), f(0.999), f(1e-8), f(0.0), 1, None),
            lib.msig_gc_train_step_multi(C.byref(b), C.byref(m), gp, addr, addr, f(0.9), f(0.999), f(1e-8), f(0.0), 1, None)]


def _small():
    """A workspace one byte short: with valid clip arguments every call stops at MSIG_E_WORKSPACE — the last check before a launch —
    so any other code seen below is the clip arguments' own, returned before anything could have been launched."""
    return L.workspace_layout(B, CH, T, K, True)[-1] - 1


def test_valid_clip_arguments_reach_the_counterparts_checks():
    b, _k, addr = _batch(_small())
    assert _calls(b, _multi(), _clip(addr), addr) == [E_WORKSPACE] * 2
    assert _calls(b, _multi(), _clip(addr, kind=1, max_norm=(float("inf"), 1e-30)), addr) == [E_WORKSPACE] * 2
    assert _calls(b, _multi(), _clip(addr, cw=addr + 4), addr) == [E_WORKSPACE] * 2


@pytest.mark.parametrize("bad", [float("nan"), 0.0, -1.0, -float("inf")])
def test_bad_max_norm_is_a_shape_error(bad):
    b, _k, addr = _batch(_small())
    assert _calls(b, _multi(), _clip(addr, max_norm=(bad, bad)), addr) == [E_SHAPE] * 2
    # the second fold's value counts in the fold batch only
    assert _calls(b, _multi(), _clip(addr, max_norm=(1.0, bad)), addr) == [E_WORKSPACE, E_SHAPE]


def test_null_misaligned_and_small_state():
    b, _k, addr = _batch(_small())
    m = _multi()
    assert _calls(b, m, None, addr) == [E_NULL] * 2
    assert _calls(b, m, _clip(addr, state=None), addr) == [E_NULL] * 2
    assert _calls(b, m, _clip(addr, state=addr + 4), addr) == [E_ALIGN] * 2
    assert _calls(b, m, _clip(addr, state=addr + 8), addr) == [E_WORKSPACE] * 2          # 8-byte alignment is enough
    need = L.gc_state_bytes(CH, K, "cnn_gru_attention")
    big = L.workspace_layout(B, CH, T, K, True)[-1]
    b2, _k2, addr2 = _batch(big)                       # a sufficient workspace: MSIG_E_WORKSPACE below is the clip state's
    b2.fwd_form = 99                                   # ... and with a state that is large enough the call goes on to the form check
    assert _calls(b2, m, _clip(addr2, state_bytes=need - 8), addr2) == [E_WORKSPACE] * 2
    assert _calls(b2, m, _clip(addr2, state_bytes=need), addr2) == [E_FORM] * 2
    assert _calls(b, m, _clip(addr, kind=2), addr) == [E_SHAPE] * 2
    assert _calls(b, m, _clip(addr, cw=addr + 2), addr) == [E_ALIGN] * 2


def test_counterpart_checks_hold():
    lib = L.lib()
    b, _k, addr = _batch(_small())
    g = _clip(addr)
    assert lib.msig_gc_train_step(None, C.byref(g), addr, addr, f(1e-3), f(0.9), f(0.999), f(1e-8), f(0.0), 1, None) == E_NULL
    assert lib.msig_gc_train_step_multi(None, C.byref(_multi()), C.byref(g), addr, addr, f(0.9), f(0.999), f(1e-8), f(0.0), 1, None) == E_NULL
    for kw in (dict(K=1), dict(K=L.MAX_K + 1), dict(B=0)):
        bb, _kk, a = _batch(1, **kw)
        assert _calls(bb, _multi(), _clip(a), a) == [E_SHAPE] * 2, kw
    bb, _kk, a = _batch(_small(), training=0)
    assert _calls(bb, _multi(), _clip(a), a) == [E_SHAPE] * 2
    bb, _kk, a = _batch(_small())
    bb.labels = None
    assert _calls(bb, _multi(), _clip(a), a) == [E_NULL] * 2
    bb, _kk, a = _batch(_small())
    bb.fwd_form = 99
    assert _calls(bb, _multi(), _clip(a), a) == [E_FORM] * 2
    bb, _kk, a = _batch(_small())
    assert _calls(bb, _multi(), _clip(a), 0)[0] == E_NULL                 # no Adam moments
    bad = _multi(2)
    bad.slot[1] = 0
    assert _calls(bb, bad, _clip(a), a)[1] == E_SHAPE
    bad = _multi(2)
    bad.stride_bytes = 100
    assert _calls(bb, bad, _clip(a), a)[1] == E_ALIGN
