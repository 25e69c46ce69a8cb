"""Entropy-minimisation adaptation (include/msig_tt.h), the C ABI checked without a GPU: every call of the header is exported beside
the unchanged headers, the binding's mirror matches the build, and each rejection happens before the first launch (descriptors with
fake, aligned, never dereferenced pointers, as in test_input_grad_cabi.py — the stand-alone calls have no later check to stop at, so
every call of theirs made here carries a defect; the step stops at a workspace one byte short)."""
import ctypes as C
import re
from pathlib import Path

import pytest

from multimodalsignal_amd import _lib as L
from multimodalsignal_amd import tta

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "msig_tt.h").read_text()
E_NULL, E_SHAPE, E_ALIGN, E_WORKSPACE, E_FORM = -1, -2, -3, -4, -5
B, CH, T, K = 8, 6, 512, 2
f = C.c_float
NAN, INF = float("nan"), float("inf")

_keep_alive = (C.c_char * 8192)()
A = (C.addressof(_keep_alive) + 255) // 256 * 256          # an aligned address nothing ever reads


def test_header_calls_are_exported_and_the_other_headers_are_unchanged():
    names = sorted(set(re.findall(r"\b(msig_tt_[a-z0-9_]+)\s*\(", HEADER)))
    assert names == ["msig_tt_abi_version", "msig_tt_adam", "msig_tt_adam_multi", "msig_tt_objective", "msig_tt_objective_multi",
                     "msig_tt_step", "msig_tt_step_multi", "msig_tt_struct_bytes"]
    lib = tta.lib()
    for n in names:
        assert getattr(lib, n) is not None
    assert lib.msig_tt_abi_version() == int(re.search(r"#define MSIG_TT_ABI_VERSION (\d+)", HEADER).group(1)) == tta.TT_ABI_VERSION == 1
    assert '#include "msig_ft.h"' in HEADER
    assert len(set(re.findall(r"\b(msig_\w+)\(", (ROOT / "include" / "msig.h").read_text()))) == 26
    assert (lib.msig_abi_version(), lib.msig_ft_abi_version(), lib.msig_ab_abi_version(), lib.msig_cg_abi_version()) == (5, 1, 1, 1)
    assert (lib.msig_struct_bytes(0), lib.msig_struct_bytes(1)) == (C.sizeof(L.Batch), C.sizeof(L.Multi))


def test_mirror_matches_the_header():
    body = re.search(r"typedef struct msig_tt \{(.*?)\} msig_tt;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n for decl in body.split(";") for n in re.findall(r"[\s*,](\w+)(?:\[\w+\])?\s*(?=,|$)", decl.strip())]
    assert fields == [n for n, _ in tta.Tt._fields_]
    assert tta.lib().msig_tt_struct_bytes() == C.sizeof(tta.Tt) == 56


def _multi(n=1, stride=1 << 20, **kw):
    m = L.Multi()
    m.n, m.stride_bytes = n, stride
    for i in range(max(n, 0) if n <= L.MAX_FOLDS else 0):
        m.slot[i] = i
    for k, v in kw.items():
        for i, x in enumerate(v):
            getattr(m, k)[i] = x
    return m


# ---- msig_tt_objective -------------------------------------------------------------------------------------------------------------
def test_objective_rejections():
    lib = tta.lib()
    call = lambda lg=A, Bv=B, Kv=K, div=0.0, dl=A + 256, st=None: lib.msig_tt_objective(lg, Bv, Kv, f(div), dl, st, None)
    assert call(lg=None) == E_NULL and call(dl=None) == E_NULL
    for Bv in (0, -1, tta.TT_MAX_BATCH + 1):                 # B = 0 and B = 2049
        assert call(Bv=Bv) == E_SHAPE
    for Kv in (1, 17):
        assert call(Kv=Kv) == E_SHAPE
    for div in (-0.5, NAN, INF):
        assert call(div=div) == E_SHAPE
    assert call(lg=A + 2) == E_ALIGN and call(dl=A + 2) == E_ALIGN and call(st=A + 4) == E_ALIGN
    assert call(lg=None, Bv=0) == E_NULL and call(Bv=0, lg=A + 2) == E_SHAPE          # the header's order: NULL, shape, alignment
    mcall = lambda m, **kw: lib.msig_tt_objective_multi(kw.get("lg", A), kw.get("Bv", B), K, f(0.0), A + 256, None, m, None)
    assert mcall(None) == E_NULL
    assert mcall(C.byref(_multi(0))) == E_SHAPE and mcall(C.byref(_multi(17))) == E_SHAPE
    assert mcall(C.byref(_multi(2, stride=100))) == E_ALIGN
    dup = _multi(2)
    dup.slot[1] = 0
    assert mcall(C.byref(dup)) == E_SHAPE
    assert mcall(C.byref(_multi(2)), Bv=2049) == E_SHAPE and mcall(C.byref(_multi(2)), lg=None) == E_NULL


# ---- msig_tt_adam --------------------------------------------------------------------------------------------------------------------
def _adam(p=A, g=A, m=A, v=A, Cv=CH, Kv=K, kind=0, select=tta.SELECT_BN, step=1):
    return tta.lib().msig_tt_adam(p, g, m, v, Cv, Kv, kind, select, f(1e-3), f(0.9), f(0.999), f(1e-8), f(0.0), step, None)


def test_adam_rejections():
    for name in ("p", "g", "m", "v"):
        assert _adam(**{name: None}) == E_NULL
    assert _adam(select=0) == E_SHAPE                                        # a bad select: nothing chosen
    assert _adam(select=1 << tta.NPARAM) == E_SHAPE                          # a bit at MSIG_NPARAM
    assert _adam(select=(1 << 31) | tta.SELECT_BN) == E_SHAPE                # or above
    assert _adam(kind=2) == E_SHAPE and _adam(kind=-1) == E_SHAPE
    assert _adam(Cv=0) == E_SHAPE and _adam(Cv=17) == E_SHAPE and _adam(Kv=1) == E_SHAPE and _adam(Kv=17) == E_SHAPE
    assert _adam(step=0) == E_SHAPE
    for name in ("p", "g", "m", "v"):
        assert _adam(**{name: A + 8}) == E_ALIGN
    assert _adam(p=None, select=0) == E_NULL and _adam(p=A + 8, select=0) == E_SHAPE
    lib = tta.lib()
    mcall = lambda m, select=tta.SELECT_BN, step=1: lib.msig_tt_adam_multi(A, A, A, A, CH, K, 0, select, f(0.9), f(0.999), f(1e-8), f(0.0),
                                                                          step, m, None)
    assert mcall(None) == E_NULL
    assert mcall(C.byref(_multi(0))) == E_SHAPE and mcall(C.byref(_multi(2, stride=128))) == E_ALIGN
    assert mcall(C.byref(_multi(2)), select=0) == E_SHAPE
    assert mcall(C.byref(_multi(2, step=[1, -1]))) == E_SHAPE and mcall(C.byref(_multi(2)), step=0) == E_SHAPE


# ---- msig_tt_step ----------------------------------------------------------------------------------------------------------------------
def _batch(training=0, keep=1, ws_bytes=None, dx=None, Bv=B):
    b = L.Batch()
    b.shape = L.Shape(Bv, CH, T, K)
    b.training, b.keep_for_backward = training, keep
    for name in ("x", "labels", "params", "grads", "bn_state", "bn_count", "ws"):
        setattr(b, name, A)
    b.ws_bytes = L.workspace_layout(Bv if Bv >= 1 else B, CH, T, K, True)[-1] - 1 if ws_bytes is None else ws_bytes      # one byte short: the last check
    b.dx = dx
    b.gru_layers = 2
    return b


def _tt(**kw):
    t = tta.Tt()
    t.kind, t.select, t.diversity = kw.get("kind", 0), kw.get("select", tta.SELECT_BN), kw.get("diversity", 0.0)
    t.beta1, t.beta2, t.eps, t.weight_decay = 0.9, 0.999, 1e-8, 0.0
    t.exp_avg, t.exp_avg_sq, t.stats = kw.get("exp_avg", A), kw.get("exp_avg_sq", A), kw.get("stats", None)
    return t


def _step(b, t, step=1):
    return tta.lib().msig_tt_step(C.byref(b) if b is not None else None, C.byref(t) if t is not None else None, f(1e-3), step, None)


def _step_multi(b, m, t, step=1):
    return tta.lib().msig_tt_step_multi(C.byref(b) if b is not None else None, C.byref(m) if m is not None else None,
                                        C.byref(t) if t is not None else None, step, None)


def test_step_passes_every_check_up_to_the_workspace():
    """The well-formed descriptor stops only at the workspace, which is one byte short of the TRAINING layout on purpose: whatever a case
    below returns instead is that case's own rejection, before any launch."""
    assert _step(_batch(), _tt()) == E_WORKSPACE
    assert _step(_batch(), _tt(kind=1, select=tta.SELECT_ALL, diversity=1.0, stats=A)) == E_WORKSPACE
    assert _step_multi(_batch(), _multi(3), _tt()) == E_WORKSPACE
    assert _step(_batch(ws_bytes=L.workspace_layout(B, CH, T, K, False)[-1]), _tt()) == E_WORKSPACE      # the evaluation layout does not do
    b = _batch()
    b.labels = None
    assert _step(b, _tt()) == E_WORKSPACE                                    # labels are optional


def test_step_rejections():
    assert _step(None, _tt()) == E_NULL and _step(_batch(), None) == E_NULL
    assert _step(_batch(training=1), _tt()) == E_SHAPE                       # training = 1
    assert _step(_batch(training=1, keep=0), _tt()) == E_SHAPE
    assert _step(_batch(keep=0), _tt()) == E_SHAPE                           # keep_for_backward = 0
    assert _step(_batch(dx=A), _tt()) == E_SHAPE                             # a non-NULL dx
    for t in (_tt(kind=2), _tt(select=0), _tt(select=1 << tta.NPARAM), _tt(diversity=-1.0), _tt(diversity=NAN), _tt(diversity=INF)):
        assert _step(_batch(), t) == E_SHAPE
    assert _step(_batch(Bv=tta.TT_MAX_BATCH + 1), _tt()) == E_SHAPE          # B = 2049
    assert _step(_batch(Bv=0), _tt()) == E_SHAPE                             # B = 0
    assert _step(_batch(), _tt(exp_avg=None)) == E_NULL and _step(_batch(), _tt(exp_avg_sq=None)) == E_NULL
    assert _step(_batch(), _tt(), step=0) == E_SHAPE
    assert _step(_batch(), _tt(exp_avg=A + 8)) == E_ALIGN and _step(_batch(), _tt(exp_avg_sq=A + 4)) == E_ALIGN
    assert _step(_batch(), _tt(stats=A + 4)) == E_ALIGN
    # msig_batch's own checks come last
    for name in ("x", "params", "grads", "bn_state", "bn_count", "ws"):
        b = _batch()
        setattr(b, name, None)
        assert _step(b, _tt()) == E_NULL, name
    b = _batch()
    b.grads = A + 8
    assert _step(b, _tt()) == E_ALIGN
    b = _batch()
    b.bwd_form = 99
    assert _step(b, _tt()) == E_FORM
    b = _batch()
    b.gru_layers = 3
    assert _step(b, _tt()) == E_SHAPE
    # the header's order: flags before the selection, the selection before the moments, the moments before msig_batch's own
    assert _step(_batch(training=1), _tt(select=0, exp_avg=None)) == E_SHAPE
    assert _step(_batch(), _tt(select=0, exp_avg=None)) == E_SHAPE
    b = _batch()
    b.x = None
    assert _step(b, _tt(exp_avg=A + 8)) == E_ALIGN


def test_step_multi_rejections():
    assert _step_multi(None, _multi(2), _tt()) == E_NULL and _step_multi(_batch(), None, _tt()) == E_NULL
    assert _step_multi(_batch(), _multi(2), None) == E_NULL
    assert _step_multi(_batch(), _multi(0), _tt()) == E_SHAPE and _step_multi(_batch(), _multi(17), _tt()) == E_SHAPE
    assert _step_multi(_batch(), _multi(2, stride=100), _tt()) == E_ALIGN
    dup = _multi(2)
    dup.slot[1] = 0
    assert _step_multi(_batch(), dup, _tt()) == E_SHAPE
    for b in (_batch(training=1), _batch(keep=0), _batch(dx=A), _batch(Bv=2049)):
        assert _step_multi(b, _multi(2), _tt()) == E_SHAPE
    assert _step_multi(_batch(), _multi(2), _tt(select=0)) == E_SHAPE
    assert _step_multi(_batch(), _multi(2, step=[3, -1]), _tt()) == E_SHAPE and _step_multi(_batch(), _multi(2), _tt(), step=0) == E_SHAPE
    b = _batch(ws_bytes=1 << 40)                                             # the forms are the last check of all: nothing else is wrong here
    b.fwd_form = L.FWD_FORMS["fp32"] + 1                                     # a form a fold batch cannot run
    assert _step_multi(b, _multi(2), _tt()) == E_FORM


def test_existing_backward_calls_are_unchanged():
    """msig_backward / msig_cg_backward still check as they did (their helper gained a fold context)."""
    lib = L.lib()
    b = _batch()
    assert lib.msig_backward(C.byref(b), None, None) == E_WORKSPACE and lib.msig_cg_backward(C.byref(b), None, None) == E_WORKSPACE
    assert lib.msig_backward(None, None, None) == E_NULL and lib.msig_cg_backward(None, None, None) == E_NULL
    assert lib.msig_backward(C.byref(_batch(keep=0)), None, None) == E_SHAPE
