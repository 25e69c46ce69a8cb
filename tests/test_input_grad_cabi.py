"""C-ABI contract of input gradients and eval-mode backward (ABI 5: msig_batch.keep_for_backward, msig_batch.dx), checked
without a GPU: every rejection happens before the first launch, so descriptors with fake (aligned, never dereferenced)
pointers are enough."""
import ctypes as C

import pytest

from multimodalsignal_amd import _lib as L

E_SHAPE, E_ALIGN, E_WORKSPACE = -2, -3, -4
B, CH, T, K = 8, 6, 512, 2


def test_abi_5_mirror():
    lib = L.lib()
    assert lib.msig_abi_version() == L.ABI_VERSION == 5
    assert [f[0] for f in L.Batch._fields_][-2:] == ["keep_for_backward", "dx"]
    assert lib.msig_struct_bytes(0) == C.sizeof(L.Batch)


def _batch(training, keep, ws_bytes, dx=None):
    keep_alive = (C.c_char * 8192)()
    addr = (C.addressof(keep_alive) + 255) // 256 * 256
    b = L.Batch()
    b.shape = L.Shape(B, CH, T, K)
    b.training, b.keep_for_backward = training, keep
    for f in ("x", "labels", "params", "grads", "bn_state", "bn_count", "ws"):
        setattr(b, f, addr)
    b.ws_bytes = ws_bytes
    b.dx = dx
    b.gru_layers = 2
    return b, keep_alive, addr


def _bytes(training):
    return L.workspace_layout(B, CH, T, K, training)[-1]


def test_keep_for_backward_sizes_the_workspace_like_training():
    """An eval forward kept for a backward needs the training layout (stashes, pooling decisions): one byte less than the training
    workspace is MSIG_E_WORKSPACE for the forward and for the backward; without the flag the evaluation layout suffices."""
    lib = L.lib()
    assert _bytes(True) > _bytes(False)
    b, _k, _ = _batch(0, 1, _bytes(True) - 1)
    assert lib.msig_forward(C.byref(b), None) == E_WORKSPACE
    assert lib.msig_backward(C.byref(b), None, None) == E_WORKSPACE
    assert lib.msig_frontend_bwd(C.byref(b), None) == E_WORKSPACE
    b, _k, _ = _batch(0, 0, _bytes(False) - 1)
    assert lib.msig_forward(C.byref(b), None) == E_WORKSPACE


def test_backward_needs_training_or_keep_for_backward():
    lib = L.lib()
    b, _k, _ = _batch(0, 0, 1 << 40)
    for rc in (lib.msig_backward(C.byref(b), None, None), lib.msig_head_ce_bwd(C.byref(b), None, None),
               lib.msig_gru_bwd(C.byref(b), None), lib.msig_frontend_bwd(C.byref(b), None)):
        assert rc == E_SHAPE


def test_dx_is_rejected_where_it_is_not_supported():
    """dx in the fused train step, in fold batches and with a forward that keeps nothing: MSIG_E_SHAPE before any launch.  The
    same descriptors without dx fail only at the workspace check (too small on purpose), so the rejection is dx's."""
    lib = L.lib()
    f = C.c_float
    small = _bytes(True) - 1
    m = L.Multi()
    m.n, m.stride_bytes = 1, 1 << 20
    for with_dx, want in ((False, E_WORKSPACE), (True, E_SHAPE)):
        b, _k, addr = _batch(1, 0, small)
        if with_dx:
            b.dx = addr
        assert lib.msig_train_step(C.byref(b), addr, addr, f(1e-3), f(0.9), f(0.999), f(1e-8), f(0.0), 1, None) == want
        assert lib.msig_train_step_multi(C.byref(b), C.byref(m), addr, addr, f(0.9), f(0.999), f(1e-8), f(0.0), 1, None) == want
        assert lib.msig_forward_multi(C.byref(b), C.byref(m), None) == want
        b, _k, addr = _batch(0, 0, _bytes(False) - 1)
        if with_dx:
            b.dx = addr
        for rc in (lib.msig_forward(C.byref(b), None), lib.msig_frontend_fwd(C.byref(b), None)):
            assert rc == (E_SHAPE if with_dx else E_WORKSPACE)


def test_dx_must_be_16_byte_aligned():
    lib = L.lib()
    b, _k, addr = _batch(0, 1, _bytes(True) - 1)
    b.dx = addr + 8
    assert lib.msig_backward(C.byref(b), None, None) == E_ALIGN
    b.dx = addr + 16
    assert lib.msig_backward(C.byref(b), None, None) == E_WORKSPACE


def test_engine_workspace_modes():
    """runtime.Engine keeps three workspace buffers apart: training, evaluation, and evaluation kept for a backward (training
    layout)."""
    from multimodalsignal_amd.runtime import Engine
    assert Engine._mode(True) is True and Engine._mode(True, True) is True
    assert Engine._mode(False) is False
    assert Engine._mode(False, True) == Engine.EVAL_KEEP
    assert len({Engine._mode(True), Engine._mode(False), Engine._mode(False, True)}) == 3
