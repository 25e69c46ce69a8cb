"""Integrated-gradients attribution on the GPU (include/msig_at.h, multimodalsignal_amd/attribute.py): the two kernels against their
numpy restatement (tests/at_reference.py), the attributor against the composition of public pieces and against the fp64 oracle,
completeness, independence of the cut into path batches, a dummy channel, channel occlusion, the absence of side effects and the
driver's --attribute stage."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

import at_reference as R
from gpu_common import GRAD_FLOOR, K_GRAD, grad_tol, rel_err, split_named, to_t
from oracle import cnn_gru_oracle as O

pytestmark = pytest.mark.gpu

CONFIGS = {"full": dict(), "embedded": dict(gru_hidden_size=32, gru_num_layers=1)}
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "the gpu tier needs an MI355X"


def _model(C_, K, config, dropout, seed=0, kind="cnn_gru_attention"):
    from multimodalsignal_amd.models import CnnGruAttentionModel, CnnGruModel
    torch.manual_seed(seed)
    cls = CnnGruAttentionModel if kind == "cnn_gru_attention" else CnnGruModel
    return cls(C_, K, dropout=dropout, **CONFIGS[config]).to(DEV)


def _case(B, C_, K, T, seed):
    rs = np.random.RandomState(seed)
    x = (rs.randn(B, C_, T) * (0.5 + rs.rand(1, C_, 1)) + rs.randn(1, C_, 1)).astype(np.float32)
    y = rs.randint(0, K, size=(B,)).astype(np.int64)
    return torch.as_tensor(x), torch.as_tensor(y)


def _trained(C_, K, config, T=256, kind="cnn_gru_attention"):
    """A model whose BatchNorm running statistics are no longer the initial ones (two training steps): the helper of
    tests/test_input_grad_gpu.py, for either model kind."""
    m = _model(C_, K, config, 0.5, seed=7 + C_, kind=kind).train()
    opt = torch.optim.SGD(m.parameters(), lr=0.05)
    for s in range(2):
        x, y = _case(16, C_, K, T, 50 + s)
        opt.zero_grad()
        torch.nn.CrossEntropyLoss()(m(x.to(DEV)), y.to(DEV)).backward()
        opt.step()
    return m


@functools.lru_cache(maxsize=None)
def _shared_model(kind, config, C_=6, K=3):
    return _trained(C_, K, config, kind=kind).eval()


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _bases(rs, N, C_, T):
    """{kind: (device tensor or None, numpy or None)} of the four baseline kinds."""
    out = {R.BASE_ZERO: None, R.BASE_CHANNEL: rs.randn(C_).astype(np.float32), R.BASE_SHARED: rs.randn(C_, T).astype(np.float32),
           R.BASE_OWN: rs.randn(N, C_, T).astype(np.float32)}
    return {k: (None if v is None else torch.as_tensor(v).to(DEV), v) for k, v in out.items()}


# ---- 1. the path kernel alone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [256, 301])
@pytest.mark.parametrize("C_", [1, 6, 16])
def test_path_kernel_against_the_restatement(C_, T):
    from multimodalsignal_amd import _lib as L
    N, P, K, GUARD = 3, 5, 3, 1024
    rs = np.random.RandomState(100 * C_ + T)
    x = rs.randn(N, C_, T).astype(np.float32)
    coef = rs.rand(P, C_).astype(np.float32)                       # per channel, in [0, 1): covers the occlusion tables' form
    coef[0, 0], coef[P - 1, C_ - 1] = 1.0, 0.0                     # and their two exact values
    v = rs.randn(N, K).astype(np.float32)
    xd, cd, vd = torch.as_tensor(x).to(DEV), torch.as_tensor(coef).to(DEV), torch.as_tensor(v).to(DEV)
    for kind, (bd, bn) in _bases(rs, N, C_, T).items():
        n = N * P * C_ * T
        xp = torch.full((n + GUARD,), -777.0, dtype=torch.float32, device=DEV)
        dl = torch.full((N * P * K + GUARD,), -777.0, dtype=torch.float32, device=DEV)
        L.check(L.lib().msig_at_path(xd.data_ptr(), _ptr(bd), kind, cd.data_ptr(), vd.data_ptr(), N, P, C_, T, K, xp.data_ptr(), dl.data_ptr(),
                                     _stream()), "msig_at_path")
        torch.cuda.synchronize()
        got, want = xp[:n].cpu().numpy().reshape(N * P, C_, T), R.path(x, bn, kind, coef)
        assert R.within_ulps(got, want, 1), (kind, float(np.abs(got - want).max()))
        assert np.array_equal(got.reshape(N, P, C_, T)[:, 0, 0], x[:, 0])                      # coef 1: the window's own bits
        assert np.array_equal(got.reshape(N, P, C_, T)[:, P - 1, C_ - 1], R.broadcast_base(bn, kind, N, C_, T, np.float32)[:, C_ - 1])
        assert np.array_equal(dl[:N * P * K].cpu().numpy().reshape(N * P, K), R.path_dlogits(v, P))      # exactly v, row by row
        assert bool((xp[n:] == -777.0).all()) and bool((dl[N * P * K:] == -777.0).all())         # the guard bands are untouched
        # without v nothing is written to dlogits
        dl.fill_(-5.0)
        L.check(L.lib().msig_at_path(xd.data_ptr(), _ptr(bd), kind, cd.data_ptr(), None, N, P, C_, T, K, xp.data_ptr(), dl.data_ptr(), _stream()),
                "msig_at_path")
        torch.cuda.synchronize()
        assert bool((dl == -5.0).all()) and np.array_equal(xp[:n].cpu().numpy().reshape(N * P, C_, T), got)


# ---- 2. the reduce kernel alone ------------------------------------------------------------------------------------------------------
def _reduce(dx, x, base, kind, w, N, P, C_, T, bin_, with_map=True):
    from multimodalsignal_amd import _lib as L
    NB = -(-T // bin_)
    amap = torch.full((N, C_, T), -777.0, dtype=torch.float32, device=DEV) if with_map else None
    bins, chan, total = (torch.full(s, -777.0, dtype=torch.float32, device=DEV) for s in ((N, C_, NB), (N, C_), (N,)))
    scratch = torch.zeros(N * C_, dtype=torch.float64, device=DEV)
    L.check(L.lib().msig_at_reduce(dx.data_ptr(), x.data_ptr(), _ptr(base), kind, w.data_ptr(), N, P, C_, T, bin_, _ptr(amap), bins.data_ptr(),
                                   chan.data_ptr(), total.data_ptr(), scratch.data_ptr(), _stream()), "msig_at_reduce")
    torch.cuda.synchronize()
    return amap, bins, chan, total


def _check_sums(amap, bins, chan, total, bin_):
    """bins, chan and total are the fp64 sums of the returned fp32 map, rounded, to within 1 ulp."""
    rb, rc, rt = R.sums_of_map(amap, bin_)
    assert bins.shape == rb.shape and R.within_ulps(bins, rb, 1), float(np.abs(bins - rb).max())
    assert R.within_ulps(chan, rc, 1) and R.within_ulps(total, rt, 1)


@pytest.mark.parametrize("T,bins_", [(301, (64, 301, 1)), (2304, (64, 1500, 5000, 7))])
def test_reduce_kernel_against_the_restatement(T, bins_):
    """T = 301: the element-wise form, a ragged last bin of 45 samples, one bin, one sample per bin.  T = 2304: the 16-byte form over
    three tiles of 1024 positions — bins inside a tile, a bin carried across tiles, a bin wider than the window, a bin width that
    divides neither the tile nor the piece."""
    N, P, C_ = 3, 5, 6
    rs = np.random.RandomState(T)
    x, dx = rs.randn(N, C_, T).astype(np.float32), rs.randn(N * P, C_, T).astype(np.float32)
    w = (0.1 + rs.rand(P)).astype(np.float32)
    xd, dxd, wd = torch.as_tensor(x).to(DEV), torch.as_tensor(dx).to(DEV), torch.as_tensor(w).to(DEV)
    for kind, (bd, bn) in _bases(rs, N, C_, T).items():
        ref, bound = R.reduce_map(dx, x, bn, kind, w)
        for bin_ in bins_:
            amap, bins, chan, total = (t.cpu().numpy() for t in _reduce(dxd, xd, bd, kind, wd, N, P, C_, T, bin_))
            err = np.abs(amap.astype(np.float64) - ref)
            assert np.all(err <= bound), (kind, bin_, float((err - bound).max()))
            _check_sums(amap, bins, chan, total, bin_)
            _, bins0, chan0, total0 = _reduce(dxd, xd, bd, kind, wd, N, P, C_, T, bin_, with_map=False)          # map = NULL: the same bits
            assert np.array_equal(bins0.cpu().numpy(), bins) and np.array_equal(chan0.cpu().numpy(), chan) and np.array_equal(total0.cpu().numpy(), total)


def test_reduce_kernel_sums_do_not_depend_on_the_number_of_windows():
    """The same window alone and as the last of three: every output of it has the same bits (no dependence on the grid)."""
    N, P, C_, T, bin_ = 3, 4, 2, 1100, 48
    rs = np.random.RandomState(5)
    x, dx = torch.as_tensor(rs.randn(N, C_, T).astype(np.float32)).to(DEV), torch.as_tensor(rs.randn(N * P, C_, T).astype(np.float32)).to(DEV)
    w = torch.as_tensor(rs.rand(P).astype(np.float32)).to(DEV)
    full = _reduce(dx, x, None, R.BASE_ZERO, w, N, P, C_, T, bin_)
    one = _reduce(dx[2 * P:].contiguous(), x[2:].contiguous(), None, R.BASE_ZERO, w, 1, P, C_, T, bin_)
    for a, b in zip(full, one):
        assert torch.equal(a[2:], b)


# ---- 3. end to end = the composition of public pieces ---------------------------------------------------------------------------------
def _autograd_dx(m, xp, vrep):
    """dx of the path batch through the model's public autograd, 16 windows at a time."""
    out = []
    for i in range(0, xp.shape[0], 16):
        xs = xp[i:i + 16].clone().requires_grad_(True)
        (g,) = torch.autograd.grad((m(xs) * vrep[i:i + 16]).sum(), xs)
        out.append(g)
    return torch.cat(out)


def _composition(m, x, base_t, kind, v, P):
    """(reference map in fp64, element-wise tolerance of test 3) from the binding's path kernel, autograd and the restatement."""
    from multimodalsignal_amd import _lib as L
    N, C_, T = x.shape
    alpha, w = R.midpoint(P)
    coef = torch.as_tensor(R.ig_coef(P, C_).astype(np.float32)).to(DEV)
    xp = torch.empty((N * P, C_, T), dtype=torch.float32, device=DEV)
    L.check(L.lib().msig_at_path(x.data_ptr(), _ptr(base_t), kind, coef.data_ptr(), None, N, P, C_, T, v.shape[1], xp.data_ptr(), None, _stream()),
            "msig_at_path")
    dx = _autograd_dx(m, xp, v.repeat_interleave(P, dim=0)).cpu().numpy()
    bn = None if base_t is None else base_t.cpu().numpy()
    ref, bound2 = R.reduce_map(dx, x.cpu().numpy(), bn, kind, w.astype(np.float32))
    d = np.abs(x.cpu().numpy().astype(np.float64) - R.broadcast_base(bn, kind, N, C_, T))
    return ref, GRAD_FLOOR * np.abs(dx).max() * d + bound2


@pytest.mark.parametrize("kind,config", [("cnn_gru_attention", "full"), ("cnn_gru", "full"), ("cnn_gru_attention", "embedded")])
def test_attributor_equals_the_composition_of_public_pieces(kind, config):
    from multimodalsignal_amd import attribute as AT
    N, C_, K, T, P = 5, 6, 3, 512, 8
    m = _shared_model(kind, config)
    x = _case(N, C_, K, T, 77)[0].to(DEV)
    v = torch.as_tensor(np.random.RandomState(3).randn(N, K).astype(np.float32)).to(DEV)
    a = AT.Attributor(m, steps=P, bin=64).attribute(x, v)
    ref, tol = _composition(m, x, None, R.BASE_ZERO, v, P)
    err = np.abs(a.map.cpu().numpy().astype(np.float64) - ref)
    assert np.all(err <= tol), float((err / np.maximum(tol, 1e-300)).max())
    assert float(np.abs(ref).max()) > 0 and torch.equal(a.target, v)
    _check_sums(a.map.cpu().numpy(), a.bins.cpu().numpy(), a.channel.cpu().numpy(), a.total.cpu().numpy(), 64)
    with torch.no_grad():
        assert torch.equal(a.f_x, AT.target_dot(m(x), v))                                        # bit for bit
        assert torch.equal(a.f_base, AT.target_dot(m(torch.zeros(1, C_, T, device=DEV)).expand(N, K), v))
    assert torch.equal(a.gap, a.total - (a.f_x - a.f_base))
    # the model's convenience call, the predicted class and a class index
    b = m.attribute(x, target="predicted", steps=P, bin=64, return_map=False)
    with torch.no_grad():
        pred = torch.argmax(m(x), dim=1)
    assert b.map is None and torch.equal(b.target, torch.stack([AT.class_target(int(k), K) for k in pred]).to(DEV))
    c = m.attribute(x, target=1, steps=P, bin=64)
    assert torch.equal(c.target, AT.class_target(1, K).to(DEV).expand(N, K))


# ---- 4. against the fp64 oracle -------------------------------------------------------------------------------------------------------
def _hip_pool_choice(eng, key, st64, B, T):
    """tests/test_input_grad_gpu.py's rule: MaxPool near-ties (two candidates equal to within fp32 resolution) adopt the HIP path's
    decision, recomputed from ITS conv outputs and BatchNorm constants; at most 8 adopted decisions."""
    L1, _, L2, _ = O.stage_lengths(T)
    choice, n = {}, 0
    for stage, yname, sname, CH, Lc in (("pool1", "Y1", "BN1_STAT", 16, L1), ("pool2", "Y2", "BN2_STAT", 32, L2)):
        yh = eng.region(yname, torch.float32, (B, Lc, CH), key=key).cpu().double().permute(0, 2, 1)
        stt = eng.region(sname, torch.float32, (4, CH), key=key).cpu().double()
        zh = (yh * stt[2][None, :, None] + stt[3][None, :, None]).float()
        ch_hip = O.first_argmax(O.pool_windows(torch.clamp_min(zh, 0)))
        win = O.pool_windows(torch.clamp_min(st64["bn" + stage[-1]].detach(), 0))
        ch_ref = O.first_argmax(win)
        top = win.max(dim=3).values
        hip_val = win.gather(3, ch_hip.to(torch.int64)[..., None]).squeeze(3)
        near = (ch_hip != ch_ref) & ((top - hip_val) <= 4e-6 * torch.clamp_min(top.abs(), 1e-3))
        n += int(near.sum())
        choice[stage] = torch.where(near, ch_hip, ch_ref)
    assert n <= 8, f"{n} adopted pooling decisions"
    return choice if n else None


def _oracle_path(named, x, base, v, P, dtype, pool_choice=None):
    """Integrated gradients by the oracle: the path is built in `dtype`, x a leaf.  Returns (G, map, total, stages, logits of the path)."""
    p, b = split_named(to_t(named, dtype))
    N = x.shape[0]
    alpha, w = R.midpoint(P)
    x_, b_ = x.to(dtype), base.to(dtype)
    a = torch.as_tensor(alpha, dtype=dtype)
    xp = (b_[:, None] + a[None, :, None, None] * (x_ - b_)[:, None]).reshape(N * P, *x.shape[1:]).clone().requires_grad_(True)
    st, _ = O.forward(p, b, xp, training=False, pool_choice=pool_choice)
    (st["logits"] * v.to(dtype).repeat_interleave(P, dim=0)).sum().backward()
    G = (xp.grad.reshape(N, P, *x.shape[1:]) * torch.as_tensor(w, dtype=dtype)[None, :, None, None]).sum(dim=1)
    amap = (x_ - b_) * G
    return G.detach(), amap.detach(), amap.sum(dim=(1, 2)).detach(), st, xp.grad.detach()


def _oracle_f(named, x, v, dtype):
    p, b = split_named(to_t(named, dtype))
    with torch.no_grad():
        st, _ = O.forward(p, b, x.to(dtype), training=False)
    return (st["logits"] * v.to(dtype)).sum(dim=1)


@pytest.mark.parametrize("C_", [3, 6])
def test_attributor_against_the_fp64_oracle(C_):
    """A random window as baseline: the path points are generic inputs.  N = 2, P = 4: eight path windows."""
    from multimodalsignal_amd import attribute as AT
    from multimodalsignal_amd.runtime import Engine
    N, K, T, P = 2, 3, 256, 4
    m = _trained(C_, K, "full").eval()
    named = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    x, base = _case(N, C_, K, T, 200 + C_)[0], _case(N, C_, K, T, 300 + C_)[0]
    v = torch.as_tensor(np.random.RandomState(C_).randn(N, K).astype(np.float32))
    a = AT.Attributor(m, steps=P, baseline=base.to(DEV)).attribute(x.to(DEV), v.to(DEV))
    torch.cuda.synchronize()
    G64, map64, _, st64, _ = _oracle_path(named, x, base, v, P, torch.float64)
    choice = _hip_pool_choice(m._engine, (N * P, T, Engine.EVAL_KEEP), st64, N * P, T)
    if choice is not None:
        G64, map64, _, st64, _ = _oracle_path(named, x, base, v, P, torch.float64, choice)
    G32, map32, _, _, _ = _oracle_path(named, x, base, v, P, torch.float32, choice)
    d32 = (x - base).numpy()
    got_map = a.map.cpu().numpy()
    ok = d32 != 0
    got_G = np.where(ok, got_map / np.where(ok, d32, 1.0), G64.numpy())          # G back from the map: one more rounding per element
    for name, got, r64, r32 in (("G", got_G, G64, G32), ("map", got_map, map64, map32)):
        own = rel_err(r32.numpy(), r64.numpy())
        err = rel_err(got, r64.numpy())
        print(f"C={C_} {name}: err {err:.3e} own {own:.3e} tol {grad_tol('x', own):.3e}")
        assert err <= grad_tol("x", own), (name, err, own)


# ---- 5. completeness with the zero baseline -------------------------------------------------------------------------------------------
def test_completeness_gap_is_the_quadrature_error():
    from multimodalsignal_amd import attribute as AT
    N, C_, K, T, P = 4, 6, 3, 512, 64
    m = _shared_model("cnn_gru_attention", "full")
    named = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    x = _case(N, C_, K, T, 41)[0]
    v = torch.stack([AT.class_target(k % K, K) for k in range(N)])
    zero = torch.zeros_like(x)
    gaps = {}
    for p in (4, 32, 64):
        gaps[p] = AT.Attributor(m, steps=p).attribute(x.to(DEV), v.to(DEV), return_map=False)
    a = gaps[P]
    _, map64, tot64, _, dxp64 = _oracle_path(named, x, zero, v, P, torch.float64)
    _, _, tot32, _, _ = _oracle_path(named, x, zero, v, P, torch.float32)
    gap64 = (tot64 - (_oracle_f(named, x, v, torch.float64) - _oracle_f(named, zero, v, torch.float64))).numpy()        # pure quadrature error
    w = R.midpoint(P)[1]
    _, bound2 = R.reduce_map(dxp64.numpy(), x.numpy(), None, R.BASE_ZERO, w.astype(np.float32))
    bound3 = (GRAD_FLOOR * float(dxp64.abs().max()) * np.abs(x.numpy().astype(np.float64)) + bound2).sum(axis=(1, 2))
    allowed = np.abs(gap64) + K_GRAD * np.abs(tot32.double().numpy() - tot64.numpy()) + bound3
    got = np.abs(a.gap.double().cpu().numpy())
    for p in (4, 32, 64):
        g = gaps[p]
        print(f"P={p}: |gap| {np.abs(g.gap.cpu().numpy())} of f(x) - f(0) {(g.f_x - g.f_base).cpu().numpy()}")
    print(f"P={P}: fp64 oracle |gap| {np.abs(gap64)} allowed {allowed}")
    assert np.all(got <= allowed), (got, allowed)


# ---- 6. independent of the cut into path batches --------------------------------------------------------------------------------------
def test_attribution_does_not_depend_on_the_path_batches():
    from multimodalsignal_amd import attribute as AT
    N, C_, K, T, P, bin_ = 9, 6, 3, 512, 8, 100
    m = _shared_model("cnn_gru_attention", "full")
    x = _case(N, C_, K, T, 61)[0].to(DEV)
    v = AT.class_target(2, K).to(DEV).expand(N, K).contiguous()
    one = AT.Attributor(m, steps=P, bin=bin_, path_batch=9 * P).attribute(x, v)
    cut = AT.Attributor(m, steps=P, bin=bin_, path_batch=2 * P + 3).attribute(x, v)           # five batches, the last of one window
    ref, tol = _composition(m, x, None, R.BASE_ZERO, v, P)
    for a in (one, cut):
        err = np.abs(a.map.cpu().numpy().astype(np.float64) - ref)
        assert np.all(err <= tol), float((err / np.maximum(tol, 1e-300)).max())
        _check_sums(a.map.cpu().numpy(), a.bins.cpu().numpy(), a.channel.cpu().numpy(), a.total.cpu().numpy(), bin_)
    assert np.all(np.abs(one.map.cpu().numpy().astype(np.float64) - cut.map.cpu().numpy()) <= tol)
    assert torch.equal(one.f_x, cut.f_x) and torch.equal(one.f_base, cut.f_base)


# ---- 7. a dummy channel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cnn_gru", "cnn_gru_attention"])
def test_a_channel_the_model_cannot_see_gets_exactly_zero(kind):
    N, C_, K, T, j = 4, 6, 3, 256, 2
    m = _trained(C_, K, "full", kind=kind).eval()
    m.engine()
    with torch.no_grad():
        m.cnn_encoder[0].weight[:, j, :] = 0.0
        if kind == "cnn_gru_attention":
            m.channel_attention.fc[0].weight[:, j] = 0.0
    x = _case(N, C_, K, T, 71)[0].to(DEV)
    a = m.attribute(x, target="predicted", steps=8)
    occ = m.channel_occlusion(x, target="predicted")
    assert bool((a.map[:, j] == 0).all()) and bool((a.channel[:, j] == 0).all()) and bool((occ[:, j] == 0).all())
    others = [c for c in range(C_) if c != j]
    assert bool((a.channel[:, others] != 0).all()) and bool((occ[:, others] != 0).all()) and bool((a.map[:, others].abs().amax(dim=2) > 0).all())


# ---- 8. occlusion ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,config", [("cnn_gru_attention", "full"), ("cnn_gru", "full"), ("cnn_gru_attention", "embedded")])
def test_occlusion_equals_plain_forwards_bit_for_bit(kind, config):
    from multimodalsignal_amd import attribute as AT
    N, C_, K, T = 5, 6, 3, 512
    m = _shared_model(kind, config)
    rs = np.random.RandomState(8)
    x = _case(N, C_, K, T, 81)[0].to(DEV)
    v = torch.as_tensor(rs.randn(N, K).astype(np.float32)).to(DEV)
    for bkind, (bd, bn) in _bases(rs, N, C_, T).items():
        # steps = 4 only so that the small path_batch is legal (>= steps); occlusion has C + 1 rows per window: three batches, the
        # last of one window
        occ = AT.Attributor(m, steps=4, baseline=bd, path_batch=2 * (C_ + 1)).channel_occlusion(x, v)
        full = torch.as_tensor(R.broadcast_base(bn, bkind, N, C_, T, np.float32)).to(DEV)
        with torch.no_grad():
            f_x = AT.target_dot(m(x), v)
            for c in range(C_):
                xc = x.clone()
                xc[:, c] = full[:, c]
                assert torch.equal(occ[:, c], f_x - AT.target_dot(m(xc), v)), (bkind, c)
    assert torch.equal(m.channel_occlusion(x, v), AT.Attributor(m).channel_occlusion(x, v))


def test_gate_values():
    from multimodalsignal_amd import attribute as AT
    N, C_, K, T = 5, 6, 3, 512
    m = _shared_model("cnn_gru_attention", "full")
    x = _case(N, C_, K, T, 91)[0].to(DEV)
    s = AT.Attributor(m).gate(x)
    named = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    ref = O.channel_gate(x.cpu().double(), named["channel_attention.fc.0.weight"].double(), named["channel_attention.fc.2.weight"].double())[2]
    assert s.shape == (N, C_) and rel_err(s.cpu().numpy(), ref.numpy()) <= 2e-6
    assert AT.Attributor(_shared_model("cnn_gru", "full")).gate(x) is None
    small = _model(3, 2, "full", 0.0).eval()
    assert torch.equal(AT.Attributor(small).gate(x[:, :3].contiguous()), torch.full((N, 3), 0.5, device=DEV))


# ---- 9. no side effects ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["full", "embedded"])
def test_attribution_has_no_side_effects(config):
    C_, K, T = 6, 3, 256
    m = _trained(C_, K, config).train()
    x, y = _case(8, C_, K, T, 11)
    torch.nn.CrossEntropyLoss()(m(x.to(DEV)), y.to(DEV)).backward()                   # a non-zero gradient buffer
    eng = m._engine
    assert float(eng.grads.abs().max()) > 0
    before = {k: v.clone() for k, v in m.state_dict().items()}
    grads, pgrads, step = eng.grads.clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}, m._step
    a = m.attribute(x.to(DEV), steps=4)
    occ = m.channel_occlusion(x.to(DEV))
    torch.cuda.synchronize()
    assert a.map.shape == (8, C_, T) and occ.shape == (8, C_)
    after = m.state_dict()
    assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert torch.equal(eng.grads, grads) and m._step == step and m.training is True
    assert all(torch.equal(p.grad, pgrads[k]) for k, p in m.named_parameters() if k in pgrads)
    # a pending autograd backward of an earlier forward must not read the attributor's activations
    m.eval()
    out = m(x.to(DEV).requires_grad_(True))
    m.attribute(x.to(DEV), steps=4)
    with pytest.raises(RuntimeError, match="overwritten by a later forward"):
        out.sum().backward()


# ---- 10. the driver -------------------------------------------------------------------------------------------------------------------
def _fold_results(run, subs):
    out = {}
    for s in subs:
        info = json.loads((run / f"fold_test_on_{s}" / "fold_result.json").read_text())
        info["history"] = [{k: v for k, v in h.items() if k != "seconds"} for h in info["history"]]
        out[s] = {k: v for k, v in info.items() if "seconds" not in k and "per_s" not in k}
    return out


def test_driver_attributes_after_loso(tmp_path, capsys):
    """cv_summary.txt and fold_result.json are compared without their wall-clock entries (the summary's last line, the results'
    seconds and rates), which differ between any two runs; everything else byte for byte."""
    from multimodalsignal_amd import attribute as AT
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.synth import CHANNELS6, make_synthetic_wesad
    subs = ["S2", "S3", "S4", "S5"]
    d = make_synthetic_wesad(tmp_path / "w", subjects=subs, windows_per_subject=12, T=256, difficulty=2.0)
    common = ["--synthetic", str(d), "--samples", "256", "--subjects", *subs, "--epochs", "1", "--batch-size", "16"]
    M.main(common + ["--attribute", "4", "--out", str(tmp_path / "at")])
    M.main(common + ["--out", str(tmp_path / "plain")])
    runs = {k: sorted((tmp_path / k).glob("simple_binary/run_*"))[0] for k in ("at", "plain")}
    cut = lambda text: text[:text.index("LOSO wall-clock")]
    assert cut((runs["at"] / "cv_summary.txt").read_text(encoding="utf-8")) == cut((runs["plain"] / "cv_summary.txt").read_text(encoding="utf-8"))
    assert _fold_results(runs["at"], subs) == _fold_results(runs["plain"], subs)
    assert sorted(p.name for p in runs["plain"].iterdir()) == sorted(p.name for p in runs["at"].iterdir() if not p.name.startswith("attribution"))
    assert not (runs["plain"] / "attribution.json").exists() and not (runs["plain"] / "fold_test_on_S2" / "attribution_result.json").exists()
    doc = json.loads((runs["at"] / "attribution.json").read_text())
    assert [f["subject"] for f in doc["folds"]] == subs and doc["n_folds"] == 4 and doc["note"] == AT.SYNTHETIC_NOTE
    assert doc["settings"] == {"steps": 4, "baseline": "zero", "target": "predicted"} and doc["channels"] == list(CHANNELS6)
    assert sorted(doc["ranking"]) == sorted(CHANNELS6)
    for s, fold in zip(subs, doc["folds"]):
        per = json.loads((runs["at"] / f"fold_test_on_{s}" / "attribution_result.json").read_text())
        assert per == fold and per["subject"] == s and per["n"] == 12 and per["steps"] == 4 and per["bin"] == 4
        assert sum(per["share"]) == pytest.approx(1.0) and len(per["share"]) == len(per["occlusion"]) == len(per["gate"]) == 6
        assert len(per["time_profile"]) == 64 and np.isfinite(per["gap_rel_max"]) and all(0.0 < g < 1.0 for g in per["gate"])
    txt = (runs["at"] / "attribution.txt").read_text(encoding="utf-8")
    assert AT.SYNTHETIC_NOTE in txt and all(s in txt for s in subs) and "channel ranking by mean share" in txt
    assert "attribution over 12 windows, 4 path points" in capsys.readouterr().out
