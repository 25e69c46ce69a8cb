"""Entropy-minimisation adaptation on the MI355X (include/msig_tt.h, tta.EntropyAdapter, model.adapt_entropy, --adapt-entropy).

1. the objective's launch against the fp64 restatement tests/tt_reference.py: dlogits within 1 fp32 ulp of the reference plus 1e-13
   absolute (the kernel is fp64 inside; its terms are at most ln 16 with ~1e-15 relative error, and lp + H cancels to rounding at
   uniform rows), the statistics within 1e-12 relative.  `make negctl TENT=1` (the gradient without H_b) must fail every case;
2. the selective Adam against msig_adam_step, bit for bit, and every unselected byte untouched;
3. msig_tt_step against its four calls, bit for bit; labels change no bit; the BatchNorm buffers are not written;
4. the objective's gradient through the model against the fp64 oracle, tolerance gpu_common.grad_tol unchanged;
5. fold batches against single calls, bit for bit, with folds of unequal size;
6. the Python layer and the driver.
Shapes are small: T = 256 or 200, a handful of windows."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import tt_reference as TR
from gpu_common import grad_tol, rel_err
from oracle import cnn_gru_oracle as O
from test_input_grad_gpu import _hip_pool_choice, _oracle
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd import tta
from multimodalsignal_amd.models import CnnGruAttentionModel, CnnGruModel
from multimodalsignal_amd.runtime import Arenas, make_batch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KINDS = {"cnn_gru_attention": CnnGruAttentionModel, "cnn_gru": CnnGruModel}
CONFIGS = {"full": dict(), "embedded": dict(gru_hidden_size=32, gru_num_layers=1)}
f = C.c_float
BETAS, EPS = (0.9, 0.999), 1e-8


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int64) if t.dtype == torch.float64 else t)


def _same(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


# ---- 1. the objective ------------------------------------------------------------------------------------------------------------------
def _objective(z, div, stats=True, steps=1):
    lg = torch.as_tensor(z, device=DEV)
    B, K = lg.shape
    dl = torch.full((B, K), float("nan"), dtype=torch.float32, device=DEV)
    st = torch.zeros(TR.TT_STATS, dtype=torch.float64, device=DEV)
    for _ in range(steps):
        L.check(tta.lib().msig_tt_objective(lg.data_ptr(), B, K, f(div), dl.data_ptr(), st.data_ptr() if stats else None, _stream()),
                "msig_tt_objective")
    torch.cuda.synchronize()
    return dl.cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize("regime", TR.REGIMES)
@pytest.mark.parametrize("div", TR.DIVERSITIES)
@pytest.mark.parametrize("K", TR.CLASSES)
@pytest.mark.parametrize("B", TR.BATCHES)
def test_objective_against_the_reference(B, K, div, regime):
    z = TR.logits_case(B, K, regime)
    ref = TR.objective(z, div)
    got, st = _objective(z, div)
    err = np.abs(got.astype(np.float64) - ref["dlogits"])
    tol = TR.ulp32(ref["dlogits"]) + 1e-13
    worst = float((err / tol).max())
    print(f"B {B} K {K} div {div} {regime}: worst dlogits error {err.max():.3e}, {worst:.3f} of its tolerance")
    assert np.isfinite(got).all() and worst <= 1.0, (float(err.max()), worst)
    rs = ref["stats"]
    srel = np.abs(st - rs) / np.where(rs != 0, np.abs(rs), 1.0)
    print(f"   worst relative error of a statistic {srel.max():.3e}")
    assert (srel <= 1e-12).all(), (st, rs)
    assert (st[TR.S_PRED:TR.S_PRED + K] == rs[TR.S_PRED:TR.S_PRED + K]).all() and st[TR.S_ROWS] == B and st[TR.S_STEPS] == 1


def test_objective_accumulates_and_stats_are_optional():
    z = TR.logits_case(65, 3, "saturated")
    d1, s1 = _objective(z, 0.5)
    d3, s3 = _objective(z, 0.5, steps=3)
    d0, s0 = _objective(z, 0.5, stats=False)
    assert (d1.view(np.int32) == d3.view(np.int32)).all() and (d1.view(np.int32) == d0.view(np.int32)).all()
    assert (s0 == 0).all() and (s3 == (s1 + s1) + s1).all()                  # one adder, in stream order
    assert (s1[TR.S_P + 3:TR.S_PRED] == 0).all() and (s1[TR.S_PRED + 3:] == 0).all()      # the slots beyond K are not touched


def test_objective_multi_has_the_single_calls_bits():
    """Three folds in arenas 2, 0 and 3 of four: each fold's dlogits and statistics are its single call's, the fourth arena is untouched."""
    B, K, div = 65, 3, 0.5
    a = Arenas(4, DEV, [("lg", B * K * 4), ("dl", B * K * 4), ("st", TR.TT_STATS * 8)])
    a.mem.fill_(0x55)
    slots = [2, 0, 3]
    zs = {s: TR.logits_case(B, K, TR.REGIMES[i], seed=s) for i, s in enumerate(slots)}
    for s in slots:
        a.view(s, "lg", torch.float32).copy_(torch.as_tensor(zs[s]).reshape(-1))
        a.view(s, "st").zero_()
    before = a.mem[1].clone()
    L.check(tta.lib().msig_tt_objective_multi(a.ptr("lg"), B, K, f(div), a.ptr("dl"), a.ptr("st"), C.byref(a.multi(slots)), _stream()),
            "msig_tt_objective_multi")
    torch.cuda.synchronize()
    assert torch.equal(a.mem[1], before)
    for s in slots:
        d, st = _objective(zs[s], div)
        assert (a.view(s, "dl", torch.float32).cpu().numpy().view(np.int32) == d.reshape(-1).view(np.int32)).all(), s
        assert (a.view(s, "st", torch.float64).cpu().numpy() == st).all(), s


# ---- 2. the selective Adam ---------------------------------------------------------------------------------------------------------------
def _adam_buffers(n, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    p = torch.randn(n, generator=g)
    return p.to(DEV), [torch.randn(n, generator=g).mul_(10.0 ** (s - 2)).to(DEV) for s in range(3)]


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("C_,K", [(3, 2), (6, 3), (3, 3), (6, 2)])
def test_selective_adam_against_adam_step(C_, K, kind):
    lib = tta.lib()
    layout = L.param_layout(C_, K, kind)
    n = layout[-1]
    p0, grads = _adam_buffers(n, 7 * C_ + K)
    lr, wd = 3e-3, 0.0
    ref = [p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
    full = [t.clone() for t in ref]
    bn = [t.clone() for t in ref]
    bn_ref = [t.clone() for t in ref]                            # msig_adam_step fed the SAME gradients: its selected elements are the target
    sel = torch.zeros(n, dtype=torch.bool, device=DEV)
    for i in (tta.P_BN1_G, tta.P_BN1_B, tta.P_BN2_G, tta.P_BN2_B):
        sel[layout[i]:layout[i + 1]] = True
    assert int(sel.sum()) == 96
    for step in range(1, 4):
        g = grads[step - 1]
        L.check(lib.msig_adam_step(ref[0].data_ptr(), g.data_ptr(), ref[1].data_ptr(), ref[2].data_ptr(), n, lr, *BETAS, EPS, wd, step, _stream()),
                "msig_adam_step")
        L.check(lib.msig_tt_adam(full[0].data_ptr(), g.data_ptr(), full[1].data_ptr(), full[2].data_ptr(), C_, K, L.FT_KINDS[kind],
                                 tta.SELECT_ALL, lr, *BETAS, EPS, wd, step, _stream()), "msig_tt_adam")
        L.check(lib.msig_tt_adam(bn[0].data_ptr(), g.data_ptr(), bn[1].data_ptr(), bn[2].data_ptr(), C_, K, L.FT_KINDS[kind],
                                 tta.SELECT_BN, lr, *BETAS, EPS, wd, step, _stream()), "msig_tt_adam")
        # the reference of the BN selection: one msig_adam_step on buffers whose unselected elements are put back afterwards
        keep = [t.clone() for t in bn_ref]
        L.check(lib.msig_adam_step(bn_ref[0].data_ptr(), g.data_ptr(), bn_ref[1].data_ptr(), bn_ref[2].data_ptr(), n, lr, *BETAS, EPS, wd, step,
                                   _stream()), "msig_adam_step")
        for t, k in zip(bn_ref, keep):
            t[~sel] = k[~sel]
        torch.cuda.synchronize()
        for name, a, b in zip(("params", "exp_avg", "exp_avg_sq"), full, ref):
            assert _same(a, b), (step, name)                                      # all bits set: msig_adam_step, bit for bit
        for name, a, b, start in zip(("params", "exp_avg", "exp_avg_sq"), bn, bn_ref, (p0, None, None)):
            assert _same(a[sel], b[sel]), (step, name)                            # the 96 selected elements are msig_adam_step's
            rest = p0[~sel] if start is not None else torch.zeros_like(a[~sel])
            assert _same(a[~sel], rest), (step, name)                             # every other byte is what it was
        assert not _same(bn[0][sel], p0[sel])


def test_selective_adam_multi_takes_rate_and_step_per_fold():
    lib, C_, K, kind = tta.lib(), 3, 2, "cnn_gru_attention"
    n = L.param_layout(C_, K, kind)[-1]
    a = Arenas(3, DEV, [("p", n * 4), ("g", n * 4), ("m", n * 4), ("v", n * 4)])
    single = []
    lrs, steps = [1e-3, 5e-2, 0.0], [1, 7, 3]
    for s in range(3):
        p0, grads = _adam_buffers(n, 50 + s)
        m0, v0 = grads[1].abs() * 0.1, grads[2].abs() * 0.01
        for name, t in (("p", p0), ("g", grads[0]), ("m", m0), ("v", v0)):
            a.view(s, name, torch.float32).copy_(t)
        bufs = [p0.clone(), m0.clone(), v0.clone()]
        L.check(lib.msig_tt_adam(bufs[0].data_ptr(), grads[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), C_, K, 0, tta.SELECT["bn+gate"],
                                 lrs[s], *BETAS, EPS, 0.0, steps[s], _stream()), "msig_tt_adam")
        single.append(bufs)
    L.check(lib.msig_tt_adam_multi(a.ptr("p"), a.ptr("g"), a.ptr("m"), a.ptr("v"), C_, K, 0, tta.SELECT["bn+gate"], *BETAS, EPS, 0.0, 1,
                                   C.byref(a.multi([0, 1, 2], lr=lrs, steps=steps)), _stream()), "msig_tt_adam_multi")
    torch.cuda.synchronize()
    for s in range(3):
        for name, t in zip(("p", "m", "v"), single[s]):
            assert _same(a.view(s, name, torch.float32), t), (s, name)
    assert _same(a.view(2, "p", torch.float32), _adam_buffers(n, 52)[0])          # lr = 0 moves no parameter


# ---- models with trained-like BatchNorm ------------------------------------------------------------------------------------------------
def _model(kind, C_, K, config="full", seed=0):
    """A model whose BatchNorm scale, shift and running statistics are off their initial values (signed scales included), in eval mode."""
    torch.manual_seed(seed)
    m = KINDS[kind](C_, K, dropout=0.5, **CONFIGS[config]).to(DEV)
    rs = np.random.RandomState(100 + seed)
    with torch.no_grad():
        for idx, CH in ((1, 16), (5, 32)):
            bn = m.cnn_encoder[idx]
            gamma = rs.uniform(0.5, 1.6, CH) * np.where(rs.rand(CH) < 0.2, -1.0, 1.0)
            bn.weight.copy_(torch.as_tensor(gamma, dtype=torch.float32))
            bn.bias.copy_(torch.as_tensor(rs.uniform(-0.6, 0.6, CH), dtype=torch.float32))
            bn.running_mean.copy_(torch.as_tensor(rs.uniform(-0.3, 0.3, CH), dtype=torch.float32))
            bn.running_var.copy_(torch.as_tensor(rs.uniform(0.5, 2.0, CH), dtype=torch.float32))
    m.engine()
    return m.eval()


def _x(n, C_, T, seed):
    rs = np.random.RandomState(seed)
    return torch.as_tensor((rs.randn(n, C_, T) * (0.5 + rs.rand(1, C_, 1)) + rs.randn(1, C_, 1)).astype(np.float32), device=DEV)


# ---- 3. the step is its four calls --------------------------------------------------------------------------------------------------------
class _Harness(Arenas):
    """One model's buffers for the raw calls: parameters, gradients, moments, BatchNorm state, a batch, a training-layout workspace."""

    def __init__(self, model, B, T):
        self.eng = e = model.engine()
        if getattr(e, "scatter", None) is not None:
            e.scatter()
        self.B, self.T = B, T
        self.ws_bytes = L.workspace_layout(B, e.C, T, e.K, True)[-1]
        flat = e.n_flat * 4
        super().__init__(1, DEV, [("params", flat), ("grads", flat), ("exp_avg", flat), ("exp_avg_sq", flat), ("bn_state", 96 * 4), ("bn_count", 16),
                                  ("x", B * e.C * T * 4), ("y", B * 8), ("ws", self.ws_bytes), ("stats", TR.TT_STATS * 8), ("acc", 16)])
        self.view(0, "params", torch.float32).copy_(e.params)
        self.view(0, "bn_state", torch.float32).copy_(e.bn_state)
        self.view(0, "bn_count", torch.int64)[:2].fill_(5)

    def desc(self, labels):
        e = self.eng
        b = make_batch(self.B, e.C, self.T, e.K, *(self.ptr(r) for r in ("x", "params", "bn_state", "bn_count", "ws")), self.ws_bytes, e.gru_layers,
                       labels=self.ptr("y") if labels else None, grads=self.ptr("grads"), loss_acc=self.ptr("acc") if labels else None)
        b.keep_for_backward = 1
        return b

    def tt(self, select, div):
        t = tta.Tt()
        t.kind, t.select, t.diversity = L.FT_KINDS[self.eng.kind], select, div
        t.beta1, t.beta2, t.eps, t.weight_decay = BETAS[0], BETAS[1], EPS, 0.0
        t.exp_avg, t.exp_avg_sq, t.stats = self.ptr("exp_avg"), self.ptr("exp_avg_sq"), self.ptr("stats")
        return t

    def region(self, name, dtype=torch.float32):
        off = L.workspace_layout(self.B, self.eng.C, self.T, self.eng.K, True)
        o = self.off["ws"][0]
        return self.mem[0, o + off[L.WS[name]]:o + off[L.WS[name] + 1]].view(dtype)


def _run_steps(model, x, y, labels, fused, select, div, lr=1e-2, steps=2):
    lib = tta.lib()
    B, _, T = x.shape
    h = _Harness(model, B, T)
    h.view(0, "x", torch.float32).copy_(x.reshape(-1))
    h.view(0, "y", torch.int64).copy_(y)
    cg = h.eng.kind == "cnn_gru"
    e = h.eng
    for step in range(1, steps + 1):
        b, t = h.desc(labels), h.tt(select, div)
        if fused:
            L.check(lib.msig_tt_step(C.byref(b), C.byref(t), lr, step, _stream()), "msig_tt_step")
        else:
            if cg:
                L.check(lib.msig_cg_forward(C.byref(b), None, _stream()), "msig_cg_forward")
            else:
                L.check(lib.msig_forward(C.byref(b), _stream()), "msig_forward")
            L.check(lib.msig_tt_objective(h.region("LOGITS").data_ptr(), B, e.K, f(div), h.region("DLOGITS").data_ptr(), h.ptr("stats"), _stream()),
                    "msig_tt_objective")
            L.check((lib.msig_cg_backward if cg else lib.msig_backward)(C.byref(b), None, _stream()), "msig_backward")
            L.check(lib.msig_tt_adam(h.ptr("params"), h.ptr("grads"), h.ptr("exp_avg"), h.ptr("exp_avg_sq"), e.C, e.K, L.FT_KINDS[e.kind], select,
                                     lr, *BETAS, EPS, 0.0, step, _stream()), "msig_tt_adam")
    torch.cuda.synchronize()
    return h


@pytest.mark.parametrize("kind,config,C_,K,select,div", [("cnn_gru_attention", "full", 6, 3, tta.SELECT_BN, 0.5),
                                                         ("cnn_gru_attention", "embedded", 6, 2, tta.SELECT_ALL, 0.0),
                                                         ("cnn_gru", "full", 3, 2, tta.SELECT["bn+gate"], 1.0)])
def test_step_is_forward_objective_backward_adam(kind, config, C_, K, select, div):
    B, T = 5, 256
    m = _model(kind, C_, K, config, seed=3)
    x = _x(B, C_, T, 11)
    y = torch.as_tensor(np.random.RandomState(1).randint(0, K, B), device=DEV)
    e = m.engine()
    runs = {(fused, labels): _run_steps(m, x, y, labels, fused, select, div) for fused in (True, False) for labels in (True, False)}
    ref = runs[(False, False)]
    for key, h in runs.items():
        for r in ("params", "grads", "exp_avg", "exp_avg_sq", "stats", "bn_state", "bn_count"):
            assert torch.equal(h.view(0, r), ref.view(0, r)), (key, r)              # the four calls' bits; labels change none
        assert _same(h.region("DLOGITS")[:B * K], ref.region("DLOGITS")[:B * K]), key
    h = runs[(True, True)]
    assert _same(h.view(0, "bn_state", torch.float32), e.bn_state)                # the BatchNorm buffers are never written
    assert h.view(0, "bn_count", torch.int64)[:2].tolist() == [5, 5]
    layout = L.param_layout(C_, K, kind)
    chosen = torch.zeros(e.n_flat, dtype=torch.bool, device=DEV)
    for i in range(tta.NPARAM):
        if (select >> i) & 1:
            chosen[layout[i]:layout[i + 1]] = True
    p1, p0 = h.view(0, "params", torch.float32), e.params
    assert _same(p1[~chosen], p0[~chosen])                                        # nothing outside the selection moved
    for r in ("exp_avg", "exp_avg_sq"):
        assert not h.view(0, r, torch.float32)[~chosen].any(), r
    bnsel = torch.zeros_like(chosen)
    for i in (tta.P_BN1_G, tta.P_BN1_B, tta.P_BN2_G, tta.P_BN2_B):
        bnsel[layout[i]:layout[i + 1]] = True
    assert int((p1[bnsel] != p0[bnsel]).sum()) > 48                               # and the selection did
    acc = h.view(0, "acc", torch.float64).cpu().numpy()
    assert acc[0] > 0 and 0 <= acc[1] <= 2 * B and float(acc[1]).is_integer()     # the online CrossEntropy of the two steps
    assert not runs[(True, False)].view(0, "acc", torch.float64).any()
    st = h.view(0, "stats", torch.float64).cpu().numpy()
    assert st[TR.S_ROWS] == 2 * B and st[TR.S_STEPS] == 2


# ---- 4. the gradient through the model against the fp64 oracle -----------------------------------------------------------------------------
@pytest.fixture
def no_gate(monkeypatch):
    """The oracle's ChannelAttention replaced by the identity (s = 1): the baseline's reference, without editing oracle/."""
    def gate(x, W1, W2):
        B, C_, _ = x.shape
        return x.mean(dim=2), torch.zeros(B, 0, dtype=x.dtype), torch.ones(B, C_, dtype=x.dtype)
    return lambda: monkeypatch.setattr(O, "channel_gate", gate)


@pytest.mark.parametrize("div", [0.0, 0.5])
@pytest.mark.parametrize("kind,config", [("cnn_gru_attention", "full"), ("cnn_gru", "full"), ("cnn_gru_attention", "embedded")])
@pytest.mark.parametrize("B,C_,K,T", [(5, 3, 2, 256), (4, 6, 3, 200)])
def test_objective_gradient_through_the_model_against_the_oracle(B, C_, K, T, kind, config, div, no_gate):
    m = _model(kind, C_, K, config, seed=B + C_)
    eng = m.engine()
    x = _x(B, C_, T, 20 + B)
    named = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    if kind == "cnn_gru":
        no_gate()
        named["channel_attention.fc.0.weight"] = torch.zeros(0, C_)
        named["channel_attention.fc.2.weight"] = torch.zeros(C_, 0)
    b = eng.forward(x, None, training=False, keep_for_backward=True)
    lg, dl = eng.region("LOGITS", torch.float32, (B, K)), eng.region("DLOGITS", torch.float32, (B, K))
    L.check(tta.lib().msig_tt_objective(lg.data_ptr(), B, K, f(div), dl.data_ptr(), None, _stream()), "msig_tt_objective")
    eng.backward(b)
    torch.cuda.synchronize()
    got = eng.gather_grads() if config == "embedded" else eng.named_param_views(eng.grads)
    got = {k: v.detach().cpu().numpy().copy() for k, v in got.items()}
    loss_fn = lambda logits: TR.loss_torch(logits, div)
    fw = dict(dropout_p=0.0, seed=0, step=0)
    xc = x.cpu()
    _, g64, st64 = _oracle(named, xc, None, torch.float64, False, fw, loss_fn)
    choice = _hip_pool_choice(eng, st64, B, T)                                    # pooling ties: that file's adopt rule
    if choice is not None:
        _, g64, st64 = _oracle(named, xc, None, torch.float64, False, fw, loss_fn, choice)
    _, g32, _ = _oracle(named, xc, None, torch.float32, False, fw, loss_fn, choice)
    checked = 0
    for k, g in got.items():
        if g.size == 0:
            continue
        ref = g64[k].numpy()
        own = rel_err(g32[k].numpy(), ref)
        err = rel_err(g, ref)
        print(f"{k:<36} err {err:.3e} own {own:.3e} tol {grad_tol(k, own):.3e}")
        assert np.isfinite(g).all() and err <= grad_tol(k, own), (k, err, own)
        checked += 1
    assert checked == len([k for k, v in g64.items() if v.numel()])
    for k in ("cnn_encoder.1.weight", "cnn_encoder.1.bias", "cnn_encoder.5.weight", "cnn_encoder.5.bias"):
        assert np.abs(g64[k].numpy()).max() > 0, k                               # what the adaptation moves has a gradient to follow


# ---- 5. fold batches ------------------------------------------------------------------------------------------------------------------------
def _jobs(sizes, C_, K, T, kind="cnn_gru_attention", labelled=True):
    jobs = []
    for i, n in enumerate(sizes):
        j = dict(model=_model(kind, C_, K, seed=40 + i), x=_x(n, C_, T, 60 + i))
        if labelled:
            j["y"] = torch.as_tensor(np.random.RandomState(i).randint(0, K, n), device=DEV)
        jobs.append(j)
    return jobs


def _adapter_state(ad):
    return [{r: ad.view(s, r).clone() for r in ("params", "exp_avg", "exp_avg_sq", "stats", "grads", "bn_state", "bn_count")} for s in range(ad.n)]


@pytest.mark.parametrize("sizes", [[13, 8, 13], [9, 17, 8, 12, 17, 5, 9, 16, 11, 8, 17, 3, 10, 9, 14]], ids=["3-folds", "15-folds"])
def test_fold_batch_has_the_single_calls_bits(sizes):
    """Folds of unequal N (ragged last batches of different sizes, folds that run out of batches early): every fold's parameters, moments
    and statistics are those of the adapter that holds it alone, fold-batched or not.  Arenas.form_folds pins the backward GRU form to
    one stand-alone fold's, as the other fold-batched analyses pin it."""
    C_, K, T = 3, 2, 256
    jobs = _jobs(sizes, C_, K, T)
    kw = dict(lr=5e-3, epochs=2, diversity=0.5, batch=8, params="bn+gate", seed=3)
    assert Arenas.form_folds == 1
    a = tta.EntropyAdapter(jobs, batched=True, **kw)
    b = tta.EntropyAdapter(jobs, batched=False, **kw)
    a.adapt(), b.adapt()
    torch.cuda.synchronize()
    sa, sb = _adapter_state(a), _adapter_state(b)
    for s in range(len(sizes)):
        for r in sa[s]:
            assert torch.equal(sa[s][r], sb[s][r]), (s, r)
    assert a.objective == b.objective and a.online == b.online
    for s in sorted({0, 1, len(sizes) - 1, int(np.argmin(sizes))}):
        one = tta.EntropyAdapter([jobs[s]], batched=True, **kw)
        one.adapt()
        torch.cuda.synchronize()
        so = _adapter_state(one)[0]
        for r in so:
            assert torch.equal(so[r], sa[s][r]), (s, r)
    st = a.view(0, "stats", torch.float64).cpu().numpy()
    assert st[TR.S_ROWS] == sizes[0] and st[TR.S_STEPS] == -(-sizes[0] // 8)       # the last epoch's: every window once
    assert not _same(a.adapted_params(0), jobs[0]["model"].engine().params)


# ---- 6. the Python layer and the driver -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,config", [("cnn_gru_attention", "full"), ("cnn_gru", "embedded")])
def test_adapt_entropy_method(kind, config):
    C_, K, T, n = 6, 3, 256, 21
    m = _model(kind, C_, K, config, seed=9)
    x = _x(n, C_, T, 5)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        pred0 = m(x).argmax(dim=1)
    kw = dict(lr=1e-2, epochs=2, diversity=0.5, batch=8)
    out = m.adapt_entropy(x, **kw)
    assert sorted(out) == ["cnn_encoder.1.bias", "cnn_encoder.1.weight", "cnn_encoder.5.bias", "cnn_encoder.5.weight"]
    for k, v in m.state_dict().items():
        assert _same(v, before[k]), k                                             # inplace=False: the model is bit-identical
    assert any(not _same(out[k], before[k]) for k in out)
    again = m.adapt_entropy(x, **kw)
    assert all(_same(out[k], again[k]) for k in out)                              # a function of (weights, x, settings, seed) alone
    other = m.adapt_entropy(x, seed=1, **kw)
    assert any(not _same(out[k], other[k]) for k in out)
    still = m.adapt_entropy(x, lr=0.0, epochs=2, batch=8)
    assert all(_same(still[k], before[k]) for k in still)                         # lr = 0: the model's own bits
    ad = tta.EntropyAdapter([dict(model=m, x=x)], lr=0.0, batch=8)
    (r,) = ad.run()
    assert r["flipped"] == 0 and r["shares"]["before"] == r["shares"]["after"] and r["entropy"]["before"] == r["entropy"]["after"]
    assert set(r) == {"n", "entropy", "shares", "flipped", "objective"} and len(r["objective"]) == 1
    sel = "bn+gate" if kind == "cnn_gru_attention" else "all"
    wide = m.adapt_entropy(x, params=sel, **kw)
    names = {k for k, p in m.named_parameters() if p.numel()}
    assert set(wide) == (set(out) | set(L.GATE_KEYS) if sel == "bn+gate" else names)
    assert all(wide[k].shape == before[k].shape for k in wide)
    loaded = m.adapt_entropy(x, inplace=True, **kw)
    for k, v in m.state_dict().items():
        assert _same(v, loaded[k] if k in loaded else before[k]), k               # inplace=True loads exactly the returned tensors
    with torch.no_grad():
        pred1 = m(x).argmax(dim=1)
    (r2,) = tta.EntropyAdapter([dict(model=KINDS[kind](C_, K, **CONFIGS[config]).to(DEV).eval(), x=x)], **kw).run()
    assert abs(sum(r2["shares"]["after"]) - 1.0) < 1e-9 and pred0.shape == pred1.shape
    with pytest.raises(ValueError):
        m.adapt_entropy(x, params="head")
    with pytest.raises(RuntimeError):
        m.adapt_entropy(x.cpu())


def test_adapter_reports_and_starts_from_given_statistics():
    from multimodalsignal_amd.adapt import BnAdapter
    C_, K, T = 3, 2, 256
    jobs = _jobs([21, 13], C_, K, T)
    bn = BnAdapter([dict(model=j["model"], x=j["x"]) for j in jobs], eval_batch=16)
    plain = tta.EntropyAdapter(jobs, lr=5e-3, batch=8, eval_batch=16).run()
    started = tta.EntropyAdapter([dict(j, bn_state=bn.adapted_state(i).clone()) for i, j in enumerate(jobs)], lr=5e-3, batch=8, eval_batch=16)
    res = started.run()
    for i, (p, r) in enumerate(zip(plain, res)):
        assert set(p) == {"n", "entropy", "shares", "flipped", "objective", "before", "after", "online"}
        assert set(r) == set(p) | {"start"} and set(r["start"]) == {"accuracy", "f1_score", "entropy", "shares"}
        assert r["before"] == p["before"] and r["n"] == jobs[i]["x"].shape[0]        # `before` is the model as it stands, either way
        assert _same(started.view(i, "bn_state", torch.float32), bn.adapted_state(i))    # the statistics it was given, unwritten
        assert len(r["online"]) == 1 and 0.0 <= r["online"][0]["accuracy"] <= 1.0
        assert abs(sum(r["shares"]["after"]) - 1.0) < 1e-9 and 0 <= r["flipped"] <= r["n"]
        assert r["entropy"]["after"] >= 0.0 and np.isfinite(r["objective"]).all()
    with pytest.raises(ValueError):
        tta.EntropyAdapter([jobs[0], dict(model=jobs[1]["model"], x=jobs[1]["x"])])         # labels: all or none


def test_driver_adapts_after_loso(tmp_path, capsys):
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.adapt import SYNTHETIC_NOTE
    from multimodalsignal_amd.synth import make_synthetic_wesad
    subs = ["S2", "S3", "S4"]
    d = make_synthetic_wesad(tmp_path / "w", subjects=subs, windows_per_subject=60, T=256, difficulty=2.0)
    common = ["--synthetic", str(d), "--samples", "256", "--subjects", *subs, "--epochs", "2", "--patience", "1", "--batch-size", "16"]
    M.main(common + ["--adapt-entropy", "1e-3:1:0.5", "--adapt-entropy-batch", "16", "--out", str(tmp_path / "te")])
    M.main(common + ["--adapt-entropy", "1e-3:1:0.5", "--adapt-entropy-batch", "16", "--adapt-entropy-sequential", "--adapt-bn",
                     "--out", str(tmp_path / "both")])
    runs = {k: sorted((tmp_path / k).glob("simple_binary/run_*"))[0] for k in ("te", "both")}
    doc = json.loads((runs["te"] / "entropy_adaptation.json").read_text())
    assert [fo["subject"] for fo in doc["folds"]] == subs and doc["n_folds"] == 3 and doc["note"] == SYNTHETIC_NOTE
    assert doc["settings"] == dict(lr=1e-3, epochs=1, diversity=0.5, params="bn", batch=16, order="shuffled", seed=0)
    txt = (runs["te"] / "entropy_adaptation.txt").read_text(encoding="utf-8")
    assert SYNTHETIC_NOTE in txt and all(s in txt for s in subs) and "mean paired difference" in txt and "not known" in txt
    assert "LOSO acc" in txt and "adapt acc" in txt and "AdaBN acc" not in txt and "predicted-class shares" in txt
    for s, fold in zip(subs, doc["folds"]):
        per = json.loads((runs["te"] / f"fold_test_on_{s}" / "entropy_adaptation_result.json").read_text())
        res = json.loads((runs["te"] / f"fold_test_on_{s}" / "fold_result.json").read_text())
        assert per["before"] == fold["before"] == {"accuracy": res["accuracy"], "f1_score": res["f1_score"]}, s      # the same windows
        assert per["after"] == fold["after"] and per["n"] == fold["n"] == 60 and per["subject"] == s
        assert {"entropy", "shares", "flipped", "objective"} <= set(fold) and "start" not in fold
        assert len(fold["shares"]["after"]) == 2 and len(fold["objective"]) == 1
    both = json.loads((runs["both"] / "entropy_adaptation.json").read_text())
    ad = json.loads((runs["both"] / "adaptation.json").read_text())
    assert both["settings"]["adabn_alpha"] == 1.0
    for fe, fa in zip(both["folds"], ad["folds"]):
        assert fe["before"] == fa["before"]                                           # LOSO
        assert {k: fe["start"][k] for k in ("accuracy", "f1_score")} == fa["after"]   # AdaBN: the column of adaptation.txt
    txt = (runs["both"] / "entropy_adaptation.txt").read_text(encoding="utf-8")
    head = next(l for l in txt.splitlines() if "LOSO acc" in l)
    assert head.index("LOSO acc") < head.index("AdaBN acc") < head.index("adapt acc")
    out = capsys.readouterr().out
    assert "entropy adaptation on 60 unlabelled windows" in out and "Entropy adaptation table written to" in out
