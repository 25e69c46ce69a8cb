"""Window embeddings and the classifier-only head epoch on the MI355X (include/msig_ft.h, models.embed, calibrate.py).

Head epoch against the float64 restatement (tests/ft_reference.py, pinned to torch by tests/test_calibration_host.py):
(a) ONE step — the four gradients its update implies (exp_avg / (1 - beta1) from zero moments) and the loss — under the project's
    gates: gpu_common.grad_tol for classifier.*, FIXED_TOL["loss"], with `own` the float32 run of the restatement;
(b) the parameters after E = 5 epochs: Adam divides by sqrt(v), so an element whose gradient passes through zero turns rounding noise
    into a change of order lr — in ANY fp32 implementation.  The bound is K_GRAD x the float32 restatement's own distance from the
    float64 one on the same case, with the floor PARAM_FLOOR: a parameter is stored once per step, each store rounds by up to 2^-24
    relative, 15-20 stores in a row are 1.2e-6 without any amplification — the project's floor for fp32 stage quantities, 2e-6.
    Measured on the MI355X, 16 cases x 4 tensors: own 3.5e-7 .. 8.5e-3, GPU error 1.2e-8 .. 9.5e-6, GPU error
    over own at most 1.78 (median 0.19).  `own` was never below 3.3e-7, so the floor decided no case.
"""
import ctypes as C
import json
import threading

import numpy as np
import pytest
import torch

import ft_reference as R
from conftest import load_golden_model
from gpu_common import FIXED_TOL, K_GRAD, STAGE_FLOOR, grad_tol, rel_err
from oracle import cnn_gru_oracle as O
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd import calibrate as CAL
from multimodalsignal_amd.models import CnnGruAttentionModel, CnnGruModel
from multimodalsignal_amd.runtime import EmbeddedEngine, Engine, FoldArena
from multimodalsignal_amd.trainer import accuracy_and_weighted_f1

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CONFIGS = {"full": dict(), "embedded": dict(gru_hidden_size=32, gru_num_layers=1)}
KINDS = {"cnn_gru_attention": CnnGruAttentionModel, "cnn_gru": CnnGruModel}
PARAM_FLOOR = STAGE_FLOOR
LR, WD = 1e-3, 1e-4


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int64) if t.dtype == torch.float64 else t)


def _same(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _x(B, C_, T, seed):
    rs = np.random.RandomState(seed)
    x = (rs.randn(B, C_, T) * (0.5 + rs.rand(1, C_, 1)) + rs.randn(1, C_, 1)).astype(np.float32)
    return torch.as_tensor(np.where(np.abs(x) < 1e-3, np.float32(1e-3), x), device=DEV)


def _model(kind, config, C_, K=3, seed=5):
    torch.manual_seed(seed)
    m = KINDS[kind](C_, K, **CONFIGS[config]).to(DEV)
    with torch.no_grad():                        # running statistics away from the initial (0, 1)
        for i, ch in ((1, 16), (5, 32)):
            g = torch.Generator().manual_seed(i)
            m.cnn_encoder[i].running_mean.copy_(torch.rand(ch, generator=g) - 0.5)
            m.cnn_encoder[i].running_var.copy_(0.5 + torch.rand(ch, generator=g))
            m.cnn_encoder[i].num_batches_tracked.fill_(3 + i)
    m.set_dropout_seed(77)
    return m


# ---- embed ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", [1, 3, 6])
@pytest.mark.parametrize("config", ["full", "embedded"])
@pytest.mark.parametrize("kind", ["cnn_gru_attention", "cnn_gru"])
def test_embed_is_the_eval_forwards_feature(kind, config, C_):
    B, T = 21, 512                                # B is not a multiple of 16
    model, x = _model(kind, config, C_), _x(B, C_, T, seed=C_)
    model.eval()
    with torch.no_grad():
        model(x)
    ws = model._engine.region("FEAT", torch.float32, (B, 128)).clone()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    e = model.embed(x)
    assert not e.requires_grad and e.dtype == torch.float32
    if config == "full":
        assert _same(e, ws)
    else:
        assert e.shape == (B, 64) and _same(e, torch.cat([ws[:, :32], ws[:, 64:96]], dim=1))
        assert float(ws[:, 32:64].abs().max()) == 0.0 and float(ws[:, 96:].abs().max()) == 0.0
    assert float(e.abs().max()) > 1e-3
    model.train()
    step = model._step
    e2 = model.embed(x)
    assert _same(e, e2) and model.training and model._step == step            # eval-mode features whatever model.training is
    after = model.state_dict()
    assert set(after) == set(before)
    for k in before:                                                          # parameters, running statistics, num_batches_tracked
        assert _same(before[k], after[k]), k
    with pytest.raises(RuntimeError):
        model.embed(x.cpu())


@pytest.mark.parametrize("kind,layers", [("cnn_gru_attention", 2), ("cnn_gru", 2), ("cnn_gru_attention", 1)])
def test_fold_batched_features_equal_single_model_ones(kind, layers):
    NF, B, C_, K, T = 3, 21, 6, 2, 512
    ar = FoldArena(C_, K, DEV, NF, B, T, gru_hidden=64 if layers == 2 else 32, gru_layers=layers, kind=kind)
    want = []
    engs = [ar.engine(f) for f in range(NF)]
    for f, eng in enumerate(engs):
        x = _x(B, C_, T, seed=30 + f)
        if layers == 2:
            named = {k: v for k, v in O.init_params(C_, K, seed=40 + f).items() if kind == "cnn_gru_attention" or k not in L.GATE_KEYS}
            eng.load_named(named)
            alone = Engine(C_, K, DEV, kind=kind)
            alone.load_named(named)
        else:
            eng.small.normal_(0, 0.1, generator=None)
            eng.scatter()
            alone = EmbeddedEngine(C_, K, DEV, 32, kind=kind)
            alone.small.copy_(eng.small)
        for e_ in (eng, alone):
            e_.bn_state[:16].fill_(0.1 * (f + 1)); e_.bn_state[16:32].fill_(1.5); e_.bn_state[32:64].fill_(-0.2); e_.bn_state[64:].fill_(0.7 + 0.1 * f)
        ar.view(f, "x", torch.float32)[:x.numel()].copy_(x.reshape(-1))
        want.append(alone.features(x))
    got = ar.features([2, 0, 1], B)
    for i, f in enumerate([2, 0, 1]):
        assert _same(got[i], want[f]), f
    assert got.shape == (3, B, 128 if layers == 2 else 64)


# ---- head epoch: a stand-alone harness over the C ABI -----------------------------------------------------------------------------
def _golden_features(name, N, seed):
    """(engine, features (N,128) of N seeded windows through the golden model's extractor, labels with every class present)."""
    meta, params, _ = load_golden_model(name)
    eng = Engine(meta["C"], meta["K"], DEV)
    eng.load_named({k: torch.as_tensor(v) for k, v in params.items()})
    feat = eng.features(_x(N, meta["C"], meta["T"], seed))
    rs = np.random.RandomState(seed + 1)
    y = rs.randint(0, meta["K"], N)
    y[:meta["K"]] = np.arange(meta["K"])
    return eng, feat, y.astype(np.int64)


GOLDEN = {2: "model_c6_k2_t512", 3: "model_c2_k3_t256"}
_cache = {}


def _seeded_features(C_, K, T, N, seed):
    """As _golden_features for a class count no golden file has: the oracle's seeded test weights (C_ channels, K classes)."""
    eng = Engine(C_, K, DEV)
    eng.load_named(O.init_params(C_, K, seed=seed))
    feat = eng.features(_x(N, C_, T, seed))
    y = np.random.RandomState(seed + 1).randint(0, K, N)
    y[:K] = np.arange(K)
    return eng, feat, y.astype(np.int64)


def _case(K, N=48):
    if K not in _cache:
        _cache[K] = _golden_features(GOLDEN[K], N, seed=100 + K) if K in GOLDEN else _seeded_features(6, K, 256, N, seed=100 + K)
    return _cache[K]


class Head:
    """Device buffers of `n` folds (arenas `stride` bytes apart) and the calls on them."""

    def __init__(self, eng, feat, y, n=1, fill=None):
        self.eng, self.K, self.N, self.n = eng, eng.K, int(feat.shape[0]), n
        self.cls = eng.layout[L.P_CLS0_W]
        sizes = [("params", eng.n_flat * 4), ("ea", eng.n_flat * 4), ("eas", eng.n_flat * 4), ("feat", self.N * 512), ("labels", self.N * 8),
                 ("order", 64 * self.N * 4), ("cw", self.K * 4), ("acc", 16)]
        self.off, at = {}, 0
        for name, nb in sizes:
            self.off[name] = (at, nb)
            at += (nb + 255) // 256 * 256
        self.stride = at
        self.mem = torch.zeros((n, at), dtype=torch.uint8, device=DEV)
        for s in range(n):
            self.view(s, "params", torch.float32).copy_(eng.params)
            if fill is not None:                # moments outside the head: arbitrary bits that must survive
                self.view(s, "ea", torch.float32).copy_(fill)
                self.view(s, "eas", torch.float32).copy_(fill.abs())
                o = self.cls
                self.view(s, "ea", torch.float32)[o:].zero_(); self.view(s, "eas", torch.float32)[o:].zero_()
            self.view(s, "feat", torch.float32).copy_(feat.reshape(-1))
            self.view(s, "labels", torch.int64).copy_(torch.as_tensor(y, device=DEV))

    def view(self, s, name, dtype=torch.uint8):
        o, nb = self.off[name]
        return self.mem[s, o:o + nb].view(dtype)

    def ptr(self, name, s=0, extra=0):
        return self.mem.data_ptr() + s * self.stride + self.off[name][0] + extra

    def set_orders(self, s, orders):
        flat = torch.as_tensor(np.asarray(orders, dtype=np.int32).reshape(-1))
        self.view(s, "order", torch.int32)[:flat.numel()].copy_(flat)

    def set_cw(self, s, cw):
        self.view(s, "cw", torch.float32).copy_(torch.as_tensor(np.asarray(cw, dtype=np.float32)))

    def desc(self, s, epoch, n_order, batch, first_step, n_steps, thr, cw, lr=LR, wd=WD, step0=1, seed=0, eps=1e-8):
        h = L.FtHead()
        h.K, h.N, h.n_order, h.batch, h.first_step, h.n_steps, h.dropout_thr = self.K, self.N, n_order, batch, first_step, n_steps, thr
        h.cls_offset, h.step0, h.seed = self.cls, step0, seed
        h.lr, h.beta1, h.beta2, h.eps, h.weight_decay = lr, 0.9, 0.999, eps, wd
        h.feat, h.labels, h.order = self.ptr("feat", s), self.ptr("labels", s), self.ptr("order", s, epoch * n_order * 4)
        h.params, h.exp_avg, h.exp_avg_sq = self.ptr("params", s), self.ptr("ea", s), self.ptr("eas", s)
        h.class_weight = self.ptr("cw", s) if cw else None
        h.loss_acc = self.ptr("acc", s)
        return h

    def call(self, h, stream=None):
        st = C.c_void_p((stream or torch.cuda.current_stream(DEV)).cuda_stream)
        L.check(L.lib().msig_ft_head_epoch(C.byref(h), st), "msig_ft_head_epoch")

    def call_multi(self, h, slots, lrs, step0s, seeds, stream=None):
        m = L.FtMulti()
        m.n, m.stride_bytes = len(slots), self.stride
        for i, s in enumerate(slots):
            m.slot[i], m.lr[i], m.step0[i], m.seed[i] = s, lrs[i], step0s[i], seeds[i]
        st = C.c_void_p((stream or torch.cuda.current_stream(DEV)).cuda_stream)
        L.check(L.lib().msig_ft_head_epoch_multi(C.byref(h), C.byref(m), st), "msig_ft_head_epoch_multi")

    def epochs(self, s, orders, batch, thr, cw, seed=0, multi=None, **kw):
        """Every row of `orders` as one call (one epoch), step counts continued."""
        n = orders.shape[1]
        spe = (n + batch - 1) // batch
        for e in range(orders.shape[0]):
            self.call(self.desc(s, e, n, batch, 0, spe, thr, cw, step0=e * spe + 1, seed=seed, **kw))

    def head(self, s, which="params"):
        flat = self.view(s, which, torch.float32)
        v = self.eng.named_param_views(flat)
        return {k: v[k].detach().cpu().numpy().astype(np.float64) for k in R.HEAD_KEYS}

    def snapshot(self, s):
        return {k: self.view(s, k).clone() for k in ("params", "ea", "eas", "acc")}


def _head0(eng):
    return {k: eng.named_param_views()[k].detach().cpu().numpy() for k in R.HEAD_KEYS}


CW = {2: [0.6, 2.5], 3: [0.5, 2.0, 1.25], 16: [0.5, 2.0, 1.25, 0.3, 1.0, 3.5, 0.8, 1.6, 0.25, 2.75, 1.1, 0.6, 4.0, 0.9, 1.4, 0.7]}      # 16 = MSIG_MAX_K
SEED = 0x5EED0123456789


def _one_step(K, thr, cw, reference_wrong=None):
    """{name: (error, tolerance)} of ONE step of 16 rows against the float64 restatement (optionally a deliberately wrong one)."""
    eng, feat, y = _case(K)
    order = np.random.RandomState(3).permutation(48)[:16]
    hd = Head(eng, feat, y)
    hd.set_orders(0, order[None])
    if cw:
        hd.set_cw(0, CW[K])
    hd.call(hd.desc(0, 0, 16, 16, 0, 1, thr, cw, wd=0.0, seed=SEED))
    torch.cuda.synchronize()
    f64 = feat.cpu().numpy().astype(np.float64)
    args = dict(idx=order, t=1, lr=LR, weight_decay=0.0, cw=CW[K] if cw else None, thr=thr, seed=SEED)
    s64, s32 = R.init_state(_head0(eng), np.float64), R.init_state(_head0(eng), np.float32)
    l64, c64, g64 = R.step(s64, f64, y, dtype=np.float64, wrong=reference_wrong, **args)
    l32, _, g32 = R.step(s32, f64, y, dtype=np.float32, wrong=reference_wrong, **args)      # `own` of the SAME restatement
    got_m = hd.head(0, "ea")
    rep = {}
    for k in R.HEAD_KEYS:
        got = R.implied_gradient(got_m[k], 0.0)
        rep[k] = (rel_err(got, g64[k]), grad_tol(k, rel_err(g32[k], g64[k])))
    acc = hd.view(0, "acc", torch.float64).cpu().numpy()
    rep["loss"] = (abs(acc[0] / 16 - l64 / 16) / max(abs(l64 / 16), 1e-6), FIXED_TOL["loss"])
    rep["correct"] = (abs(acc[1] - c64), 0.0)
    return rep


@pytest.mark.parametrize("cw", [False, True])
@pytest.mark.parametrize("thr", [0, 128])
@pytest.mark.parametrize("K", [2, 3, 16])
def test_one_step_gradients_and_loss(K, thr, cw):
    rep = _one_step(K, thr, cw)
    for k, (err, tol) in rep.items():
        print(f"K={K} thr={thr} cw={cw} {k}: err {err:.3e} tol {tol:.3e}")
    bad = {k: v for k, v in rep.items() if not v[0] <= v[1]}
    assert not bad, bad


@pytest.mark.parametrize("wrong", ["no_dropout_scale"])
def test_negative_control_a_wrong_head_fails_the_one_step_gate(wrong):
    """The gate of test_one_step_gradients_and_loss against a restatement WITHOUT dropout's 1 / (1 - p): every gradient is off by a
    factor of two or four and the loss moves — the gate sees a wrong head."""
    rep = _one_step(2, 128, False, reference_wrong=wrong)
    bad = {k for k, (err, tol) in rep.items() if not err <= tol}
    print(rep)
    assert {"classifier.0.weight", "classifier.3.weight", "loss"} <= bad


@pytest.mark.parametrize("cw", [False, True])
@pytest.mark.parametrize("thr", [0, 128])
@pytest.mark.parametrize("batch", [16, 20])           # 20: a short last step of 8 rows
@pytest.mark.parametrize("K", [2, 3, 16])
def test_parameters_after_five_epochs(K, batch, thr, cw):
    E, N = 5, 48
    eng, feat, y = _case(K)
    orders = CAL.epoch_orders(N, E, seed=17 + K)
    hd = Head(eng, feat, y)
    hd.set_orders(0, orders)
    if cw:
        hd.set_cw(0, CW[K])
    hd.epochs(0, orders, batch, thr, cw, seed=SEED)
    torch.cuda.synchronize()
    f64 = feat.cpu().numpy().astype(np.float64)
    kw = dict(batch=batch, lr=LR, weight_decay=WD, cw=CW[K] if cw else None, thr=thr, seed=SEED)
    s64, l64 = R.epochs(_head0(eng), f64, y, orders, dtype=np.float64, **kw)
    s32, _ = R.epochs(_head0(eng), f64, y, orders, dtype=np.float32, **kw)
    got = hd.head(0)
    bad = {}
    for k in R.HEAD_KEYS:
        own, err = rel_err(s32["p"][k], s64["p"][k]), rel_err(got[k], s64["p"][k])
        tol = max(PARAM_FLOOR, K_GRAD * own)
        print(f"K={K} batch={batch} thr={thr} cw={cw} {k}: own {own:.3e} gpu {err:.3e} tol {tol:.3e}")
        if not err <= tol:
            bad[k] = (err, tol)
        assert rel_err(got[k], _head0(eng)[k]) > 1e-3                         # it trained
    loss = hd.view(0, "acc", torch.float64).cpu().numpy()[0]
    assert abs(loss - sum(l64)) / sum(l64) < 1e-4
    assert not bad, bad


# ---- bit-exact properties ---------------------------------------------------------------------------------------------------------
def _fill(eng, seed=9):
    return torch.randn(eng.n_flat, generator=torch.Generator().manual_seed(seed)).to(DEV)


@pytest.mark.parametrize("K,cw", [(2, True), (3, False)])
def test_one_call_of_s_steps_equals_s_calls_of_one_step(K, cw):
    eng, feat, y = _case(K)
    N, batch, thr = 48, 20, 128
    orders = CAL.epoch_orders(N, 2, seed=5)
    a, b = Head(eng, feat, y, fill=_fill(eng)), Head(eng, feat, y, fill=_fill(eng))
    for hd in (a, b):
        hd.set_orders(0, orders); hd.set_cw(0, CW[K])
    a.epochs(0, orders, batch, thr, cw, seed=SEED)
    for e in range(2):
        for s in range(3):
            b.call(b.desc(0, e, N, batch, s, 1, thr, cw, step0=e * 3 + s + 1, seed=SEED))
    torch.cuda.synchronize()
    sa, sb = a.snapshot(0), b.snapshot(0)
    for k in sa:
        assert _same(sa[k], sb[k]), k
    # nothing outside the four classifier tensors moved, in any of the three flat buffers
    o = eng.layout[L.P_CLS0_W]
    assert _same(a.view(0, "params", torch.float32)[:o], eng.params[:o])
    assert _same(a.view(0, "ea", torch.float32)[:o], _fill(eng)[:o]) and _same(a.view(0, "eas", torch.float32)[:o], _fill(eng).abs()[:o])
    assert not _same(a.view(0, "params", torch.float32)[o:], eng.params[o:])
    assert _same(a.view(0, "feat"), b.view(0, "feat")) and _same(a.view(0, "feat", torch.float32), feat.reshape(-1))


def test_fold_batch_equals_single_calls_and_leaves_other_arenas_alone():
    K, N, batch, thr = 2, 48, 16, 128
    eng, feat, y = _case(K)
    slots, lrs, seeds, step0s = [2, 0, 3], [1e-3, 3e-3, 5e-4], [11, 12, SEED], [1, 4, 9]
    multi, single = Head(eng, feat, y, n=4, fill=_fill(eng)), Head(eng, feat, y, n=4, fill=_fill(eng))
    for hd in (multi, single):
        for s in range(4):
            hd.set_orders(s, CAL.epoch_orders(N, 1, seed=50 + s))
            hd.set_cw(s, [1.0 + 0.1 * s, 2.0])
            hd.view(s, "params", torch.float32)[hd.cls:].mul_(1.0 + 0.01 * s)          # folds differ in their heads too
    untouched = multi.mem[1].clone()
    multi.call_multi(multi.desc(0, 0, N, batch, 0, 3, thr, True), slots, lrs, step0s, seeds)
    for s, lr, sd, s0 in zip(slots, lrs, seeds, step0s):
        single.call(single.desc(s, 0, N, batch, 0, 3, thr, True, lr=lr, step0=s0, seed=sd))
    torch.cuda.synchronize()
    for s in slots:
        for k, v in multi.snapshot(s).items():
            assert _same(v, single.snapshot(s)[k]), (s, k)
    assert torch.equal(multi.mem[1], untouched)
    assert not torch.equal(multi.mem[2], single.mem[1])


def test_all_ones_class_weights_equal_no_class_weights():
    K = 3
    eng, feat, y = _case(K)
    orders = CAL.epoch_orders(48, 2, seed=8)
    a, b = Head(eng, feat, y), Head(eng, feat, y)
    for hd in (a, b):
        hd.set_orders(0, orders)
    b.set_cw(0, [1.0] * K)
    a.epochs(0, orders, 20, 128, False, seed=SEED)
    b.epochs(0, orders, 20, 128, True, seed=SEED)
    torch.cuda.synchronize()
    for k, v in a.snapshot(0).items():
        assert _same(v, b.snapshot(0)[k]), k


def test_same_bits_again_and_beside_a_busy_second_stream():
    K, N = 2, 48
    eng, feat, y = _case(K)
    orders = CAL.epoch_orders(N, 4, seed=21)

    def run(stream):
        hd = Head(eng, feat, y)
        hd.set_orders(0, orders)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            hd.epochs(0, orders, 16, 128, False, seed=SEED)
        stream.synchronize()
        return hd.snapshot(0)

    want = run(torch.cuda.Stream(DEV))
    again = run(torch.cuda.Stream(DEV))
    for k in want:
        assert _same(want[k], again[k]), k
    xb = _x(64, eng.C, 512, seed=1)
    yb = torch.zeros(64, dtype=torch.int64, device=DEV)
    other = Engine(eng.C, K, DEV)
    other.load_named({k: v for k, v in O.init_params(eng.C, K, seed=2).items()})
    stop = threading.Event()

    def noise():
        with torch.cuda.stream(torch.cuda.Stream(DEV)):
            k = 0
            while not stop.is_set() and k < 400:
                k += 1
                other.train_step(xb, yb, LR, step=k, dropout_p=0.5, seed=1)
            torch.cuda.current_stream(DEV).synchronize()

    th = threading.Thread(target=noise)
    th.start()
    try:
        busy = run(torch.cuda.Stream(DEV))
    finally:
        stop.set()
        th.join()
    for k in want:
        assert _same(want[k], busy[k]), k


def test_embedded_heads_padded_columns_stay_exactly_zero():
    C_, K, N = 3, 2, 32
    torch.manual_seed(4)
    model = CnnGruAttentionModel(C_, K, **CONFIGS["embedded"]).to(DEV)
    eng = model.engine()
    eng.scatter()
    feat = eng.features(_x(N, C_, 512, seed=6), padded=True)
    assert float(feat[:, 32:64].abs().max()) == 0.0 and float(feat[:, 96:].abs().max()) == 0.0
    y = np.arange(N) % K
    hd = Head(eng, feat, y)
    orders = CAL.epoch_orders(N, 3, seed=2)
    hd.set_orders(0, orders)
    hd.epochs(0, orders, 16, 128, False, seed=SEED)
    torch.cuda.synchronize()
    for which in ("params", "ea", "eas"):
        w0 = eng.named_param_views(hd.view(0, which, torch.float32))["classifier.0.weight"]
        assert float(w0[:, 32:64].abs().max()) == 0.0 and float(w0[:, 96:].abs().max()) == 0.0, which
        assert float(w0[:, :32].abs().max()) > 0.0
    assert _same(hd.view(0, "params", torch.float32)[eng.padding], eng.params[eng.padding])


# ---- launches ---------------------------------------------------------------------------------------------------------------------
def _launches(fn):
    torch.cuda.synchronize()
    L.profile_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        return L.profile_report()
    finally:
        L.profile_enable(False)


def test_one_launch_per_head_epoch_call():
    K, N = 2, 48
    eng, feat, y = _case(K)
    hd = Head(eng, feat, y, n=3)
    for s in range(3):
        hd.set_orders(s, CAL.epoch_orders(N, 1, seed=s))
    one = _launches(lambda: hd.call(hd.desc(0, 0, N, 16, 0, 3, 128, False)))
    assert {k: c for k, (c, _) in one.items()} == {"head_epoch": 1}
    many = _launches(lambda: hd.call_multi(hd.desc(0, 0, N, 16, 0, 3, 128, False), [0, 1, 2], [LR] * 3, [1] * 3, [1, 2, 3]))
    assert {k: c for k, (c, _) in many.items()} == {"head_epoch": 1}
    x = _x(8, eng.C, 512, seed=3)
    ft = _launches(lambda: eng.features(x))
    fw = _launches(lambda: eng.forward(x, None, training=False))
    assert "head_fwd" not in ft and "head_fwd" in fw and ft.get("ft_feat_copy", (0,))[0] == 1


# ---- HeadCalibrator and the driver --------------------------------------------------------------------------------------------------
def test_head_calibrator_leaves_the_model_alone_and_batched_equals_sequential():
    C_, K, T = 3, 2, 256
    jobs = []
    for f, kind in enumerate(["cnn_gru_attention", "cnn_gru_attention", "cnn_gru_attention"]):
        model = _model(kind, "full", C_, K=K, seed=20 + f)
        rs = np.random.RandomState(f)
        n_cal = 16 if f < 2 else 12                      # folds of unequal calibration size do not share a launch
        jobs.append(dict(model=model, x_cal=_x(n_cal, C_, T, 60 + f), y_cal=torch.as_tensor(np.arange(n_cal) % K, device=DEV),
                         x_eval=_x(40, C_, T, 70 + f), y_eval=torch.as_tensor(rs.randint(0, K, 40), device=DEV), lr=1e-2, seed=5 + f,
                         shuffle_seed=9 + f, class_weight=[1.0, 2.0] if f == 1 else None))
    before = [{k: v.clone() for k, v in j["model"].state_dict().items()} for j in jobs]
    a = CAL.HeadCalibrator(jobs, epochs=6, batch_size=8, weight_decay=WD, batched=True)
    ra = a.run()
    b = CAL.HeadCalibrator(jobs, epochs=6, batch_size=8, weight_decay=WD, batched=False)
    rb = b.run()
    assert ra == rb
    for s in range(3):
        assert _same(a.tuned_flat(s), b.tuned_flat(s))
        o = a.cls_offset
        assert _same(a.tuned_flat(s)[:o], jobs[s]["model"].engine().params[:o]) and not _same(a.tuned_flat(s)[o:], jobs[s]["model"].engine().params[o:])
        for k, v in jobs[s]["model"].state_dict().items():
            assert _same(v, before[s][k]), k
        r = ra[s]
        assert r["n_cal"] == (16 if s < 2 else 12) and r["n_eval"] == 40 and len(r["train_loss"]) == 6
        assert r["train_loss"][-1] < r["train_loss"][0]
        # `before` is the model's own eval forward on the remainder
        m = jobs[s]["model"].eval()
        with torch.no_grad():
            pred = m(jobs[s]["x_eval"]).argmax(dim=1).cpu().numpy()
        acc, f1 = accuracy_and_weighted_f1(jobs[s]["y_eval"].cpu().numpy(), pred)
        assert (r["before"]["accuracy"], r["before"]["f1_score"]) == (acc, f1)
        st = a.tuned_state(s)
        assert st["classifier.0.weight"].shape == (64, 128) and st["classifier.3.weight"].shape == (K, 64)
    with pytest.raises(RuntimeError):
        a.run()


def _fold_results(run, subs):
    out = {}
    for s in subs:
        info = json.loads((run / f"fold_test_on_{s}" / "fold_result.json").read_text())
        hist = [{k: v for k, v in h.items() if k != "seconds"} for h in info["history"]]
        out[s] = (info["accuracy"], info["f1_score"], info["epochs"], hist)
    return out


def _loso_part(text):
    return text[:text.index("LOSO wall-clock")]


def test_driver_calibrates_after_loso(tmp_path, capsys):
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.dataset import WesadDataset
    from multimodalsignal_amd.synth import CHANNELS6, make_synthetic_wesad
    subs = ["S2", "S3", "S4", "S5"]
    d = make_synthetic_wesad(tmp_path / "w", subjects=subs, windows_per_subject=150, T=256, difficulty=2.0)
    common = ["--synthetic", str(d), "--samples", "256", "--subjects", *subs, "--epochs", "2", "--patience", "1", "--batch-size", "16"]
    cal = ["--calibrate", "8", "--calibration-epochs", "5", "--calibration-lr", "0.01"]
    M.main(common + cal + ["--out", str(tmp_path / "cal")])
    M.main(common + ["--out", str(tmp_path / "plain")])
    M.main(common + cal + ["--calibration-sequential", "--out", str(tmp_path / "seq")])
    M.main(common + cal + ["--concurrent-folds", "1", "--out", str(tmp_path / "one")])
    runs = {k: sorted((tmp_path / k).glob("simple_binary/run_*"))[0] for k in ("cal", "plain", "seq", "one")}
    # the LOSO part of the run is what it is without the flag
    assert _loso_part((runs["cal"] / "cv_summary.txt").read_text(encoding="utf-8")) == _loso_part((runs["plain"] / "cv_summary.txt").read_text(encoding="utf-8"))
    assert _fold_results(runs["cal"], subs) == _fold_results(runs["plain"], subs) == _fold_results(runs["one"], subs)
    assert not (runs["plain"] / "calibration.json").exists() and not (runs["plain"] / "fold_test_on_S2" / "calibration_result.json").exists()
    doc = json.loads((runs["cal"] / "calibration.json").read_text())
    assert [f["subject"] for f in doc["folds"]] == subs and doc["n_folds"] == 4 and "synthetic" in doc["note"]
    assert doc["settings"] == {"windows_per_class": 8, "gap": 5, "epochs": 5, "lr": 0.01, "batch_size": 16, "weight_decay": M.WEIGHTS_DECAY}
    txt = (runs["cal"] / "calibration.txt").read_text(encoding="utf-8")
    assert CAL.SYNTHETIC_NOTE in txt and all(s in txt for s in subs) and "mean paired difference" in txt
    # fold-batched == sequential == the folds trained one after the other, bit for bit (JSON round-trips doubles exactly)
    for other in ("seq", "one"):
        assert json.loads((runs[other] / "calibration.json").read_text())["folds"] == doc["folds"], other
    with open(d / "_channel_names.txt") as f:
        names = [ln.strip() for ln in f if ln.strip()]
    for s, fold in zip(subs, doc["folds"]):
        per = json.loads((runs["cal"] / f"fold_test_on_{s}" / "calibration_result.json").read_text())
        assert per["before"] == fold["before"] and per["after"] == fold["after"] and per["n_cal"] == fold["n_cal"] == 16
        assert len(per["train_loss"]) == 5
        # an independent evaluation of best_model.pt on the remainder indices
        ds = WesadDataset(d, [s], list(CHANNELS6), names, classification_mode="stress_binary")
        cal_idx, eval_idx = CAL.calibration_split(ds.labels, 8, 5)
        assert fold["n_eval"] == eval_idx.size
        model = CnnGruAttentionModel(6, 2).to(DEV)
        model.load_state_dict(torch.load(runs["cal"] / f"fold_test_on_{s}" / "best_model.pt", weights_only=True))
        model.eval()
        x, y = ds.device_tensors(DEV)
        with torch.no_grad():
            pred = model(x[torch.as_tensor(eval_idx, device=DEV)]).argmax(dim=1).cpu().numpy()
        acc, f1 = accuracy_and_weighted_f1(np.asarray(ds.labels)[eval_idx], pred)
        assert (fold["before"]["accuracy"], fold["before"]["f1_score"]) == (acc, f1), s
    out = capsys.readouterr().out
    assert "calibration on 16 windows" in out


def test_driver_calibrates_both_kinds_of_a_comparison_run(tmp_path):
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.synth import make_synthetic_wesad
    subs = ["S2", "S3", "S4"]
    d = make_synthetic_wesad(tmp_path / "w", subjects=subs, windows_per_subject=150, T=256, difficulty=2.0)
    M.main(["--synthetic", str(d), "--samples", "256", "--subjects", *subs, "--epochs", "2", "--patience", "1", "--batch-size", "16",
            "--model", "cnn_gru_attention", "cnn_gru", "--class-weights", "balanced", "--calibrate", "8", "--calibration-epochs", "3",
            "--out", str(tmp_path / "o")])
    (run,) = sorted((tmp_path / "o").glob("simple_binary/run_*"))
    assert (run / "comparison.json").exists()
    for kind in ("cnn_gru_attention", "cnn_gru"):
        doc = json.loads((run / kind / "calibration.json").read_text())
        assert [f["subject"] for f in doc["folds"]] == subs and doc["settings"]["epochs"] == 3
        for f in doc["folds"]:
            assert f["n_cal"] == 16 and 0.0 <= f["after"]["accuracy"] <= 1.0
            assert (run / kind / f"fold_test_on_{f['subject']}" / "calibration_result.json").exists()
