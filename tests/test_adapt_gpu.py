"""Label-free BatchNorm adaptation on the MI355X (include/msig_ab.h, adapt.BnAdapter, model.adapt_bn, --adapt-bn).

Shapes are small: T = 256 (L1 = 128, L2 = 32), N = 37 windows in batches of 16 (16, 16 and a ragged 5), C = 2 (gate hidden width 0:
the gate is the constant 0.5) and C = 6.  Weights are O.init_params, the source statistics the defaults (mean 0, variance 1), and the
inputs carry a per-channel gain and offset, so the target statistics are far from the source's.

The gate (`_gate`): every adapted tensor against the float64 restatement tests/ab_reference.py, error gpu_common.rel_err, bound
gpu_common.stage_tol(name, own) with `own` the float32 mode of the SAME restatement against its float64 mode.
"""
import ctypes as C
import json
import threading

import numpy as np
import pytest
import torch

import ab_reference as R
import input_regimes as IR
from gpu_common import rel_err, stage_tol
from oracle import cnn_gru_oracle as O
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd import adapt as A
from multimodalsignal_amd.models import CnnGruAttentionModel, CnnGruModel
from multimodalsignal_amd.runtime import Engine

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KINDS = {"cnn_gru_attention": CnnGruAttentionModel, "cnn_gru": CnnGruModel}
T, N, K = 256, 37, 2
CUTS = {16: [16, 16, 5], 37: [37], 32: [32, 5]}


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int64) if t.dtype == torch.float64 else t)


def _same(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _x_host(C_, seed, n=N, regime=None):
    """Windows with a per-channel gain in [1.5, 3] and offset in [-1, 1] (numpy), optionally moved into an input regime
    (tests/input_regimes.py)."""
    rs = np.random.RandomState(seed)
    x = rs.randn(n, C_, T) * (1.5 + 1.5 * rs.rand(1, C_, 1)) + (2.0 * rs.rand(1, C_, 1) - 1.0)
    x = x.astype(np.float32)
    return x if regime is None else IR.apply(x, regime, signs=IR.case_signs(regime, n, C_, T))


def _x(C_, seed, n=N, regime=None):
    return torch.as_tensor(_x_host(C_, seed, n, regime), device=DEV)


def _named(kind, C_, seed, layers=2):
    named = O.init_params(C_, K, seed=seed, hidden=64 if layers == 2 else 32, layers=layers)
    return {k: v for k, v in named.items() if kind == "cnn_gru_attention" or k not in L.GATE_KEYS}


def _model(kind, C_, seed, layers=2):
    cfg = {} if layers == 2 else dict(gru_hidden_size=32, gru_num_layers=1)
    m = KINDS[kind](C_, K, **cfg)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in _named(kind, C_, seed, layers).items()}, strict=False)
    return m.to(DEV).eval()


def _engine(kind, C_, seed):
    eng = Engine(C_, K, DEV, kind=kind)
    eng.load_named(_named(kind, C_, seed))
    return eng


# ---- a stand-alone harness over the C ABI -------------------------------------------------------------------------------------------
class Arena:
    """Device buffers of `n` models (arenas `stride` bytes apart) of one kind and C, and the msig_ab calls on them."""

    def __init__(self, kind, C_, n=1, max_b=N):
        self.kind, self.C, self.n = kind, C_, n
        self.n_flat = L.param_layout(C_, K, kind)[-1]
        self.ws_bytes = max(L.workspace_layout(b, C_, T, K, False)[-1] for b in range(1, max_b + 1))      # the EVALUATION layout
        sizes = [("params", self.n_flat * 4), ("bn_state", 96 * 4), ("bn_count", 16), ("x", max_b * C_ * T * 4), ("ws", self.ws_bytes),
                 ("ab", L.AB_ACC_DOUBLES * 8), ("bn_dst", 96 * 4)]
        self.off, at = {}, 0
        for name, nb in sizes:
            self.off[name] = (at, nb)
            at += (nb + 255) // 256 * 256
        self.stride = at
        self.mem = torch.zeros((n, at), dtype=torch.uint8, device=DEV)

    def view(self, s, name, dtype=torch.uint8):
        o, nb = self.off[name]
        return self.mem[s, o:o + nb].view(dtype)

    def ptr(self, name, s=0):
        return self.mem.data_ptr() + s * self.stride + self.off[name][0]

    def load(self, s, eng, bn_state=None, bn_count=(3, 7)):
        self.view(s, "params", torch.float32).copy_(eng.params)
        self.view(s, "bn_state", torch.float32).copy_(eng.bn_state if bn_state is None else bn_state)
        self.view(s, "bn_count", torch.int64)[:2].copy_(torch.as_tensor(bn_count))
        self.view(s, "ab").zero_()

    @staticmethod
    def _st():
        return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)

    def desc(self, B, s=0):
        b = L.Batch()
        b.shape = L.Shape(B, self.C, T, K)
        b.training, b.bn_momentum, b.bn_eps = 0, 0.1, 1e-5
        b.x, b.params = self.ptr("x", s), self.ptr("params", s)
        b.bn_state, b.bn_count = self.ptr("bn_state", s), self.ptr("bn_count", s)
        b.ws, b.ws_bytes = self.ptr("ws", s), self.ws_bytes
        b.gru_layers = 2
        return b

    def multi(self, slots):
        m = L.Multi()
        m.n, m.stride_bytes = len(slots), self.stride
        for i, s in enumerate(slots):
            m.slot[i] = s
        return m

    def put_x(self, s, xb):
        self.view(s, "x", torch.float32)[:xb.numel()].copy_(xb.reshape(-1))

    def accumulate(self, s, xb, stage):
        self.put_x(s, xb)
        L.check(L.lib().msig_ab_accumulate(C.byref(self.desc(xb.shape[0], s)), L.FT_KINDS[self.kind], stage, self.ptr("ab", s), self._st()),
                "msig_ab_accumulate")

    def accumulate_multi(self, slots, xbs, stage):
        for s, xb in zip(slots, xbs):
            self.put_x(s, xb)
        L.check(L.lib().msig_ab_accumulate_multi(C.byref(self.desc(xbs[0].shape[0])), C.byref(self.multi(slots)), L.FT_KINDS[self.kind], stage,
                                                 self.ptr("ab"), self._st()), "msig_ab_accumulate_multi")

    def commit(self, s, stage, alpha, dst="bn_state"):
        L.check(L.lib().msig_ab_commit(self.ptr("ab", s), stage, alpha, self.ptr("bn_state", s), self.ptr(dst, s), self._st()), "msig_ab_commit")

    def commit_multi(self, slots, stage, alpha, dst="bn_state"):
        L.check(L.lib().msig_ab_commit_multi(self.ptr("ab"), stage, alpha, self.ptr("bn_state"), self.ptr(dst), C.byref(self.multi(slots)),
                                             self._st()), "msig_ab_commit_multi")

    def adapt(self, s, x, cuts, alpha=1.0):
        """The whole protocol with single calls, in place on arena s's bn_state."""
        for stage in (1, 2):
            i = 0
            for b in cuts:
                self.accumulate(s, x[i:i + b], stage)
                i += b
            self.commit(s, stage, alpha)

    def adapt_multi(self, slots, xs, cuts, alpha=1.0):
        for stage in (1, 2):
            i = 0
            for b in cuts:
                self.accumulate_multi(slots, [x[i:i + b] for x in xs], stage)
                i += b
            self.commit_multi(slots, stage, alpha)

    def state(self, s, name="bn_state"):
        return self.view(s, name, torch.float32).clone()


# ---- 1. stage-1 bits against the training forward -------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", [2, 6])
@pytest.mark.parametrize("m", [0.1, 1.0])
def test_stage_one_equals_the_training_forwards_running_statistics_bit_for_bit(m, C_):
    """One batch, alpha = m: what a training-mode msig_frontend_fwd with bn_momentum = m writes into rm1 / rv1 from the same source."""
    eng, x = _engine("cnn_gru_attention", C_, seed=10 + C_), _x(C_, seed=C_)
    src = eng.bn_state.clone()
    ar = Arena("cnn_gru_attention", C_)
    ar.load(0, eng)
    ar.accumulate(0, x, 1)
    ar.commit(0, 1, m)
    b = eng._batch(x, None, True, 0.0, 0, 0)
    b.bn_momentum = m
    eng.stage("frontend_fwd", b)
    torch.cuda.synchronize()
    got = ar.state(0)
    assert _same(got[:32], eng.bn_state[:32])
    assert _same(got[32:], src[32:]) and not _same(got[:32], src[:32])
    acc = ar.view(0, "ab", torch.float64).cpu().numpy()
    assert acc[L.AB_N1] == N * 128 and acc[L.AB_N2] == 0 and not acc[L.AB_SUM2:].any()


# ---- 2.-4. both stages against the float64 restatement ----------------------------------------------------------------------------------
_refs, _adapted = {}, {}


def _reference(kind, C_, layers, wrong=None, regime=None):
    """(float64 restatement, `own` of every tensor) of the case, computed once (batches of 16: it does not depend on the batching,
    tests/test_adapt_host.py)."""
    key = (kind, C_, layers, wrong, regime)
    if key not in _refs:
        named, x = _named(kind, C_, 20 + C_, layers), torch.as_tensor(_x_host(C_, seed=30 + C_, regime=regime))
        r64 = R.adapt(named, O.init_buffers(), x, batch=16, kind=kind, wrong=wrong)
        r32 = R.adapt(named, O.init_buffers(), x, batch=16, kind=kind, wrong=wrong, dtype=torch.float32)
        _refs[key] = ({k: v.numpy() for k, v in r64.items()}, {k: rel_err(r32[k].numpy(), r64[k].numpy()) for k in R.KEYS})
    return _refs[key]


def _gpu(kind, C_, layers, batch, regime=None):
    key = (kind, C_, layers, batch, regime)
    if key not in _adapted:
        model, x = _model(kind, C_, 20 + C_, layers), _x(C_, seed=30 + C_, regime=regime)
        ad = A.BnAdapter([dict(model=model, x=x)], alpha=1.0, eval_batch=batch)
        assert [b for _, b, _ in A.batch_plan(ad.sizes, ad.batch)] == CUTS[batch]
        _adapted[key] = {k: v.cpu().numpy() for k, v in ad.adapted_buffers(0).items()}
    return _adapted[key]


def _gate(kind, C_, layers=2, batch=16, wrong=None, regime=None):
    """{tensor: (error, tolerance)} of the adapted statistics against the restatement (optionally a deliberately wrong one)."""
    ref, own = _reference(kind, C_, layers, wrong, regime)
    got = _gpu(kind, C_, layers, batch, regime)
    rep = {k: (rel_err(got[k], ref[k]), stage_tol(k, own[k])) for k in R.KEYS}
    for k, (err, tol) in rep.items():
        print(f"{kind} C={C_} layers={layers} batch={batch} wrong={wrong} regime={regime} {k}: own {own[k]:.3e} gpu {err:.3e} tol {tol:.3e}")
    return rep


CASES = [("cnn_gru_attention", 2, 2), ("cnn_gru_attention", 6, 2), ("cnn_gru", 2, 2), ("cnn_gru", 6, 2), ("cnn_gru_attention", 6, 1)]


# the same gate on windows whose channels sit 10 spreads from zero (tests/input_regimes.py "offset"): msig_ab_accumulate reduces the
# conv kernels' BatchNorm partials.  tests/test_input_regimes_host.py asserts, on the host, that this case's `own` stays under OWN_CAP.
REGIME_CASES = [IR.ADAPT_CASE]


@pytest.mark.parametrize("kind,C_,layers,regime", [(*c, None) for c in CASES] + REGIME_CASES,
                         ids=["-".join(map(str, c)) for c in CASES] + ["-".join(map(str, c)) for c in REGIME_CASES])
def test_both_stages_against_the_float64_restatement(kind, C_, layers, regime):
    rep = _gate(kind, C_, layers, regime=regime)
    bad = {k: v for k, v in rep.items() if not v[0] <= v[1]}
    assert not bad, bad
    ref, _ = _reference(kind, C_, layers, regime=regime)
    src = O.init_buffers()
    for k in R.KEYS:                                   # the target statistics are far from the source's
        assert rel_err(src[k].numpy(), ref[k]) > 0.2, k


@pytest.mark.parametrize("wrong", ["biased", "source_bn1"])
@pytest.mark.parametrize("kind,C_,layers", CASES)
def test_negative_controls_fail_the_gate(kind, C_, layers, wrong):
    """The same gate against a restatement with the BIASED variance (off by 1 / n: 2e-4 at n1 = 37 x 128, 8e-4 at n2 = 37 x 32) and
    against one whose stage 2 runs under the SOURCE BatchNorm-1 statistics: the gate sees both."""
    rep = _gate(kind, C_, layers, wrong=wrong)
    bad = {k for k, (err, tol) in rep.items() if not err <= tol}
    if wrong == "biased":
        assert {R.KEYS[1], R.KEYS[3]} <= bad, rep
    else:
        assert {R.KEYS[2], R.KEYS[3]} & bad, rep


@pytest.mark.parametrize("batch", [16, 37, 32])
@pytest.mark.parametrize("kind,C_", [("cnn_gru_attention", 6), ("cnn_gru", 2)])
def test_every_batching_passes_the_gate(kind, C_, batch):
    rep = _gate(kind, C_, batch=batch)
    bad = {k: v for k, v in rep.items() if not v[0] <= v[1]}
    assert not bad, bad


# ---- 5. fold batch against single calls ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cnn_gru_attention", "cnn_gru"])
def test_fold_batch_equals_single_calls_and_leaves_other_arenas_alone(kind):
    C_, slots = 6, [4, 0, 2]
    multi, single = Arena(kind, C_, n=5), Arena(kind, C_, n=5)
    xs = [_x(C_, seed=40 + s) for s in slots]
    for ar in (multi, single):
        for s in slots:
            ar.load(s, _engine(kind, C_, seed=50 + s))
        for s in (1, 3):
            ar.mem[s].fill_(0xA5)                       # canary arenas
    canary = multi.mem[1].clone()
    multi.adapt_multi(slots, xs, CUTS[16], alpha=0.7)
    for s, x in zip(slots, xs):
        single.adapt(s, x, CUTS[16], alpha=0.7)
    torch.cuda.synchronize()
    for s in slots:
        assert _same(multi.state(s), single.state(s)), s
        assert _same(multi.view(s, "ab", torch.float64), single.view(s, "ab", torch.float64)), s
        assert not _same(multi.state(s), multi.state(slots[0])) or s == slots[0]
    assert torch.equal(multi.mem[1], canary) and torch.equal(multi.mem[3], canary)


# ---- 6. nothing else is written ---------------------------------------------------------------------------------------------------
def test_nothing_but_the_destination_slices_is_written():
    kind, C_ = "cnn_gru_attention", 6
    eng, x = _engine(kind, C_, seed=60), _x(C_, seed=61)
    g = torch.Generator().manual_seed(1)
    src = torch.cat([torch.rand(16, generator=g) - 0.5, 0.5 + torch.rand(16, generator=g), torch.rand(32, generator=g) - 0.5,
                     0.5 + torch.rand(32, generator=g)]).to(DEV)
    ar = Arena(kind, C_)
    ar.load(0, eng, bn_state=src)
    canary = torch.full((96,), float("nan"), device=DEV)
    ar.view(0, "bn_dst", torch.float32).copy_(canary)
    # an empty accumulator: the commit copies the source, and only that stage's slices
    ar.commit(0, 1, 1.0, dst="bn_dst")
    torch.cuda.synchronize()
    got = ar.state(0, "bn_dst")
    assert _same(got[:32], src[:32]) and bool(torch.isnan(got[32:]).all())
    ar.commit(0, 2, 1.0, dst="bn_dst")
    torch.cuda.synchronize()
    assert _same(ar.state(0, "bn_dst"), src)
    ar.view(0, "bn_dst", torch.float32).copy_(canary)
    before = {k: ar.view(0, k).clone() for k in ("params", "bn_state", "bn_count")}
    # alpha = 0: the source bits, from a full accumulator, into a separate destination
    for stage in (1, 2):
        i = 0
        for b in CUTS[16]:
            ar.accumulate(0, x[i:i + b], stage)
            i += b
        ar.commit(0, stage, 0.0, dst="bn_dst")
    torch.cuda.synchronize()
    assert _same(ar.state(0, "bn_dst"), src)
    # alpha = 1 into the separate destination: it moves, and the source state, the counters and every parameter do not
    ar.commit(0, 1, 1.0, dst="bn_dst")
    ar.commit(0, 2, 1.0, dst="bn_dst")
    torch.cuda.synchronize()
    got = ar.state(0, "bn_dst")
    assert bool(torch.isfinite(got).all()) and not _same(got[:32], src[:32]) and not _same(got[32:], src[32:])
    for k, v in before.items():
        assert torch.equal(ar.view(0, k), v), k
    acc = ar.view(0, "ab", torch.float64).cpu().numpy()
    assert acc[L.AB_N1] == N * 128 and acc[L.AB_N2] == N * 32


# ---- 7. determinism -----------------------------------------------------------------------------------------------------------------
def test_same_bits_again_and_beside_a_busy_second_stream():
    kind, C_ = "cnn_gru_attention", 6
    eng, x = _engine(kind, C_, seed=70), _x(C_, seed=71)

    def run(stream):
        ar = Arena(kind, C_)
        ar.load(0, eng)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            ar.adapt(0, x, CUTS[16])
        stream.synchronize()
        return ar.state(0), ar.view(0, "ab", torch.float64).clone()

    want = run(torch.cuda.Stream(DEV))
    again = run(torch.cuda.Stream(DEV))
    assert _same(want[0], again[0]) and _same(want[1], again[1])
    xb = _x(C_, seed=1, n=64)
    yb = torch.zeros(64, dtype=torch.int64, device=DEV)
    other = _engine(kind, C_, seed=2)
    stop = threading.Event()

    def noise():
        with torch.cuda.stream(torch.cuda.Stream(DEV)):
            k = 0
            while not stop.is_set() and k < 400:
                k += 1
                other.train_step(xb, yb, 1e-3, step=k, dropout_p=0.5, seed=1)
            torch.cuda.current_stream(DEV).synchronize()

    th = threading.Thread(target=noise)
    th.start()
    try:
        busy = run(torch.cuda.Stream(DEV))
    finally:
        stop.set()
        th.join()
    assert _same(want[0], busy[0]) and _same(want[1], busy[1])


# ---- 8. the adapted model -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", [2, 1])
def test_adapted_model_against_the_oracles_eval_forward(layers):
    kind, C_ = "cnn_gru_attention", 6
    model, x = _model(kind, C_, 20 + C_, layers), _x(C_, seed=30 + C_)
    named = _named(kind, C_, 20 + C_, layers)
    with torch.no_grad():
        plain = model(x).clone()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    bufs = model.adapt_bn(x)                                      # inplace=False: the model is as it was
    assert set(bufs) == set(R.KEYS)
    for k, v in model.state_dict().items():
        assert _same(v, sd[k]), k
    with torch.no_grad():
        assert _same(model(x), plain)
    same = model.adapt_bn(x, inplace=True)
    for k in R.KEYS:
        assert _same(same[k], bufs[k]) and _same(model.state_dict()[k], bufs[k]), k
    for k, v in model.state_dict().items():                       # nothing but the four running statistics moved
        assert _same(v, sd[k]) or k in R.KEYS, k
    assert not model.training
    with torch.no_grad():
        adapted = model(x)
    # the oracle's eval forward with the restatement's buffers, float64 and — `own` — float32 end to end
    xc = x.cpu()
    logits = {}
    for dtype in (torch.float64, torch.float32):
        b = R.adapt(named, O.init_buffers(), xc, batch=16, dtype=dtype)
        p = {k: torch.as_tensor(v).to(dtype) for k, v in named.items()}
        logits[dtype] = O.forward(p, b, xc.to(dtype), training=False)[0]["logits"].numpy()
    tol = stage_tol("logits", rel_err(logits[torch.float32], logits[torch.float64]))
    err = rel_err(adapted.cpu().numpy(), logits[torch.float64])
    moved = rel_err(plain.cpu().numpy(), logits[torch.float64])
    print(f"layers={layers}: adapted logits err {err:.3e} tol {tol:.3e}; un-adapted logits differ by {moved:.3e}")
    assert err <= tol
    assert moved > 100 * tol                                      # the adaptation does something


@pytest.mark.parametrize("layers", [2, 1])
def test_adapt_bn_of_the_baseline_model(layers):
    C_ = 2
    model, x = _model("cnn_gru", C_, 20 + C_, layers), _x(C_, seed=30 + C_)
    with torch.no_grad():
        plain = model(x).clone()
    bufs = model.adapt_bn(x, alpha=0.5)
    with torch.no_grad():
        assert _same(model(x), plain)
    named = _named("cnn_gru", C_, 20 + C_, layers)
    ref = R.adapt(named, O.init_buffers(), x.cpu(), alpha=0.5, kind="cnn_gru")
    own = R.adapt(named, O.init_buffers(), x.cpu(), alpha=0.5, kind="cnn_gru", dtype=torch.float32)
    for k in R.KEYS:
        assert rel_err(bufs[k].cpu().numpy(), ref[k].numpy()) <= stage_tol(k, rel_err(own[k].numpy(), ref[k].numpy())), k
    model.adapt_bn(x, alpha=0.5, inplace=True)
    with torch.no_grad():
        assert not _same(model(x), plain)
    with pytest.raises(ValueError):
        model.adapt_bn(x, alpha=1.5)
    with pytest.raises(RuntimeError):
        model.adapt_bn(x.cpu())


# ---- 9. launches ------------------------------------------------------------------------------------------------------------------
def _launches(fn):
    torch.cuda.synchronize()
    L.profile_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        return {k: c for k, (c, _) in L.profile_report().items()}
    finally:
        L.profile_enable(False)


@pytest.mark.parametrize("kind", ["cnn_gru_attention", "cnn_gru"])
def test_launch_counts(kind):
    C_ = 6
    ar = Arena(kind, C_, n=3)
    xs = [_x(C_, seed=80 + s) for s in range(3)]
    for s in range(3):
        ar.load(s, _engine(kind, C_, seed=90 + s))
    one = _launches(lambda: ar.adapt(0, xs[0], CUTS[16]))
    want = {"conv1_fwd": 6, "ab_merge": 6, "bn_finalize": 3, "pool1_conv2_fwd": 3, "ab_commit": 2}      # 3 batches x 2 stages
    if kind == "cnn_gru_attention":
        want["gate"] = 6
    assert one == want
    assert not any(w in k for k in one for w in ("gru", "head", "bn_relu_pool"))
    for s in range(3):
        ar.view(s, "ab").zero_()
    many = _launches(lambda: ar.adapt_multi([0, 1, 2], xs, CUTS[16]))
    assert many == one                                            # 3 folds as a batch launch as many kernels as 1


# ---- 10. BnAdapter and the driver -------------------------------------------------------------------------------------------------
def test_bn_adapter_batched_equals_sequential_for_folds_of_unequal_size():
    kind, C_ = "cnn_gru_attention", 6
    sizes = [37, 21, 37]
    f_ids = list(range(len(sizes)))
    jobs = []
    for f, n in enumerate(sizes):
        rs = np.random.RandomState(f)
        jobs.append(dict(model=_model(kind, C_, 100 + f), x=_x(C_, seed=110 + f, n=n), y=torch.as_tensor(rs.randint(0, K, n), device=DEV)))
    before = [{k: v.clone() for k, v in j["model"].state_dict().items()} for j in jobs]
    a = A.BnAdapter(jobs, alpha=1.0, batched=True, eval_batch=16)
    b = A.BnAdapter(jobs, alpha=1.0, batched=False, eval_batch=16)
    ra, rb = a.run(), b.run()
    assert ra == rb and [r["n"] for r in ra] == sizes
    for s, j in enumerate(jobs):
        assert _same(a.adapted_state(s), b.adapted_state(s))
        named = _named(kind, C_, 100 + f_ids[s])
        ref = R.adapt(named, O.init_buffers(), j["x"].cpu(), batch=16)
        own = R.adapt(named, O.init_buffers(), j["x"].cpu(), batch=16, dtype=torch.float32)
        for k, v in a.adapted_buffers(s).items():                 # every fold of the batch passes the gate on its own windows
            assert rel_err(v.cpu().numpy(), ref[k].numpy()) <= stage_tol(k, rel_err(own[k].numpy(), ref[k].numpy())), (s, k)
        for k, v in j["model"].state_dict().items():
            assert _same(v, before[s][k]), k
        assert set(ra[s]) == {"n", "before", "after"} and 0.0 <= ra[s]["after"]["accuracy"] <= 1.0
    nolabel = A.BnAdapter([dict(model=jobs[0]["model"], x=jobs[0]["x"])], eval_batch=16).run()
    assert nolabel == [{"n": 37}]


def _fold_results(run, subs):
    out = {}
    for s in subs:
        info = json.loads((run / f"fold_test_on_{s}" / "fold_result.json").read_text())
        hist = [{k: v for k, v in h.items() if k != "seconds"} for h in info["history"]]
        out[s] = (info["accuracy"], info["f1_score"], info["epochs"], hist)
    return out


def _loso_part(text):
    return text[:text.index("LOSO wall-clock")]


def test_driver_adapts_after_loso(tmp_path, capsys):
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.synth import make_synthetic_wesad
    subs = ["S2", "S3", "S4", "S5"]
    d = make_synthetic_wesad(tmp_path / "w", subjects=subs, windows_per_subject=150, T=256, difficulty=2.0)
    common = ["--synthetic", str(d), "--samples", "256", "--subjects", *subs, "--epochs", "2", "--patience", "1", "--batch-size", "16"]
    M.main(common + ["--adapt-bn", "--out", str(tmp_path / "ad")])
    M.main(common + ["--out", str(tmp_path / "plain")])
    M.main(common + ["--adapt-bn", "1.0", "--adapt-bn-sequential", "--out", str(tmp_path / "seq")])
    runs = {k: sorted((tmp_path / k).glob("simple_binary/run_*"))[0] for k in ("ad", "plain", "seq")}
    # the LOSO part of the run is what it is without the flag
    assert _loso_part((runs["ad"] / "cv_summary.txt").read_text(encoding="utf-8")) == _loso_part((runs["plain"] / "cv_summary.txt").read_text(encoding="utf-8"))
    assert _fold_results(runs["ad"], subs) == _fold_results(runs["plain"], subs)
    assert sorted(p.name for p in runs["plain"].iterdir()) == sorted(p.name for p in runs["ad"].iterdir() if not p.name.startswith("adaptation"))
    assert not (runs["plain"] / "adaptation.json").exists() and not (runs["plain"] / "fold_test_on_S2" / "adaptation_result.json").exists()
    doc = json.loads((runs["ad"] / "adaptation.json").read_text())
    assert [f["subject"] for f in doc["folds"]] == subs and doc["n_folds"] == 4 and doc["note"] == A.SYNTHETIC_NOTE
    assert doc["settings"] == {"alpha": 1.0}
    txt = (runs["ad"] / "adaptation.txt").read_text(encoding="utf-8")
    assert A.SYNTHETIC_NOTE in txt and all(s in txt for s in subs) and "mean paired difference" in txt
    assert json.loads((runs["seq"] / "adaptation.json").read_text())["folds"] == doc["folds"]          # fold-batched == single calls
    for s, fold in zip(subs, doc["folds"]):
        per = json.loads((runs["ad"] / f"fold_test_on_{s}" / "adaptation_result.json").read_text())
        res = json.loads((runs["ad"] / f"fold_test_on_{s}" / "fold_result.json").read_text())
        assert per["before"] == fold["before"] == {"accuracy": res["accuracy"], "f1_score": res["f1_score"]}, s
        assert per["after"] == fold["after"] and per["n"] == fold["n"] == 150 and per["subject"] == s
    assert "BatchNorm adaptation on 150 unlabelled windows" in capsys.readouterr().out


def test_driver_adapts_both_kinds_of_a_comparison_run_beside_a_calibration(tmp_path):
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.synth import make_synthetic_wesad
    subs = ["S2", "S3", "S4"]
    d = make_synthetic_wesad(tmp_path / "w", subjects=subs, windows_per_subject=150, T=256, difficulty=2.0)
    M.main(["--synthetic", str(d), "--samples", "256", "--subjects", *subs, "--epochs", "2", "--patience", "1", "--batch-size", "16",
            "--model", "cnn_gru_attention", "cnn_gru", "--adapt-bn", "0.5", "--calibrate", "8", "--calibration-epochs", "2",
            "--out", str(tmp_path / "o")])
    (run,) = sorted((tmp_path / "o").glob("simple_binary/run_*"))
    assert (run / "comparison.json").exists()
    for kind in ("cnn_gru_attention", "cnn_gru"):
        doc = json.loads((run / kind / "adaptation.json").read_text())
        assert [f["subject"] for f in doc["folds"]] == subs and doc["settings"] == {"alpha": 0.5}
        assert (run / kind / "calibration.json").exists()
        for f in doc["folds"]:
            res = json.loads((run / kind / f"fold_test_on_{f['subject']}" / "fold_result.json").read_text())
            assert f["before"] == {"accuracy": res["accuracy"], "f1_score": res["f1_score"]}          # against the LOSO model, not the calibrated one
            assert f["n"] == 150 and 0.0 <= f["after"]["accuracy"] <= 1.0
            assert (run / kind / f"fold_test_on_{f['subject']}" / "adaptation_result.json").exists()
