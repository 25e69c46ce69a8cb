"""GPU tier: gradient-norm clipping inside the fused and fold-batched train steps (include/msig_gc.h).

1. max_norm = inf is the unclipped step, bit for bit (single models of every kind, with class weights, a fold batch).
2. The clip is exactly the formula: the reported norm is sqrt(sum g^2) of the unclipped step's gradient tensors, the clipped buffer
   is g * coef as one fp32 multiplication.
3. Three clipped steps against the fp64 oracle with torch.nn.utils.clip_grad_norm_ and torch.optim.Adam.
4. Fold batches equal their single clipped steps; a fold's bits do not depend on its companions' max_norm.
5. The Trainer's history and log, the drivers.
6. model(x) -> loss.backward() -> torch's clip_grad_norm_ -> MsigAdam.step() against the fused clipped step.

Seeds and shapes follow test_class_weights_gpu.py and test_trainer_gpu.py."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from gpu_common import legacy_train_step
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd.runtime import EmbeddedEngine, Engine, FoldArena
from oracle import cnn_gru_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LR, WD, P = 1e-3, 1e-4, 0.5
INF = float("inf")
STATE = ("params", "grads", "exp_avg", "exp_avg_sq", "bn_state", "bn_count", "loss_acc")


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def _data(B, Cc, K, T, seed):
    rs = np.random.RandomState(seed)
    y = rs.randint(0, K, size=B).astype(np.int64)
    y[:K] = np.arange(K)
    return torch.as_tensor(rs.randn(B, Cc, T).astype(np.float32)).to(DEV), torch.as_tensor(y).to(DEV)


def _engine(Cc, K, config="full", seed=3, storage_engine=None):
    """config: "full" (attention model, 64 x 2), "embedded" (attention model, 32 x 1) or "cnn_gru" (the baseline, 64 x 2)."""
    hidden, layers = (32, 1) if config == "embedded" else (64, 2)
    kind = "cnn_gru" if config == "cnn_gru" else "cnn_gru_attention"
    params = O.init_params(Cc, K, seed=seed, hidden=hidden, layers=layers)
    if kind == "cnn_gru":
        params = {k: v for k, v in params.items() if k not in L.GATE_KEYS}
    e = storage_engine
    if e is None:
        e = EmbeddedEngine(Cc, K, DEV, hidden) if layers == 1 else Engine(Cc, K, DEV, kind=kind)
    if layers == 1:
        for k, v in e.small_views().items():
            v.copy_(params[k])
    else:
        e.load_named(params)
    return e, params


def _named_grads(e):
    """The gradient tensors by name (not the flat buffer's padding), as float32 CPU tensors."""
    views = e.gather_grads() if isinstance(e, EmbeddedEngine) else e.named_param_views(e.grads)
    return {k: v.detach().cpu().clone() for k, v in views.items()}


def _assert_same_state(a, b, B, K, what=""):
    for name in STATE:
        assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), (what, name)
    for r, shape in (("LOSS", (3,)), ("LOGITS", (B, K)), ("DLOGITS", (B, K))):
        assert torch.equal(_bits(a.region(r, torch.float32, shape)), _bits(b.region(r, torch.float32, shape))), (what, r)
    if isinstance(a, EmbeddedEngine):
        assert torch.equal(_bits(a.small), _bits(b.small)), (what, "small")


# ---- 1. off = unclipped, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config,B,T,weighted", [("full", 64, 256, False), ("full", 3000, 64, False), ("cnn_gru", 64, 256, False),
                                                 ("embedded", 64, 256, False), ("full", 64, 256, True), ("cnn_gru", 3000, 64, True)])
def test_max_norm_inf_is_the_unclipped_step_bit_for_bit(config, B, T, weighted):
    """msig_gc_train_step with max_norm = inf against the existing fused step from the same state, two steps: parameters, gradients,
    both moments, BatchNorm state, loss and loss_acc.  B = 64 runs the one-launch head with the loss in the reduction launch, B = 3000
    the separate head and ce_kernel."""
    Cc, K = 6, 2
    x, y = _data(B, Cc, K, T, 1)
    cw = torch.tensor([0.3, 2.5], device=DEV) if weighted else None
    out = []
    for mn in (None, INF):
        e, _ = _engine(Cc, K, config)
        for s in (1, 2):
            if mn is None:       # the counterpart: the existing fused step's own entry point (msig_train_step / _cw_ / _cg_)
                legacy_train_step(e, x, y, LR, weight_decay=WD, step=s, dropout_p=P, seed=7, class_weight=cw)
            else:
                e.train_step(x, y, LR, weight_decay=WD, step=s, dropout_p=P, seed=7, class_weight=cw, max_grad_norm=mn)
        out.append(e)
    torch.cuda.synchronize()
    a, b = out
    _assert_same_state(a, b, B, K, config)
    st = b.grad_stats()
    assert a.grad_stats() is None and st["clipped"] == 0 and np.isfinite(st["last"]) and 0 < st["last"] <= st["max"] <= st["sum"]


def _arena_run(n, B, T, Cc, K, data, max_norms=None, weights=None, steps=2, config="full"):
    """n folds in one FoldArena: `steps` fused multi steps — msig_gc_train_step_multi with the folds' max_norms, or, max_norms None,
    the unclipped call in an arena built without a clip state.  Returns the arena and its engines."""
    hidden, layers = (32, 1) if config == "embedded" else (64, 2)
    kind = "cnn_gru" if config == "cnn_gru" else "cnn_gru_attention"
    arena = FoldArena(Cc, K, DEV, n, B, T, gru_hidden=hidden, gru_layers=layers, kind=kind, grad_clip=max_norms is not None)
    engs = [_engine(Cc, K, config, seed=10 + f, storage_engine=arena.engine(f))[0] for f in range(n)]
    if layers == 1:
        for e in engs:
            e.scatter()
    if weights is not None:
        for f in range(n):
            arena.set_class_weight(f, weights[f])
    if max_norms is not None:
        for f in range(n):
            arena.set_max_norm(f, max_norms[f])
    cw = arena.ptr("cw") if weights is not None else None
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    lib = L.lib()
    for s in range(1, steps + 1):
        for f in range(n):
            x, y = data[f][s - 1]
            arena.view(f, "x", torch.float32)[:x.numel()].copy_(x.reshape(-1))
            arena.view(f, "y", torch.int64)[:B].copy_(y)
        slots = list(range(n))
        m = arena.multi(slots, key_gru=[L.dropout_key(100 + f, s, 1) for f in range(n)],
                        key_head=[L.dropout_key(100 + f, s, 2) for f in range(n)], lr=[LR] * n, steps=[s] * n)
        desc = arena.batch(B, True, P)
        ea, eas = arena.ptr("exp_avg"), arena.ptr("exp_avg_sq")
        if max_norms is not None:
            g = arena.clip(slots, cw)
            rc = lib.msig_gc_train_step_multi(C.byref(desc), C.byref(m), C.byref(g), ea, eas, 0.9, 0.999, 1e-8, WD, s, st)
        elif kind == "cnn_gru":
            rc = lib.msig_cg_train_step_multi(C.byref(desc), C.byref(m), cw, ea, eas, 0.9, 0.999, 1e-8, WD, s, st)
        elif cw is None:
            rc = lib.msig_train_step_multi(C.byref(desc), C.byref(m), ea, eas, 0.9, 0.999, 1e-8, WD, s, st)
        else:
            rc = lib.msig_cw_train_step_multi(C.byref(desc), C.byref(m), cw, ea, eas, 0.9, 0.999, 1e-8, WD, s, st)
        L.check(rc, "train_step_multi")
    torch.cuda.synchronize()
    return arena, engs


def _fold_data(n, B, Cc, K, T, steps=2):
    return [[_data(B, Cc, K, T, 1000 * f + s) for s in range(steps)] for f in range(n)]


@pytest.mark.parametrize("weighted", [False, True])
def test_max_norm_inf_fold_batch_is_bit_identical(weighted):
    """A 5-fold msig_gc_train_step_multi with every max_norm = inf against the unclipped fold batch: every byte of the arenas apart
    from the clip state, which is the last region of an arena and absent from the arena built without it."""
    n, B, T, Cc, K = 5, 64, 128, 6, 2
    data = _fold_data(n, B, Cc, K, T)
    ws = [np.array([0.5 + 0.1 * f, 2.0 - 0.2 * f]) for f in range(n)] if weighted else None
    a, _ = _arena_run(n, B, T, Cc, K, data, None, ws)
    b, _ = _arena_run(n, B, T, Cc, K, data, [INF] * n, ws)
    gc0 = b.off["gc"][0]
    assert "gc" not in a.off and all(o + nb <= gc0 for k, (o, nb) in b.off.items() if k != "gc")
    assert {k: v for k, v in b.off.items() if k != "gc"} == a.off and a.stride <= gc0
    assert torch.equal(a.mem[:, :a.stride], b.mem[:, :a.stride])


# ---- 2. the clip is exactly the formula ---------------------------------------------------------------------------------------
def _coef(max_norm, N):
    q = np.float64(max_norm) / (np.float64(N) + np.float64(1e-6))
    return np.float32(min(np.float64(1.0), q))


@pytest.mark.parametrize("config,B,T", [("full", 64, 256), ("full", 3000, 64), ("embedded", 64, 256), ("cnn_gru", 64, 256)])
def test_clip_is_the_formula(config, B, T):
    """From one state, one unclipped and one clipped step.  The reported N against sqrt(sum g_unclipped^2) summed in fp64 on the
    host over the named tensors, to 1e-12 relative (the order of summation only: a tensor missed or counted twice is far outside);
    the clipped buffer against g_unclipped * coef as a torch fp32 multiplication, every bit, with coef recomputed from the reported
    N; the clipped buffer's norm against max_norm."""
    Cc, K = 6, 3
    x, y = _data(B, Cc, K, T, 4)
    plain, _ = _engine(Cc, K, config)
    plain.train_step(x, y, LR, weight_decay=WD, step=1, dropout_p=P, seed=7)
    g = _named_grads(plain)
    N_host = float(np.sqrt(sum(float((v.double() ** 2).sum()) for v in g.values())))
    max_norm = 0.5 * N_host
    clipped, _ = _engine(Cc, K, config)
    clipped.train_step(x, y, LR, weight_decay=WD, step=1, dropout_p=P, seed=7, max_grad_norm=max_norm)
    torch.cuda.synchronize()
    st = clipped.grad_stats()
    N = st["last"]
    print(f"\n{config} B={B}: N reported {N!r} host {N_host!r} rel {abs(N - N_host) / N_host:.3e}")
    assert abs(N - N_host) <= 1e-12 * N_host
    assert st["sum"] == N and st["max"] == N and st["clipped"] == 1
    coef = _coef(max_norm, N)
    assert coef < 1
    gc = _named_grads(clipped)
    assert sorted(gc) == sorted(g)
    for k, v in g.items():
        assert torch.equal(_bits(gc[k]), _bits(v * torch.tensor(coef))), k
    got = float(np.sqrt(sum(float((v.double() ** 2).sum()) for v in gc.values())))
    print(f"clipped norm {got!r} max_norm {max_norm!r}")
    assert got <= max_norm * (1 + 2.0 ** -22)          # coef and each product round once (2^-24 each); the 1e-6 only lowers it
    assert got >= max_norm * (1 - 1e-5)
    # and the update is Adam's on the clipped gradient: it differs from the unclipped step's
    assert not torch.equal(plain.params, clipped.params)


def test_a_norm_below_max_norm_is_not_clipped_and_is_counted_so():
    Cc, K, B, T = 3, 2, 64, 128
    x, y = _data(B, Cc, K, T, 6)
    a, _ = _engine(Cc, K)
    b, _ = _engine(Cc, K)
    for s in (1, 2, 3):
        legacy_train_step(a, x, y, LR, weight_decay=WD, step=s, dropout_p=P, seed=7)          # msig_train_step itself
        b.train_step(x, y, LR, weight_decay=WD, step=s, dropout_p=P, seed=7, max_grad_norm=1e6)
    torch.cuda.synchronize()
    _assert_same_state(a, b, B, K)
    st = b.grad_stats()
    assert st["clipped"] == 0 and st["max"] < 1e6 and st["sum"] >= st["max"] >= st["last"] > 0
    b.zero_grad_stats()
    assert b.grad_stats() == dict(sum=0.0, max=0.0, clipped=0, last=0.0)


def test_engine_rejects_bad_max_norm_before_any_launch():
    e, _ = _engine(3, 2)
    x, y = _data(8, 3, 2, 64, 4)
    before = e.params.clone()
    for bad in (0.0, -1.0, float("nan"), "1"):
        with pytest.raises(ValueError):
            e.train_step(x, y, LR, max_grad_norm=bad)
    with pytest.raises(RuntimeError):
        FoldArena(3, 2, DEV, 1, 8, 64).set_max_norm(0, 1.0)
    with pytest.raises(ValueError):
        FoldArena(3, 2, DEV, 1, 8, 64, grad_clip=True).set_max_norm(0, 0.0)
    torch.cuda.synchronize()
    assert torch.equal(before, e.params) and int(e.bn_count[0]) == 0


# ---- 3. against the fp64 oracle -------------------------------------------------------------------------------------------------
def _three_step_rule(got, ref, key):
    """The existing rule and constants of the three-step comparison (tests/test_parity_gpu.py::
    test_three_fused_train_steps_match_reference; gpu_common.py has the one-step tolerances only): an element is off when it differs
    by more than 3e-5 + 2e-3 |ref|; at most 5e-3 of a tensor's elements may be, and none by more than 6e-3 + 3e-5 — Adam's first
    steps move a weight by lr * g / (|g| + eps), so an element whose gradient is rounding noise moves by up to 2 * lr per step in
    either direction.  Returns (fraction off, largest difference) for the record."""
    if ref.size == 0:
        return 0.0, 0.0
    diff = np.abs(got.astype(np.float64) - ref)
    bad = diff > 3e-5 + 2e-3 * np.abs(ref)
    assert bad.mean() <= 5e-3 and diff.max() <= 6e-3 + 3e-5, (key, bad.mean(), diff.max())
    return float(bad.mean()), float(diff.max())


def _oracle_three_steps(params, x, y, dtype, p, seed, max_norm=None, steps=3):
    """oracle forward + autograd + torch.nn.utils.clip_grad_norm_ + torch.optim.Adam(weight_decay).  max_norm None: half the first
    step's norm.  Returns (parameters after the steps, max_norm, [(norm, coefficient) per step])."""
    leaf = {k: v.to(dtype).clone().requires_grad_(v.numel() > 0) for k, v in params.items()}
    bufs = {k: (v if "num_batches" in k else v.to(dtype)) for k, v in O.init_buffers().items()}
    live = [v for v in leaf.values() if v.numel()]
    opt = torch.optim.Adam(live, lr=LR, weight_decay=WD)
    xc, yc = x.cpu().to(dtype), y.cpu()
    rec = []
    for s in range(1, steps + 1):
        opt.zero_grad()
        st, bufs = O.forward(leaf, bufs, xc, training=True, dropout_p=p, seed=seed, step=s)
        O.cross_entropy(st["logits"], yc).backward()
        if max_norm is None:
            max_norm = 0.5 * float(torch.sqrt(sum((v.grad.double() ** 2).sum() for v in live)))
        N = float(torch.nn.utils.clip_grad_norm_(live, max_norm, norm_type=2))
        rec.append((N, max_norm / (N + 1e-6)))
        opt.step()
    return {k: v.detach().double().numpy() for k, v in leaf.items()}, max_norm, rec


@pytest.fixture
def no_gate(monkeypatch):
    """The oracle's ChannelAttention replaced by the identity (s = 1): the baseline's reference, without editing oracle/
    (tests/test_cnngru_gpu.py)."""
    def gate(x, W1, W2):
        B, C_, _ = x.shape
        return x.mean(dim=2), torch.zeros(B, 0, dtype=x.dtype), torch.ones(B, C_, dtype=x.dtype)
    return lambda: monkeypatch.setattr(O, "channel_gate", gate)


@pytest.mark.parametrize("config,Cc,K,B,T,p", [("full", 6, 2, 4, 3840, 0.5), ("full", 3, 3, 16, 256, 0.0), ("cnn_gru", 6, 3, 16, 512, 0.5),
                                               ("cnn_gru", 3, 2, 64, 256, 0.0), ("full", 6, 2, 64, 256, 0.0)])
def test_three_clipped_steps_against_the_fp64_oracle(no_gate, config, Cc, K, B, T, p):
    """Parameters after three clipped fused steps against the fp64 oracle run through torch's own clip_grad_norm_ and Adam, under
    the three-step rule above.  max_norm is half the oracle's first-step norm, and the oracle's coefficient is asserted below 1 on
    every step: the case cannot pass without clipping.  The fp32 oracle's own distance from the fp64 one is printed beside each figure.
    The batch sizes come from the oracle alone: the same batch is presented three times, and a batch of 16 windows without dropout is
    fitted so fast that the fp64 oracle's norm halves after one step (C = 3 baseline, B = 16: coefficients 0.50, 1.05, 0.89 — the
    premise above does not hold there), so the dropout-free C = 3 baseline case has 64 windows (oracle: 0.50, 0.40, 0.58)."""
    if config == "cnn_gru":
        no_gate()
    e, params = _engine(Cc, K, config, seed=Cc + K)
    if config == "cnn_gru":
        params = dict(params, **{"channel_attention.fc.0.weight": torch.zeros(0, Cc), "channel_attention.fc.2.weight": torch.zeros(Cc, 0)})
    x, y = _data(B, Cc, K, T, B + Cc)
    ref, max_norm, rec = _oracle_three_steps(params, x, y, torch.float64, p, 11)
    own, _, _ = _oracle_three_steps(params, x, y, torch.float32, p, 11, max_norm)
    print(f"\n{config} C={Cc} K={K} B={B} T={T} p={p}: max_norm {max_norm:.6g}, oracle (N, coef) per step {rec}")
    assert all(c < 1.0 for _, c in rec), rec
    norms = []
    for s in (1, 2, 3):
        e.train_step(x, y, LR, weight_decay=WD, step=s, dropout_p=p, seed=11, max_grad_norm=max_norm)
        norms.append(e.grad_stats()["last"])
    torch.cuda.synchronize()
    assert e.grad_stats()["clipped"] == 3
    for s, (N, (N64, _)) in enumerate(zip(norms, rec), start=1):
        print(f"step {s}: N {N:.9g} oracle {N64:.9g} rel {abs(N - N64) / N64:.2e}")
    got = e.named_param_views()
    assert {k for k, v in got.items() if v.numel()} == {k for k, v in ref.items() if v.size}
    for k, v in got.items():
        if not v.numel():
            continue
        frac, worst = _three_step_rule(v.detach().cpu().numpy(), ref[k], k)
        d32 = np.abs(own[k] - ref[k])
        print(f"  {k:36s} off {frac:.2e} max diff {worst:.2e} | fp32 oracle: off {float((d32 > 3e-5 + 2e-3 * np.abs(ref[k])).mean()):.2e} max diff {float(d32.max()):.2e}")


# ---- 4. fold batches -------------------------------------------------------------------------------------------------------------
def test_clipped_fold_batch_equals_its_single_clipped_steps():
    """A 5-fold clipped batch, each fold with its own max_norm (half its own second-step norm), against five single clipped steps,
    bit for bit, statistics included; then the same batch with other max_norms (and inf) for the companions of fold 0."""
    n, B, T, Cc, K = 5, 64, 128, 3, 3
    data = _fold_data(n, B, Cc, K, T)
    probe, _ = _arena_run(n, B, T, Cc, K, data, [INF] * n)
    mns = [0.5 * probe.grad_stats(f)["last"] for f in range(n)]
    arena, engs = _arena_run(n, B, T, Cc, K, data, mns)
    for f in range(n):
        e, _ = _engine(Cc, K, seed=10 + f)
        for s in (1, 2):
            x, y = data[f][s - 1]
            e.train_step(x, y, LR, weight_decay=WD, step=s, dropout_p=P, seed=100 + f, max_grad_norm=mns[f])
        torch.cuda.synchronize()
        for name in ("params", "grads", "exp_avg", "exp_avg_sq", "bn_state"):
            assert torch.equal(_bits(getattr(e, name)), _bits(getattr(engs[f], name))), (f, name)
        assert arena.grad_stats(f) == e.grad_stats(), f
        assert arena.grad_stats(f)["clipped"] >= 1
        assert torch.equal(e.gc_state[:L.GC_NSTAT], engs[f].gc_state[:L.GC_NSTAT])
    assert len({arena.grad_stats(f)["last"] for f in range(n)}) == n          # per fold
    other = [mns[0], INF, 3.0 * mns[2], 0.1 * mns[3], INF]
    arena2, _ = _arena_run(n, B, T, Cc, K, data, other)
    assert torch.equal(arena.mem[0], arena2.mem[0])
    for f in (1, 2, 3, 4):
        o, nb = arena.off["params"]
        assert not torch.equal(arena.mem[f, o:o + nb], arena2.mem[f, o:o + nb]), f
    # a fold's bits do not depend on how many folds share its launches either
    alone, _ = _arena_run(1, B, T, Cc, K, data[:1], mns[:1])
    for name in ("params", "grads", "exp_avg", "exp_avg_sq", "bn_state", "acc"):
        o, nb = arena.off[name]
        assert torch.equal(arena.mem[0, o:o + nb], alone.mem[0, o:o + nb]), name
    assert arena.grad_stats(0) == alone.grad_stats(0)


# ---- 5. trainer and drivers ------------------------------------------------------------------------------------------------------
def _trainer(tmp_path, tag, d, names, max_grad_norm, epochs=2):
    from multimodalsignal_amd.dataset import DeviceLoader, WesadDataset
    from multimodalsignal_amd.models import CnnGruAttentionModel
    from multimodalsignal_amd.trainer import Trainer
    mk = lambda s: WesadDataset(d, s, names, names, classification_mode="stress_binary")
    torch.manual_seed(1234)
    model = CnnGruAttentionModel(in_channels=len(names), num_classes=2)
    model.set_dropout_seed(5)
    cfg = {"trainer": {"epochs": epochs, "learning_rate": 1e-3, "early_stopping": {"enabled": True, "patience": 20, "delta": 0},
                       "weight_decay": 1e-4, "verbose": False}}
    if max_grad_norm is not None:
        cfg["trainer"]["max_grad_norm"] = max_grad_norm
    t = Trainer(model, tmp_path / tag, cfg)
    return t, DeviceLoader(mk(["S2", "S3"]), 16, True, DEV, seed=1), DeviceLoader(mk(["S4"]), 16, False, DEV)


def test_trainer_history_and_log(tmp_path):
    from multimodalsignal_amd.synth import make_synthetic_wesad
    d = make_synthetic_wesad(tmp_path / "w", subjects=["S2", "S3", "S4"], windows_per_subject=40, T=256, difficulty=2.0)
    names = (d / "_channel_names.txt").read_text().split()
    plain, tr, va = _trainer(tmp_path, "plain", d, names, None)
    plain.train(tr, va)
    assert all(set(h) == {"epoch", "train_loss", "val_loss", "val_acc", "val_f1", "lr", "seconds"} for h in plain.history)
    log = (tmp_path / "plain" / "training_log.txt").read_text()
    assert "梯度范数" not in log and "max_grad_norm" not in log
    assert all(ln.rstrip().endswith("windows/s") for ln in log.splitlines() if ln.startswith("Epoch "))
    assert plain.model.engine().gc_state is None
    # the norms of every step, by a probe that never clips
    probe, tr, va = _trainer(tmp_path, "probe", d, names, 1e30)
    seen = []
    eng = probe.model.engine()
    step = eng.train_step

    def spy(*a, **k):
        step(*a, **k)
        seen.append(eng.grad_stats()["last"])
    eng.train_step = spy
    probe.train(tr, va)
    n_steps = len(tr)
    assert len(seen) == 2 * n_steps and n_steps > 2
    assert [h["clipped_steps"] for h in probe.history] == [0, 0]
    assert [h["val_loss"] for h in probe.history] == [h["val_loss"] for h in plain.history]      # never clipped: the unclipped run
    for i, h in enumerate(probe.history):
        ep = seen[i * n_steps:(i + 1) * n_steps]
        assert h["grad_norm_max"] == max(ep) and abs(h["grad_norm_mean"] - sum(ep) / n_steps) <= 1e-12 * h["grad_norm_max"]
    max_norm = float(np.median(seen[:n_steps]))
    t, tr, va = _trainer(tmp_path, "clip", d, names, max_norm)
    seen = []
    eng = t.model.engine()
    step = eng.train_step
    eng.train_step = spy
    t.train(tr, va)
    assert len(t.history) == 2
    for i, h in enumerate(t.history):
        ep = seen[i * n_steps:(i + 1) * n_steps]
        assert np.isfinite([h["grad_norm_mean"], h["grad_norm_max"]]).all() and h["grad_norm_max"] == max(ep)
        assert h["clipped_steps"] == sum(N > max_norm for N in ep)
    assert t.history[0]["clipped_steps"] >= 1          # up to its first clipped step the run is the probe's, whose median is max_norm
    lines = [ln for ln in (tmp_path / "clip" / "training_log.txt").read_text().splitlines() if ln.startswith("Epoch ")]
    assert len(lines) == 2 and all("梯度范数" in ln and f"max_grad_norm={max_norm:g}" in ln for ln in lines)


def _fold_outputs(root, subs):
    out = []
    for s in subs:
        info = json.loads((root / f"fold_test_on_{s}" / "fold_result.json").read_text())
        info.pop("seconds", None), info.pop("train_windows_per_s", None)
        for h in info.get("history", []):
            h.pop("seconds", None)
        out.append((info, torch.load(root / f"fold_test_on_{s}" / "best_model.pt", weights_only=True)))
    return out


def test_loso_drivers_with_max_grad_norm(tmp_path):
    """--max-grad-norm on the standard LOSO: the CLI's fold batches and the sequential driver give identical per-fold results,
    histories (gradient norms included) and checkpoints; cv_summary.txt names the setting; the clip changes the run."""
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.synth import CHANNELS6, make_synthetic_wesad
    subs = ["S2", "S3", "S4", "S5"]
    d = make_synthetic_wesad(tmp_path / "w", subjects=subs, windows_per_subject=30, T=256, difficulty=2.0, window_spread=3)
    names = (d / "_channel_names.txt").read_text().split()
    M.main(["--synthetic", str(d), "--samples", "256", "--subjects", *subs, "--epochs", "3", "--patience", "1", "2", "--batch-size", "16",
            "--max-grad-norm", "0.02", "--out", str(tmp_path / "cli")])
    runs = sorted((tmp_path / "cli").glob("simple_binary/run_*"))
    assert len(runs) == 1
    cfg = M.default_cfg()
    cfg.update(data_path=d, channels=list(CHANNELS6), subjects=subs, epochs=3, patience=[1, 2], batch_size=16, concurrent_folds=1,
               max_grad_norm=0.02)
    M.run_simple_experiment(tmp_path / "seq", DEV, names, cfg)
    a, b = _fold_outputs(runs[0], subs), _fold_outputs(tmp_path / "seq", subs)
    for (ia, wa), (ib, wb) in zip(a, b):
        assert ia == ib
        assert list(wa) == list(wb) and all(torch.equal(wa[k], wb[k]) for k in wa)
        assert all({"grad_norm_mean", "grad_norm_max", "clipped_steps"} <= set(h) for h in ia["history"])
        assert sum(h["clipped_steps"] for h in ia["history"]) > 0
    assert "MAX_GRAD_NORM: 0.02\n" in (runs[0] / "cv_summary.txt").read_text(encoding="utf-8")
    plain = dict(cfg)
    del plain["max_grad_norm"]
    M.run_simple_experiment(tmp_path / "plain", DEV, names, plain)
    assert "MAX_GRAD_NORM" not in (tmp_path / "plain" / "cv_summary.txt").read_text(encoding="utf-8")
    assert "梯度范数" not in (tmp_path / "plain" / "fold_test_on_S2" / "training_log.txt").read_text()
    pl = _fold_outputs(tmp_path / "plain", subs)
    assert all("grad_norm_mean" not in h for info, _ in pl for h in info["history"])
    assert any(ha["val_loss"] != hb["val_loss"] for pa, pb in zip(pl, b) for ha, hb in zip(pa[0]["history"], pb[0]["history"]))


def test_hierarchical_with_max_grad_norm(tmp_path):
    """--hierarchical (M1 on the 64 x 2 model, M2 on the embedded 32 x 1 model): the fold-batched driver gives the sequential one's results."""
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.synth import make_synthetic_wesad
    subs = ["S2", "S3", "S4", "S5"]
    d = make_synthetic_wesad(tmp_path / "w", subjects=subs, windows_per_subject=40, T=256, difficulty=2.0)
    names = (d / "_channel_names.txt").read_text().split()
    cfg = M.default_cfg()
    cfg.update(data_path=d, subjects=subs, epochs=3, patience=[1, 2], batch_size=16, max_grad_norm=0.02)
    res_b, _ = M.run_hierarchical_experiment(tmp_path / "batched", DEV, names, cfg)
    res_s, _ = M.run_hierarchical_experiment(tmp_path / "seq", DEV, names, dict(cfg, concurrent_folds=1))
    assert res_b == res_s
    for s in subs:
        for tag in ("model_m1", "model_m2"):
            a = torch.load(tmp_path / "batched" / f"fold_test_on_{s}" / tag / "best_model.pt", weights_only=True)
            b = torch.load(tmp_path / "seq" / f"fold_test_on_{s}" / tag / "best_model.pt", weights_only=True)
            assert all(torch.equal(a[k], b[k]) for k in a), (s, tag)
            assert "梯度范数" in (tmp_path / "batched" / f"fold_test_on_{s}" / tag / "training_log.txt").read_text()
    assert "MAX_GRAD_NORM: 0.02" in (tmp_path / "batched" / "hierarchical_summary.txt").read_text(encoding="utf-8").splitlines()


# ---- 6. the autograd path --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("embedded", [False, True])
def test_autograd_path_with_torch_clip_matches_the_fused_clipped_step(embedded):
    """model(x) -> CrossEntropyLoss -> loss.backward() -> torch.nn.utils.clip_grad_norm_(model.parameters()) -> MsigAdam.step()
    against one fused clipped step from the same weights, under the three-step rule (one step here).  torch forms the norm and the
    coefficient in fp32; the fused step in fp64."""
    from multimodalsignal_amd.models import CnnGruAttentionModel
    from multimodalsignal_amd.trainer import MsigAdam
    kw = dict(gru_hidden_size=32, gru_num_layers=1) if embedded else {}
    x, y = _data(32, 6, 2, 256, 9)
    torch.manual_seed(7)
    ma = CnnGruAttentionModel(6, 2, dropout=0.0, **kw)
    mb = CnnGruAttentionModel(6, 2, dropout=0.0, **kw)
    mb.load_state_dict(ma.state_dict())
    ma.to(DEV).train(); mb.to(DEV).train()
    opt = MsigAdam(ma, lr=LR, weight_decay=WD)
    opt.zero_grad()
    loss = torch.nn.CrossEntropyLoss()(ma(x), y)
    loss.backward()
    N0 = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in ma.parameters() if p.numel())))
    max_norm = 0.5 * N0
    N_t = float(torch.nn.utils.clip_grad_norm_(ma.parameters(), max_norm))
    opt.step()
    eb = mb.engine()
    eb.train_step(x, y, LR, weight_decay=WD, step=1, max_grad_norm=max_norm)
    torch.cuda.synchronize()
    N = eb.grad_stats()["last"]
    print(f"\nembedded={embedded}: torch norm {N_t!r}, fused {N!r}, fp64 of p.grad {N0!r}")
    # N0 is of the staged backward's gradients, N of the fused step's: two paths, fp32 agreement
    assert abs(N - N0) <= 1e-6 * N0 and abs(N_t - N0) <= 1e-5 * N0 and eb.grad_stats()["clipped"] == 1
    sa, sb = ma.state_dict(), mb.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        if "num_batches" in k:
            continue
        _three_step_rule(sa[k].cpu().numpy(), sb[k].double().cpu().numpy(), k)
