"""GPU tier: class-weighted CrossEntropy (include/msig_cw.h) through every layer — the msig_cw_* calls against the unweighted
calls (all-ones weights: the same bits) and against an fp64 reference (oracle.cnn_gru_oracle.forward + torch's
cross_entropy(weight=w) + autograd), fold batches against stand-alone runs, the epoch's loss sum, and the drivers."""
import ctypes as C
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_common import grad_tol, legacy_forward, legacy_train_step, rel_err, stage_tol
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd.runtime import EmbeddedEngine, Engine, FoldArena
from oracle import cnn_gru_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LR, WD, P = 1e-3, 1e-4, 0.5
W2, W3 = (0.3, 2.5), (1.0, 0.2, 4.0)


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def _data(B, Cc, K, T, seed):
    rs = np.random.RandomState(seed)
    y = rs.randint(0, K, size=B).astype(np.int64)
    y[:K] = np.arange(K)
    return torch.as_tensor(rs.randn(B, Cc, T).astype(np.float32)).to(DEV), torch.as_tensor(y).to(DEV)


def _engine(Cc, K, hidden=64, layers=2, seed=3, storage_engine=None):
    params = O.init_params(Cc, K, seed=seed, hidden=hidden, layers=layers)
    e = storage_engine
    if e is None:
        e = EmbeddedEngine(Cc, K, DEV, hidden) if layers == 1 else Engine(Cc, K, DEV)
    if layers == 1:
        for k, v in e.small_views().items():
            v.copy_(params[k])
    else:
        e.load_named(params)
    return e, params


def _regions(e, B, K):
    return {"LOSS": e.region("LOSS", torch.float32, (3,)), "PROBS": e.region("PROBS", torch.float32, (B, K)),
            "PRED": e.region("PRED", torch.int32, (B,)), "LOGITS": e.region("LOGITS", torch.float32, (B, K))}


@pytest.mark.parametrize("B,T", [(64, 256), (3000, 64)])
def test_all_ones_train_step_is_bit_identical(B, T):
    """msig_cw_train_step with w = 1 against msig_train_step: B = 64 runs the one-launch head (head_step_kernel + the loss in
    colsum_adam's launch), B = 3000 the separate head and ce_kernel."""
    Cc, K = 6, 2
    x, y = _data(B, Cc, K, T, 1)
    out = []
    for cw in (None, torch.ones(K, device=DEV)):
        e, _ = _engine(Cc, K)
        for s in (1, 2):
            if cw is None:       # the counterpart: msig_train_step itself (Engine.train_step issues the widest call either way)
                assert legacy_train_step(e, x, y, LR, weight_decay=WD, step=s, dropout_p=P, seed=7) == "msig_train_step"
            else:
                e.train_step(x, y, LR, weight_decay=WD, step=s, dropout_p=P, seed=7, class_weight=cw)
        out.append(e)
    torch.cuda.synchronize()
    a, b = out
    for name in ("params", "grads", "exp_avg", "exp_avg_sq", "bn_state"):
        assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name
    assert torch.equal(a.loss_acc, b.loss_acc)
    ra, rb = _regions(a, B, K), _regions(b, B, K)
    ra["DLOGITS"], rb["DLOGITS"] = a.region("DLOGITS", torch.float32, (B, K)), b.region("DLOGITS", torch.float32, (B, K))
    for k in ra:
        assert torch.equal(_bits(ra[k]), _bits(rb[k])), k


def test_all_ones_eval_forward_is_bit_identical():
    Cc, K, B, T = 3, 3, 100, 256
    x, y = _data(B, Cc, K, T, 2)
    for keep in (False, True):
        out = []
        for cw in (None, torch.ones(K, device=DEV)):
            e, _ = _engine(Cc, K)
            if cw is None:       # the counterpart: msig_forward itself
                assert legacy_forward(e, x, y, keep_for_backward=keep) == "msig_forward"
            else:
                e.forward(x, y, training=False, keep_for_backward=keep, class_weight=cw)
            out.append(e)
        torch.cuda.synchronize()
        a, b = out
        ra, rb = _regions(a, B, K), _regions(b, B, K)
        if keep:
            ra["DLOGITS"], rb["DLOGITS"] = a.region("DLOGITS", torch.float32, (B, K)), b.region("DLOGITS", torch.float32, (B, K))
        for k in ra:
            assert torch.equal(_bits(ra[k]), _bits(rb[k])), (keep, k)
        assert torch.equal(a.loss_acc, b.loss_acc)


def _arena_run(n, B, T, Cc, K, weights, data, steps=2, eval_B=None):
    """n folds of (64, 2) models in one FoldArena: `steps` msig_cw_train_step_multi calls (weights None: msig_train_step_multi), then
    one evaluation pass (msig_cw_forward_multi / msig_forward_multi).  Returns the arena and its engines."""
    arena = FoldArena(Cc, K, DEV, n, B, T, eval_batch=eval_B or B)
    engs = [_engine(Cc, K, seed=10 + f, storage_engine=arena.engine(f))[0] for f in range(n)]
    if weights is not None:
        for f in range(n):
            arena.set_class_weight(f, weights[f])
    cw = arena.ptr("cw") if weights is not None else None
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    lib = L.lib()
    for s in range(1, steps + 1):
        for f in range(n):
            x, y = data[f][s - 1]
            arena.view(f, "x", torch.float32)[:x.numel()].copy_(x.reshape(-1))
            arena.view(f, "y", torch.int64)[:B].copy_(y)
        m = arena.multi(list(range(n)), key_gru=[L.dropout_key(100 + f, s, 1) for f in range(n)],
                        key_head=[L.dropout_key(100 + f, s, 2) for f in range(n)], lr=[LR] * n, steps=[s] * n)
        desc = arena.batch(B, True, P)
        if cw is None:
            rc = lib.msig_train_step_multi(C.byref(desc), C.byref(m), arena.ptr("exp_avg"), arena.ptr("exp_avg_sq"), 0.9, 0.999, 1e-8, WD, s, st)
        else:
            rc = lib.msig_cw_train_step_multi(C.byref(desc), C.byref(m), cw, arena.ptr("exp_avg"), arena.ptr("exp_avg_sq"), 0.9, 0.999, 1e-8, WD, s, st)
        L.check(rc, "train_step_multi")
    arena.across("acc", 0, torch.float64, 2).zero_()
    desc = arena.batch(B, False, 0.0)
    m = arena.multi(list(range(n)))
    L.check(lib.msig_forward_multi(C.byref(desc), C.byref(m), st) if cw is None else lib.msig_cw_forward_multi(C.byref(desc), C.byref(m), cw, st),
            "forward_multi")
    torch.cuda.synchronize()
    return arena, engs


def _fold_data(n, B, Cc, K, T, steps=2):
    return [[_data(B, Cc, K, T, 1000 * f + s) for s in range(steps)] for f in range(n)]


def test_all_ones_fold_batch_is_bit_identical():
    """A 5-fold msig_cw_train_step_multi with every fold's weights = 1 against msig_train_step_multi, then the evaluation pass: every
    byte of the arenas but the weight region itself (parameters, moments, BatchNorm state, loss sums, workspace)."""
    n, B, T, Cc, K = 5, 64, 128, 6, 2
    data = _fold_data(n, B, Cc, K, T)
    a, _ = _arena_run(n, B, T, Cc, K, None, data)
    b, _ = _arena_run(n, B, T, Cc, K, [np.ones(K)] * n, data)
    cw0 = a.off["cw"][0]
    assert cw0 + a.off["cw"][1] <= a.stride and all(o + nb <= cw0 for o, nb in a.off.values() if o != cw0)
    assert torch.equal(a.mem[:, :cw0], b.mem[:, :cw0])


def test_folds_with_different_weights_equal_their_standalone_runs():
    """Folds with different weight vectors in one fold batch give each fold's stand-alone msig_cw_train_step bits (the backward GRU
    form pinned as FoldArena pins it); a fold's bits do not depend on its companions' weights."""
    n, B, T, Cc, K = 3, 64, 128, 3, 3
    data = _fold_data(n, B, Cc, K, T)
    ws = [W3, (0.5, 0.5, 2.0), (3.0, 1.0, 0.25)]
    arena, engs = _arena_run(n, B, T, Cc, K, ws, data)
    for f in range(n):
        e, _ = _engine(Cc, K, seed=10 + f)
        wt = torch.tensor(ws[f], dtype=torch.float32, device=DEV)
        for s in (1, 2):
            x, y = data[f][s - 1]
            e.train_step(x, y, LR, weight_decay=WD, step=s, dropout_p=P, seed=100 + f, class_weight=wt)
        torch.cuda.synchronize()
        for name in ("params", "exp_avg", "exp_avg_sq", "bn_state"):
            assert torch.equal(_bits(getattr(e, name)), _bits(getattr(engs[f], name))), (f, name)
    ws2 = [ws[0], (1.0, 1.0, 1.0), (7.0, 0.0, 1.0)]
    arena2, engs2 = _arena_run(n, B, T, Cc, K, ws2, data)
    assert torch.equal(arena.mem[0], arena2.mem[0])
    assert not torch.equal(arena.mem[1, :arena.off["cw"][0]], arena2.mem[1, :arena.off["cw"][0]])


def _reference(params, x, y, w, seed, step, dropout_p):
    """fp64 and fp32 runs of oracle forward + cross_entropy(weight=w) + autograd: {dtype: (loss, {key: grad})}."""
    out = {}
    xc, yc = x.cpu(), y.cpu()
    for dt in (torch.float64, torch.float32):
        leaf = {k: v.to(dt).clone().requires_grad_(v.numel() > 0) for k, v in params.items()}
        bufs = {k: (v if "num_batches" in k else v.to(dt)) for k, v in O.init_buffers().items()}
        st, _ = O.forward(leaf, bufs, xc.to(dt), training=True, dropout_p=dropout_p, seed=seed, step=step)
        loss = F.cross_entropy(st["logits"], yc, weight=torch.tensor(w, dtype=dt))
        loss.backward()
        out[dt] = (float(loss.detach()), {k: (v.grad if v.grad is not None else torch.zeros_like(v)).double().numpy() for k, v in leaf.items()})
    return out


W16 = (0.5, 2.0, 1.25, 0.3, 1.0, 3.5, 0.8, 1.6, 0.25, 2.75, 1.1, 0.6, 4.0, 0.9, 1.4, 0.7)      # K = MSIG_MAX_K
WEIGHTED = [(w, Cc, B) for B in (64, 2049) for Cc in (1, 3, 6) for w in (W2, W3)] + [(W16, Cc, 64) for Cc in (1, 3, 6)]      # W16 at B = 64 only


@pytest.mark.parametrize("model", [(64, 2), (32, 1)])
@pytest.mark.parametrize("w,Cc,B", WEIGHTED, ids=[f"w{(W2, W3, W16).index(w)}-{Cc}-{B}" for w, Cc, B in WEIGHTED])
def test_weighted_step_matches_fp64_reference(w, Cc, B, model):
    """The weighted train step's loss and parameter gradients (left in `grads` by the fused step) against torch's weighted
    CrossEntropyLoss over the fp64 oracle, within gpu_common's adaptive tolerances.  B = 64: one-launch head; B = 2049: separate
    head (129 groups of 16 rows > HEAD_WG)."""
    hidden, layers = model
    K, T = len(w), (128 if B == 64 else 32)
    e, params = _engine(Cc, K, hidden, layers, seed=Cc + K)
    x, y = _data(B, Cc, K, T, B + Cc)
    e.train_step(x, y, LR, weight_decay=WD, step=1, dropout_p=P, seed=11, class_weight=torch.tensor(w, dtype=torch.float32, device=DEV))
    torch.cuda.synchronize()
    got_loss = float(e.region("LOSS", torch.float32, (3,))[0])
    got = e.gather_grads() if layers == 1 else e.named_param_views(e.grads)
    ref = _reference(params, x, y, w, 11, 1, P)
    (l64, g64), (l32, g32) = ref[torch.float64], ref[torch.float32]
    own = abs(l32 - l64) / max(abs(l64), 1e-6)
    assert abs(got_loss - l64) / max(abs(l64), 1e-6) <= stage_tol("loss", own), (got_loss, l64)
    assert set(got) == set(g64)
    for k, g in g64.items():
        err, tol = rel_err(got[k].detach().cpu().numpy(), g), grad_tol(k, rel_err(g32[k], g))
        assert err <= tol, (k, err, tol)


@pytest.mark.parametrize("B,T", [(64, 128), (2049, 32)])
def test_staged_equals_fused(B, T):
    """msig_cw_forward(training) + msig_backward(NULL) gives msig_cw_train_step's gradient bits."""
    Cc, K = 3, 3
    x, y = _data(B, Cc, K, T, 5)
    wt = torch.tensor(W3, dtype=torch.float32, device=DEV)
    a, _ = _engine(Cc, K)
    b, _ = _engine(Cc, K)
    a.backward(a.forward(x, y, training=True, dropout_p=P, seed=5, step=1, class_weight=wt))
    b.train_step(x, y, LR, weight_decay=WD, step=1, dropout_p=P, seed=5, class_weight=wt)
    torch.cuda.synchronize()
    assert torch.equal(_bits(a.grads), _bits(b.grads))
    for r, shape in (("LOSS", (3,)), ("DLOGITS", (B, K))):
        assert torch.equal(_bits(a.region(r, torch.float32, shape)), _bits(b.region(r, torch.float32, shape))), r
    assert torch.equal(a.loss_acc, b.loss_acc)


def test_epoch_loss_sum_over_a_ragged_epoch():
    """loss_acc[0] over an epoch of 64 + 64 + 22 windows = sum_i B_i x (weighted mean of batch i), the latter computed in fp64 from
    each step's logits; WS_LOSS[1] = B x WS_LOSS[0]."""
    Cc, K, T = 3, 3, 128
    e, _ = _engine(Cc, K)
    wt = torch.tensor(W3, dtype=torch.float32, device=DEV)
    want = 0.0
    for s, Bi in enumerate((64, 64, 22), start=1):
        x, y = _data(Bi, Cc, K, T, 50 + s)
        e.train_step(x, y, LR, weight_decay=WD, step=s, dropout_p=P, seed=9, class_weight=wt)
        lg = e.region("LOGITS", torch.float32, (Bi, K)).double().cpu()
        mean = float(F.cross_entropy(lg, y.cpu(), weight=torch.tensor(W3, dtype=torch.float64)))
        want += Bi * mean
        lossbuf = e.region("LOSS", torch.float32, (3,)).double().cpu()
        assert abs(float(lossbuf[0]) - mean) <= 2e-6 * abs(mean)
        assert abs(float(lossbuf[1]) - Bi * float(lossbuf[0])) <= 1e-6 * Bi * abs(float(lossbuf[0]))
    got = float(e.loss_acc[0])
    assert abs(got - want) <= 1e-6 * abs(want), (got, want)


def test_zero_total_weight_gives_nan_like_torch():
    Cc, K, B, T = 3, 2, 16, 64
    e, _ = _engine(Cc, K)
    x, _ = _data(B, Cc, K, T, 3)
    y = torch.zeros(B, dtype=torch.int64, device=DEV)
    e.forward(x, y, training=False, class_weight=torch.tensor([0.0, 1.0], device=DEV))
    torch.cuda.synchronize()
    assert torch.isnan(e.region("LOSS", torch.float32, (3,))[:2]).all()
    assert bool(torch.isnan(F.cross_entropy(torch.zeros(B, K, dtype=torch.float64), y.cpu(), weight=torch.tensor([0.0, 1.0], dtype=torch.float64))))


def test_engine_rejects_bad_vectors_before_any_launch():
    e, _ = _engine(3, 2)
    x, y = _data(8, 3, 2, 64, 4)
    before = e.params.clone()
    for bad in (torch.tensor([1.0, -1.0], device=DEV), torch.tensor([1.0, float("nan")], device=DEV), torch.ones(3, device=DEV),
                torch.ones(2, dtype=torch.float64, device=DEV)):
        with pytest.raises(ValueError):
            e.train_step(x, y, LR, class_weight=bad)
        with pytest.raises(ValueError):
            e.forward(x, y, class_weight=bad)
    w = torch.ones(2, device=DEV)
    e.forward(x, y, class_weight=w)
    w[1] = -2.0                                              # an in-place change is seen
    with pytest.raises(ValueError):
        e.forward(x, y, class_weight=w)
    with pytest.raises(ValueError):
        FoldArena(3, 2, DEV, 1, 8, 64).set_class_weight(0, [1.0, float("inf")])
    torch.cuda.synchronize()
    assert torch.equal(before, e.params) and int(e.bn_count[0]) == 0


# ---- drivers ---------------------------------------------------------------------------------------------------------------
def _fold_outputs(root, subs, sub=""):
    out = []
    for s in subs:
        fd = root / f"fold_test_on_{s}" / sub
        info = json.loads((root / f"fold_test_on_{s}" / "fold_result.json").read_text())
        info.pop("seconds", None), info.pop("train_windows_per_s", None)
        for h in info.get("history", []):
            h.pop("seconds", None)
        out.append((info, torch.load(fd / "best_model.pt", weights_only=True)))
    return out


def _same(a, b):
    for (ia, wa), (ib, wb) in zip(a, b):
        assert ia == ib
        assert list(wa) == list(wb) and all(torch.equal(wa[k], wb[k]) for k in wa)


def _weights_logged(log):
    lines = [ln for ln in log.splitlines() if ln.startswith("已启用类别加权损失，权重为:")]
    assert len(lines) == 1, lines
    return np.array([float(v) for v in lines[0].split("[")[1].split("]")[0].split()])


def test_loso_drivers_with_balanced_weights(tmp_path):
    """--class-weights balanced on the standard LOSO: the CLI's fold batches and the sequential driver give identical per-fold results
    and checkpoints; every fold logs its own 'balanced' vector once; cv_summary.txt names the setting; the weights change the run."""
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.synth import CHANNELS6, make_synthetic_wesad
    from multimodalsignal_amd.trainer import balanced_class_weights
    subs = ["S2", "S3", "S4", "S5"]
    d = make_synthetic_wesad(tmp_path / "w", subjects=subs, windows_per_subject=30, T=256, difficulty=2.0, window_spread=3)
    names = (d / "_channel_names.txt").read_text().split()
    M.main(["--synthetic", str(d), "--samples", "256", "--subjects", *subs, "--epochs", "3", "--patience", "1", "2", "--batch-size", "16",
            "--class-weights", "balanced", "--out", str(tmp_path / "cli")])
    runs = sorted((tmp_path / "cli").glob("simple_binary/run_*"))
    assert len(runs) == 1
    cfg = M.default_cfg()
    cfg.update(data_path=d, channels=list(CHANNELS6), subjects=subs, epochs=3, patience=[1, 2], batch_size=16, concurrent_folds=1,
               class_weights="balanced")
    M.run_simple_experiment(tmp_path / "seq", DEV, names, cfg)
    _same(_fold_outputs(runs[0], subs), _fold_outputs(tmp_path / "seq", subs))
    assert "CLASS_WEIGHTS: balanced" in (runs[0] / "cv_summary.txt").read_text(encoding="utf-8")
    from multimodalsignal_amd.dataset import SubjectStore
    from multimodalsignal_amd.loso import split_train_val
    store = SubjectStore(d, subs, list(CHANNELS6), names, classification_mode="stress_binary", device=DEV)
    for s in subs:
        tr, _ = split_train_val(subs, s, cfg["seed"])
        want = balanced_class_weights(store.view(tr).labels, 2).astype(np.float32)
        for root in (runs[0], tmp_path / "seq"):
            got = _weights_logged((root / f"fold_test_on_{s}" / "training_log.txt").read_text())
            np.testing.assert_allclose(got, want, rtol=1e-6)
        assert abs(want[1] - want[0]) > 0.3                           # stress is the minority class: the weights bite
    M.run_simple_experiment(tmp_path / "plain", DEV, names, dict(cfg, class_weights="none"))
    assert "CLASS_WEIGHTS" not in (tmp_path / "plain" / "cv_summary.txt").read_text(encoding="utf-8")
    assert "类别加权" not in (tmp_path / "plain" / "fold_test_on_S2" / "training_log.txt").read_text()
    plain = _fold_outputs(tmp_path / "plain", subs)
    assert any(pa[0]["history"] != pb[0]["history"] for pa, pb in zip(plain, _fold_outputs(tmp_path / "seq", subs)))


def test_ablation_sweep_with_balanced_weights(tmp_path):
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.synth import make_synthetic_wesad
    subs = ["S2", "S3", "S4"]
    d = make_synthetic_wesad(tmp_path / "w", subjects=subs, windows_per_subject=20, T=256, difficulty=2.0)
    names = (d / "_channel_names.txt").read_text().split()
    sets = M.ablation_sets(names)
    base = M.default_cfg()
    base.update(data_path=d, subjects=subs, epochs=2, patience=20, batch_size=16, concurrent_folds=8, class_weights="balanced")
    sweep, _ = M.run_experiments(tmp_path / "sweep", DEV, names, {n: dict(base, channels=ch) for n, ch in sets.items()})
    for n in sets:
        assert "CLASS_WEIGHTS: balanced" in (tmp_path / "sweep" / n / "cv_summary.txt").read_text(encoding="utf-8")
        _weights_logged((tmp_path / "sweep" / n / "fold_test_on_S3" / "training_log.txt").read_text())
    single, _ = M.run_simple_experiment(tmp_path / "single", DEV, names, dict(base, channels=sets["eda_only"], concurrent_folds=1))
    assert [(r["subject"], r["accuracy"], r["f1_score"]) for r in sweep["eda_only"]] == [(r["subject"], r["accuracy"], r["f1_score"]) for r in single]


def test_hierarchical_with_balanced_weights(tmp_path):
    """--hierarchical with balanced weights: M1's vector from its stress_binary training labels, M2's from its amusement_binary ones;
    the fold-batched driver gives the sequential driver's results, checkpoints and summary."""
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.synth import make_synthetic_wesad
    subs = ["S2", "S3", "S4", "S5"]
    d = make_synthetic_wesad(tmp_path / "w", subjects=subs, windows_per_subject=40, T=256, difficulty=2.0)
    names = (d / "_channel_names.txt").read_text().split()
    cfg = M.default_cfg()
    cfg.update(data_path=d, subjects=subs, epochs=3, patience=[1, 2], batch_size=16, class_weights="balanced")
    res_b, _ = M.run_hierarchical_experiment(tmp_path / "batched", DEV, names, cfg)
    res_s, _ = M.run_hierarchical_experiment(tmp_path / "seq", DEV, names, dict(cfg, concurrent_folds=1))
    assert res_b == res_s
    for s in subs:
        fa, fb = tmp_path / "batched" / f"fold_test_on_{s}", tmp_path / "seq" / f"fold_test_on_{s}"
        assert json.loads((fa / "fold_result.json").read_text()) == json.loads((fb / "fold_result.json").read_text())
        vec = {}
        for tag in ("model_m1", "model_m2"):
            a = torch.load(fa / tag / "best_model.pt", weights_only=True)
            b = torch.load(fb / tag / "best_model.pt", weights_only=True)
            assert all(torch.equal(a[k], b[k]) for k in a), (s, tag)
            vec[tag] = _weights_logged((fa / tag / "training_log.txt").read_text())
            np.testing.assert_array_equal(vec[tag], _weights_logged((fb / tag / "training_log.txt").read_text()))
        assert not np.array_equal(vec["model_m1"], vec["model_m2"])
    strip = lambda r: [ln for ln in (r / "hierarchical_summary.txt").read_text(encoding="utf-8").splitlines() if not ln.startswith("wall-clock")]
    assert strip(tmp_path / "batched") == strip(tmp_path / "seq")
    assert "CLASS_WEIGHTS: balanced" in strip(tmp_path / "batched")
