"""GPU tier: the hierarchical experiment on fold batches.  One-layer models (M2: gru_hidden_size 32, gru_num_layers 1) in a fold
batch give the bits of their stand-alone runs, and the fold-batched hierarchical driver gives the sequential driver's results."""
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from multimodalsignal_amd import _lib as L
from multimodalsignal_amd.models import CnnGruAttentionModel
from multimodalsignal_amd.runtime import EmbeddedEngine, FoldArena

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
DEV = torch.device("cuda", 0)
LR, WD, P = 1e-3, 1e-4, 0.5


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def _one_layer_fold_batch_vs_alone(n, B, steps, adaptive, alone_bwd):
    """n one-layer folds: `steps` train steps (batch sizes) as fold batches and stand-alone, then one evaluation pass."""
    Cc, K, T = 3, 2, 256
    rs = np.random.RandomState(7 + n)
    data = [[(torch.as_tensor(rs.randn(b, Cc, T).astype(np.float32)), torch.as_tensor(rs.randint(0, K, size=(b,)))) for b in steps]
            for _ in range(n)]
    xe = [torch.as_tensor(rs.randn(B, Cc, T).astype(np.float32)) for _ in range(n)]
    seeds = [101 + f for f in range(n)]
    alone, arena_engs = [], []
    arena = FoldArena(Cc, K, DEV, n, B, T, adaptive_forms=adaptive, gru_hidden=32, gru_layers=1)
    for f in range(n):
        torch.manual_seed(seeds[f])
        m = CnnGruAttentionModel(Cc, K, gru_hidden_size=32, gru_num_layers=1).to(DEV)
        e = m.engine()
        assert isinstance(e, EmbeddedEngine)
        alone.append(e)
        a = arena.engine(f)
        assert isinstance(a, EmbeddedEngine) and a.gru_layers == 1
        a.small.copy_(e.small)
        a.scatter()
        arena_engs.append(a)
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    for s, b in enumerate(steps, start=1):
        form = alone_bwd(b)
        L.set_kernel_form("auto", form)
        try:
            for f in range(n):
                x, y = data[f][s - 1]
                alone[f].train_step(x.to(DEV), y.to(DEV), LR, weight_decay=WD, step=s, dropout_p=P, seed=seeds[f])
        finally:
            L.set_kernel_form("auto", "auto")
        for f in range(n):
            x, y = data[f][s - 1]
            arena.view(f, "x", torch.float32)[:x.numel()].copy_(x.reshape(-1).to(DEV))
            arena.view(f, "y", torch.int64)[:b].copy_(y.to(DEV))
        m = arena.multi(list(range(n)), key_gru=[L.dropout_key(sd, s, 1) for sd in seeds],
                        key_head=[L.dropout_key(sd, s, 2) for sd in seeds], lr=[LR] * n, steps=[s] * n)
        desc = arena.batch(b, True, P)
        assert desc.gru_layers == 1
        L.check(L.lib().msig_train_step_multi(C.byref(desc), C.byref(m), arena.ptr("exp_avg"), arena.ptr("exp_avg_sq"),
                                              0.9, 0.999, 1e-8, WD, s, st), "msig_train_step_multi")
    # evaluation pass (running BN statistics, no dropout)
    for f in range(n):
        alone[f].loss_acc.zero_()
        alone[f].forward(xe[f].to(DEV), data[f][0][1][:1].repeat(B).to(DEV), training=False)
        arena.view(f, "x", torch.float32)[:xe[f].numel()].copy_(xe[f].reshape(-1).to(DEV))
        arena.view(f, "y", torch.int64)[:B].copy_(data[f][0][1][:1].repeat(B).to(DEV))
    arena.across("acc", 0, torch.float64, 2).zero_()
    L.check(L.lib().msig_forward_multi(C.byref(arena.batch(B, False, 0.0)), C.byref(arena.multi(list(range(n)))), st), "msig_forward_multi")
    off = L.workspace_layout(B, Cc, T, K, False)
    logits = arena.across("ws", off[L.WS["LOGITS"]], torch.float32, B * K)
    torch.cuda.synchronize()
    for f in range(n):
        e, a = alone[f], arena_engs[f]
        a.gather()
        for (k, va), vb in zip(a.small_views().items(), e.small_views().values()):
            assert torch.equal(_bits(va), _bits(vb)), (f, k)
        for name in ("exp_avg", "exp_avg_sq"):
            ma, mb = getattr(a, name), getattr(e, name)
            assert torch.equal(_bits(ma[a.index]), _bits(mb[e.index])), (f, name)
            assert not ma[a.padding].any(), (f, name, "padding")
        assert not a.params[a.padding].any() and not a.grads[a.padding].any(), (f, "padding")
        for k, v in a.bn_views().items():
            assert torch.equal(_bits(v), _bits(e.bn_views()[k])), (f, k)
        assert int(a.bn_count[0]) == len(steps)
        assert torch.equal(logits[f].view(B, K).contiguous().view(torch.int32),
                           e.region("LOGITS", torch.float32, (B, K)).contiguous().view(torch.int32)), (f, "logits")
        assert torch.equal(a.loss_acc, e.loss_acc), (f, "loss_acc")
    return alone


def test_one_layer_fold_batch_equals_standalone_runs():
    """Three one-layer arenas, three steps of 64 and a ragged one of 16 (latency backward form, as pinned by FoldArena.multi), then
    an evaluation pass: every bit of the stand-alone EmbeddedEngine runs; the padding of every arena stays exactly zero."""
    alone = _one_layer_fold_batch_vs_alone(3, 64, [64, 64, 64, 16], False, lambda b: "auto")
    assert float(alone[0].small.abs().max()) > 0


def test_one_layer_fold_batch_fused_backward_forms():
    """adaptive_forms with 4 folds x 64 windows (16 tiles per launch: the fused backward kernels run) against stand-alone runs pinned
    to the same backward form (gru_bwd_b6 for full steps; the ragged step of 16 has 4 tiles per launch: the latency form)."""
    _one_layer_fold_batch_vs_alone(4, 64, [64, 64, 64, 16], True, lambda b: "b6" if b == 64 else "split")


def test_one_layer_large_evaluation_batch():
    """An evaluation pass of 1024 windows per fold (64 tiles per fold, gru_fwd_ws) over two one-layer arenas."""
    _one_layer_fold_batch_vs_alone(2, 1024, [64], False, lambda b: "auto")


def _hier_cfg(d, subs, **kw):
    from multimodalsignal_amd import main as M
    cfg = M.default_cfg()
    cfg.update(data_path=d, subjects=subs, epochs=4, patience=[1, 2], batch_size=16, **kw)
    return cfg


def _compare_runs(ra, rb, subs):
    for s in subs:
        fa, fb = ra / f"fold_test_on_{s}", rb / f"fold_test_on_{s}"
        assert json.loads((fa / "fold_result.json").read_text()) == json.loads((fb / "fold_result.json").read_text()), s
        for tag in ("model_m1", "model_m2"):
            a = torch.load(fa / tag / "best_model.pt", weights_only=True, map_location="cpu")
            b = torch.load(fb / tag / "best_model.pt", weights_only=True, map_location="cpu")
            assert list(a) == list(b)
            for k in a:
                assert torch.equal(a[k], b[k]), (s, tag, k)
    strip = lambda r: [ln for ln in (r / "hierarchical_summary.txt").read_text(encoding="utf-8").splitlines() if not ln.startswith("wall-clock")]
    assert strip(ra) == strip(rb)


def test_hierarchical_fold_batches_equal_sequential(tmp_path, monkeypatch):
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd import multifold
    from multimodalsignal_amd.synth import make_synthetic_wesad
    subs = ["S2", "S3", "S4", "S5", "S6"]
    d = make_synthetic_wesad(tmp_path / "w", subjects=subs, windows_per_subject=40, T=256, difficulty=2.0)
    names = (d / "_channel_names.txt").read_text().split()
    calls = []
    real_run = multifold.LockstepTrainer.run

    def counted(self, *a, **k):
        calls.append(tuple(int(getattr(p["model"], "gru_num_layers")) for p in self.preps))
        return real_run(self, *a, **k)
    monkeypatch.setattr(multifold.LockstepTrainer, "run", counted)
    res_b, _ = M.run_hierarchical_experiment(tmp_path / "batched", DEV, names, _hier_cfg(d, subs))
    assert calls and sorted(sum(calls, ())) == [1] * 5 + [2] * 5, calls
    assert all(len(set(c)) == 1 for c in calls)                     # every fold batch uniform in depth
    n_calls = len(calls)
    res_s, _ = M.run_hierarchical_experiment(tmp_path / "seq", DEV, names, _hier_cfg(d, subs, concurrent_folds=1))
    assert len(calls) == n_calls                                    # the sequential driver does not go through LockstepTrainer
    assert res_b == res_s
    _compare_runs(tmp_path / "batched", tmp_path / "seq", subs)
    sd2 = torch.load(tmp_path / "batched" / "fold_test_on_S3" / "model_m2" / "best_model.pt", weights_only=True)
    assert tuple(sd2["gru.weight_hh_l0"].shape) == (96, 32) and "gru.weight_ih_l1" not in sd2
    assert not (tmp_path / "batched" / "fold_test_on_S3" / "model_m1" / "fold_result.json").exists()


def test_zero_epoch_budget_through_fold_batches(tmp_path):
    """epochs = 0 in the fold-batch driver: every fold goes straight to its test pass, as in the sequential one."""
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.synth import make_synthetic_wesad
    subs = ["S2", "S3", "S4"]
    d = make_synthetic_wesad(tmp_path / "w", subjects=subs, windows_per_subject=20, T=256, difficulty=2.0)
    names = (d / "_channel_names.txt").read_text().split()
    cfg = M.default_cfg()
    cfg.update(data_path=d, subjects=subs, epochs=0, patience=2, batch_size=16, concurrent_folds=3)
    batched, _ = M.run_simple_experiment(tmp_path / "b", DEV, names, cfg)
    seq, _ = M.run_simple_experiment(tmp_path / "s", DEV, names, dict(cfg, concurrent_folds=1))
    assert [(r["subject"], r["accuracy"], r["f1_score"]) for r in batched] == [(r["subject"], r["accuracy"], r["f1_score"]) for r in seq]


def _run_main(world, out, data):
    env = dict(os.environ, MSIG_DIST_BACKEND="gloo", PYTHONPATH=str(ROOT))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    args = ["--hierarchical", "--synthetic", str(data), "--synthetic-windows", "30", "--window-spread", "4", "--samples", "256",
            "--difficulty", "4", "--subjects", "S2", "S3", "S4", "S5", "S6", "--epochs", "5", "--patience", "1", "2", "3",
            "--batch-size", "16", "--out", str(out)]
    if world == 1:
        cmd = [sys.executable, "-m", "multimodalsignal_amd.main", *args]
    else:
        import socket
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), "-m", "multimodalsignal_amd.main", *args]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=800, cwd=str(ROOT))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    runs = sorted(Path(out).glob("simple_binary/run_*"))
    assert len(runs) == 1, runs
    return runs[0]


@pytest.mark.timeout(1500)
def test_hierarchical_results_do_not_depend_on_sharding(tmp_path):
    data = tmp_path / "w"
    r1 = _run_main(1, tmp_path / "o1", data)
    r2 = _run_main(2, tmp_path / "o2", data)          # folds dealt round-robin: rank 0 gets 3, rank 1 gets 2
    _compare_runs(r1, r2, ["S2", "S3", "S4", "S5", "S6"])
