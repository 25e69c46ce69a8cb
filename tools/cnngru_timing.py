"""Train-step cost of the cnn_gru baseline (include/msig_cg.h) against CnnGruAttentionModel, C = 6, T = 3840:

  - the single-model fused step (msig_train_step / msig_cg_train_step) at B = 64 and B = 8192, wall time per step (HIP events over
    `--reps` steps) and, from one profiled step each, the gate kernels' times (msig_profile_enable: gate, gate_eo, gate_bwd);
  - the eval forward at B = 64 (the gate launch the baseline drops);
  - a 15-fold B = 64 fold batch (msig_train_step_multi / msig_cg_train_step_multi);
  - with --data, the 15-fold synthetic LOSO with --model cnn_gru_attention cnn_gru as one job (a child process).

    python tools/cnngru_timing.py [--data /tmp/synth] > profiles/cnngru_timing.log
"""
import argparse
import ctypes as C
import json
import subprocess
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from multimodalsignal_amd import _lib as L  # noqa: E402
from multimodalsignal_amd.runtime import Engine, FoldArena  # noqa: E402

KINDS = ("cnn_gru_attention", "cnn_gru")
GATE_KERNELS = ("gate", "gate_eo", "gate_bwd")


def timed(fn, reps):
    for _ in range(3):
        fn(0)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for r in range(reps):
        fn(r + 1)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def profiled(fn):
    """{kernel: ms} of the gate kernels in one call, and the call's launch count."""
    torch.cuda.synchronize()
    L.profile_enable(True)
    fn(0)
    torch.cuda.synchronize()
    rep = L.profile_report()
    L.profile_enable(False)
    return {k: round(rep[k][1] * 1e3, 1) for k in GATE_KERNELS if k in rep}, sum(c for c, _ in rep.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--folds", type=int, default=15)
    ap.add_argument("--data", type=Path, default=None, help="synthetic set for the LOSO comparison run (generated if missing)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    Cc, T, K = 6, 3840, 2
    g = torch.Generator().manual_seed(0)
    out = {"C": Cc, "T": T, "reps": a.reps}
    for B in (64, 8192):
        x = torch.randn(B, Cc, T, generator=g).to(dev)
        y = torch.randint(0, K, (B,), generator=g).to(dev)
        reps = a.reps if B <= 64 else max(10, a.reps // 5)
        for kind in KINDS:
            eng = Engine(Cc, K, dev, kind=kind)
            torch.manual_seed(3)
            eng.params.normal_(0.0, 0.05)
            step = lambda s: eng.train_step(x, y, 1e-4, weight_decay=1e-4, step=s + 1, dropout_p=0.5, seed=1)
            out[f"B{B}_{kind}_step_ms"] = round(timed(step, reps), 4)
            out[f"B{B}_{kind}_step_gate_us"], out[f"B{B}_{kind}_step_launches"] = profiled(step)
            if B == 64:
                ev = lambda s: eng.forward(x, y, training=False)
                out[f"B{B}_{kind}_eval_ms"] = round(timed(ev, reps), 4)
                out[f"B{B}_{kind}_eval_gate_us"], out[f"B{B}_{kind}_eval_launches"] = profiled(ev)
            eng.drop_workspaces()
            del eng
            torch.cuda.empty_cache()
        del x, y
    n, B = a.folds, 64
    x = torch.randn(B, Cc, T, generator=g).to(dev)
    y = torch.randint(0, K, (B,), generator=g).to(dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for kind in KINDS:
        arena = FoldArena(Cc, K, dev, n, B, T, kind=kind)
        for f in range(n):
            arena.view(f, "params", torch.float32).normal_(0.0, 0.05)
            arena.view(f, "x", torch.float32)[:x.numel()].copy_(x.reshape(-1))
            arena.view(f, "y", torch.int64)[:B].copy_(y)
        desc = arena.batch(B, True, 0.5)
        m = arena.multi(list(range(n)), key_gru=list(range(1, n + 1)), key_head=list(range(2, n + 2)), lr=[1e-4] * n)
        fn = L.lib().msig_cg_train_step_multi if kind == "cnn_gru" else L.lib().msig_cw_train_step_multi

        def step(s):
            L.check(fn(C.byref(desc), C.byref(m), None, arena.ptr("exp_avg"), arena.ptr("exp_avg_sq"), 0.9, 0.999, 1e-8, 1e-4, s + 1, st),
                    fn.__name__)
        out[f"folds{n}_B{B}_{kind}_step_ms"] = round(timed(step, a.reps), 4)
        del arena
    print(json.dumps(out), flush=True)
    if a.data is not None:
        with __import__("tempfile").TemporaryDirectory() as tmp:
            cmd = [sys.executable, "-m", "multimodalsignal_amd.main", "--synthetic", str(a.data), "--model", *KINDS, "--out", tmp]
            t0 = time.time()
            r = subprocess.run(cmd, cwd=str(ROOT), capture_output=True, text=True)
            wall = time.time() - t0
            tail = [ln for ln in r.stdout.splitlines() if "wall-clock" in ln or "平均准确率" in ln]
            print("\n".join(tail[-3:]))
            runs = sorted(Path(tmp).glob("simple_binary/run_*"))
            if r.returncode != 0 or not runs:
                print(r.stdout[-2000:], r.stderr[-2000:])
                raise SystemExit(r.returncode or 1)
            cmp = json.loads((runs[-1] / "comparison.json").read_text())
            print((runs[-1] / "comparison.txt").read_text(encoding="utf-8"))
            st_ = cmp["sets"][""]["summary"]
            print(json.dumps({"loso_two_kinds_process_s": round(wall, 1), "folds": cmp["sets"][""]["n_folds"],
                              "acc_mean": {k: round(v["accuracy"]["mean"], 4) for k, v in st_.items()}}), flush=True)


if __name__ == "__main__":
    main()
