"""What gradient-norm clipping (include/msig_gc.h) costs a fused train step, C = 6, T = 3840:

  - the single-model step at B = 64 and at B = 8192, and a 15-fold B = 64 fold batch, each as "off" (the unclipped step: the
    yardstick), "inf" (msig_gc_train_step with max_norm = inf: the two launches, nothing clipped) and "clip" (max_norm below the
    norm).  The variants ALTERNATE in blocks inside one process — A B C A B C ... — each block timed by HIP events after a warm-up,
    so drift of the clocks hits them alike; reported per variant: median, minimum and the spread (max - min) over the blocks,
    and the difference of the medians against "off" beside the spread of "off" itself;
  - --kernels: one short block of each variant at B = 64 (single model and fold batch), for `rocprofv3 --kernel-trace --stats --
    python tools/grad_clip_timing.py --kernels` (a run of its own: colsum_sq_kernel and clip_adam_kernel of the clipped steps
    beside colsum_adam_kernel of the unclipped ones).
Every case ends with the last step's gradient norm and loss, which must be finite: the steps share one model on random data, and a
run that had diverged would time a degenerate clip.

    python tools/grad_clip_timing.py > profiles/grad_clip_timing.log
"""
import argparse
import ctypes as C
import json
import math
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from multimodalsignal_amd import _lib as L  # noqa: E402
from multimodalsignal_amd.runtime import Engine, FoldArena  # noqa: E402

VARIANTS = ("off", "inf", "clip")


def block_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(fns, reps, blocks, warmup):
    """{variant: [ms per step of each block]}, the variants taking turns block by block."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(blocks):
        for k, fn in fns.items():
            out[k].append(block_ms(fn, reps))
    return out


def summary(tag, times):
    rec = {"case": tag}
    med_off = statistics.median(times["off"])
    for k, v in times.items():
        rec[k] = dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), spread_ms=round(max(v) - min(v), 4))
        if k != "off":
            rec[k]["minus_off_ms"] = round(statistics.median(v) - med_off, 4)
    return rec


def single(dev, B, reps, blocks, warmup, g):
    Cc, T, K = 6, 3840, 2
    x = torch.randn(B, Cc, T, generator=g).to(dev)
    y = torch.randint(0, K, (B,), generator=g).to(dev)
    eng = Engine(Cc, K, dev)
    torch.manual_seed(3)
    eng.params.normal_(0.0, 0.05)
    step = [0]

    def make(mn):
        def fn():
            step[0] += 1
            eng.train_step(x, y, 1e-4, weight_decay=1e-4, step=step[0], dropout_p=0.5, seed=1, max_grad_norm=mn)
        return fn
    make(float("inf"))()
    torch.cuda.synchronize()
    norm = eng.grad_stats()["last"]
    rec = summary(f"single B={B}", alternate({"off": make(None), "inf": make(float("inf")), "clip": make(0.5 * norm)}, reps, blocks, warmup))
    rec["norm"] = norm
    make(0.5 * norm)()
    torch.cuda.synchronize()
    rec["final_norm"], rec["final_loss"] = eng.grad_stats()["last"], float(eng.region("LOSS")[0])
    assert math.isfinite(rec["final_norm"]) and math.isfinite(rec["final_loss"]), rec
    eng.drop_workspaces()
    return rec


def folds(dev, n, reps, blocks, warmup, g):
    Cc, T, K, B = 6, 3840, 2, 64
    x = torch.randn(B, Cc, T, generator=g).to(dev)
    y = torch.randint(0, K, (B,), generator=g).to(dev)
    arena = FoldArena(Cc, K, dev, n, B, T, grad_clip=True)
    for f in range(n):
        arena.view(f, "params", torch.float32).normal_(0.0, 0.05)
        arena.view(f, "x", torch.float32)[:x.numel()].copy_(x.reshape(-1))
        arena.view(f, "y", torch.int64)[:B].copy_(y)
    desc = arena.batch(B, True, 0.5)
    slots = list(range(n))
    m = arena.multi(slots, key_gru=list(range(1, n + 1)), key_head=list(range(2, n + 2)), lr=[1e-4] * n)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lib, ea, eas = L.lib(), arena.ptr("exp_avg"), arena.ptr("exp_avg_sq")
    step = [0]

    def off():
        step[0] += 1
        L.check(lib.msig_train_step_multi(C.byref(desc), C.byref(m), ea, eas, 0.9, 0.999, 1e-8, 1e-4, step[0], st), "msig_train_step_multi")

    def make():
        g_ = arena.clip(slots)

        def fn():
            step[0] += 1
            L.check(lib.msig_gc_train_step_multi(C.byref(desc), C.byref(m), C.byref(g_), ea, eas, 0.9, 0.999, 1e-8, 1e-4, step[0], st),
                    "msig_gc_train_step_multi")
        return fn
    inf = make()
    inf()
    torch.cuda.synchronize()
    for f in range(n):
        arena.set_max_norm(f, 0.5 * arena.grad_stats(f)["last"])
    rec = summary(f"{n} folds B={B}", alternate({"off": off, "inf": inf, "clip": make()}, reps, blocks, warmup))
    make()()
    torch.cuda.synchronize()
    last = [arena.grad_stats(f)["last"] for f in range(n)]
    rec["final_norm_min"], rec["final_norm_max"] = min(last), max(last)
    assert all(math.isfinite(v) for v in last), last
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40, help="steps per timed block")
    ap.add_argument("--blocks", type=int, default=9, help="blocks per variant")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--folds", type=int, default=15)
    ap.add_argument("--kernels", action="store_true", help="one short block of each variant at B = 64 only, for a kernel trace")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    if a.kernels:
        print(json.dumps(single(dev, 64, 20, 1, 5, g)), flush=True)
        print(json.dumps(folds(dev, a.folds, 20, 1, 5, g)), flush=True)
        return
    print(json.dumps(single(dev, 64, a.reps, a.blocks, a.warmup, g)), flush=True)
    print(json.dumps(folds(dev, a.folds, a.reps, a.blocks, a.warmup, g)), flush=True)
    print(json.dumps(single(dev, 8192, max(2, a.reps // 10), a.blocks, 2, g)), flush=True)


if __name__ == "__main__":
    main()
