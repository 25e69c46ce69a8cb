"""Launches the B = 64 train step, unweighted and class-weighted (include/msig_cw.h), in its single-model form (msig_train_step /
msig_cw_train_step) and its 15-fold form (msig_train_step_multi / msig_cw_train_step_multi), C = 6, T = 3840, `--reps` times each,
for a kernel trace:

    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format rocpd -- python tools/class_weight_timing.py
    python tools/kernel_trace_stats.py OUT/.../run_results.db head_step colsum_adam ce_kernel

The kernels whose instantiation differs are head_step_kernel<CW> and colsum_adam_kernel<CW> (grid_z / grid_y = folds); everything
else is the same launch.  Also prints the wall time per step of each variant (CUDA events over the loop) as one JSON line.
"""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from multimodalsignal_amd import _lib as L  # noqa: E402
from multimodalsignal_amd.runtime import Engine, FoldArena  # noqa: E402
from oracle import cnn_gru_oracle as O  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--folds", type=int, default=15)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, Cc, T, K = 64, 6, 3840, 2
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, Cc, T, generator=g).to(dev)
    y = torch.randint(0, K, (B,), generator=g).to(dev)
    w = torch.tensor([0.7, 1.9], device=dev)
    eng = Engine(Cc, K, dev)
    eng.load_named(O.init_params(Cc, K, seed=3))
    out = {}
    for tag, cw in (("single_plain_ms", None), ("single_weighted_ms", w)):
        out[tag] = round(timed(lambda s: eng.train_step(x, y, 1e-4, weight_decay=1e-4, step=s + 1, dropout_p=0.5, seed=1, class_weight=cw), a.reps), 4)
    n = a.folds
    arena = FoldArena(Cc, K, dev, n, B, T)
    for f in range(n):
        arena.engine(f).load_named(O.init_params(Cc, K, seed=10 + f))
        arena.view(f, "x", torch.float32)[:x.numel()].copy_(x.reshape(-1))
        arena.view(f, "y", torch.int64)[:B].copy_(y)
        arena.set_class_weight(f, np.array([0.5 + 0.1 * f, 1.5]))
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    desc = arena.batch(B, True, 0.5)
    m = arena.multi(list(range(n)), key_gru=list(range(1, n + 1)), key_head=list(range(2, n + 2)), lr=[1e-4] * n)
    for tag, cw in (("folds_plain_ms", None), ("folds_weighted_ms", arena.ptr("cw"))):
        def step(s, cw=cw):
            L.check(L.lib().msig_cw_train_step_multi(C.byref(desc), C.byref(m), cw, arena.ptr("exp_avg"), arena.ptr("exp_avg_sq"),
                                                     0.9, 0.999, 1e-8, 1e-4, s + 1, st), "msig_cw_train_step_multi")
        out[tag] = round(timed(step, a.reps), 4)
    out.update(B=B, C=Cc, T=T, folds=n, reps=a.reps)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
