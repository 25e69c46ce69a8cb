"""What the supervised contrastive term (include/msig_sc.h) costs a fused train step at B = 64, C = 6, T = 3840:

  - the single-model step and a 15-fold fold batch, each as "off" (the step without the option: the yardstick), "probe" (weight 0:
    the loss is measured, the gradient contraction is skipped) and "on" (weight 0.1, cross-subject positives, 11 subjects as in a
    WESAD fold).  The variants ALTERNATE in blocks inside one process — A B C A B C ... — each block timed by HIP events after a
    warm-up, so drift of the clocks hits them alike; reported per variant: median, minimum and the spread (max - min) over the blocks,
    and the difference of the medians against "off" beside the spread of "off" itself;
  - --without-only: the "off" columns alone, through calls that exist without msig_sc.h — the same script then runs on a tree that
    does not have the option, which is how "the step without the flag did not get slower" is checked against the parent commit;
  - the term's own two kernels from the library's per-kernel HIP events (msig_profile_report), in a short block of their own, and
    once more through msig_sc_apply alone at B = 64 and at the limit B = 2048.
Every case ends with the last step's loss, which must be finite.

    python tools/supcon_timing.py > profiles/supcon_timing.log
"""
import argparse
import ctypes as C
import json
import math
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from multimodalsignal_amd import _lib as L  # noqa: E402
from multimodalsignal_amd.runtime import Engine, FoldArena  # noqa: E402

SUBJECTS = 11


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
        rec[k] = dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), spread_ms=round(max(v) - min(v), 4),
                      runs_ms=[round(t, 4) for t in v])
        if k != "off":
            rec[k]["minus_off_us"] = round(1e3 * (statistics.median(v) - med_off), 2)
    return rec


def kernel_us(fn, reps):
    """Mean time of each of the term's two launches over `reps` calls, from the library's own per-kernel events."""
    L.profile_enable(True)
    try:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        rep = L.profile_report()
    finally:
        L.profile_enable(False)
    return {k: round(1e3 * rep[k][1] / rep[k][0], 2) for k in ("sc_rows", "sc_grad")}


def single(dev, reps, blocks, warmup, g, without_only):
    Cc, T, K, B = 6, 3840, 2, 64
    x = torch.randn(B, Cc, T, generator=g).to(dev)
    y = torch.randint(0, K, (B,), generator=g).to(dev)
    eng = Engine(Cc, K, dev)
    torch.manual_seed(3)
    eng.params.normal_(0.0, 0.05)
    step = [0]

    def make(**kw):
        def fn():
            step[0] += 1
            eng.train_step(x, y, 1e-4, weight_decay=1e-4, step=step[0], dropout_p=0.5, seed=1, **kw)
        return fn
    fns = {"off": make()}
    if not without_only:
        from multimodalsignal_amd.supcon import SupCon
        table = np.arange(B, dtype=np.int32) % SUBJECTS
        for name, w in (("probe", 0.0), ("on", 0.1)):
            fns[name] = make(supcon=SupCon(w, 0.1, "cross-subject").set_subjects(table).bind(dev, max_batch=B))
    rec = summary(f"single B={B}", alternate(fns, reps, blocks, warmup))
    if not without_only:
        rec["kernel_us"] = kernel_us(fns["on"], 20)
    rec["final_loss"] = float(eng.region("LOSS")[0])
    assert math.isfinite(rec["final_loss"]), rec
    eng.drop_workspaces()
    return rec


def folds(dev, n, reps, blocks, warmup, g, without_only):
    Cc, T, K, B = 6, 3840, 2, 64
    x = torch.randn(B, Cc, T, generator=g).to(dev)
    y = torch.randint(0, K, (B,), generator=g).to(dev)
    arena = FoldArena(Cc, K, dev, n, B, T) if without_only else FoldArena(Cc, K, dev, n, B, T, supcon=B)
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
    fns = {"off": off}
    if not without_only:
        from multimodalsignal_amd.supcon import SupCon
        table = np.arange(B, dtype=np.int32) % SUBJECTS
        for f in range(n):
            SupCon(0.1, 0.1, "cross-subject").set_subjects(table).bind(dev, arena.side_storage("supcon", f))
        sd = arena.soft(slots, 0.0)

        def make(w):
            d = arena.sc("cross-subject", 0.1, [w] * n)

            def fn():
                step[0] += 1
                L.check(lib.msig_sc_train_step_multi(C.byref(desc), C.byref(m), C.byref(sd), None, None, None, None, C.byref(d), ea, eas, 0.9,
                                                     0.999, 1e-8, 1e-4, step[0], st), "msig_sc_train_step_multi")
            return fn
        fns.update(probe=make(0.0), on=make(0.1))
    rec = summary(f"{n} folds B={B}", alternate(fns, reps, blocks, warmup))
    if not without_only:
        rec["kernel_us"] = kernel_us(fns["on"], 20)
    off()
    torch.cuda.synchronize()
    losses = arena.across("ws", L.workspace_layout(B, Cc, T, K, True)[L.WS["LOSS"]], torch.float32, 1).cpu().reshape(-1).tolist()
    rec["final_loss_min"], rec["final_loss_max"] = min(losses), max(losses)
    assert all(math.isfinite(v) for v in losses), losses
    return rec


def alone(dev, B, g):
    """The two kernels through msig_sc_apply on random features: B = 64 is a step's, B = 2048 the limit (1.6 GFLOP in three contractions)."""
    from multimodalsignal_amd.supcon import SupCon
    K = 2
    feat = torch.randn(B, 128, generator=g).to(dev)
    y = torch.randint(0, K, (B,), generator=g).to(dev)
    dfeat = torch.zeros(B, 128, device=dev)
    sc = SupCon(0.1, 0.1, "cross-subject").set_subjects(np.arange(B, dtype=np.int32) % SUBJECTS).bind(dev, max_batch=B)
    d = sc.descriptor()

    def fn():
        L.check(L.lib().msig_sc_apply(C.byref(d), feat.data_ptr(), y.data_ptr(), dfeat.data_ptr(), B, K, None), "msig_sc_apply")
    for _ in range(5):
        fn()
    rec = dict(case=f"msig_sc_apply B={B}", kernel_us=kernel_us(fn, 50), loss=float(sc.stats[0] / sc.stats[1]))
    assert math.isfinite(rec["loss"]) and bool(torch.isfinite(dfeat).all()), rec
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200, help="steps per timed block")
    ap.add_argument("--blocks", type=int, default=3, help="blocks (runs) per variant")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--folds", type=int, default=15)
    ap.add_argument("--without-only", action="store_true", help="the 'off' columns alone (runs on a tree without msig_sc.h)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    print(json.dumps(single(dev, a.reps, a.blocks, a.warmup, g, a.without_only)), flush=True)
    print(json.dumps(folds(dev, a.folds, a.reps, a.blocks, a.warmup, g, a.without_only)), flush=True)
    if not a.without_only:
        for B in (64, 2048):
            print(json.dumps(alone(dev, B, g)), flush=True)


if __name__ == "__main__":
    main()
