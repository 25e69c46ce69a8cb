"""Cost of soft targets (include/msig_st.h; DESIGN.md section 17, profiles/soft_target_timing.log).

    python tools/soft_target_timing.py                  the three gathers (plain / augmenting / augmenting + mixing) and the train
                                                        step with (label smoothing 0.1, mixup) against off
    python tools/soft_target_timing.py --loso DIR [E]   the synthetic 15-fold LOSO with and without --label-smoothing 0.1 --mixup 0.2,
                                                        twice each, alternating; E: exactly E epochs per fold (no early stop), so
                                                        that both sides do the same work

HIP events, warm-up, medians; run from the repository root."""
import ctypes as C
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd.augment import Augment
from multimodalsignal_amd.runtime import Engine, FoldArena

DEV = torch.device("cuda", 0)
lib = L.lib()
ALL = Augment(scale=0.1, jitter=0.05, mask_prob=0.5, mask_max=320, chan_drop=0.1)
Cn, T, K = 6, 3840, 2
EPS, LAM = 0.1, 0.3


def timed(fn, reps=30, warm=5, inner=1):
    st = torch.cuda.current_stream(DEV)
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        for _ in range(inner):
            fn()
        b.record(st)
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / inner)
    return statistics.median(ts), min(ts), max(ts)


def report(tag, fns, nbytes=None):
    base = None
    for name, fn, inner in fns:
        assert fn() in (0, None)
        med, lo, hi = timed(fn, inner=inner)
        base = base or med
        bw = f"  {nbytes / med / 1e6:7.3f} TB/s" if nbytes else ""
        print(f"{tag:28s} {name:16s} median {med:9.2f} us  (min {lo:9.2f}, max {hi:9.2f}){bw}  x{med / base:5.2f} of the first", flush=True)


def gathers(B, folds, nstore, inner):
    store = torch.randn(nstore, Cn, T, device=DEV)
    sy = torch.zeros(nstore, dtype=torch.int64, device=DEV)
    idx = torch.randint(0, nstore, (folds, B), device=DEV)
    stride = (B * Cn * T * 4 + 8 * B + 4096 + 255) // 256 * 256
    mem = torch.empty(folds, stride, dtype=torch.uint8, device=DEV)
    xo, yo = mem.data_ptr(), mem.data_ptr() + B * Cn * T * 4 + 256
    m = L.Multi()
    m.n, m.stride_bytes = folds, stride
    for z in range(folds):
        m.slot[z] = z
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    a = ALL.struct(range(1, folds + 1))
    lam = (C.c_float * L.MAX_FOLDS)(*([LAM] * folds))
    plain = lambda: lib.msig_gather_windows_multi(store.data_ptr(), sy.data_ptr(), idx.data_ptr(), B, B, Cn * T, xo, yo, C.byref(m), st)
    aug = lambda: lib.msig_aug_gather_windows_multi(store.data_ptr(), sy.data_ptr(), idx.data_ptr(), B, B, Cn, T, xo, yo, C.byref(m), C.byref(a), st)
    mix = lambda: lib.msig_st_gather_windows_multi(store.data_ptr(), sy.data_ptr(), idx.data_ptr(), B, B, Cn, T, xo, yo, C.byref(m), None, lam, st)
    augmix = lambda: lib.msig_st_gather_windows_multi(store.data_ptr(), sy.data_ptr(), idx.data_ptr(), B, B, Cn, T, xo, yo, C.byref(m), C.byref(a), lam, st)
    report(f"gather {folds} x B={B}", [("plain", plain, inner), ("aug", aug, inner), ("mix", mix, inner), ("aug + mix", augmix, inner)],
           2 * folds * B * Cn * T * 4)


def single_step(B):
    x = torch.randn(B, Cn, T, device=DEV)
    y = torch.randint(0, K, (B,), device=DEV)
    fns = []
    for name, kw in (("off", {}), ("eps 0.1", dict(label_smoothing=EPS)), ("eps 0.1 + mixup", dict(label_smoothing=EPS, mix_lambda=LAM))):
        e = Engine(Cn, K, DEV)
        e.params.normal_(0.0, 0.05)
        step = [0]

        def fn(e=e, kw=kw, step=step):
            step[0] += 1
            e.train_step(x, y, 1e-3, step=step[0], dropout_p=0.5, seed=1, **kw)
        fns.append((name, fn, 5))
    report(f"train step B={B}", fns)


def fold_step(B, folds):
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    fns = []
    for name, soft in (("off", None), ("eps 0.1 + mixup", (EPS, [LAM] * folds))):
        arena = FoldArena(Cn, K, DEV, folds, B, T)
        for f in range(folds):
            arena.engine(f).params.normal_(0.0, 0.05)
            arena.view(f, "x", torch.float32)[:B * Cn * T].normal_()
            arena.view(f, "y", torch.int64)[:B].copy_(torch.randint(0, K, (B,), device=DEV))
        slots = list(range(folds))
        desc = arena.batch(B, True, 0.5)
        sd = arena.soft(slots, *soft) if soft else None
        step = [0]

        def fn(arena=arena, sd=sd, step=step, desc=desc):
            step[0] += 1
            m = arena.multi(slots, key_gru=[step[0]] * folds, key_head=[step[0] + 7] * folds, lr=[1e-3] * folds, steps=[step[0]] * folds)
            if sd is None:
                return lib.msig_train_step_multi(C.byref(desc), C.byref(m), arena.ptr("exp_avg"), arena.ptr("exp_avg_sq"), 0.9, 0.999, 1e-8, 0.0,
                                                 step[0], st)
            return lib.msig_st_train_step_multi(C.byref(desc), C.byref(m), C.byref(sd), arena.ptr("exp_avg"), arena.ptr("exp_avg_sq"), 0.9, 0.999,
                                                1e-8, 0.0, step[0], st)
        fns.append((name, fn, 5))
    report(f"fold step {folds} x B={B}", fns)


def loso(data_dir, epochs=None):
    import json
    import tempfile
    from multimodalsignal_amd import main as M
    flags = ["--label-smoothing", "0.1", "--mixup", "0.2"]
    common = ["--synthetic", str(data_dir), "--difficulty", "2"] + (["--epochs", str(epochs), "--patience", "100000"] if epochs else [])
    print(f"synthetic LOSO (15 subjects x 270 windows, C=6 T=3840, B=64, fold batches), {' '.join(flags)} vs none", flush=True)
    with tempfile.TemporaryDirectory() as out:
        M.main(common + ["--epochs", "2", "--out", out + "/warm"])                       # data generation, first-launch costs
        for rep in range(2):
            for tag, extra in (("off", []), ("soft", flags)):
                results, wall = M.main(common + extra + ["--out", f"{out}/{tag}{rep}"])
                run = next(Path(f"{out}/{tag}{rep}").glob("*/run_*"))
                infos = [json.loads(p.read_text()) for p in sorted(run.glob("fold_test_on_*/fold_result.json"))]
                n_ep = sum(i["epochs"] for i in infos)
                acc = sum(r["accuracy"] for r in results) / len(results)
                print(f"  {tag:5s} run {rep}: wall {wall:6.2f} s, {n_ep:4d} fold-epochs, {1e3 * wall / n_ep:6.2f} ms per fold-epoch, "
                      f"mean accuracy {acc:.4f}", flush=True)


if len(sys.argv) > 2 and sys.argv[1] == "--loso":
    loso(Path(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else None)
    sys.exit(0)

print(f"soft-target timings, C={Cn} T={T}, {torch.cuda.get_device_name(0)}; median of 30 event-timed repetitions after 5 warm-ups "
      f"(B=64 gathers: 20 back-to-back launches per repetition, steps: 5); TB/s = (bytes read + written by the plain gather) / time", flush=True)
gathers(64, 1, 4050, 20)
gathers(64, 15, 4050, 20)
gathers(8192, 1, 4050, 1)
single_step(64)
fold_step(64, 15)
torch.cuda.synchronize()
