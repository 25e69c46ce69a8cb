"""Cost of the augmenting gather (include/msig_aug.h; DESIGN.md section 16, profiles/augment_timing.log).

    python tools/augment_timing.py                  the plain gather vs the augmenting gather (all four transforms / jitter off)
    python tools/augment_timing.py --loso DIR [E]   the synthetic 15-fold LOSO with and without --augment, twice each, alternating;
                                                    E: exactly E epochs per fold (no early stop), so that both sides do the same work

HIP events, warm-up, medians; run from the repository root."""
import ctypes as C
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd.augment import Augment

DEV = torch.device("cuda", 0)
lib = L.lib()
ALL = Augment(scale=0.1, jitter=0.05, mask_prob=0.5, mask_max=320, chan_drop=0.1)
NOJ = Augment(scale=0.1, mask_prob=0.5, mask_max=320, chan_drop=0.1)
Cn, T = 6, 3840


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


def report(tag, B, folds, fns):
    nbytes = 2 * folds * B * Cn * T * 4
    base = None
    for name, fn, inner in fns:
        med, lo, hi = timed(fn, inner=inner)
        base = base or med
        print(f"{tag:28s} {name:14s} median {med:9.2f} us  (min {lo:9.2f}, max {hi:9.2f})  {nbytes / med / 1e6:7.3f} TB/s  x{med / base:5.2f} of plain", flush=True)


def single(B, nstore, inner):
    store = torch.randn(nstore, Cn, T, device=DEV)
    sy = torch.zeros(nstore, dtype=torch.int64, device=DEV)
    idx = torch.randint(0, nstore, (B,), device=DEV)
    ox = torch.empty(B, Cn, T, device=DEV)
    oy = torch.empty(B, dtype=torch.int64, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    a_all, a_noj = ALL.struct([123]), NOJ.struct([123])
    plain = lambda: lib.msig_gather_windows(store.data_ptr(), sy.data_ptr(), idx.data_ptr(), B, Cn * T, ox.data_ptr(), oy.data_ptr(), st)
    aug = lambda a: (lambda: lib.msig_aug_gather_windows(store.data_ptr(), sy.data_ptr(), idx.data_ptr(), B, Cn, T, ox.data_ptr(), oy.data_ptr(), C.byref(a), st))
    for f in (plain, aug(a_all), aug(a_noj)):
        assert f() == 0
    report(f"single B={B}", B, 1, [("plain", plain, inner), ("aug all four", aug(a_all), inner), ("aug no jitter", aug(a_noj), inner)])


def multi(B, folds, nstore, inner):
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
    a_all, a_noj = ALL.struct(range(1, folds + 1)), NOJ.struct(range(1, folds + 1))
    plain = lambda: lib.msig_gather_windows_multi(store.data_ptr(), sy.data_ptr(), idx.data_ptr(), B, B, Cn * T, xo, yo, C.byref(m), st)
    aug = lambda a: (lambda: lib.msig_aug_gather_windows_multi(store.data_ptr(), sy.data_ptr(), idx.data_ptr(), B, B, Cn, T, xo, yo, C.byref(m), C.byref(a), st))
    for f in (plain, aug(a_all), aug(a_noj)):
        assert f() == 0
    report(f"multi {folds} folds x B={B}", B, folds, [("plain", plain, inner), ("aug all four", aug(a_all), inner), ("aug no jitter", aug(a_noj), inner)])


def loso(data_dir, epochs=None):
    import json
    import tempfile
    from multimodalsignal_amd import main as M
    spec = "scale=0.1,jitter=0.05,mask=0.5:320,chandrop=0.1"
    common = ["--synthetic", str(data_dir), "--difficulty", "2"] + (["--epochs", str(epochs), "--patience", "100000"] if epochs else [])
    print(f"synthetic LOSO (15 subjects x 270 windows, C=6 T=3840, B=64, fold batches), --augment {spec} vs none", flush=True)
    with tempfile.TemporaryDirectory() as out:
        M.main(common + ["--epochs", "2", "--out", out + "/warm"])                       # data generation, first-launch costs
        for rep in range(2):
            for tag, extra in (("plain", []), ("augment", ["--augment", spec])):
                results, wall = M.main(common + extra + ["--out", f"{out}/{tag}{rep}"])
                run = next(Path(f"{out}/{tag}{rep}").glob("*/run_*"))
                infos = [json.loads(p.read_text()) for p in sorted(run.glob("fold_test_on_*/fold_result.json"))]
                epochs = sum(i["epochs"] for i in infos)
                acc = sum(r["accuracy"] for r in results) / len(results)
                print(f"  {tag:8s} run {rep}: wall {wall:6.2f} s, {epochs:4d} fold-epochs, {1e3 * wall / epochs:6.2f} ms per fold-epoch, "
                      f"mean accuracy {acc:.4f}", flush=True)


if len(sys.argv) > 2 and sys.argv[1] == "--loso":
    loso(Path(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else None)
    sys.exit(0)

print(f"gather timings, C={Cn} T={T}, {torch.cuda.get_device_name(0)}; median of 30 event-timed repetitions after 5 warm-ups "
      f"(B=64 cases: 20 back-to-back launches per repetition); TB/s = (bytes read + written) / time", flush=True)
single(64, 4050, 20)
multi(64, 15, 4050, 20)
single(8192, 4050, 1)
torch.cuda.synchronize()
