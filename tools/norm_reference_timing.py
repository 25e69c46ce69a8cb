#!/usr/bin/env python3
"""Times of the reference-masked normalisation (include/msig_nr.h) on one MI355X.

1. msig_nr_normalise_subject against msig_normalise_subject on the same (270, 3840, 8) float64 subject, 6 of its 8 columns
   selected: device events around blocks of calls, the two calls alternating block by block, after a warm-up of both.
2. The SubjectStore build time (read, normalise, upload) of the synthetic 15-subject set under --normalise host and device, for
   each reference; host clock around a build that ends in a device synchronise, the first build of each path not counted.

    python tools/norm_reference_timing.py --work /tmp/norm_reference_timing > profiles/norm_reference_timing.log
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from multimodalsignal_amd.dataset import SubjectStore, normalise_subject_device, reference_mask      # noqa: E402
from multimodalsignal_amd.synth import ALL_SUBJECTS, CHANNELS6, make_synthetic_wesad                   # noqa: E402


def stat(v):
    v = np.asarray(v)
    return f"median {np.median(v):.4f} (min {v.min():.4f}, max {v.max():.4f}; {len(v)} blocks)"


def kernel_times(dev, blocks, calls):
    N, T, C_all, cols = 270, 3840, 8, [7, 1, 0, 3, 5, 2]
    names = ["chest_ECG", "chest_EDA", "chest_Resp", "chest_EMG", "wrist_BVP", "wrist_EDA", "aux_0", "aux_1"]
    rs = np.random.RandomState(0)
    raw = rs.randn(N, T, C_all) * (0.5 + rs.rand(C_all)) + rs.randn(C_all)
    raw[:, :, 1] = np.exp(0.8 * rs.randn(N, T)) + 0.1
    y = rs.choice([1, 2, 3, 4], size=N, p=[0.4, 0.2, 0.13, 0.27])
    ref = torch.from_numpy(reference_mask(y, "baseline")).to(dev)
    x = torch.from_numpy(raw).to(dev)
    sel = [names[c] for c in cols]
    run = {"msig_normalise_subject": lambda: normalise_subject_device(x, cols, sel),
           "msig_nr_normalise_subject": lambda: normalise_subject_device(x, cols, sel, ref)}
    for f in run.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in run}
    for _ in range(blocks):
        for k, f in run.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / calls)
    gb = (2 * N * T * C_all * 8 + N * len(cols) * T * 4) / 1e9          # two passes over the raw rows, one store of the output
    print(f"one subject (N, T, C_all) = ({N}, {T}, {C_all}) float64 -> C = {len(cols)} fp32, chest_EDA under log1p, {int(ref.sum())} reference "
          f"windows; {calls} calls per block, the two calls alternating; the time includes each call's output and scratch allocation")
    for k, v in ms.items():
        print(f"  {k}: {stat(v)} ms per call = {gb / (np.median(v) * 1e-3):.0f} GB/s of the {gb * 1e3:.1f} MB the three launches move")
    print(f"  msig_nr_normalise_subject / msig_normalise_subject: {np.median(ms['msig_nr_normalise_subject']) / np.median(ms['msig_normalise_subject']):.3f}")


def store_times(dev, work, runs):
    data = work / "synthetic"
    if not (data / "_channel_names.txt").exists():
        make_synthetic_wesad(data)
    names = [ln.strip() for ln in open(data / "_channel_names.txt") if ln.strip()]
    print(f"SubjectStore of the synthetic set: {len(ALL_SUBJECTS)} subjects x 270 windows, T = 3840, C = {len(CHANNELS6)}; seconds per build "
          f"(files in the page cache; {runs} builds after one that is not counted)")
    import contextlib
    import io
    for path in ("host", "device"):
        for reference in ("subject", "baseline", "baseline:6"):
            t = []
            for i in range(runs + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    SubjectStore(data, ALL_SUBJECTS, list(CHANNELS6), names, device=dev, normalise=path, reference=reference)
                torch.cuda.synchronize()
                if i:
                    t.append(time.perf_counter() - t0)
            print(f"  --normalise {path:<6} --norm-reference {reference:<10}: median {np.median(t):.3f} s (min {min(t):.3f}, max {max(t):.3f})")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--work", type=Path, required=True, help="scratch directory (the synthetic set is written here if missing)")
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--store-runs", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("norm_reference_timing.py needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    print("# python tools/norm_reference_timing.py --work WORKDIR   (one MI355X, this tree)")
    print(f"device: {torch.cuda.get_device_name(0)}")
    kernel_times(dev, args.blocks, args.calls)
    store_times(dev, args.work, args.store_runs)


if __name__ == "__main__":
    main()
