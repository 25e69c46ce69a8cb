#!/usr/bin/env python3
"""Times of the recording monitor's input side and of Monitor.run (include/msig_rec.h) on one MI355X.

1. One 40-minute, 8-column, 64 Hz recording, 60 s windows every 10 s, 6 columns selected: msig_rec_stats + msig_rec_windows (all
   windows into one (N, 6, 3840) fp32 tensor) against the materialising route — preprocess.windows_device +
   msig_nr_normalise_subject with every window as reference.  Device events around blocks of calls, the two routes alternating
   block by block, after a warm-up of both; three runs of the whole comparison.
2. Monitor.run on that recording with M = 1 and M = 15 randomly initialised members (the time does not depend on the weights): host
   clock around blocks of runs, each run ending with its results on the host, the first block of each not counted.

    python tools/recording_timing.py > profiles/recording_timing.log
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from multimodalsignal_amd.dataset import normalise_subject_device       # noqa: E402
from multimodalsignal_amd.monitor import Monitor, RecordingWindows      # noqa: E402
from multimodalsignal_amd.preprocess import windows_device              # noqa: E402

NAMES = ["chest_ECG", "chest_EDA", "chest_Resp", "chest_EMG", "wrist_BVP", "wrist_EDA", "aux_0", "aux_1"]
CHANNELS = ["aux_1", "chest_EDA", "chest_ECG", "chest_EMG", "wrist_EDA", "chest_Resp"]
FS, T, S = 64, 3840, 640


def stat(v):
    v = np.asarray(v)
    return f"median {np.median(v):.4f} (min {v.min():.4f}, max {v.max():.4f}; {len(v)} blocks)"


def recording(dev):
    L_ = 40 * 60 * FS
    rs = np.random.RandomState(0)
    sig = rs.randn(L_, len(NAMES)) * (0.5 + rs.rand(len(NAMES))) + rs.randn(len(NAMES))
    sig[:, 1] = np.exp(0.8 * rs.randn(L_)) + 0.1
    return torch.from_numpy(np.ascontiguousarray(sig)).to(dev)


def input_side(sig, blocks, calls, runs):
    cols = [NAMES.index(c) for c in CHANNELS]
    L_ = sig.shape[0]

    def direct():
        return RecordingWindows(sig, NAMES, CHANNELS, T, S).materialise()

    def materialising():
        X, _ = windows_device(sig, [(0, L_, 1)], T, S)
        return normalise_subject_device(X, cols, CHANNELS, torch.ones(X.shape[0], dtype=torch.bool, device=sig.device))

    a, b = direct(), materialising()
    torch.cuda.synchronize()
    N = a.shape[0]
    assert a.shape == b.shape == (N, len(cols), T)
    diff = float((a.double() - b.double()).abs().max())
    print(f"one recording (L, C_all) = ({L_}, {len(NAMES)}) float64, {L_ / FS / 60:.0f} min at {FS} Hz -> {N} windows of T = {T} every {S}, "
          f"C = {len(cols)} fp32, chest_EDA under log1p, every window a reference window; {calls} calls per block, the two routes alternating; "
          f"each time includes its route's allocations")
    print(f"  max |direct - materialising| over the {a.numel()} outputs: {diff:.3e} (the two routes' statistics agree to a few float64 ulps)")
    run = {"msig_rec_stats + msig_rec_windows": direct, "windows_device + msig_nr_normalise_subject": materialising}
    for f in run.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    for r in range(runs):
        ms = {k: [] for k in run}
        for _ in range(blocks):
            for k, f in run.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    f()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1) / calls)
        print(f" run {r + 1}")
        for k, v in ms.items():
            print(f"  {k}: {stat(v)} ms per call")
        keys = list(run)
        print(f"  direct / materialising: {np.median(ms[keys[0]]) / np.median(ms[keys[1]]):.3f}")
    from multimodalsignal_amd import _lib as L
    L.profile_enable(True)                      # the library's own device events around each of its kernels, 20 calls of the direct route
    for _ in range(20):
        direct()
    torch.cuda.synchronize()
    rep = L.profile_report()
    L.profile_enable(False)
    print("  kernels of the direct route, device events around each launch: "
          + ", ".join(f"{k} {ms / n * 1e3:.1f} us" for k, (n, ms) in sorted(rep.items()) if k.startswith("rec_")))
    out_mb = N * len(cols) * T * 4 / 1e6
    print(f"  bytes: the recording {L_ * len(NAMES) * 8 / 1e6:.1f} MB, the fp32 batch {out_mb:.1f} MB; the materialising route also writes and "
          f"reads twice the float64 windows, {N * T * len(NAMES) * 8 / 1e6:.1f} MB")


def monitor_runs(sig, runs, per_block=50):
    from multimodalsignal_amd.models import CnnGruAttentionModel
    dev = sig.device
    print(f"Monitor.run on the same recording (cnn_gru_attention, C = {len(CHANNELS)}, K = 2, eval_batch 256, reference 'recording'); ms per run, "
          f"host clock around blocks of {per_block} runs, each ending with its results on the host; {runs} blocks after one that is not counted")
    for M in (1, 15):
        models = []
        for r in range(M):
            torch.manual_seed(r)
            models.append(CnnGruAttentionModel(len(CHANNELS), 2).to(dev).eval())
        mon = Monitor(models, FS, channels=CHANNELS, eval_batch=256)
        t = []
        for i in range(runs + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(per_block):
                tl = mon.run(sig, NAMES)
            torch.cuda.synchronize()
            if i:
                t.append((time.perf_counter() - t0) / per_block * 1e3)
        print(f"  M = {M:>2}: median {np.median(t):.3f} ms (min {min(t):.3f}, max {max(t):.3f}) for {len(tl.t_end)} windows, "
              f"{len(tl.t_end) * M / (np.median(t) * 1e-3):.0f} member-windows/s")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("recording_timing.py needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    print("# python tools/recording_timing.py   (one MI355X, this tree)")
    print(f"device: {torch.cuda.get_device_name(0)}")
    sig = recording(dev)
    input_side(sig, args.blocks, args.calls, args.runs)
    monitor_runs(sig, args.runs)


if __name__ == "__main__":
    main()
