"""Times integrated-gradients attribution (include/msig_at.h, multimodalsignal_amd/attribute.py) at C = 6, T = 3840, P = 32,
path_batch = 2048: the two new kernels on their own (the library's event-bracketed profile; under
`rocprofv3 --kernel-trace --stats -- python tools/attribution_timing.py` the trace has the dispatch times, summarised by
tools/kernel_trace_stats.py RESULTS.db at_), their effective bandwidth against the bytes they must move, their share of the
forward + backward of the same path batch, and the wall-clock of attributing one 270-window subject.  Prints one JSON line.

    python tools/attribution_timing.py [--steps 32] [--path-batch 2048] [--windows 270] [--reps 5]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from multimodalsignal_amd import _lib as L  # noqa: E402
from multimodalsignal_amd.attribute import Attributor, default_bin  # noqa: E402
from multimodalsignal_amd.models import CnnGruAttentionModel  # noqa: E402


def path_bytes(N, P, C, T):
    """HBM bytes msig_at_path must move: x once, xp P times (zero baseline: nothing else)."""
    return (1 + P) * N * C * T * 4


def reduce_bytes(N, P, C, T, NB, with_map):
    """HBM bytes msig_at_reduce must move: dx (P rows), x, the map when asked for, and the small outputs."""
    return (P + 1 + int(with_map)) * N * C * T * 4 + N * C * NB * 4 + N * C * 12 + N * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--path-batch", type=int, default=2048)
    ap.add_argument("--windows", type=int, default=270)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    C, T, K, P = 6, 3840, 2, a.steps
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = CnnGruAttentionModel(C, K).to(dev).eval()
    g = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn(a.windows, C, T, generator=g).to(dev)
    at = Attributor(model, steps=P, path_batch=a.path_batch)
    nb = a.path_batch // P                              # windows of a full path batch
    at.attribute(x, "predicted")                        # warm-up: workspaces, buffers
    torch.cuda.synchronize()
    walls = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        at.attribute(x, "predicted")
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    walls.sort()
    # one full path batch under the library's per-launch event brackets
    L.profile_enable(True)
    for _ in range(a.reps):
        at.attribute(x[:nb], "predicted")
    torch.cuda.synchronize()
    prof = L.profile_report()
    L.profile_enable(False)
    per = {k: ms / a.reps for k, (n, ms) in prof.items()}          # ms per attribute() call of ONE path batch
    NB = -(-T // default_bin(T))
    pb, rb = path_bytes(nb, P, C, T), reduce_bytes(nb, P, C, T, NB, True)
    new = per["at_path"] + per["at_reduce"] + per.get("at_total", 0.0)
    # the plain eval forwards of x and of the baseline launch the same kernels as the path batch's forward: they are part of `model`
    model_ms = sum(v for k, v in per.items() if not k.startswith("at_"))
    out = {"C": C, "T": T, "P": P, "path_batch": a.path_batch, "windows_per_batch": nb,
           "at_path_ms": round(per["at_path"], 5), "at_path_bytes": pb, "at_path_tb_s": round(pb / (per["at_path"] * 1e-3) / 1e12, 3),
           "at_reduce_ms": round(per["at_reduce"], 5), "at_reduce_bytes": rb, "at_reduce_tb_s": round(rb / (per["at_reduce"] * 1e-3) / 1e12, 3),
           "at_total_ms": round(per.get("at_total", 0.0), 5), "model_forward_backward_ms": round(model_ms, 4),
           "new_kernels_share_of_model": round(new / model_ms, 4), "subject_windows": a.windows,
           "subject_wall_s": round(walls[len(walls) // 2], 4), "subject_wall_s_min": round(walls[0], 4)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
