"""Times msig_backward with and without the input gradient (msig_batch.dx) at the reference's batch (B = 64) and the bench batch
(B = 8192), C = 6, T = 3840, and the conv1_bwd_dx kernel on its own (the library's event-bracketed profile; under
`rocprofv3 --kernel-trace --stats` the trace has the dispatch times).  Prints one JSON line per batch size.

    python tools/input_grad_timing.py [--batches 64,8192] [--reps 20]
"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from multimodalsignal_amd import _lib as L  # noqa: E402
from multimodalsignal_amd.runtime import Engine  # noqa: E402
from oracle import cnn_gru_oracle as O  # noqa: E402


def dx_kernel_bytes(B, C, T):
    """HBM bytes conv1_bwd_dx moves once: y1 and dP1 (fp32, 16 channels), the pooling decisions (4 bytes per pooled position) and dx."""
    L1, P1, _, _ = O.stage_lengths(T)
    return B * L1 * 16 * 4 + B * P1 * 16 * 4 + B * P1 * 4 + B * C * T * 4


def run(B, C, T, K, reps, dev):
    eng = Engine(C, K, dev)
    eng.load_named({k: v for k, v in O.init_params(C, K, seed=3).items()})
    g = torch.Generator(device="cpu").manual_seed(B)
    x = torch.randn(B, C, T, generator=g).to(dev)
    y = torch.randint(0, K, (B,), generator=g).to(dev)
    dx = torch.empty_like(x)
    out = {"B": B, "C": C, "T": T}
    for name, want in (("backward_ms", None), ("backward_with_dx_ms", dx)):
        times = []
        for r in range(reps + 2):
            b = eng.forward(x, y, training=True, dropout_p=0.5, seed=1, step=r + 1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.backward(b, None, dx=want)
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:
                times.append(e0.elapsed_time(e1))
        times.sort()
        out[name] = round(times[len(times) // 2], 4)
        out[name + "_min"] = round(times[0], 4)
    # the new kernel alone: the library's per-launch event brackets
    b = eng.forward(x, y, training=True, dropout_p=0.5, seed=1, step=1)
    torch.cuda.synchronize()
    L.profile_enable(True)
    for _ in range(reps):
        eng.backward(b, None, dx=dx)
    torch.cuda.synchronize()
    prof = L.profile_report()
    L.profile_enable(False)
    n, ms = prof["conv1_bwd_dx"]
    k_ms = ms / n
    nbytes = dx_kernel_bytes(B, C, T)
    out.update(conv1_bwd_dx_ms=round(k_ms, 5), conv1_bwd_dx_bytes=nbytes, conv1_bwd_dx_tb_s=round(nbytes / (k_ms * 1e-3) / 1e12, 3),
               extra_ms=round(out["backward_with_dx_ms"] - out["backward_ms"], 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,8192")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for B in (int(v) for v in a.batches.split(",")):
        print(json.dumps(run(B, 6, 3840, 2, a.reps, dev)), flush=True)


if __name__ == "__main__":
    main()
