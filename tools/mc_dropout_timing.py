"""Times Monte-Carlo dropout (include/msig_mc.h, multimodalsignal_amd/uncertainty.py) at N = 64 windows, S = 32 samples, C = 6,
T = 3840 against its naive form — S whole eval-mode forwards model(x) of the same 64 windows — alternating the two in one process,
host clock around work that ends in a device synchronise, median of --reps.  Then one predict_mc call under the library's
event-bracketed profile (msig_profile_report): the per-launch breakdown.  Prints one JSON line.

    python tools/mc_dropout_timing.py [--windows 64] [--samples 32] [--reps 20]
    python tools/mc_dropout_timing.py --baseline-only        # the S eval forwards alone: runs on a tree without msig_mc.h
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
from multimodalsignal_amd.models import CnnGruAttentionModel  # noqa: E402


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=64)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--baseline-only", action="store_true")
    a = ap.parse_args()
    C, T, K, N, S = 6, 3840, 2, a.windows, a.samples
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = CnnGruAttentionModel(C, K).to(dev).eval()
    g = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn(N, C, T, generator=g).to(dev)

    def naive():
        with torch.no_grad():
            for _ in range(S):
                model(x)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    out = {"C": C, "T": T, "windows": N, "samples": S, "reps": a.reps}
    if a.baseline_only:
        naive()
        base = [timed(naive) for _ in range(a.reps)]
        out.update(eval_forwards_ms=round(median(base), 3), eval_forwards_ms_min=round(min(base), 3), eval_forwards_ms_max=round(max(base), 3))
        print(json.dumps(out), flush=True)
        return
    from multimodalsignal_amd.uncertainty import McDropout
    mc = McDropout(model, samples=S, seed=0)
    mc.predict(x)                                       # warm-up: workspaces, the staging buffer, code objects
    naive()
    base, mine = [], []
    for _ in range(a.reps):                             # alternating: both see the same neighbours on a shared host
        base.append(timed(naive))
        mine.append(timed(lambda: mc.predict(x)))
    L.profile_enable(True)
    mc.predict(x)
    torch.cuda.synchronize()
    prof = L.profile_report()
    L.profile_enable(False)
    eng = model.engine()
    rows = min(N, mc.chunk) * S
    out.update(chunk=mc.chunk, rows=rows,
               workspace_bytes_per_row=round(L.workspace_layout(rows, C, T, K, False)[-1] / rows),
               predict_mc_ms=round(median(mine), 3), predict_mc_ms_min=round(min(mine), 3), predict_mc_ms_max=round(max(mine), 3),
               eval_forwards_ms=round(median(base), 3), eval_forwards_ms_min=round(min(base), 3), eval_forwards_ms_max=round(max(base), 3),
               ratio=round(median(mine) / median(base), 4),
               launches={k: {"n": n, "ms": round(ms, 4)} for k, (n, ms) in prof.items()},
               launches_total_ms=round(sum(ms for _, ms in prof.values()), 4), evaluation_pool_bytes=int(eng._ws_pool[False].numel()))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
