"""What gap-tolerant monitoring costs (multimodalsignal_amd/live.py with gaps=Gaps(...)), on one MI355X with
device events.

One live tick — every one of N sessions delivers one stride of samples (host arrays) and completes one window — at N = 1, 16, 64,
256 under "expanding" and "decayed:60", in three variants: gaps off (msig_rn_lv_step / msig_rd_lv_step, as ever), gaps on with
nothing missing, and gaps on with 5 % of the samples dropped (NaN).  Where --parent-tree names a built checkout of the parent commit,
its gaps-off tick runs alongside: that code path is untouched, so the two must agree within their own spread.

The set-up is tools/running_timing.py's: every variant runs in a process of its own (python tools/gaps_timing.py --child ...), the
variants alternating, three runs of each; per run the median tick; the log gives the median of the three and their spread.

python tools/gaps_timing.py [--members 3] [--parent-tree DIR] [--out profiles/gaps_timing.log]
"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve()
FS, WINDOW_S, STRIDE_S = 64.0, 60.0, 10.0
SESSIONS = (1, 16, 64, 256)
REPS = {1: 20, 16: 10, 64: 6, 256: 4}
REFERENCES = ("expanding", "decayed:60")


def child(a):
    """One variant in this process: `reference|off`, `reference|on` or `reference|drop`; prints one JSON line."""
    sys.path.insert(0, str(Path(a.tree).resolve()))
    import numpy as np
    import torch
    from multimodalsignal_amd.live import LiveMonitor
    from multimodalsignal_amd.models import CnnGruAttentionModel
    from multimodalsignal_amd.synth import CHANNELS6
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    names = list(CHANNELS6) + ["spare_a", "spare_b"]                # 8 columns, the models read 6
    T, S = int(WINDOW_S * FS), int(STRIDE_S * FS)
    reference, variant = a.child.split("|")
    kw = {}
    if variant != "off":
        from multimodalsignal_amd.reference import Gaps
        kw["gaps"] = Gaps()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    models = []
    for r in range(a.members):
        torch.manual_seed(5 + r)
        models.append(CnnGruAttentionModel(6, 2).to(dev).eval())
    rs = np.random.RandomState(0)

    def samples(n):
        x = np.abs(rs.randn(n, 8)) + 0.1                            # positive: chest_EDA goes through log1p
        if variant == "drop":
            x[rs.rand(n, 8) < 0.05] = np.nan
        return x

    out = {}
    for N in SESSIONS:
        live = LiveMonitor(models, FS, window_s=WINDOW_S, stride_s=STRIDE_S, reference=reference, eval_batch=256, channels=list(CHANNELS6),
                           max_sessions=N, **kw)
        for k in range(N):
            live.open(k, names)
        chunks = {k: samples(S) for k in range(N)}                  # the same host arrays every tick: the values do not matter here
        live.push({k: samples(T - S) for k in range(N)})
        got = 0
        for _ in range(8):
            got = sum(len(u) for u in live.push(chunks).values())
        assert got == N, (got, N)                                   # steady state: one new window per session and tick
        out[str(N)] = statistics.median(timed(lambda: live.push(chunks)) for _ in range(REPS[N]))
        del live
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=3)
    ap.add_argument("--parent-tree", type=Path, default=None, help="a built checkout of the parent commit: its gaps-off tick is timed too")
    ap.add_argument("--out", type=Path, default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=str(HERE.parent.parent), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        return child(a)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def run(kind, tree):
        r = subprocess.run([sys.executable, str(HERE), "--child", kind, "--tree", str(tree), "--members", str(a.members)], check=True,
                           capture_output=True, text=True, timeout=600)
        print(f"  done: {kind} from {tree}", file=sys.stderr, flush=True)
        return json.loads(r.stdout.strip().splitlines()[-1])

    here = HERE.parent.parent
    variants = []
    for ref in REFERENCES:
        variants.append((f"{ref}, gaps off", f"{ref}|off", here))
        if a.parent_tree is not None:
            variants.append((f"{ref}, gaps off, parent commit", f"{ref}|off", a.parent_tree))
        variants += [(f"{ref}, gaps on, nothing missing", f"{ref}|on", here), (f"{ref}, gaps on, 5 % dropped", f"{ref}|drop", here)]
    live = {name: [] for name, _k, _t in variants}
    for _ in range(3):                                              # the variants alternate, run by run
        for name, kind, tree in variants:
            live[name].append(run(kind, tree))
    say(f"{a.members} members (cnn_gru_attention, C = 6 of 8 columns, K = 2), T = {int(WINDOW_S * FS)}, S = {int(STRIDE_S * FS)}, fs = {FS:g}, eval_batch 256; "
        "device events around calls that end synchronised; every variant in a process of its own, the variants alternating; per run the "
        "median tick, three runs: median (min .. max)")
    say()
    say("one live tick, N sessions, one new window each [ms]:")
    for N in SESSIONS:
        say(f"  N = {N:3d}")
        for name, _k, _t in variants:
            v = [r[str(N)] for r in live[name]]
            say(f"    {name:<40} {statistics.median(v):9.3f}  ({min(v):.3f} .. {max(v):.3f})   runs " + " ".join(f"{x:.3f}" for x in v)
                + f"   {statistics.median(v) / N * 1e3:8.1f} us per session")
    if a.out is not None:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
