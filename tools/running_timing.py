"""What the causal running references cost (multimodalsignal_amd/live.py and monitor.py), on one MI355X with
device events.

1. One live tick — every one of N sessions delivers one stride of samples (host arrays) and completes one window — at N = 1, 16,
   64, 256 under "expanding" and "trailing:180" (timed in steady state: after 180 windows per session, so that every window adds
   its full 180 records), beside "head:6" from this tree and, where --parent-tree names a built checkout of the parent commit,
   "head:6" from that tree: its code path is untouched, so the two must agree within their own spread.
2. The offline RecordingWindows construction plus the fill of all 235 windows of the 40-minute synthetic recording under
   "recording", "head:6", "expanding" and "trailing:180".

Every variant runs in a process of its own (python tools/running_timing.py --child ...), the variants alternating, three runs of
each; per run the median tick; the log gives the median of the three and their spread (min .. max).

python tools/running_timing.py [--members 3] [--parent-tree DIR] [--out profiles/running_timing.log]
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
OFFLINE = ("recording", "head:6", "expanding", "trailing:180")


def child(a):
    """One variant in this process; prints one JSON line."""
    sys.path.insert(0, str(Path(a.tree).resolve()))
    import numpy as np
    import torch
    from multimodalsignal_amd.live import LiveMonitor
    from multimodalsignal_amd.models import CnnGruAttentionModel
    from multimodalsignal_amd.monitor import RecordingWindows
    from multimodalsignal_amd.synth import CHANNELS6, make_synthetic_recording
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    names = list(CHANNELS6) + ["spare_a", "spare_b"]                # 8 columns, the models read 6
    T, S = int(WINDOW_S * FS), int(STRIDE_S * FS)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    out = {}
    if a.child == "offline":
        from multimodalsignal_amd.monitor import SYNTHETIC_PHASES
        sig, _table = make_synthetic_recording(SYNTHETIC_PHASES, fs=FS, channels=list(CHANNELS6), seed=42, difficulty=1.0)
        sig = torch.from_numpy(np.ascontiguousarray(sig, dtype=np.float64)).to(dev)
        for ref in OFFLINE:
            n = RecordingWindows(sig, list(CHANNELS6), list(CHANNELS6), T, S, ref).n
            x = torch.empty((n, 6, T), dtype=torch.float32, device=dev)

            def build(ref=ref, x=x, n=n):
                RecordingWindows(sig, list(CHANNELS6), list(CHANNELS6), T, S, ref).batch(0, n, x)

            for _ in range(3):
                build()
            out[ref] = {"windows": n, "ms": statistics.median(timed(build) for _ in range(20))}
        print(json.dumps(out))
        return
    models = []
    for r in range(a.members):
        torch.manual_seed(5 + r)
        models.append(CnnGruAttentionModel(6, 2).to(dev).eval())
    rs = np.random.RandomState(0)
    warm = 180 if a.child.startswith("trailing") else 6             # windows per session before a tick is timed
    for N in SESSIONS:
        live = LiveMonitor(models, FS, window_s=WINDOW_S, stride_s=STRIDE_S, reference=a.child, eval_batch=256, channels=list(CHANNELS6),
                           max_sessions=N)
        for k in range(N):
            live.open(k, names)
        chunks = {k: rs.randn(S, 8) for k in range(N)}              # the same host arrays every tick: the values do not matter here
        live.push({k: rs.randn(T - S, 8) for k in range(N)})
        got = 0
        for _ in range(warm + 2):
            got = sum(len(u) for u in live.push(chunks).values())
        assert got == N, (got, N)                                   # steady state: one new window per session and tick
        ticks = [timed(lambda: live.push(chunks)) for _ in range(REPS[N])]
        out[str(N)] = statistics.median(ticks)
        del live
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=3)
    ap.add_argument("--parent-tree", type=Path, default=None, help="a built checkout of the parent commit: head:6 is timed from it too")
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
    variants = [("head:6", "head:6", here), ("expanding", "expanding", here), ("trailing:180", "trailing:180", here)]
    if a.parent_tree is not None:
        variants.insert(1, ("head:6, parent commit", "head:6", a.parent_tree))
    live = {name: [] for name, _k, _t in variants}
    offline = []
    for _ in range(3):                                              # the variants alternate, run by run
        for name, kind, tree in variants:
            live[name].append(run(kind, tree))
        offline.append(run("offline", here))
    say(f"{a.members} members (cnn_gru_attention, C = 6 of 8 columns, K = 2), T = {int(WINDOW_S * FS)}, S = {int(STRIDE_S * FS)}, fs = {FS:g}, eval_batch 256; "
        "device events around calls that end synchronised; every variant in a process of its own, the variants alternating; per run the "
        "median tick, three runs: median (min .. max)")
    say()
    say("one live tick, N sessions, one new window each [ms]:")
    for N in SESSIONS:
        say(f"  N = {N:3d}")
        for name, _k, _t in variants:
            v = [r[str(N)] for r in live[name]]
            say(f"    {name:<24} {statistics.median(v):9.3f}  ({min(v):.3f} .. {max(v):.3f})   runs " + " ".join(f"{x:.3f}" for x in v)
                + f"   {statistics.median(v) / N * 1e3:8.1f} us per session")
    say()
    say("RecordingWindows construction + fill of every window of the 40-minute synthetic recording [ms]:")
    for ref in OFFLINE:
        v = [r[ref]["ms"] for r in offline]
        say(f"  {ref:<14} {offline[0][ref]['windows']} windows  {statistics.median(v):9.3f}  ({min(v):.3f} .. {max(v):.3f})   runs "
            + " ".join(f"{x:.3f}" for x in v))
    if a.out is not None:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
