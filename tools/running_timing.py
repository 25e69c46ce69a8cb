"""What the causal running references cost (multimodalsignal_amd/live.py, monitor.py and dataset.py, DESIGN.md sections 36 and 37), on
one MI355X with device events.

1. One live tick — every one of N sessions delivers one stride of samples (host arrays) and completes one window — at N = 1, 16,
   64, 256 under "expanding", "trailing:180" and "decayed:60" (timed in steady state: after 180 windows per session, so that every
   window adds its full 180 records), beside "head:6" from this tree and, where --parent-tree names a built checkout of the parent commit,
   "head:6" from that tree: its code path is untouched, so the two must agree within their own spread.
2. The offline RecordingWindows construction plus the fill of all 235 windows of the 40-minute synthetic recording under
   "recording", "head:6", "expanding", "trailing:180" and "decayed:60".
3. With --store-work DIR: the device store build (dataset.SubjectStore(normalise="device"): file reads, uploads and kernels, wall
   clock around a build that ends synchronised) of the synthetic 15-subject set, generated into DIR if it is not there, under
   --norm-reference subject, baseline:6, expanding, trailing:60 and decayed:60.

Every variant runs in a process of its own (python tools/running_timing.py --child ...), the variants alternating, three runs of
each; per run the median tick; the log gives the median of the three and their spread (min .. max).

python tools/running_timing.py [--members 3] [--parent-tree DIR] [--store-work DIR] [--out profiles/decayed_timing.log]
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
OFFLINE = ("recording", "head:6", "expanding", "trailing:180", "decayed:60")
STORE = ("subject", "baseline:6", "expanding", "trailing:60", "decayed:60")


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
    if a.child == "store":
        import time
        from multimodalsignal_amd.dataset import SubjectStore
        from multimodalsignal_amd.synth import ALL_SUBJECTS, make_synthetic_wesad
        work = Path(a.store_work)
        if not (work / "_channel_names.txt").exists():
            make_synthetic_wesad(work)
        all_names = (work / "_channel_names.txt").read_text().split()

        def build(ref):
            t0 = time.perf_counter()
            st = SubjectStore(work, list(ALL_SUBJECTS), list(CHANNELS6), all_names, device=dev, normalise="device", reference=ref)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, int(st.x.shape[0])

        import contextlib
        import io
        with contextlib.redirect_stdout(io.StringIO()):             # the store names every subject's reference windows
            build("subject")                                        # the files into the page cache, the kernels loaded
            for ref in STORE:
                t = [build(ref) for _ in range(3)]
                out[ref] = {"windows": t[0][1], "ms": statistics.median(v for v, _n in t)}
        print(json.dumps(out))
        return
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
    ap.add_argument("--store-work", type=Path, default=None, help="time the device store build of the synthetic 15-subject set kept here")
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
        r = subprocess.run([sys.executable, str(HERE), "--child", kind, "--tree", str(tree), "--members", str(a.members)]
                           + (["--store-work", str(a.store_work)] if a.store_work is not None else []), check=True,
                           capture_output=True, text=True, timeout=600)
        print(f"  done: {kind} from {tree}", file=sys.stderr, flush=True)
        return json.loads(r.stdout.strip().splitlines()[-1])

    here = HERE.parent.parent
    variants = [("head:6", "head:6", here), ("expanding", "expanding", here), ("trailing:180", "trailing:180", here),
                ("decayed:60", "decayed:60", here)]
    if a.parent_tree is not None:
        variants.insert(1, ("head:6, parent commit", "head:6", a.parent_tree))
    live = {name: [] for name, _k, _t in variants}
    offline, store = [], []
    for _ in range(3):                                              # the variants alternate, run by run
        for name, kind, tree in variants:
            live[name].append(run(kind, tree))
        offline.append(run("offline", here))
        if a.store_work is not None:
            store.append(run("store", here))
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
    if store:
        say()
        say("device store build of the synthetic 15-subject set, SubjectStore(normalise=\"device\"), per run the median of three builds [ms]:")
        base = statistics.median(r["subject"]["ms"] for r in store)
        for ref in STORE:
            v = [r[ref]["ms"] for r in store]
            say(f"  {ref:<14} {store[0][ref]['windows']} windows  {statistics.median(v):9.1f}  ({min(v):.1f} .. {max(v):.1f})   runs "
                + " ".join(f"{x:.1f}" for x in v) + f"   {statistics.median(v) / base:.3f} x subject")
    if a.out is not None:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
