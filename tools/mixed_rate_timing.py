"""What mixed-rate pushes cost (multimodalsignal_amd/live.py with resampler=MixedResampler(...)), on one MI355X with
device events.

One live tick — every one of N sessions delivers 2.5 s of samples (host arrays) and completes one window (the stride is 2.5 s here, so
that every tick is the same work) — at N = 1, 16, 64, 256 under "expanding", the six channels of synth.CHANNELS6:
  mixed   the chest's four channels at 700 Hz, wrist_BVP at 64 Hz and wrist_EDA at 4 Hz, one msig_mx_lv_push for the 3 N chunks
          (1750 x 4 + 160 + 10 values a session);
  fir     all six columns at 700 Hz through FirResampler, msig_rs_lv_push (1750 x 6 values a session) — what a host has to send
          without per-stream rates once it has upsampled the wrist streams;
  plain   all six columns at 64 Hz, msig_lv_push (160 x 6 values a session).
Where --parent-tree names a built checkout of the parent commit, its fir and plain ticks run alongside: those code paths are meant to
be untouched, so each of this tree's must lie inside the parent's own run-to-run spread.  The tick is split in two: the append
launches alone on a staging buffer that is already on the device, and the upload of a tick's chunks alone (concatenate + copy).

Offline: MixedResampler.apply on the 40-minute synthetic streams beside FirResampler.apply on the six columns at 700 Hz.

The set-up is tools/resample_timing.py's: every variant runs in a process of its own (python tools/mixed_rate_timing.py --child ...),
the variants alternating, three runs of each; per run the median; the log gives the median of the three and their spread.

python tools/mixed_rate_timing.py [--members 3] [--parent-tree DIR] [--out profiles/mixed_rate_timing.log]
"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve()
FS, FS_RAW, WINDOW_S, STRIDE_S, CHUNK_S = 64.0, 700.0, 60.0, 2.5, 2.5
SESSIONS = (1, 16, 64, 256)
REPS = {1: 20, 16: 10, 64: 6, 256: 4}
STREAMS = (("chest", 700.0, ("chest_ECG", "chest_EDA", "chest_Resp", "chest_EMG")), ("bvp", 64.0, ("wrist_BVP",)), ("eda", 4.0, ("wrist_EDA",)))


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def child_tick(a, kind):
    """The tick, the append launches alone and the upload alone: `kind` mixed, fir or plain."""
    import ctypes as C
    import numpy as np
    import torch
    from multimodalsignal_amd import _lib as L
    from multimodalsignal_amd.live import LiveMonitor
    from multimodalsignal_amd.models import CnnGruAttentionModel
    from multimodalsignal_amd.synth import CHANNELS6
    dev = torch.device("cuda:0")
    names = list(CHANNELS6)
    kw, rate, rsm = {}, FS, None
    if kind == "fir":
        from multimodalsignal_amd.resample import FirResampler
        kw["resampler"], rate = FirResampler(FS_RAW, FS, dev), FS_RAW
        rsm = kw["resampler"]
    if kind == "mixed":
        from multimodalsignal_amd.resample import MixedResampler, Stream
        kw["resampler"] = rsm = MixedResampler([Stream(n, f, list(c)) for n, f, c in STREAMS], FS, device=dev)
    models = []
    for r in range(a.members):
        torch.manual_seed(5 + r)
        models.append(CnnGruAttentionModel(6, 2).to(dev).eval())
    rs = np.random.RandomState(0)
    pos = lambda n, c: np.abs(rs.randn(n, c)) + 0.1                 # noqa: E731  positive: chest_EDA goes through log1p
    if kind == "mixed":
        samples = lambda sec: {g.name: pos(int(round(sec * g.fs)), g.ncols) for g in rsm.streams}      # noqa: E731
    else:
        samples = lambda sec: pos(int(round(sec * rate)), 6)       # noqa: E731
    out = {"tick": {}, "launch": {}, "upload": {}, "bytes": {}}
    for N in SESSIONS:
        live = LiveMonitor(models, FS, window_s=WINDOW_S, stride_s=STRIDE_S, reference="expanding", eval_batch=256, channels=names,
                           max_sessions=N, **kw)
        for k in range(N):
            live.open(k, None if kind == "mixed" else names)
        chunks = {k: samples(CHUNK_S) for k in range(N)}            # the same host arrays every tick: the values do not matter here
        live.push({k: samples(WINDOW_S - STRIDE_S + (0 if kind == "plain" else 3.0)) for k in range(N)})      # and the resamplers' latency
        got = 0
        for _ in range(8):
            got = sum(len(u) for u in live.push(chunks).values())
        assert got == N, (got, N)                                   # steady state: one new window per session and tick
        out["tick"][str(N)] = statistics.median(timed(torch, lambda: live.push(chunks)) for _ in range(REPS[N]))
        # the append alone, on a pool of its own (the monitor's rings stay consistent): the chunks already on the device
        if kind == "mixed":
            parts = [chunks[k][g.name].reshape(-1) for k in range(N) for g in rsm.streams]
        else:
            parts = [chunks[k].reshape(-1) for k in range(N)]
        upload = lambda: torch.from_numpy(np.concatenate(parts) if len(parts) > 1 else parts[0]).to(dev)      # noqa: E731
        staging = upload()
        out["bytes"][str(N)] = int(staging.numel() * 8)
        pool = torch.zeros_like(live.pool)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        head = (pool.data_ptr(), N, live.R, pool.shape[1] * 8, 6)
        sess = (C.c_int32 * N)(*range(N))
        rows = int(CHUNK_S * rate)
        length, written = (C.c_int64 * N)(*[rows] * N), (C.c_int64 * N)(*[7 * rows] * N)
        if kind == "mixed":
            G, tails, groups = len(rsm.streams), torch.zeros_like(live.tails), rsm.groups()
            n = N * G
            sess = (C.c_int32 * n)(*[k for k in range(N) for _g in range(G)])
            group = (C.c_int32 * n)(*[g for _k in range(N) for g in range(G)])
            length = (C.c_int64 * n)(*[int(CHUNK_S * g.fs) for _k in range(N) for g in rsm.streams])
            written = (C.c_int64 * n)(*[7 * int(CHUNK_S * g.fs) for _k in range(N) for g in rsm.streams])
            call = lambda: L.check(L.lib().msig_mx_lv_push(*head, tails.data_ptr(), tails.shape[1] * 8, rsm.h.data_ptr(), groups, G, sess, group,      # noqa: E731
                                                           written, length, n, staging.data_ptr(), stream), "msig_mx_lv_push")
        elif kind == "fir":
            tails = torch.zeros_like(live.tails)
            call = lambda: L.check(L.lib().msig_rs_lv_push(*head, tails.data_ptr(), rsm.tail_rows, tails.shape[1] * 8, *rsm.ratio_args(), sess,      # noqa: E731
                                                           written, length, N, staging.data_ptr(), stream), "msig_rs_lv_push")
        else:
            call = lambda: L.check(L.lib().msig_lv_push(*head, sess, written, length, N, staging.data_ptr(), stream), "msig_lv_push")      # noqa: E731
        for _ in range(3):
            call()
        out["launch"][str(N)] = statistics.median(timed(torch, call) for _ in range(5 * REPS[N]))
        out["upload"][str(N)] = statistics.median(timed(torch, upload) for _ in range(5 * REPS[N]))
        del live
    print(json.dumps(out))


def child_offline(a):
    """MixedResampler.apply on the 40-minute synthetic streams and FirResampler.apply on six columns at 700 Hz, already on the device."""
    import numpy as np
    import torch
    from multimodalsignal_amd.monitor import SYNTHETIC_PHASES
    from multimodalsignal_amd.resample import FirResampler, MixedResampler, Stream
    from multimodalsignal_amd.synth import make_synthetic_streams
    dev = torch.device("cuda:0")
    streams = [Stream(n, f, list(c)) for n, f, c in STREAMS]
    mx = MixedResampler(streams, FS, device=dev)
    host, _table = make_synthetic_streams(SYNTHETIC_PHASES, streams, fs=FS)
    sig = {n: torch.from_numpy(x).to(dev) for n, x in host.items()}
    r = FirResampler(FS_RAW, FS, dev)
    six = torch.from_numpy(np.random.RandomState(1).randn(sig["chest"].shape[0], 6)).to(dev)
    for fn in (lambda: mx.apply(sig), lambda: r.apply(six)):
        fn()
    out = {"mixed": statistics.median(timed(torch, lambda: mx.apply(sig)) for _ in range(10)),
           "fir": statistics.median(timed(torch, lambda: r.apply(six)) for _ in range(10)),
           "rows": [{n: int(x.shape[0]) for n, x in sig.items()}, int(mx.apply(sig).shape[0]), int(six.shape[0]), r.out_count(int(six.shape[0]))]}
    print(json.dumps(out))


def child(a):
    sys.path.insert(0, str(Path(a.tree).resolve()))
    import torch
    assert torch.cuda.is_available(), "a timing needs the GPU"
    if a.child == "offline":
        return child_offline(a)
    return child_tick(a, a.child)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=3)
    ap.add_argument("--parent-tree", type=Path, default=None, help="a built checkout of the parent commit: its fir and plain ticks are timed too")
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
    variants = [("mixed 700 / 64 / 4 Hz, msig_mx_lv_push", "mixed", here), ("700 Hz, msig_rs_lv_push", "fir", here)]
    if a.parent_tree is not None:
        variants.append(("700 Hz, msig_rs_lv_push, parent commit", "fir", a.parent_tree))
    variants.append(("64 Hz, msig_lv_push", "plain", here))
    if a.parent_tree is not None:
        variants.append(("64 Hz, msig_lv_push, parent commit", "plain", a.parent_tree))
    live = {name: [] for name, _k, _t in variants}
    offline = []
    for _ in range(3):                                              # the variants alternate, run by run
        for name, kind, tree in variants:
            live[name].append(run(kind, tree))
        offline.append(run("offline", here))
    say(f"{a.members} members (cnn_gru_attention, C = 6 columns, K = 2), windows of {WINDOW_S:g} s every {STRIDE_S:g} s at {FS:g} Hz, reference "
        f"expanding, eval_batch 256, a tick of {CHUNK_S:g} s a session: mixed — " + ", ".join(f"{n} {int(CHUNK_S * f)} x {len(c)} at {f:g} Hz" for n, f, c in STREAMS) +
        f"; fir — {int(CHUNK_S * FS_RAW)} x 6 at {FS_RAW:g} Hz; plain — {int(CHUNK_S * FS)} x 6 at {FS:g} Hz; device events around calls that end "
        "synchronised; every variant in a process of its own, the variants alternating; per run the median, three runs: median (min .. max)")
    say()
    say("bytes uploaded per tick: " + "; ".join(f"N = {N}: " + ", ".join(f"{k} {live[name][0]['bytes'][str(N)]}" for name, k, t in variants if t == here)
                                                for N in SESSIONS))
    for what, title in (("tick", "one live tick, N sessions, one new window each [ms]:"),
                        ("launch", "the append launches alone, staging already on the device [ms]:"),
                        ("upload", "the upload of a tick's chunks alone (concatenate + copy) [ms]:")):
        say()
        say(title)
        for N in SESSIONS:
            say(f"  N = {N:3d}")
            for name, _k, _t in variants:
                v = [r[what][str(N)] for r in live[name]]
                say(f"    {name:<42} {statistics.median(v):9.3f}  ({min(v):.3f} .. {max(v):.3f})   runs " + " ".join(f"{x:.3f}" for x in v))
    if a.parent_tree is not None:
        say()
        say("the untouched paths: this tree's tick against the parent's own run-to-run spread [ms]:")
        for mine, theirs in (("700 Hz, msig_rs_lv_push", "700 Hz, msig_rs_lv_push, parent commit"), ("64 Hz, msig_lv_push", "64 Hz, msig_lv_push, parent commit")):
            for N in SESSIONS:
                v, p = [r["tick"][str(N)] for r in live[mine]], [r["tick"][str(N)] for r in live[theirs]]
                inside = min(p) <= statistics.median(v) <= max(p)
                say(f"    {mine:<26} N = {N:3d}: {statistics.median(v):.3f} against {min(p):.3f} .. {max(p):.3f}: {'inside' if inside else 'OUTSIDE'}")
    say()
    raw, n_mx, n_six, n_fir = offline[0]["rows"]
    say(f"offline, the 40-minute synthetic recording on the device [ms]: streams {raw}; six columns of {n_six} rows at {FS_RAW:g} Hz")
    for key, name, rows in (("mixed", "MixedResampler.apply (3 x msig_mx_resample)", n_mx), ("fir", "FirResampler.apply (msig_rs_resample)", n_fir)):
        v = [r[key] for r in offline]
        say(f"    {name:<44} {statistics.median(v):9.3f}  ({min(v):.3f} .. {max(v):.3f})   runs " + " ".join(f"{x:.3f}" for x in v) + f"   {rows} rows out")
    if a.out is not None:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
