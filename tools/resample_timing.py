"""What raw-rate pushes cost (multimodalsignal_amd/live.py with resampler=FirResampler(700, 64)), on one MI355X
with device events.

One live tick — every one of N sessions delivers 2.5 s of samples (host arrays) and completes one window (the stride is 2.5 s here, so
that every tick is the same work) — at N = 1, 16, 64, 256 under "expanding": at the models' rate (160 rows a session, msig_lv_push, as
ever) and at 700 Hz through the resampler (1750 rows a session, msig_rs_lv_push).  Where --parent-tree names a built checkout of the
parent commit, its 64 Hz tick runs alongside: that code path is untouched, so the two must agree within their own spread.  The added
cost is split in two: the append launches alone on a staging buffer that is already on the device (msig_lv_push's one against
msig_rs_lv_push's pair), and the upload of a tick's chunks alone (concatenate + host-to-device copy), which grows by 700 / 64.

Offline: FirResampler.apply on a 40-minute, 8-column recording at 700 Hz beside preprocess.resample_device (the FFT method) on the same.

The set-up is tools/gaps_timing.py's: every variant runs in a process of its own (python tools/resample_timing.py --child ...), the
variants alternating, three runs of each; per run the median; the log gives the median of the three and their spread.

python tools/resample_timing.py [--members 3] [--parent-tree DIR] [--out profiles/resample_timing.log]
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


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def child_tick(a, fir):
    """The tick, the append launches alone and the upload alone, at 64 Hz (`fir` False) or at 700 Hz through the resampler."""
    import ctypes as C
    import numpy as np
    import torch
    from multimodalsignal_amd import _lib as L
    from multimodalsignal_amd.live import LiveMonitor
    from multimodalsignal_amd.models import CnnGruAttentionModel
    from multimodalsignal_amd.synth import CHANNELS6
    dev = torch.device("cuda:0")
    names = list(CHANNELS6) + ["spare_a", "spare_b"]                # 8 columns, the models read 6
    kw, rate = {}, FS
    if fir:
        from multimodalsignal_amd.resample import FirResampler
        kw["resampler"], rate = FirResampler(FS_RAW, FS, dev), FS_RAW
    rows = int(CHUNK_S * rate)
    models = []
    for r in range(a.members):
        torch.manual_seed(5 + r)
        models.append(CnnGruAttentionModel(6, 2).to(dev).eval())
    rs = np.random.RandomState(0)
    samples = lambda n: np.abs(rs.randn(n, 8)) + 0.1                # noqa: E731  positive: chest_EDA goes through log1p
    out = {"tick": {}, "launch": {}, "upload": {}}
    for N in SESSIONS:
        live = LiveMonitor(models, FS, window_s=WINDOW_S, stride_s=STRIDE_S, reference="expanding", eval_batch=256, channels=list(CHANNELS6),
                           max_sessions=N, **kw)
        for k in range(N):
            live.open(k, names)
        chunks = {k: samples(rows) for k in range(N)}               # the same host arrays every tick: the values do not matter here
        live.push({k: samples(int((WINDOW_S - STRIDE_S) * rate) + (300 if fir else 0)) for k in range(N)})
        got = 0
        for _ in range(8):
            got = sum(len(u) for u in live.push(chunks).values())
        assert got == N, (got, N)                                   # steady state: one new window per session and tick
        out["tick"][str(N)] = statistics.median(timed(torch, lambda: live.push(chunks)) for _ in range(REPS[N]))
        # the append alone, on a pool of its own (the monitor's rings stay consistent): the chunks already on the device
        parts = list(chunks.values())
        upload = lambda: torch.from_numpy(np.concatenate(parts) if N > 1 else parts[0]).to(dev)      # noqa: E731
        staging = upload()
        pool = torch.zeros_like(live.pool)
        sess = (C.c_int32 * N)(*range(N))
        length = (C.c_int64 * N)(*[rows] * N)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        head = (pool.data_ptr(), N, live.R, pool.shape[1] * 8, 8)
        if fir:
            rsm = kw["resampler"]
            tails = torch.zeros_like(live.tails)
            written = (C.c_int64 * N)(*[7 * rows] * N)
            call = lambda: L.check(L.lib().msig_rs_lv_push(*head, tails.data_ptr(), rsm.tail_rows, tails.shape[1] * 8, *rsm.ratio_args(), sess,      # noqa: E731
                                                           written, length, N, staging.data_ptr(), stream), "msig_rs_lv_push")
        else:
            written = (C.c_int64 * N)(*[7 * rows] * N)
            call = lambda: L.check(L.lib().msig_lv_push(*head, sess, written, length, N, staging.data_ptr(), stream), "msig_lv_push")      # noqa: E731
        for _ in range(3):
            call()
        out["launch"][str(N)] = statistics.median(timed(torch, call) for _ in range(5 * REPS[N]))
        out["upload"][str(N)] = statistics.median(timed(torch, upload) for _ in range(5 * REPS[N]))
        del live
    print(json.dumps(out))


def child_offline(a):
    """FirResampler.apply and resample_device on a 40-minute recording at 700 Hz, 8 columns, already on the device."""
    import numpy as np
    import torch
    from multimodalsignal_amd.preprocess import resample_device
    from multimodalsignal_amd.resample import FirResampler
    dev = torch.device("cuda:0")
    n = int(40 * 60 * FS_RAW)
    sig = torch.from_numpy(np.random.RandomState(1).randn(n, 8)).to(dev)
    r = FirResampler(FS_RAW, FS, dev)
    num = int(n * (FS / FS_RAW))
    for fn in (lambda: r.apply(sig), lambda: resample_device(sig, num)):
        fn()
    out = {"fir": statistics.median(timed(torch, lambda: r.apply(sig)) for _ in range(10)),
           "fft": statistics.median(timed(torch, lambda: resample_device(sig, num)) for _ in range(10)),
           "rows": [n, r.out_count(n), num]}
    print(json.dumps(out))


def child(a):
    sys.path.insert(0, str(Path(a.tree).resolve()))
    import torch
    assert torch.cuda.is_available(), "a timing needs the GPU"
    if a.child == "offline":
        return child_offline(a)
    return child_tick(a, a.child == "fir")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=3)
    ap.add_argument("--parent-tree", type=Path, default=None, help="a built checkout of the parent commit: its 64 Hz tick is timed too")
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
    variants = [("64 Hz, msig_lv_push", "plain", here)]
    if a.parent_tree is not None:
        variants.append(("64 Hz, msig_lv_push, parent commit", "plain", a.parent_tree))
    variants.append(("700 Hz, msig_rs_lv_push", "fir", here))
    live = {name: [] for name, _k, _t in variants}
    offline = []
    for _ in range(3):                                              # the variants alternate, run by run
        for name, kind, tree in variants:
            live[name].append(run(kind, tree))
        offline.append(run("offline", here))
    say(f"{a.members} members (cnn_gru_attention, C = 6 of 8 columns, K = 2), windows of {WINDOW_S:g} s every {STRIDE_S:g} s at {FS:g} Hz, reference "
        f"expanding, eval_batch 256, a tick of {CHUNK_S:g} s: {int(CHUNK_S * FS)} rows a session at {FS:g} Hz, {int(CHUNK_S * FS_RAW)} at {FS_RAW:g} Hz; "
        "device events around calls that end synchronised; every variant in a process of its own, the variants alternating; per run the "
        "median, three runs: median (min .. max)")
    for what, title in (("tick", "one live tick, N sessions, one new window each [ms]:"),
                        ("launch", "the append launches alone, staging already on the device [ms]:"),
                        ("upload", "the upload of a tick's chunks alone (concatenate + copy) [ms]:")):
        say()
        say(title)
        for N in SESSIONS:
            say(f"  N = {N:3d}")
            for name, _k, _t in variants:
                v = [r[what][str(N)] for r in live[name]]
                say(f"    {name:<40} {statistics.median(v):9.3f}  ({min(v):.3f} .. {max(v):.3f})   runs " + " ".join(f"{x:.3f}" for x in v))
    say()
    n, n_fir, n_fft = offline[0]["rows"]
    say(f"offline, a 40-minute recording of {n} rows x 8 columns at {FS_RAW:g} Hz, on the device [ms]:")
    for key, name, rows in (("fir", "FirResampler.apply (msig_rs_resample)", n_fir), ("fft", "resample_device (msig_prep_resample)", n_fft)):
        v = [r[key] for r in offline]
        say(f"    {name:<40} {statistics.median(v):9.3f}  ({min(v):.3f} .. {max(v):.3f})   runs " + " ".join(f"{x:.3f}" for x in v) + f"   {rows} rows out")
    if a.out is not None:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
