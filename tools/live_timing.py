"""What one live tick costs (multimodalsignal_amd/live.py), on one MI355X with device events.

A tick: every one of N sessions delivers exactly one stride of samples (host arrays) and completes one window; LiveMonitor.push
appends the N chunks, fills one mixed batch per piece, runs the ensemble and returns the N updates.  Beside it, what the code offered
before for the same work: one Monitor.run per session over that session's trailing window (a host array of T samples) with a given
statistics tensor, all in one process.  N = 1, 16, 64, 256; three runs of each, the two variants alternating run by run; per run the
median tick.  Then where a tick's GPU time goes: the fill (msig_lv_windows_multi), the forward (msig_st_forward_multi) and the
reduction (msig_en_reduce_multi) of the same batch, each timed on its own.

python tools/live_timing.py [--members 3] [--out profiles/live_timing.log]
"""
import argparse
import ctypes as C
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from multimodalsignal_amd import _lib as L                      # noqa: E402
from multimodalsignal_amd.live import LiveBatch, LiveMonitor    # noqa: E402
from multimodalsignal_amd.models import CnnGruAttentionModel    # noqa: E402
from multimodalsignal_amd.monitor import Monitor                # noqa: E402
from multimodalsignal_amd.synth import CHANNELS6                # noqa: E402

FS, WINDOW_S, STRIDE_S = 64.0, 60.0, 10.0
NAMES = list(CHANNELS6) + ["spare_a", "spare_b"]                # 8 columns, the models read 6


def timed(fn, reps):
    """Device-event milliseconds of each of `reps` calls of fn (each call ends synchronised)."""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=3)
    ap.add_argument("--out", type=Path, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    models = []
    for r in range(a.members):
        torch.manual_seed(5 + r)
        models.append(CnnGruAttentionModel(6, 2).to(dev).eval())
    T, S = int(WINDOW_S * FS), int(STRIDE_S * FS)
    rs = np.random.RandomState(0)
    stats = torch.zeros(2 * L.MAX_C + 1, dtype=torch.float64, device=dev)
    stats[L.MAX_C:2 * L.MAX_C] = 1.0
    stats[2 * L.MAX_C] = 6.0
    say(f"device: {torch.cuda.get_device_name(0)}")
    say(f"{a.members} members (cnn_gru_attention, C = 6 of 8 columns, K = 2), T = {T}, S = {S}, fs = {FS:g}, eval_batch 256, given statistics; "
        "device events around calls that end synchronised; per run the median tick, three runs, the variants alternating")
    say()
    common = dict(window_s=WINDOW_S, stride_s=STRIDE_S, reference=stats, eval_batch=256, channels=list(CHANNELS6))
    mon = Monitor(models, FS, **common)
    for N in (1, 16, 64, 256):
        live = LiveMonitor(models, FS, max_sessions=N, **common)
        trail = [rs.randn(T, 8) for _ in range(N)]                            # each session's trailing window, on the host
        for k in range(N):
            live.open(k, NAMES)
        assert sum(len(u) for u in live.push({k: trail[k] for k in range(N)}).values()) == N          # window 0 of every session

        def tick_live():
            chunks = {k: rs.randn(S, 8) for k in range(N)}
            ms = timed(lambda: live.push(chunks), 1)[0]
            for k in range(N):
                trail[k] = np.concatenate([trail[k][S:], chunks[k]])
            return ms

        def tick_offline():
            return timed(lambda: [mon.run(trail[k], NAMES) for k in range(N)], 1)[0]

        reps = {1: 30, 16: 20, 64: 10, 256: 5}[N]
        for _ in range(3):                                                    # warm-up: every shape the timed ticks use
            tick_live()
        tick_offline()
        runs = {"live": [], "offline": []}
        for _ in range(3):
            runs["live"].append(statistics.median(tick_live() for _ in range(reps)))
            runs["offline"].append(statistics.median(tick_offline() for _ in range(max(2, reps // 2))))
        lv, of = statistics.median(runs["live"]), statistics.median(runs["offline"])
        # the last live windows are the offline ones: the same bits, or the two variants did not do the same work
        got = [live.timeline(k).mean_p[-1] for k in range(N)]
        want = [mon.run(trail[k], NAMES).mean_p[-1] for k in range(N)]
        same = all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
        say(f"N = {N:3d} sessions, one new window each:")
        say(f"  LiveMonitor.push, one tick            median {lv:9.3f} ms   runs " + " ".join(f"{v:.3f}" for v in runs["live"])
            + f"   {lv / N * 1e3:8.1f} us per session")
        say(f"  {N} x Monitor.run on a trailing window median {of:9.3f} ms   runs " + " ".join(f"{v:.3f}" for v in runs["offline"])
            + f"   {of / N * 1e3:8.1f} us per session   live / offline = {lv / of:.3f}   same bits: {same}")
        # where the tick goes: the three launches of the batch, each on its own
        ens, lib = live.ensemble, L.lib()
        batch = LiveBatch(live, [(live.sessions[k].slot, live.sessions[k].book.next_window - 1, live.sessions[k].book.written) for k in range(N)])
        n = ens.slots
        ens._arenas(T, [N])
        ens._load(0, n)
        multi, st = ens.arenas.multi(range(n)), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        p = ens.predict(batch)
        outs = (p.mean_p.data_ptr(), p.std_p.data_ptr(), p.pred.data_ptr(), p.entropy.data_ptr(), p.expected_entropy.data_ptr(),
                p.mutual_info.data_ptr(), p.votes.data_ptr(), p.member_pred.data_ptr(), p.disagreement.data_ptr())
        parts = {"fill (msig_lv_windows_multi)": lambda: batch.fill(ens.arenas.ptr("x"), multi, 0, N),
                 "forward (msig_st_forward_multi)": lambda: L.check(lib.msig_st_forward_multi(C.byref(ens._desc(N)), C.byref(multi), C.byref(ens._st), st), "forward"),
                 "reduction (msig_en_reduce_multi)": lambda: L.check(lib.msig_en_reduce_multi(ens._logits(0, N).data_ptr(), C.byref(multi), N, ens.K, *outs, st), "reduce"),
                 "the three in a row": lambda: ens.predict(batch)}
        for name, fn in parts.items():
            timed(fn, 3)
            say(f"  {name:<34} median {statistics.median(timed(fn, 20)):9.3f} ms")
        say()
    if a.out is not None:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
