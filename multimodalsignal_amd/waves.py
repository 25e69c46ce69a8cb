"""Fold batches on HIP streams: which of a rank's work units train together (`deal`) and how a wave of fold batches runs
(`run_wave`).  Both LOSO drivers of main.py (run_experiments, run_hierarchical_experiment) define their units and what happens to
a finished one; the mechanics are here, once.
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor

import torch

from . import _lib as L
from .multifold import LockstepTrainer

# Concurrent HIP streams per GPU.  Measured (profiles/r05_stream_sweep.log: G single-fold step loops on G streams, GPU_MAX_HW_QUEUES
# 4 / 8 / 16 / 24): 1.04 / 1.12 / 1.19 / 1.26 ms per step with 1 / 2 / 3 / 4 streams, then 1.9-2.3 ms with FIVE whatever the queue
# count — the command processor's four pipes each work on one queue at a time, and a stream whose next launch waits behind a
# 200-us recurrence of another stream on the same pipe waits for all of it.  Nothing in the drivers runs more than four streams of
# training at once: four fold batches per configuration (+ a side stream for finished folds' short test passes), one per configuration
# in a sweep, and at most four single-fold streams with --no-lockstep (round 4 ran fifteen there).
MAX_TRAIN_STREAMS = 4


def cap_waves(waves, cap=MAX_TRAIN_STREAMS):
    """Splits every wave (a list of fold batches that run concurrently, one stream each) into waves of at most `cap` fold batches,
    in order: what does not fit spills into the next wave."""
    return [wv[i:i + cap] for wv in waves for i in range(0, len(wv), cap)]


def chunk_schedule(chunk_preps):
    """(epoch budget, smallest patience) of a fold batch, from its own folds' trainer configurations (main.trainer_config): a sweep's
    configurations need not share one.  The folds of one batch share one budget (LockstepTrainer checks it and runs to it)."""
    tcs = [p["config"]["trainer"] for p in chunk_preps]
    return max(int(t["epochs"]) for t in tcs), min(int(t["early_stopping"]["patience"]) for t in tcs)


def deal(groups, folds, concurrent_folds, lockstep_groups, fold_of=None, sweep=False):
    """Which units share a fold batch and which batches run side by side: a list of waves, each a list of fold batches (lists of
    units), the waves one after another.  Pure data -> data; it changes no fold's bits, only the wall-clock.

    `groups` holds the unit lists that train side by side — one per configuration, or one per model of the hierarchical experiment;
    `folds` are the rank's folds in training order and `fold_of(unit)` a unit's fold (default: the unit itself).  At most
    `concurrent_folds` folds are resident at a time: the folds are cut into windows that wide, and the units of a window's folds
    form its waves.  Within a window each group is dealt round-robin into min(ng, len // 2) batches, every batch cut at MAX_FOLDS,
    with ng = `lockstep_groups` as far as MAX_TRAIN_STREAMS streams go round the groups; `cap_waves` then splits what is still wider
    than MAX_TRAIN_STREAMS.

    Each group's folds are dealt round-robin into several batches (default 4), each advancing in lockstep on its own HIP stream: one
    batch of 15 is bound by the latency of its ~30 dependent launches per step (2.1 ms at 15 folds, 0.96 ms at one) and runs as
    many epochs as its slowest fold; several smaller batches overlap each other's latency (and each other's per-epoch host work and
    sync), let early finishers free their share sooner and — what decides the wall-clock — keep the few folds that train longest in
    SMALL batches: a step costs 0.96 + 0.11 ms per further fold of its batch, and which folds stop late is not known when they are
    dealt.  As many batches as the command processor has pipes (MAX_TRAIN_STREAMS = 4).  Round 5, bench LOSO, the same 558
    fold-epochs: 7.44 s with 1 batch, 7.03 with 2, 7.06-7.12 with 3 (round 2-4's default: its deal puts the folds of 76, 70 and 59
    epochs into one batch), 6.59-6.69 with 4 (profiles/r05_loso_groups.log) — the short test pass of a finished fold on the side
    stream is a fifth stream for a few milliseconds and is inside those numbers.

    `sweep` (several configurations, e.g. the channel ablation's 4 x 15 folds): ONE window of everything — a sweep ignores
    `concurrent_folds` — and one batch per configuration (ng = 1), the configurations' batches concurrently, at most
    MAX_TRAIN_STREAMS at a time; round 4 ran them as sequential waves of three streams, each wave ending in a multi-second tail with
    one or two folds left on an otherwise idle GPU."""
    fold_of = fold_of or (lambda u: u)
    ng = 1 if sweep else max(1, min(int(lockstep_groups), MAX_TRAIN_STREAMS // len(groups)))
    width = max(1, int(concurrent_folds))
    waves = []
    for window in [None] if sweep else [set(folds[w0:w0 + width]) for w0 in range(0, len(folds), width)]:
        wave = []
        for g in groups:
            g = [u for u in g if window is None or fold_of(u) in window]
            k = min(ng, max(1, len(g) // 2))
            wave += [part[i:i + L.MAX_FOLDS] for part in (g[j::k] for j in range(k)) for i in range(0, len(part), L.MAX_FOLDS)]
        waves.append(wave)
    return cap_waves(waves)                              # never more than MAX_TRAIN_STREAMS training streams at once


def on_streams(fn, jobs, device, workers=None):
    """[fn(job) for job in jobs], every job under a HIP stream of its own that is synchronised when the job returns: one job
    inline, several on a thread pool of `workers` threads (default: one per job).  Whatever the jobs read must be complete on the
    device before the call (uploads are issued on the caller's stream)."""
    def work(job):
        torch.cuda.set_device(device)
        with torch.cuda.stream(torch.cuda.Stream(device)):
            out = fn(job)
            torch.cuda.current_stream(device).synchronize()
        return out
    if len(jobs) == 1:
        return [work(jobs[0])]
    with ThreadPoolExecutor(max_workers=workers or len(jobs)) as ex:
        return list(ex.map(work, jobs))


def run_wave(wave, preps, device, adaptive_forms=False, t_start=None):
    """Runs the fold batches of `wave` (lists of units; `preps` maps a unit to its prep dict) concurrently, each as one
    LockstepTrainer on its own stream — constructed there, so that its arenas are filled under that stream — every fold to its early
    stop or its batch's epoch budget.  Returns [(unit, result dict)] in batch order, then position order; every prep then carries
    its Trainer."""
    def batch(units):
        return LockstepTrainer([preps[u] for u in units], device, adaptive_forms=adaptive_forms).run(t_start=t_start)
    return [(u, info) for units, infos in zip(wave, on_streams(batch, wave, device)) for u, info in zip(units, infos)]
