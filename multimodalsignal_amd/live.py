"""Live monitoring: push(samples) for many wearers, bit-equal to the offline timeline (include/msig_lv.h).

A wearable delivers a few seconds of samples at a time, and one GPU serves many wearers.  `LiveMonitor` keeps one ring of the last
`ring_s` seconds per open session in a device pool.  One `push` appends every session's chunk (msig_lv_push), collects every window
that became complete across all sessions, and runs them through the ensemble as mixed batches of at most `eval_batch` rows: one
msig_lv_windows_multi, one msig_st_forward_multi and one msig_en_reduce_multi per piece and member chunk, on `Ensemble`'s own
forward and reduction code (`LiveEnsemble` overrides the filling of the arenas, as monitor.RecordingEnsemble does, and their size).  What a
session reports equals, bit for bit, what `Monitor.run` reports for the same samples as one recording, under every causal reference:
"head:K", and the running references "expanding", "trailing:K" (include/msig_rn.h) and "decayed:H"
(include/msig_rd.h, section 37), whose statistics follow the wearer: a per-session state block on the device, one msig_rn_lv_step or
msig_rd_lv_step per piece that forms each new window's sums from the ring and its statistics record, and msig_rn_lv_windows_multi,
which normalises every row with its own record.  "decayed:H" keeps one carry per session whatever H is.  A row's eval bits do not
depend on its batch, and the smoothing is `monitor.ema`'s recurrence continued.

Missing samples (include/msig_gp.h): with `gaps=Gaps(...)`, under a running reference, a chunk may hold NaN and
`skip({sid: n_samples})` stands for a stretch in which nothing arrived at all — it completes windows exactly as a push of n NaN rows
would (msig_gp_lv_skip writes them into the ring without a staging buffer).  The per-session state, the step and the row fill are
msig_gp_lv_step's and msig_gp_lv_windows_multi's; an update carries the window's coverage and validity, the smoother and the alarm
machine hold through invalid windows (GapSmoother, GapAlarmMachine) and raise `lost` / `back`.  `timeline(sid)` equals `Monitor.run`
with the same `gaps` on the same samples, the skipped stretches as NaN rows, in every field.

The offline state drops episodes shorter than `min_on` after the fact; a live system cannot take back an alarm.  So an `onset` alarm
is raised at the window where a run of the raw hysteresis state reaches `min_on` windows (it carries the run's first window), and an
`offset` alarm at the window where such a run ends: every offline event (a, b) yields one onset at window a + min_on - 1 and one
offset at window b; runs the offline timeline drops yield nothing.  `timeline(sid)` is the offline `Timeline` of everything pushed
so far.

Raw-rate samples (include/msig_rs.h): with `resampler=FirResampler(fs_in, fs)`, push and skip take samples
and counts at the device's own rate fs_in.  One msig_rs_lv_push per round resamples every chunk straight into the rings — there is no
buffer of resampled rows — and keeps each session's tail of raw rows, which the next chunk's first outputs need.  Everything behind
the ring is the code above; `timeline(sid)` equals `Monitor.run` with the same resampler on the same raw samples.

Mixed rates (include/msig_mx.h): with `resampler=MixedResampler([Stream(...), ...], fs)` the columns of a session
arrive as streams, each at its own rate: push({sid: {stream: samples}}), skip({sid: {stream: n_raw}}), room(sid).  A session keeps one
raw count per stream; its ring rows are complete up to the slowest stream's output count, which is the `written` every window call
receives (`MixedBook`).  A round costs one msig_mx_lv_push for the chunks of every (session, stream) that delivered samples and one for
those that delivered none.  A stream may run ahead of the slowest one by what the ring holds beyond the windows still to be handed
out; a push that would need more is refused before anything is launched.  `timeline(sid)` equals `Monitor.run` with the same resampler
on the same streams.

The host parts (`Smoother`, `AlarmMachine`, `RingBook`, `MixedBook`, the CLI's argument checks) need no GPU.  `LiveMonitor` has no CPU fallback.

Out of scope: sharing the front end between overlapping windows (not exact, see monitor.py) and any network or serial front end —
push() is the interface.  Training under the matching causal normalisation is --norm-reference expanding | trailing:K | decayed:H
(dataset.py); --reference auto picks a run's counterpart (monitor.resolve_reference).

CLI:  python -m multimodalsignal_amd.live --run RUN [--subject S5] [--config NAME] (--recording X.npy --names FILE |
      --synthetic-recording) [--sessions N] [--chunk-s 2.5] [--reference head:6|expanding[:W]|trailing:K[:W]|decayed:H[:W]|auto]
      [--gaps [MIN_COVERAGE[:LOST_AFTER]]] [--synthetic-gaps SPEC] [--resample-from 700 [--resampler fft|fir] | --streams SPEC] --out DIR
"""
from __future__ import annotations

import ctypes as C
import json
from dataclasses import asdict, dataclass
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib as L
from .ensemble import Ensemble, load_members
from .monitor import (SYNTHETIC_NOTE, SYNTHETIC_PHASES, Monitor, Timeline, build_parser as _monitor_parser, check_gap_args, check_source_args, ema,
                      ema_gaps, find_events, hysteresis, hysteresis_gaps, lost_windows, parse_recording_reference, phase_shares, raw_phase_table,
                      resolve_reference, run_norm_reference, running_reference)
from .reference import Gaps, gp_mode_fields
from .resample import FirResampler, MixedResampler, out_count as rs_out_count

FIELDS = ("mean_p", "std_p", "pred", "entropy", "mutual_info", "votes")      # what a session stores per window, as Ensemble.predict gives it


# ---- the parts that need no GPU ---------------------------------------------------------------------------------------------------
class Smoother:
    """monitor.ema one score at a time: the same float64 operations in the same order, so after n scores `value` holds
    ema(scores, halflife)[n - 1] bit for bit."""

    def __init__(self, halflife: float):
        ema([], halflife)
        self.a = 1.0 if halflife == 0 else 1.0 - 2.0 ** (-1.0 / float(halflife))
        self.n, self.value = 0, 0.0

    def push(self, score) -> float:
        v = float(score)
        self.value = v if self.n == 0 else self.value + self.a * (v - self.value)
        self.n += 1
        return self.value


@dataclass(frozen=True)
class Alarm:
    """kind "onset": at `window` a run of the raw hysteresis state that began at `start_window` reached min_on windows; "offset":
    `window` is the first window after such a run.  t_s and start_s are the end times of `window` and `start_window` in seconds
    (None where the machine was given no clock)."""
    kind: str
    window: int
    start_window: int
    t_s: Optional[float] = None
    start_s: Optional[float] = None


class AlarmMachine:
    """monitor.hysteresis one smoothed score at a time, with the live min_on rule (module docstring).  step(v) returns (on, alarm):
    `on` — a run of at least min_on windows is in progress at this window; `alarm` — the Alarm raised at this window or None."""

    def __init__(self, on: float, off: float, min_on: int = 1):
        hysteresis([], on, off, min_on)
        self.on, self.off, self.min_on = float(on), float(off), int(min_on)
        self.n, self.raw, self.start = 0, False, 0

    def step(self, v) -> Tuple[bool, Optional[Alarm]]:
        v, n, alarm = float(v), self.n, None
        if not self.raw and v >= self.on:
            self.raw, self.start = True, n
        elif self.raw and v <= self.off:
            self.raw = False
            if n - self.start >= self.min_on:
                alarm = Alarm("offset", n, self.start)
        if self.raw and n - self.start + 1 == self.min_on:
            alarm = Alarm("onset", n, self.start)
        self.n += 1
        return self.raw and n - self.start + 1 >= self.min_on, alarm


class GapSmoother:
    """monitor.ema_gaps one (score, valid) at a time: the same float64 operations in the same order, so after n windows `value`
    holds ema_gaps(scores, valid, halflife, lost_after)[n - 1] bit for bit."""

    def __init__(self, halflife: float, lost_after: int):
        ema([], halflife)
        lost_windows([], lost_after)
        self.a = 1.0 if halflife == 0 else 1.0 - 2.0 ** (-1.0 / float(halflife))
        self.lost_after, self.run, self.fresh, self.value = int(lost_after), 0, True, 0.0

    def push(self, score, valid) -> float:
        if valid:
            v = float(score)
            self.value = v if self.fresh else self.value + self.a * (v - self.value)
            self.fresh, self.run = False, 0
        else:
            self.run += 1
            if self.run >= self.lost_after:
                self.fresh = True
        return self.value


class GapAlarmMachine:
    """monitor.hysteresis_gaps one (smoothed, valid) at a time, with AlarmMachine's live min_on rule.  step(v, valid) returns (on,
    alarms): `alarms` — the Alarms raised at this window, in order.  Beside onset and offset: "lost" at the window where a run of
    invalid windows reaches lost_after (start_window: the run's first window) — preceded by an "offset" where an alarm was active,
    since the state is forced off there — and "back" at the next valid window (start_window: the same run's first window)."""

    def __init__(self, on: float, off: float, min_on: int = 1, lost_after: int = 6):
        hysteresis([], on, off, min_on)
        lost_windows([], lost_after)
        self.on, self.off, self.min_on, self.lost_after = float(on), float(off), int(min_on), int(lost_after)
        self.n, self.raw, self.start = 0, False, 0
        self.run, self.gap_start, self.lost = 0, 0, False

    def step(self, v, valid) -> Tuple[bool, List[Alarm]]:
        v, n, alarms = float(v), self.n, []
        if valid:
            if self.lost:
                alarms.append(Alarm("back", n, self.gap_start))
            self.run, self.lost = 0, False
            if not self.raw and v >= self.on:
                self.raw, self.start = True, n
            elif self.raw and v <= self.off:
                self.raw = False
                if n - self.start >= self.min_on:
                    alarms.append(Alarm("offset", n, self.start))
        else:
            if self.run == 0:
                self.gap_start = n
            self.run += 1
            if self.run >= self.lost_after:
                if self.raw:
                    self.raw = False
                    if n - self.start >= self.min_on:
                        alarms.append(Alarm("offset", n, self.start))
                if not self.lost:
                    alarms.append(Alarm("lost", n, self.gap_start))
                self.lost = True
        if self.raw and n - self.start + 1 == self.min_on:
            alarms.append(Alarm("onset", n, self.start))
        self.n += 1
        return self.raw and n - self.start + 1 >= self.min_on, alarms


def alarms_of_gaps(state, valid, lost_after: int, min_on: int) -> List[Tuple[str, int, int]]:
    """(kind, window, start_window) of the alarms the offline state and validity vectors imply: alarms_of_events' onsets and offsets,
    a "lost" at the first lost window of every invalid run that reaches lost_after and a "back" at the valid window that ends it —
    in window order, at one window back before offset before lost before onset (GapAlarmMachine's order)."""
    ok, lost = np.asarray(valid, dtype=bool), lost_windows(valid, lost_after)
    out = list(alarms_of_events(state, min_on))
    for n in range(len(ok)):
        if lost[n] and not (n > 0 and lost[n - 1]):
            out.append(("lost", n, n - int(lost_after) + 1))
        if n > 0 and lost[n - 1] and ok[n]:
            k = n - 1
            while k > 0 and not ok[k - 1]:
                k -= 1
            out.append(("back", n, k))
    rank = {"back": 0, "offset": 1, "lost": 2, "onset": 3}
    return sorted(out, key=lambda e: (e[1], rank[e[0]]))


def alarms_of_events(state, min_on: int) -> List[Tuple[str, int, int]]:
    """(kind, window, start_window) of the alarms the offline state vector implies: per episode (a, b) an onset at a + min_on - 1
    and, where the episode ends inside the vector, an offset at b — in window order."""
    s = np.concatenate(([False], np.asarray(state, dtype=bool), [False]))
    edges = np.flatnonzero(s[1:] != s[:-1])
    out = []
    for a, b in zip(edges[0::2], edges[1::2]):
        out.append(("onset", int(a) + int(min_on) - 1, int(a)))
        if b < len(s) - 2:
            out.append(("offset", int(b), int(a)))
    return sorted(out, key=lambda e: e[1])


class RingBook:
    """The bookkeeping of one session's ring of R rows, windows of T samples every S, `warm` leading windows that supply the
    statistics (0: the statistics are given).  `written` samples so far, windows below `next_window` are handed out.

    A push of n samples is appended in segments.  A segment never overwrites a sample that a window not yet handed out still needs:
    its length is at most next_window * S + R - written (>= 1 while R >= T), and at most R (S > T: the samples between two windows
    are needed by none).  While the statistics are pending no window is handed
    out, so next_window = 0 and no segment wraps: the head span (warm - 1) * S + T <= R lies unwrapped at the ring's start when the
    segment that completes it has been appended — that is where the statistics are taken, before the next segment is.  After each
    segment `advance` says whether the statistics are due and which windows became complete."""

    def __init__(self, R: int, T: int, S: int, warm: int = 0):
        R, T, S, warm = int(R), int(T), int(S), int(warm)
        if T < 1 or S < 1 or warm < 0:
            raise ValueError(f"a ring needs T >= 1, S >= 1 and warm >= 0, got {T}, {S}, {warm}")
        self.head = (warm - 1) * S + T if warm else 0
        if R < max(T, self.head):
            raise ValueError(f"a ring of {R} rows cannot hold {'the head span of ' + str(self.head) if warm else 'one window of ' + str(T)} samples")
        self.R, self.T, self.S, self.warm = R, T, S, warm
        self.written, self.next_window, self.pending = 0, 0, warm > 0

    def complete(self) -> int:
        """The number of complete windows (msig_rec_count of the samples written)."""
        return 0 if self.written < self.T else (self.written - self.T) // self.S + 1

    def segment(self, n: int) -> int:
        """How many of n waiting samples the next append may take."""
        return min(int(n), self.R, self.next_window * self.S + self.R - self.written)

    def advance(self, a: int) -> Tuple[bool, range]:
        """`a` samples were appended: (the statistics are due now, the windows to hand out now)."""
        if not 0 <= a <= min(self.R, self.next_window * self.S + self.R - self.written):
            raise ValueError(f"a segment of {a} samples would overwrite window {self.next_window}")
        self.written += int(a)
        due = self.pending and self.written >= self.head
        if due:
            self.pending = False
        if self.pending:
            return False, range(0)
        w = range(self.next_window, self.complete())
        self.next_window = w.stop if len(w) else self.next_window
        return due, w

    def plan(self, n: int) -> List[Tuple[int, bool, range]]:
        """The segments of a push of n samples as (length, statistics due after it, windows handed out after it); advances the book."""
        out, n = [], int(n)
        while n > 0:
            a = self.segment(n)
            out.append((a, *self.advance(a)))
            n -= a
        return out


class MixedStuck(ValueError):
    """MixedBook.plan: stream `ahead` cannot take its waiting rows — its outputs would lie `lead_rows` rows ahead of what the slowest
    stream, `slowest`, can reach in this call; a ring of `need_rows` rows would hold them."""

    def __init__(self, ahead: int, slowest: int, lead_rows: int, need_rows: int):
        super().__init__(f"stream {ahead} is {lead_rows} rows ahead of stream {slowest}; a ring of {need_rows} rows would hold it")
        self.ahead, self.slowest, self.lead_rows, self.need_rows = ahead, slowest, lead_rows, need_rows


class MixedBook:
    """The bookkeeping of one session whose columns arrive as streams with the ratios `ratios` = [(L, M, half), ...] ((1, 1, 0): a
    stream at the ring's rate), on integers only.  `raw[g]` raw rows of stream g so far; `book` is the session's RingBook, whose
    `written` is the minimum of the streams' output counts: the rows every stream has delivered.  A stream that is ahead has its rows
    in the ring already; nothing reads them until the slowest stream reaches them.

    A call's waiting rows are taken in rounds.  With bound = book.written + book.segment(1 << 62) — the first row whose ring slot a
    window not yet handed out (or, while the statistics are pending, the unwrapped head) still needs — every stream with waiting rows
    takes as many as keep its output count at or below the bound, at most max_rows_g(bound) - raw[g]; then the book advances to the
    new minimum, which may hand out windows and raise the bound.  `plan` runs this on copies and raises MixedStuck where a round can
    take nothing: rows are still waiting and no stream can move — the slowest stream has nothing waiting.  Nothing has changed then."""

    def __init__(self, book: RingBook, ratios: Sequence[Tuple[int, int, int]]):
        self.book, self.ratios = book, [(int(a), int(b), int(h)) for a, b, h in ratios]
        if not self.ratios:
            raise ValueError("a mixed book has at least one stream")
        self.raw = [0] * len(self.ratios)

    def count(self, g: int, n: int) -> int:
        return rs_out_count(n, *self.ratios[g])

    def max_rows(self, g: int, k: int) -> int:
        """The largest raw count of stream g with count(g, n) <= k."""
        up, down, half = self.ratios[g]
        return (int(k) * down + half) // up

    def counts(self) -> List[int]:
        return [self.count(g, n) for g, n in enumerate(self.raw)]

    def _rounds(self, waiting: Sequence[int]):
        """(rounds, stuck): rounds = [(rows taken per stream, statistics due, windows handed out)], on copies; stuck is None or the
        MixedStuck of the round that could take nothing."""
        G = len(self.ratios)
        if len(waiting) != G or any(int(n) < 0 for n in waiting):
            raise ValueError(f"waiting rows are {G} counts >= 0, got {list(waiting)}")
        b = RingBook(self.book.R, self.book.T, self.book.S, self.book.warm)
        b.written, b.next_window, b.pending = self.book.written, self.book.next_window, self.book.pending
        raw, left, rounds = list(self.raw), [int(n) for n in waiting], []
        while any(left):
            bound = b.written + b.segment(1 << 62)
            take = [max(0, min(left[g], (1 << 31) - 1, self.max_rows(g, bound) - raw[g])) for g in range(G)]
            if not any(take):
                final = [self.count(g, raw[g] + left[g]) for g in range(G)]
                ahead = max((g for g in range(G) if left[g]), key=lambda g: final[g])
                slowest = min(range(G), key=lambda g: final[g])
                return rounds, MixedStuck(ahead, slowest, final[ahead] - final[slowest], final[ahead] - b.next_window * b.S)
            raw = [raw[g] + take[g] for g in range(G)]
            left = [left[g] - take[g] for g in range(G)]
            due, wins = b.advance(min(self.count(g, raw[g]) for g in range(G)) - b.written)
            rounds.append((take, due, wins))
        return rounds, None

    def plan(self, waiting: Sequence[int]) -> List[Tuple[List[int], bool, range]]:
        """The rounds of a call that delivers waiting[g] raw rows of stream g; changes nothing.  MixedStuck where it cannot finish."""
        rounds, stuck = self._rounds(waiting)
        if stuck is not None:
            raise stuck
        return rounds

    def apply(self, take: Sequence[int]) -> Tuple[bool, range]:
        """One planned round has been appended: (the statistics are due now, the windows to hand out now)."""
        self.raw = [n + int(a) for n, a in zip(self.raw, take)]
        return self.book.advance(min(self.counts()) - self.book.written)

    def push(self, waiting: Sequence[int]) -> List[Tuple[List[int], bool, range]]:
        """plan and apply: the call as a whole."""
        rounds = self.plan(waiting)
        for take, _due, _wins in rounds:
            self.apply(take)
        return rounds

    def room(self, g: int) -> int:
        """The raw rows stream g can take now, the others delivering nothing."""
        if len(self.ratios) == 1:
            return (1 << 31) - 1
        waiting = [0] * len(self.ratios)
        waiting[g] = 1 << 40
        return sum(take[g] for take, _due, _wins in self._rounds(waiting)[0])


@dataclass
class LiveUpdate:
    """One new window of one session: its index, t_end = (window S + T) / fs, the timeline's row (score = mean_p[positive], std =
    std_p[positive], entropy, mutual_info, pred, smoothed, warmup), `on` (AlarmMachine: an alarm is active) and the Alarm raised at
    this window, if any.  A monitor with `gaps` also fills `coverage` (per selected channel the share of valid samples) and `valid`,
    and `alarms` with every Alarm of this window in order (a forced offset comes before its `lost`); `alarm` is the last of them."""
    sid: object
    window: int
    t_end: float
    score: float
    std: float
    entropy: float
    mutual_info: float
    pred: int
    smoothed: float
    warmup: bool
    on: bool
    alarm: Optional[Alarm] = None
    valid: bool = True
    coverage: Optional[Tuple[float, ...]] = None
    alarms: Tuple[Alarm, ...] = ()


# ---- the sessions on the GPU -------------------------------------------------------------------------------------------------------
class LiveBatch:
    """Rows of a mixed batch: window win[b] of the session in pool slot sess[b], which holds written[b] samples."""

    def __init__(self, monitor: "LiveMonitor", rows: Sequence[Tuple[int, int, int]]):
        self.monitor, self.device = monitor, monitor.device
        self.sess = np.ascontiguousarray([r[0] for r in rows], dtype=np.int32)
        self.win = np.ascontiguousarray([r[1] for r in rows], dtype=np.int64)
        self.written = np.ascontiguousarray([r[2] for r in rows], dtype=np.int64)
        self.C, self.T = monitor.ensemble.C, monitor.T
        self.shape = (len(rows), self.C, self.T)
        self.table, self.coverage, self.stepped = None, None, set()
        if monitor.running is not None:          # a statistics record per row, written by msig_rn_lv_step piece by piece
            self.table = torch.zeros((len(rows), 2 * L.MAX_C + 1), dtype=torch.float64, device=self.device)
        if monitor.gaps is not None:             # and a coverage record per row (msig_gp_lv_step)
            self.coverage = torch.zeros((len(rows), L.MAX_C), dtype=torch.float64, device=self.device)

    def _step(self, i: int, b: int):
        """msig_rn_lv_step for rows i .. i + b - 1, once: the sessions' states advance in row order (a piece is filled once per
        member chunk, and the pieces of the first chunk come in row order)."""
        if i in self.stepped:
            return
        mon = self.monitor
        p32, p64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        nxt = np.ascontiguousarray([mon.rn_next[int(s)] for s in self.sess[i:i + b]], dtype=np.int64)
        if mon.gaps is not None:
            mode = L.GpMode(*gp_mode_fields(mon.running))
            L.check(L.lib().msig_gp_lv_step(*mon._pool_args(), mon.cols, self.C, mon.mask, mon.T, mon.S, C.byref(mode), mon.rn_state.data_ptr(),
                                            mon.rn_state.shape[1] * 8, self.sess[i:].ctypes.data_as(p32), self.win[i:].ctypes.data_as(p64),
                                            self.written[i:].ctypes.data_as(p64), nxt.ctypes.data_as(p64), int(b), self.table[i].data_ptr(),
                                            self.coverage[i].data_ptr(), mon._stream()), "msig_gp_lv_step")
            self._stepped(i, b)
            return
        decayed = mon.running.kind == "decayed"          # msig_rd_lv_step: the same call with the decay in K's place
        step, name = (L.lib().msig_rd_lv_step, "msig_rd_lv_step") if decayed else (L.lib().msig_rn_lv_step, "msig_rn_lv_step")
        L.check(step(*mon._pool_args(), mon.cols, self.C, mon.mask, mon.T, mon.S, mon.running.decay if decayed else mon.running[0],
                     mon.rn_state.data_ptr(), mon.rn_state.shape[1] * 8, self.sess[i:].ctypes.data_as(p32), self.win[i:].ctypes.data_as(p64),
                     self.written[i:].ctypes.data_as(p64), nxt.ctypes.data_as(p64), int(b), self.table[i].data_ptr(), mon._stream()), name)
        self._stepped(i, b)

    def _stepped(self, i: int, b: int):
        mon = self.monitor
        self.stepped.add(i)
        for r in range(i, i + b):
            mon.rn_next[int(self.sess[r])] += 1
            mon.rn_latest[int(self.sess[r])] = self.table[r]

    def fill(self, x0: int, multi: L.Multi, i: int, b: int):
        """Rows i .. i + b - 1 into the x buffer of every arena slot of `multi`; x0 is arena 0's (msig_lv_windows_multi, or under a
        running reference msig_rn_lv_step and msig_rn_lv_windows_multi)."""
        mon = self.monitor
        p32, p64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        if self.table is not None:
            self._step(i, b)
            rows = L.lib().msig_gp_lv_windows_multi if mon.gaps is not None else L.lib().msig_rn_lv_windows_multi
            L.check(rows(*mon._pool_args(), mon.cols, self.C, mon.mask, mon.T, mon.S, self.sess[i:].ctypes.data_as(p32),
                                                     self.win[i:].ctypes.data_as(p64), self.written[i:].ctypes.data_as(p64), int(b),
                                                     self.table[i].data_ptr(), x0, C.byref(multi), mon._stream()),
                    "msig_gp_lv_windows_multi" if mon.gaps is not None else "msig_rn_lv_windows_multi")
            return
        L.check(L.lib().msig_lv_windows_multi(*mon._pool_args(), mon.cols, self.C, mon.mask, mon.T, mon.S, self.sess[i:].ctypes.data_as(p32),
                                              self.win[i:].ctypes.data_as(p64), self.written[i:].ctypes.data_as(p64), int(b),
                                              mon.stats.data_ptr(), x0, C.byref(multi), mon._stream()), "msig_lv_windows_multi")


class LiveEnsemble(Ensemble):
    """An Ensemble whose input is a LiveBatch: predict(batch) runs Ensemble's own pieces, forwards and reduction; only the filling
    of the arenas differs — one msig_lv_windows_multi per piece.  Its arenas are sized for eval_batch rows once: a tick's pieces
    have any size up to that, and none of them allocates."""

    def _arenas(self, T: int, sizes):
        super()._arenas(T, [self.eval_batch])

    def _check_x(self, x):
        if not isinstance(x, LiveBatch):
            return super()._check_x(x)
        if x.device != self.device or x.C != self.C or x.T < 16 or x.shape[0] < 1:
            raise ValueError(f"expected windows of {self.C} channels and T >= 16 on {self.device}, got {x.C} channels, T = {x.T} on {x.device}")
        return x

    def _fill(self, x, i: int, b: int, n: int):
        if not isinstance(x, LiveBatch):
            return super()._fill(x, i, b, n)
        x.fill(self.arenas.ptr("x"), self.arenas.multi(range(n)), i, b)


class _Session:
    def __init__(self, sid, slot: int, book: RingBook, mon: "LiveMonitor"):
        self.sid, self.slot, self.book = sid, slot, book
        self.raw = 0                             # resampler: the raw rows taken so far (book.written counts the ring's rows, the outputs)
        self.mx = MixedBook(book, [(g.L, g.M, g.half) for g in mon.resampler.streams]) if mon.mixed else None      # a raw count per stream
        self.smoother, self.machine = Smoother(mon.halflife), AlarmMachine(mon.on, mon.off, mon.min_on)
        if mon.gaps is not None:
            self.smoother = GapSmoother(mon.halflife, mon.gaps.lost_after)
            self.machine = GapAlarmMachine(mon.on, mon.off, mon.min_on, mon.gaps.lost_after)
        self.coverage: List[np.ndarray] = []     # gaps: every window's coverage of the selected channels, and its validity
        self.valid: List[bool] = []
        self.given = book.warm == 0 and mon.running is None
        self.flagged = mon.running[1] if mon.running is not None else book.warm      # leading windows flagged warmup
        self.rows: Dict[str, list] = {k: [] for k in FIELDS}
        self.score: List[float] = []
        self.smoothed: List[float] = []
        self.alarms: List[Alarm] = []
        self.counts: List[float] = []            # decayed: every window's c_n, read from its statistics record


class LiveMonitor:
    """An ensemble of 1..256 trained models over up to `max_sessions` live sessions sampled at `fs` Hz: windows of `window_s` seconds
    every `stride_s`, a ring of `ring_s` seconds per session (None: the head span or one window, plus 8 strides), `eval_batch` rows
    per piece.  `reference`: "head:K" — a session's first K windows supply its statistics and are emitted together, flagged warmup,
    when window K - 1 completes — "expanding[:W]", "trailing:K[:W]" or "decayed:H[:W]" (monitor.running_reference) — window n is
    normalised with windows 0..n, with the last K or with all so far at a half-life of H windows, emitted in the push that completes
    it, the first W flagged warmup — or a float64 statistics
    tensor (msig_nr.h's layout): wearers enrolled earlier, no warm-up.  "recording" is refused: it is not causal; "expanding" is
    its causal counterpart.  positive, halflife, on, off, min_on, channels: as for monitor.Monitor.  `gaps` (a Gaps, with a running
    reference only): samples may be NaN and stretches may be skipped (module docstring).  `resampler` (a FirResampler whose fs_out is
    `fs`): push and skip take samples and counts at the resampler's fs_in; the monitor owns a tail of raw rows per session.  Or a
    MixedResampler: the columns are the resampler's `.names`, push and skip take {stream: samples} and {stream: n_raw} per session, and
    the default ring is longer by the resampler's latency_spread_rows (an explicit ring must hold the head span, that spread and the
    outputs of one raw sample).

    open(sid, names, stats=None) / close(sid); push({sid: samples}) or push(sid, samples); skip({sid: n}) or skip(sid, n);
    timeline(sid); alarms(sid); room(sid) (mixed rates)."""

    def __init__(self, models: Sequence, fs: float, window_s: float = 60, stride_s: float = 10, reference="head:6", max_sessions: int = 64,
                 ring_s: Optional[float] = None, eval_batch: int = 256, positive: int = 1, halflife: float = 3, on: float = 0.6,
                 off: float = 0.4, min_on: int = 2, channels: Optional[Sequence[str]] = None, gaps: Optional[Gaps] = None,
                 resampler: Union[FirResampler, MixedResampler, None] = None):
        if not float(fs) > 0:
            raise ValueError(f"fs must be > 0, got {fs!r}")
        self.fs = float(fs)
        self.T, self.S = int(round(float(window_s) * self.fs)), int(round(float(stride_s) * self.fs))
        if self.T < 16 or self.S < 1:
            raise ValueError(f"a window needs >= 16 samples and a stride >= 1, got {self.T} and {self.S}")
        if gaps is not None and not isinstance(gaps, Gaps):
            raise ValueError(f"gaps is a Gaps(min_coverage, lost_after) or None, got {gaps!r}")
        if resampler is not None and (not isinstance(resampler, (FirResampler, MixedResampler)) or resampler.fs_out != self.fs):
            raise ValueError(f"resampler is a FirResampler or a MixedResampler whose fs_out is the monitor's fs = {self.fs:g}, or None; got {resampler!r}")
        self.resampler, self.mixed = resampler, isinstance(resampler, MixedResampler)
        if gaps is not None and (isinstance(reference, torch.Tensor) or running_reference(reference) is None):
            raise ValueError("a live monitor with gaps takes a running reference ('expanding', 'trailing:K', 'decayed:H'): 'head:K' statistics "
                             f"weight samples and have no per-channel count of valid ones, and given statistics have no live coverage; got {reference!r}")
        self.gaps = gaps
        if isinstance(reference, torch.Tensor):
            if reference.dtype != torch.float64 or reference.numel() < 2 * L.MAX_C + 1:
                raise ValueError(f"a statistics tensor holds 2 * {L.MAX_C} + 1 float64 values")
            self.warm = 0
        elif isinstance(reference, str) and reference.startswith("head:"):
            self.warm = parse_recording_reference(reference, 1 << 62)[2]
        elif running_reference(reference) is not None:
            self.warm = 0                        # no delay: a window's statistics are complete with the window
        else:
            raise ValueError("a live reference is 'head:K', 'expanding[:W]', 'trailing:K[:W]', 'decayed:H[:W]' or a statistics tensor (anything else is not "
                             f"causal; 'expanding' is the causal counterpart of 'recording'), got {reference!r}")
        self.running = running_reference(reference)
        if isinstance(max_sessions, bool) or not 1 <= int(max_sessions) <= L.LV_MAX_SESSIONS:
            raise ValueError(f"max_sessions must be an integer in 1..{L.LV_MAX_SESSIONS}, got {max_sessions!r}")
        head = (self.warm - 1) * self.S + self.T if self.warm else self.T
        spread = resampler.latency_spread_rows if self.mixed else 0      # a low-rate stream's outputs trail the others' by that many rows
        self.R = head + 8 * self.S + spread if ring_s is None else int(round(float(ring_s) * self.fs))
        RingBook(self.R, self.T, self.S, self.warm)                  # refuses a ring shorter than the head span
        if self.mixed:
            most = max(-(-g.L // g.M) for g in resampler.streams)
            if self.R < head + spread + most:
                raise ValueError(f"a ring of {self.R} rows has no room for the streams' latency spread of {spread} rows and the {most} outputs one "
                                 f"raw sample yields beside {'the head span of' if self.warm else 'a window of'} {head}: ring_s >= "
                                 f"{(head + spread + most) / self.fs:g}")
        elif resampler is not None and self.R < head + -(-resampler.L // resampler.M):
            raise ValueError(f"a ring of {self.R} rows has no room for the {-(-resampler.L // resampler.M)} outputs one raw sample yields beside "
                             f"{'the head span of' if self.warm else 'a window of'} {head}")
        if self.R >= 1 << 31:
            raise ValueError(f"a ring holds fewer than 2^31 samples, got {self.R}")
        hysteresis([], on, off, min_on)
        ema([], halflife)
        self.models = list(models)
        self.ensemble = LiveEnsemble(self.models, eval_batch=eval_batch)
        self.device = self.ensemble.device
        if resampler is not None and resampler.h.device != self.device:
            raise ValueError(f"the resampler's taps are on {resampler.h.device}, the models on {self.device}")
        if not 0 <= int(positive) < self.ensemble.K:
            raise ValueError(f"positive must be a class in 0..{self.ensemble.K - 1}, got {positive!r}")
        self.reference, self.positive, self.halflife, self.on, self.off, self.min_on = reference, int(positive), float(halflife), float(on), float(off), int(min_on)
        self.reference_requested = None          # "auto" where from_run resolved the reference from the run
        self.channels = None if channels is None else list(channels)
        if self.channels is not None and len(self.channels) != self.ensemble.C:
            raise ValueError(f"the models take {self.ensemble.C} channels, got {len(self.channels)} names")
        self.max_sessions = int(max_sessions)
        self.files: List[Path] = []
        self.names: Optional[List[str]] = None       # the columns of every session's samples: fixed by the first open()
        self.sessions: Dict[object, _Session] = {}
        self.free = list(range(self.max_sessions))
        self.stats = torch.zeros((self.max_sessions, 2 * L.MAX_C + 1), dtype=torch.float64, device=self.device)
        self.scratch = torch.empty(L.lib().msig_rec_scratch_bytes(), dtype=torch.uint8, device=self.device)
        self.pool = None
        if self.running is not None:             # per session: the pivot, the expanding carry and the ring of the last K window sums
            state_bytes = L.lib().msig_rn_state_bytes(self.running[0]) if gaps is None else L.lib().msig_gp_state_bytes(self.running[0])
            self.rn_state = torch.zeros((self.max_sessions, state_bytes // 8), dtype=torch.float64, device=self.device)
            self.rn_next = [0] * self.max_sessions               # the host's mirror of every state's next expected window
            self.rn_latest: Dict[int, torch.Tensor] = {}         # slot -> the session's latest statistics record
        if self.mixed:                           # the resampler defines the sessions' columns
            self._bind(resampler.names)

    @classmethod
    def from_run(cls, run_dir, subject: Optional[str] = None, config_name: Optional[str] = None, fs: float = 64.0, device="cuda", **kw) -> "LiveMonitor":
        """The checkpoints Monitor.from_run loads (Monitor.run_files) and the run's channels (Monitor.run_channels).  reference="auto":
        the causal counterpart of the run's NORM_REFERENCE (monitor.resolve_reference), resolved before anything is loaded."""
        auto = isinstance(kw.get("reference"), str) and kw["reference"] == "auto"
        if auto:
            kw["reference"] = resolve_reference(run_norm_reference(run_dir, config_name), live=True)
        files = Monitor.run_files(run_dir, subject, config_name)
        kw.setdefault("channels", Monitor.run_channels(run_dir, config_name))
        self = cls(load_members(files, device), fs, **kw)
        self.files = files
        self.reference_requested = "auto" if auto else None
        return self

    # ---- sessions ---------------------------------------------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _pool_args(self):
        return self.pool.data_ptr(), self.max_sessions, self.R, self.pool.shape[1] * 8, self.C_all

    def _bind(self, names: Sequence[str]):
        names = list(names)
        channels = self.channels if self.channels is not None else names
        if not 1 <= len(channels) <= L.MAX_C or len(channels) != self.ensemble.C:
            raise ValueError(f"the models take {self.ensemble.C} channels, the sessions supply {len(channels)}")
        missing = [c for c in channels if c not in names]
        if missing:
            raise ValueError(f"the sessions have no channel {missing}; they have {names}")
        self.names, self.C_all = names, len(names)
        self.cols = (C.c_int32 * len(channels))(*[names.index(c) for c in channels])
        self.mask = sum(1 << c for c, name in enumerate(channels) if name == "chest_EDA")
        self.pool = torch.empty((self.max_sessions, self.R * self.C_all), dtype=torch.float64, device=self.device)
        if self.mixed:                           # per session every stream's last tail_rows raw rows, side by side (msig_mx.h)
            self.tails = torch.zeros((self.max_sessions, self.resampler.tail_doubles), dtype=torch.float64, device=self.device)
            self.groups = self.resampler.groups()
        elif self.resampler is not None:         # per session the last tail_rows raw rows: the support of a later chunk's first outputs
            self.tails = torch.zeros((self.max_sessions, self.resampler.tail_rows * self.C_all), dtype=torch.float64, device=self.device)

    def open(self, sid, names: Optional[Sequence[str]] = None, stats: Optional[torch.Tensor] = None):
        """A new session `sid` (any hashable) whose samples have the columns `names` — every session of a monitor has the same
        columns, so after the first open `names` may be None.  `stats`: this wearer's statistics, enrolled earlier: no warm-up."""
        if sid in self.sessions:
            raise ValueError(f"session {sid!r} is open")
        if self.names is None:
            if names is None:
                raise ValueError("the first open() names the columns of the samples")
            self._bind(names)
        elif names is not None and list(names) != self.names:
            raise ValueError(f"every session of a monitor has the columns {self.names}, got {list(names)}")
        given = stats if stats is not None else (self.reference if isinstance(self.reference, torch.Tensor) else None)
        if given is not None and (not isinstance(given, torch.Tensor) or given.dtype != torch.float64 or given.numel() < 2 * L.MAX_C + 1):
            raise ValueError(f"a statistics tensor holds 2 * {L.MAX_C} + 1 float64 values")
        if given is not None and self.running is not None:
            raise ValueError(f"a monitor with the running reference {self.reference!r} takes no given statistics")
        if not self.free:
            raise ValueError(f"all {self.max_sessions} sessions of the pool are open")
        slot = self.free.pop(0)
        if self.running is not None:
            self._reset_state(slot)
        if self.resampler is not None:
            self.tails[slot].zero_()
        if given is not None:
            self.stats[slot].copy_(given.reshape(-1)[:2 * L.MAX_C + 1].to(self.device))
        self.sessions[sid] = _Session(sid, slot, RingBook(self.R, self.T, self.S, 0 if given is not None else self.warm), self)

    def close(self, sid):
        """Ends session `sid`; its slot of the pool is free for the next open()."""
        self.free.append(self._session(sid).slot)
        self.free.sort()
        if self.running is not None:
            self._reset_state(self._session(sid).slot)
        if self.resampler is not None:           # the raw count goes with the session; the slot's tail remembers nothing
            self.tails[self._session(sid).slot].zero_()
        del self.sessions[sid]

    def _reset_state(self, slot: int):
        self.rn_state[slot].zero_()
        self.rn_next[slot] = 0
        self.rn_latest.pop(slot, None)

    def _session(self, sid) -> _Session:
        if sid not in self.sessions:
            raise ValueError(f"no open session {sid!r}")
        return self.sessions[sid]

    # ---- push -------------------------------------------------------------------------------------------------------------------
    def _samples(self, x):
        if isinstance(x, np.ndarray):
            x = np.ascontiguousarray(x, dtype=np.float64)
        elif not isinstance(x, torch.Tensor) or not x.is_cuda or x.device != self.device or x.dtype != torch.float64:
            raise ValueError("samples are a (n, C_all) float64 array: numpy, or a tensor on the monitor's GPU (there is no CPU fallback)")
        if x.ndim != 2 or x.shape[1] != self.C_all:
            raise ValueError(f"samples are (n, {self.C_all}) — the columns {self.names} — got {tuple(x.shape)}")
        return x

    def _stream_dict(self, sid, d, what: str) -> dict:
        rs = self.resampler
        if not isinstance(d, dict) or not set(d) <= set(rs.stream):
            raise ValueError(f"session {sid!r}: {what} takes {{stream: ...}} with streams among {[g.name for g in rs.streams]}, got "
                             f"{sorted(d, key=str) if isinstance(d, dict) else d!r}")
        return d

    def room(self, sid) -> Dict[str, int]:
        """Mixed rates: per stream the raw rows it can take now (the other streams delivering nothing)."""
        if not self.mixed:
            raise ValueError("room(sid) belongs to a monitor with a MixedResampler")
        s = self._session(sid)
        return {g.name: s.mx.room(i) for i, g in enumerate(self.resampler.streams)}

    @torch.no_grad()
    def push(self, samples, chunk=None) -> Union[Dict[object, List[LiveUpdate]], List[LiveUpdate]]:
        """push({sid: samples, ...}) -> {sid: [LiveUpdate, ...]}; push(sid, samples) -> [LiveUpdate, ...].  Everything is checked
        before anything is appended."""
        single = chunk is not None or not isinstance(samples, dict)
        if single:
            if chunk is None:
                raise ValueError("push takes {sid: samples} or (sid, samples)")
            samples = {samples: chunk}
        if self.mixed:
            rs = self.resampler
            todo = [(self._session(sid), {rs.streams.index(rs.stream[k]): rs.samples(rs.stream[k], x, self.device)
                                          for k, x in self._stream_dict(sid, d, "push").items()}) for sid, d in samples.items()]
        else:
            todo = [(self._session(sid), self._samples(x)) for sid, x in samples.items()]
        out = self._feed(todo, {sid: [] for sid in samples})
        return out[next(iter(samples))] if single else out

    @torch.no_grad()
    def skip(self, counts, n=None) -> Union[Dict[object, List[LiveUpdate]], List[LiveUpdate]]:
        """skip({sid: n_samples, ...}) -> {sid: [LiveUpdate, ...]}; skip(sid, n_samples) -> [LiveUpdate, ...].  Nothing arrived from
        these sessions for n samples' time: the stretch is appended as missing rows (msig_gp_lv_skip, no staging buffer) and
        completes windows exactly as a push of n NaN rows would.  Needs a monitor with `gaps`."""
        if self.gaps is None:
            raise ValueError("skip needs a monitor with gaps=Gaps(...): without it a stretch without samples has no representation")
        single = n is not None or not isinstance(counts, dict)
        if single:
            if n is None:
                raise ValueError("skip takes {sid: n_samples} or (sid, n_samples)")
            counts = {counts: n}
        per = [k for sid, d in counts.items() for k in self._stream_dict(sid, d, "skip").values()] if self.mixed else list(counts.values())
        for k in per:
            if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or int(k) < 0:
                raise ValueError(f"skip takes a number of samples >= 0 per session, got {k!r}")
        if self.mixed:
            rs = self.resampler
            todo = [(self._session(sid), {rs.streams.index(rs.stream[k]): int(n) for k, n in d.items()}) for sid, d in counts.items()]
        else:
            todo = [(self._session(sid), int(k)) for sid, k in counts.items()]
        out = self._feed(todo, {sid: [] for sid in counts})
        return out[next(iter(counts))] if single else out

    def _feed(self, todo, out: Dict[object, List[LiveUpdate]]):
        """Appends every session's samples — an array, or a count of missing rows — segment by segment (RingBook) and evaluates the
        windows that became complete after each round.  With a resampler the samples and counts are raw: a segment is cut in raw
        rows so that it yields no more outputs than RingBook.segment allows (_raw_segment), and is resampled into the ring."""
        at = [0] * len(todo)
        size = lambda x: x if isinstance(x, int) else x.shape[0]      # noqa: E731
        lib, rs = L.lib(), self.resampler
        if self.mixed:
            return self._feed_mixed(todo, out)
        if rs is not None:
            return self._feed_raw(todo, out)
        while True:
            seg = [(j, s, s.book.segment(size(x) - at[j])) for j, (s, x) in enumerate(todo) if size(x) > at[j]]
            if not seg:
                break
            args = lambda part: ((C.c_int32 * len(part))(*[s.slot for _j, s, _a in part]),      # noqa: E731
                                 (C.c_int64 * len(part))(*[s.book.written for _j, s, _a in part]),
                                 (C.c_int64 * len(part))(*[a for _j, _s, a in part]), len(part))
            data = [e for e in seg if not isinstance(todo[e[0]][1], int)]
            gone = [e for e in seg if isinstance(todo[e[0]][1], int)]
            if data:
                parts = [todo[j][1][at[j]:at[j] + a] for j, _s, a in data]
                if all(isinstance(p, np.ndarray) for p in parts):                  # one upload of the round's chunks, back to back
                    staging = torch.from_numpy(np.concatenate(parts) if len(parts) > 1 else parts[0]).to(self.device)
                else:
                    staging = torch.cat([torch.from_numpy(p).to(self.device) if isinstance(p, np.ndarray) else p for p in parts]).contiguous()
                L.check(lib.msig_lv_push(*self._pool_args(), *args(data), staging.data_ptr(), self._stream()), "msig_lv_push")
            if gone:
                L.check(lib.msig_gp_lv_skip(*self._pool_args(), *args(gone), self._stream()), "msig_gp_lv_skip")
            rows, owners = [], []
            for j, s, a in seg:
                at[j] += a
                due, windows = s.book.advance(a)
                if due:          # the head span lies unwrapped at the ring's start: the offline call's statistics (RingBook)
                    L.check(lib.msig_rec_stats(self.pool[s.slot].data_ptr(), s.book.head, self.C_all, self.cols, self.ensemble.C, self.mask,
                                               self.T, self.S, 0, s.book.warm, self.stats[s.slot].data_ptr(), self.scratch.data_ptr(),
                                               self._stream()), "msig_rec_stats")
                rows += [(s.slot, w, s.book.written) for w in windows]
                owners += [s] * len(windows)
            if rows:
                self._evaluate(rows, owners, out)
        return out

    def _raw_segment(self, s: _Session, left: int) -> int:
        """How many of `left` waiting raw rows the next append may take: as many as yield RingBook.segment's outputs at most."""
        rs = self.resampler
        a = min(int(left), (1 << 31) - 1, rs.max_rows(s.book.written + s.book.segment(1 << 62)) - s.raw)
        if a < 1:
            raise RuntimeError(f"session {s.sid!r}: the ring has no room for the outputs of one raw sample")      # refused by __init__
        return a

    def _feed_raw(self, todo, out: Dict[object, List[LiveUpdate]]):
        """_feed with a resampler: the same rounds, a round's chunks in raw rows, one msig_rs_lv_push for the sessions that delivered
        samples and one, without a staging buffer, for those that delivered none (skip)."""
        at = [0] * len(todo)
        size = lambda x: x if isinstance(x, int) else x.shape[0]      # noqa: E731
        lib, rs = L.lib(), self.resampler
        while True:
            seg = [(j, s, self._raw_segment(s, size(x) - at[j])) for j, (s, x) in enumerate(todo) if size(x) > at[j]]
            if not seg:
                break
            args = lambda part: ((C.c_int32 * len(part))(*[s.slot for _j, s, _a in part]),      # noqa: E731
                                 (C.c_int64 * len(part))(*[s.raw for _j, s, _a in part]),
                                 (C.c_int64 * len(part))(*[a for _j, _s, a in part]), len(part))
            tails = (self.tails.data_ptr(), rs.tail_rows, self.tails.shape[1] * 8)
            data = [e for e in seg if not isinstance(todo[e[0]][1], int)]
            gone = [e for e in seg if isinstance(todo[e[0]][1], int)]
            if data:
                parts = [todo[j][1][at[j]:at[j] + a] for j, _s, a in data]
                if all(isinstance(p, np.ndarray) for p in parts):                  # one upload of the round's chunks, back to back
                    staging = torch.from_numpy(np.concatenate(parts) if len(parts) > 1 else parts[0]).to(self.device)
                else:
                    staging = torch.cat([torch.from_numpy(p).to(self.device) if isinstance(p, np.ndarray) else p for p in parts]).contiguous()
                L.check(lib.msig_rs_lv_push(*self._pool_args(), *tails, *rs.ratio_args(), *args(data), staging.data_ptr(), self._stream()),
                        "msig_rs_lv_push")
            if gone:
                L.check(lib.msig_rs_lv_push(*self._pool_args(), *tails, *rs.ratio_args(), *args(gone), None, self._stream()), "msig_rs_lv_push")
            rows, owners = [], []
            for j, s, a in seg:
                at[j] += a
                s.raw += a
                due, windows = s.book.advance(rs.out_count(s.raw) - s.book.written)
                if due:          # the head span lies unwrapped at the ring's start: the offline call's statistics (RingBook)
                    L.check(lib.msig_rec_stats(self.pool[s.slot].data_ptr(), s.book.head, self.C_all, self.cols, self.ensemble.C, self.mask,
                                               self.T, self.S, 0, s.book.warm, self.stats[s.slot].data_ptr(), self.scratch.data_ptr(),
                                               self._stream()), "msig_rec_stats")
                rows += [(s.slot, w, s.book.written) for w in windows]
                owners += [s] * len(windows)
            if rows:
                self._evaluate(rows, owners, out)
        return out

    def _feed_mixed(self, todo, out: Dict[object, List[LiveUpdate]]):
        """_feed_raw with a chunk per (session, stream): every session's rounds are planned on integers first (MixedBook.plan), so a
        call that cannot finish is refused before anything is launched or changed; then round r of every session goes into one
        msig_mx_lv_push for the chunks with samples and one, without a staging buffer, for the missing ones."""
        size = lambda x: x if isinstance(x, int) else x.shape[0]      # noqa: E731
        lib, rs = L.lib(), self.resampler
        G = len(rs.streams)
        plans = []
        for s, d in todo:
            try:
                plans.append(s.mx.plan([size(d[g]) if g in d else 0 for g in range(G)]))
            except MixedStuck as e:
                raise ValueError(f"session {s.sid!r}: stream {rs.streams[e.ahead].name!r} would be {e.lead_rows / self.fs:.3f} s ahead of stream "
                                 f"{rs.streams[e.slowest].name!r}, more than the ring of {self.R / self.fs:g} s holds beside the windows still to be "
                                 f"handed out; push the lagging streams first, or build the monitor with ring_s >= {e.need_rows / self.fs:g}") from None
        at = [[0] * G for _ in todo]
        tails = (self.tails.data_ptr(), self.tails.shape[1] * 8, rs.h.data_ptr(), self.groups, G)
        for r in range(max((len(p) for p in plans), default=0)):
            seg = [(j, g, a) for j, p in enumerate(plans) if r < len(p) for g, a in enumerate(p[r][0]) if a > 0]
            args = lambda part: ((C.c_int32 * len(part))(*[todo[j][0].slot for j, _g, _a in part]),      # noqa: E731
                                 (C.c_int32 * len(part))(*[g for _j, g, _a in part]),
                                 (C.c_int64 * len(part))(*[todo[j][0].mx.raw[g] for j, g, _a in part]),
                                 (C.c_int64 * len(part))(*[a for _j, _g, a in part]), len(part))
            data = [e for e in seg if not isinstance(todo[e[0]][1][e[1]], int)]
            gone = [e for e in seg if isinstance(todo[e[0]][1][e[1]], int)]
            if data:
                parts = [todo[j][1][g][at[j][g]:at[j][g] + a].reshape(-1) for j, g, a in data]      # the chunks' rows differ in width: back to back
                if all(isinstance(p, np.ndarray) for p in parts):                  # one upload of the round's chunks
                    staging = torch.from_numpy(np.concatenate(parts) if len(parts) > 1 else np.ascontiguousarray(parts[0])).to(self.device)
                else:
                    staging = torch.cat([torch.from_numpy(p).to(self.device) if isinstance(p, np.ndarray) else p for p in parts]).contiguous()
                L.check(lib.msig_mx_lv_push(*self._pool_args(), *tails, *args(data), staging.data_ptr(), self._stream()), "msig_mx_lv_push")
            if gone:
                L.check(lib.msig_mx_lv_push(*self._pool_args(), *tails, *args(gone), None, self._stream()), "msig_mx_lv_push")
            rows, owners = [], []
            for j, p in enumerate(plans):
                if r >= len(p):
                    continue
                s, take = todo[j][0], p[r][0]
                for g in range(G):
                    at[j][g] += take[g]
                due, windows = s.mx.apply(take)
                if due:          # the head span lies unwrapped at the ring's start, complete in every stream's columns
                    L.check(lib.msig_rec_stats(self.pool[s.slot].data_ptr(), s.book.head, self.C_all, self.cols, self.ensemble.C, self.mask,
                                               self.T, self.S, 0, s.book.warm, self.stats[s.slot].data_ptr(), self.scratch.data_ptr(),
                                               self._stream()), "msig_rec_stats")
                rows += [(s.slot, w, s.book.written) for w in windows]
                owners += [s] * len(windows)
            if rows:
                self._evaluate(rows, owners, out)
        return out

    def _evaluate(self, rows, owners: List[_Session], out):
        batch = LiveBatch(self, rows)
        p = self.ensemble.predict(batch)
        host = {k: getattr(p, k).cpu().numpy() for k in FIELDS}
        counts = batch.table[:, 2 * L.MAX_C].cpu().numpy() if self.running is not None and self.running.kind == "decayed" else None
        if self.gaps is not None:
            coverage = np.ascontiguousarray(batch.coverage.cpu().numpy()[:, :self.ensemble.C])
            valid = self.gaps.valid(coverage)
        for b, s in enumerate(owners):
            n = rows[b][1]
            if counts is not None:
                s.counts.append(float(counts[b]))
            for k in FIELDS:
                s.rows[k].append(host[k][b].copy())
            score = float(host["mean_p"][b, self.positive].astype(np.float64))
            t_end = lambda w: (float(w) * self.S + self.T) / self.fs      # noqa: E731
            clocked = lambda al: Alarm(al.kind, al.window, al.start_window, t_end(al.window), t_end(al.start_window))      # noqa: E731
            extra = {}
            if self.gaps is None:
                smoothed = s.smoother.push(score)
                on, alarm = s.machine.step(smoothed)
                if alarm is not None:
                    alarm = clocked(alarm)
                    s.alarms.append(alarm)
            else:
                ok = bool(valid[b])
                smoothed = s.smoother.push(score, ok)
                on, raised = s.machine.step(smoothed, ok)
                raised = tuple(clocked(al) for al in raised)
                s.alarms.extend(raised)
                s.coverage.append(coverage[b].copy())
                s.valid.append(ok)
                alarm = raised[-1] if raised else None
                extra = dict(valid=ok, coverage=tuple(float(v) for v in coverage[b]), alarms=raised)
            s.score.append(score)
            s.smoothed.append(smoothed)
            out[s.sid].append(LiveUpdate(sid=s.sid, window=int(n), t_end=t_end(n), score=score, std=float(host["std_p"][b, self.positive]),
                                         entropy=float(host["entropy"][b]), mutual_info=float(host["mutual_info"][b]), pred=int(host["pred"][b]),
                                         smoothed=smoothed, warmup=n < s.flagged, on=on, alarm=alarm, **extra))

    # ---- what a session has reported so far -------------------------------------------------------------------------------------
    def alarms(self, sid) -> List[Alarm]:
        return list(self._session(sid).alarms)

    def session_stats(self, sid) -> torch.Tensor:
        """The statistics of session `sid` on the device (undefined while its warm-up is pending); under a running reference the
        latest window's record (None before the first window)."""
        if self.running is not None:
            return self.rn_latest.get(self._session(sid).slot)
        return self.stats[self._session(sid).slot]

    def timeline(self, sid) -> Timeline:
        """The Timeline of everything pushed to `sid` so far, Monitor.run's fields: state and events by the offline rule."""
        s = self._session(sid)
        n, K, M = len(s.score), self.ensemble.K, self.ensemble.M
        empty = dict(mean_p=((0, K), np.float32), std_p=((0, K), np.float32), pred=((0,), np.int32), entropy=((0,), np.float32),
                     mutual_info=((0,), np.float32), votes=((0, K), np.int32))
        f = {k: np.stack(s.rows[k]) if n else np.zeros(*empty[k]) for k in FIELDS}
        score, smoothed = np.array(s.score, dtype=np.float64), np.array(s.smoothed, dtype=np.float64)
        t_end = (np.arange(n, dtype=np.float64) * self.S + self.T) / self.fs
        extra = {}
        if self.gaps is None:
            state = hysteresis(smoothed, self.on, self.off, self.min_on)
        else:
            valid = np.array(s.valid, dtype=bool)
            state = hysteresis_gaps(smoothed, valid, self.on, self.off, self.min_on, self.gaps.lost_after)
            extra = dict(coverage=np.stack(s.coverage) if n else np.zeros((0, self.ensemble.C)), valid=valid,
                         lost=lost_windows(valid, self.gaps.lost_after))
        meta = dict(fs=self.fs, window_samples=self.T, stride_samples=self.S, members=M, positive=self.positive, halflife=self.halflife,
                    on=self.on, off=self.off, min_on=self.min_on, samples=s.book.written,
                    reference="statistics" if s.given else self.reference, warmup_windows=int(s.flagged),
                    files=[str(p) for p in self.files])
        if self.running is not None:
            meta["reference_window_counts"] = list(s.counts) if self.running.kind == "decayed" else self.running.counts(n)
        if self.reference_requested is not None:
            meta["reference_requested"] = self.reference_requested
        if self.gaps is not None:
            meta.update(gaps=self.gaps.spelling, invalid_windows=int((~extra["valid"]).sum()), lost_windows=int(extra["lost"].sum()))
        if self.resampler is not None:
            raw = {g.name: s.mx.raw[i] for i, g in enumerate(self.resampler.streams)} if self.mixed else s.raw
            meta.update(resampler=self.resampler.spelling, resampler_latency_s=self.resampler.latency_s, raw_samples=raw)
        return Timeline(t_end=t_end, score=score, smoothed=smoothed, state=state, warmup=np.arange(n) < s.flagged,
                        events=find_events(state, smoothed, t_end), meta=meta, **f, **extra)


def timelines_equal(a: Timeline, b: Timeline) -> bool:
    """Every per-window field of two timelines bit for bit, and their events."""
    for k in ("t_end", "mean_p", "std_p", "pred", "entropy", "mutual_info", "votes", "score", "smoothed", "state", "warmup"):
        x, y = getattr(a, k), getattr(b, k)
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            return False
    for k in ("coverage", "valid", "lost"):          # filled by a monitor with gaps: in both or in neither
        x, y = getattr(a, k), getattr(b, k)
        if (x is None) != (y is None) or (x is not None and (x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes())):
            return False
    return a.events == b.events


# ---- the command line ----------------------------------------------------------------------------------------------------------------
def build_parser():
    ap = _monitor_parser()
    ap.prog = "python -m multimodalsignal_amd.live"
    ap.description = ("Replays a recording into N live sessions in chunks, out of phase: timeline.csv / timeline.json of session 0 (the files "
                      "monitor writes for the recording), alarms.json, and whether session 0's timeline equals Monitor.run's bit for bit.")
    ap.add_argument("--sessions", type=int, default=1, help="live sessions fed with the recording; session k starts k chunks late")
    ap.add_argument("--chunk-s", type=float, default=2.5, help="seconds of samples per push and session")
    ap.set_defaults(reference="head:6")
    return ap


def parse_args(argv=None):
    """The arguments, checked before anything touches the GPU."""
    ap = build_parser()
    a = ap.parse_args(argv)
    check_source_args(ap, a)
    if not a.window_s > 0 or not a.stride_s > 0 or not a.chunk_s > 0:
        ap.error("--window-s, --stride-s and --chunk-s must be > 0")
    if not 1 <= a.sessions <= L.LV_MAX_SESSIONS:
        ap.error(f"--sessions must be in 1..{L.LV_MAX_SESSIONS}")
    check_gap_args(ap, a)
    try:
        if a.reference == "auto":
            return a
        if not (isinstance(a.reference, str) and a.reference.startswith("head:")) and running_reference(a.reference) is None:
            ap.error("a live --reference is head:K, expanding[:W], trailing:K[:W], decayed:H[:W] or auto ('recording' is not causal; "
                     "'expanding' is its causal counterpart)")
        parse_recording_reference(a.reference, 1 << 62)
    except ValueError as e:
        ap.error(str(e))
    return a


def replay_pieces(lo: int, hi: int, spans) -> List[Tuple[int, int, bool]]:
    """The samples [lo, hi) cut at the all-channel gap spans: (first, one past last, skipped) pieces in order."""
    out, at = [], lo
    for a, b in spans:
        a, b = max(a, lo), min(b, hi)
        if a >= b:
            continue
        if a > at:
            out.append((at, a, False))
        out.append((a, b, True))
        at = b
    if hi > at:
        out.append((at, hi, False))
    return out


def main_streams(a) -> Timeline:
    """main with --streams: every session is fed stream by stream at the streams' own rates, chunk_s seconds of each per tick; the
    spans in which a stream is off (--synthetic-gaps all= and stream=) are not pushed but skipped on that stream."""
    from .monitor import load_streams
    mx = MixedResampler(a.streams, a.fs)
    live = LiveMonitor.from_run(a.run, a.subject, a.config, fs=a.fs, window_s=a.window_s, stride_s=a.stride_s, reference=a.reference,
                                max_sessions=a.sessions, gaps=a.gaps, resampler=mx)
    sig, table = load_streams(a, mx)
    sig = {k: torch.from_numpy(v.reshape(v.shape[0], -1)).to(live.device) for k, v in sig.items()}
    chunk = {g.name: max(1, int(round(a.chunk_s * g.fs))) for g in mx.streams}
    ticks = max(-(-int(sig[g.name].shape[0]) // chunk[g.name]) for g in mx.streams)
    spans = {g.name: [] for g in mx.streams}
    if a.gaps is not None and a.synthetic_gaps is not None:
        from .synth import gap_spans
        spans = {g.name: gap_spans(a.synthetic_gaps, g.fs, int(sig[g.name].shape[0]), stream=g.name) for g in mx.streams}
    for k in range(a.sessions):
        live.open(k)
    skipped = {g.name: 0 for g in mx.streams}
    for t in range(ticks + a.sessions - 1):          # session k is k chunks behind session 0
        pieces = {}
        for k in range(a.sessions):
            if 0 <= t - k < ticks:
                for g in mx.streams:
                    lo, hi = (t - k) * chunk[g.name], min((t - k + 1) * chunk[g.name], int(sig[g.name].shape[0]))
                    if hi > lo:
                        pieces[k, g.name] = replay_pieces(lo, hi, spans[g.name])
        for r in range(max((len(v) for v in pieces.values()), default=0)):      # a stream's pieces in their order, streams and sessions side by side
            data: Dict[int, dict] = {}
            gone: Dict[int, dict] = {}
            for (k, name), v in pieces.items():
                if r < len(v):
                    lo, hi, off = v[r]
                    if off:
                        gone.setdefault(k, {})[name] = hi - lo
                        skipped[name] += (hi - lo) if k == 0 else 0
                    else:
                        data.setdefault(k, {})[name] = sig[name][lo:hi]
            if data:
                live.push(data)
            if gone:
                live.skip(gone)
    tl = live.timeline(0)
    offline = Monitor(live.models, a.fs, window_s=a.window_s, stride_s=a.stride_s, reference=live.reference, channels=live.channels, gaps=a.gaps,
                      resampler=mx)
    equal = timelines_equal(tl, offline.run(sig))
    if table is not None:
        tl.meta.update(note=SYNTHETIC_NOTE, phases=table, flagged_by_label=phase_shares(tl, table, live.T, live.S))
    a.out.mkdir(parents=True, exist_ok=True)
    tl.to_csv(a.out / "timeline.csv")
    path = tl.to_json(a.out / "timeline.json")
    (a.out / "alarms.json").write_text(json.dumps({str(k): [asdict(al) for al in live.alarms(k)] for k in range(a.sessions)}, indent=1))
    print(f"{a.sessions} sessions, {ticks} ticks of {a.chunk_s:g} s — {chunk} raw rows per stream; session 0: {len(tl.t_end)} windows, "
          f"{int(tl.state.sum())} flagged, {len(tl.events)} events, {len(live.alarms(0))} alarms; timeline written to: {path}")
    print(f"session 0's timeline and Monitor.run's for the same recording: {'equal' if equal else 'NOT EQUAL'} bit for bit")
    print(f"resampler {mx.spelling}: {tl.meta['raw_samples']} raw samples -> {tl.meta['samples']}, latency {mx.latency_s:.3f} s, a ring of "
          f"{live.R} rows; Monitor.run used the same resampler")
    if a.gaps is not None:
        print(f"gaps {a.gaps.spelling}: {tl.meta['invalid_windows']} invalid windows, {tl.meta['lost_windows']} lost; {skipped} of session 0's "
              f"raw samples were skipped, not pushed; {int((~np.isfinite(tl.score)).sum())} of {len(tl.score)} scores are not finite")
    if table is not None:
        print("NOTE: " + SYNTHETIC_NOTE + ".")
    return tl


def main(argv=None) -> Timeline:
    a = parse_args(argv)
    if a.streams is not None:
        return main_streams(a)
    fir = FirResampler(a.resample_from, a.fs) if a.resampler == "fir" else None
    fs_in = a.fs if fir is None else a.resample_from                 # the rate of what is pushed: under fir the recording's own
    live = LiveMonitor.from_run(a.run, a.subject, a.config, fs=a.fs, window_s=a.window_s, stride_s=a.stride_s, reference=a.reference,
                                max_sessions=a.sessions, gaps=a.gaps, resampler=fir)
    table, spans = None, []
    if a.synthetic_recording:
        from .synth import CHANNELS6, gap_spans, make_synthetic_recording
        names = list(CHANNELS6)
        sig, table = make_synthetic_recording(SYNTHETIC_PHASES, fs=fs_in, channels=names, seed=a.seed, difficulty=a.difficulty,
                                              gaps=a.synthetic_gaps)
        if a.gaps is not None and a.synthetic_gaps is not None:      # the stretches in which every channel is off are not pushed but skipped
            spans = gap_spans(a.synthetic_gaps, fs_in, int(sig.shape[0]))
        if fir is not None:
            table = raw_phase_table(table, a.fs)
    else:
        sig = np.load(a.recording)
        names = [ln.strip() for ln in a.names.read_text().splitlines() if ln.strip()]
    sig = torch.from_numpy(np.ascontiguousarray(sig, dtype=np.float64)).to(live.device)
    if a.resample_from is not None and fir is None:
        from .preprocess import resample_device
        sig = resample_device(sig, int(sig.shape[0] * (a.fs / a.resample_from)))
    chunk = max(1, int(round(a.chunk_s * fs_in)))
    ticks = -(-int(sig.shape[0]) // chunk)
    for k in range(a.sessions):
        live.open(k, names)
    skipped = 0
    for t in range(ticks + a.sessions - 1):          # session k is k chunks behind session 0
        if not spans:
            live.push({k: sig[(t - k) * chunk:(t - k + 1) * chunk] for k in range(a.sessions) if 0 <= t - k < ticks})
            continue
        pieces = {k: replay_pieces((t - k) * chunk, min((t - k + 1) * chunk, int(sig.shape[0])), spans) for k in range(a.sessions) if 0 <= t - k < ticks}
        for r in range(max(len(v) for v in pieces.values())):      # a session's pieces in their order, the sessions side by side
            data = {k: sig[v[r][0]:v[r][1]] for k, v in pieces.items() if r < len(v) and not v[r][2]}
            gone = {k: v[r][1] - v[r][0] for k, v in pieces.items() if r < len(v) and v[r][2]}
            if data:
                live.push(data)
            if gone:
                live.skip(gone)
                skipped += gone.get(0, 0)
    tl = live.timeline(0)
    offline = Monitor(live.models, a.fs, window_s=a.window_s, stride_s=a.stride_s, reference=live.reference, channels=live.channels, gaps=a.gaps,
                      resampler=fir)
    equal = timelines_equal(tl, offline.run(sig, names))
    if table is not None:
        tl.meta.update(note=SYNTHETIC_NOTE, phases=table, flagged_by_label=phase_shares(tl, table, live.T, live.S))
    a.out.mkdir(parents=True, exist_ok=True)
    tl.to_csv(a.out / "timeline.csv")
    path = tl.to_json(a.out / "timeline.json")
    (a.out / "alarms.json").write_text(json.dumps({str(k): [asdict(al) for al in live.alarms(k)] for k in range(a.sessions)}, indent=1))
    print(f"{a.sessions} sessions, {ticks} pushes of {chunk} samples each; session 0: {len(tl.t_end)} windows, {int(tl.state.sum())} flagged, "
          f"{len(tl.events)} events, {len(live.alarms(0))} alarms; timeline written to: {path}")
    print(f"session 0's timeline and Monitor.run's for the same recording: {'equal' if equal else 'NOT EQUAL'} bit for bit")
    if fir is not None:
        print(f"resampler {fir.spelling}: pushed at {fs_in:g} Hz, {tl.meta['raw_samples']} raw samples -> {tl.meta['samples']}, "
              f"latency {fir.latency_s:.3f} s; Monitor.run used the same resampler")
    if a.gaps is not None:
        print(f"gaps {a.gaps.spelling}: {tl.meta['invalid_windows']} invalid windows, {tl.meta['lost_windows']} lost; {skipped} of session 0's "
              f"samples were skipped, not pushed; {int((~np.isfinite(tl.score)).sum())} of {len(tl.score)} scores are not finite")
    if table is not None:
        print("NOTE: " + SYNTHETIC_NOTE + ".")
    return tl


if __name__ == "__main__":
    main()
