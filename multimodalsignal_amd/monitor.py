"""A finished run applied to a continuous recording: the stress timeline (include/msig_rec.h).

A wearable's output is one multichannel signal, not windows.  `RecordingWindows` holds the (L, C_all) float64 recording on the GPU
and hands out its 60 s / 10 s-stride windows normalised and transposed — msig_rec_stats and msig_rec_windows[_multi] read the
recording itself, the windows are never materialised.  `Monitor` runs an ensemble's eval forwards over them on `Ensemble`'s arenas
(msig_st_forward[_multi], msig_en_reduce[_multi]; each piece of windows is filled into every member's arena by one
msig_rec_windows_multi) and turns the positive class's probability into a smoothed score, a hysteresis state and a list of events.

The host helpers (`parse_recording_reference`, `ema`, `hysteresis`, `find_events`, `Timeline`, the CLI's argument checks) need no
GPU (`count_windows` asks the library, which loads without one).  `RecordingWindows` and `Monitor.run` have no CPU fallback.

Out of scope: sharing the front end between overlapping windows (not exact: the channel gate is a mean over ONE window and the
convolutions pad at ITS edges) and the hand-crafted feature branch.  The live push(samples) interface is live.py.

Causal running references (include/msig_rn.h): "expanding" normalises window n with windows 0..n, "trailing:K"
with the last K, "decayed:H" (include/msig_rd.h, section 37) with every window so far, window n - k weighted 2^(-k / H) — a
statistics record per window (one msig_rn_sums, one msig_rn_stats or msig_rd_stats) and batches whose every row has its own record
(msig_rn_windows[_multi]).  "auto" takes the counterpart of the reference the run was trained under (resolve_reference).

Missing samples (include/msig_gp.h): `gaps=Gaps(...)` / --gaps [MIN_COVERAGE[:LOST_AFTER]].  A sample that is
NaN or +-Inf (after log1p) is missing: it enters no statistic and is the reference mean, +0.0, in its window's rows; every window has
a coverage per channel, a window below MIN_COVERAGE is invalid — scored, but the smoother and the hysteresis hold (ema_gaps,
hysteresis_gaps) — and after LOST_AFTER invalid windows in a row the state is off until the next valid one.  Under a running
reference or a statistics tensor; without `gaps` nothing here differs from what it was.

Raw-rate recordings (include/msig_rs.h): `resampler=FirResampler(fs_in, fs)` / --resample-from 700 --resampler fir.
`run` takes the recording at the device's own rate and monitors the causal polyphase FIR resampler's outputs (`apply`), which is what
live.LiveMonitor with the same resampler computes chunk by chunk.  The default, --resampler fft, is the whole-recording FFT method.
Mixed rates (include/msig_mx.h): `resampler=MixedResampler([Stream(...), ...], fs)` / --streams SPEC.  `run` takes
{stream: array}, each at its stream's rate (--recording X.npz keyed by stream name), and monitors the rows every stream has delivered.

CLI:  python -m multimodalsignal_amd.monitor --run RUN [--subject S5] [--config NAME] (--recording X.npy --names FILE |
      --synthetic-recording) [--fs 64] [--resample-from 700 [--resampler fft|fir] | --streams SPEC] [--reference recording|head:K|expanding[:W]|trailing:K[:W]|decayed:H[:W]|auto] [--stride-s 10] [--gaps [MIN_COVERAGE[:LOST_AFTER]]] [--synthetic-gaps SPEC] --out DIR
"""
from __future__ import annotations

import argparse
import ast
import ctypes as C
import json
import re
from dataclasses import dataclass, field
from pathlib import Path
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib as L
from .ensemble import Ensemble, load_members, member_files
from .reference import (GAPS_REFERENCES, RUNNING_WARMUP, Gaps, Running, gp_mode_fields, parse_gaps,      # noqa: F401  (RUNNING_WARMUP and Gaps
                        parse_running)                                                                  # are part of this module's interface)
from .resample import FirResampler, MixedResampler, parse_streams, ratio as resample_ratio

SYNTHETIC_NOTE = ("synthetic recording: the stress phases are planted and easy, so the timeline shows that the recording-to-events "
                  "machinery works, not what detection is worth on WESAD")
SYNTHETIC_PHASES = [(1, 600.0), (2, 300.0), (4, 300.0), (3, 240.0), (2, 360.0), (1, 600.0)]      # 40 minutes


# ---- the parts that need no GPU ---------------------------------------------------------------------------------------------------
def count_windows(L_: int, T: int, S: int) -> int:
    """msig_rec_count: the windows [n * S, n * S + T) inside L samples; 0 if L < T."""
    n = int(L.lib().msig_rec_count(int(L_), int(T), int(S)))
    if n < 0:
        raise ValueError(f"window length and stride must be >= 1, got {T} and {S}")
    return n


REFERENCE_FORMS = ("'recording', 'head:K' with K >= 1, 'expanding[:W]', 'trailing:K[:W]' with K in 1..%d, 'decayed:H[:W]' with H in 1..%d and "
                   "W >= 0, a (w0, w1) pair or a statistics tensor" % (L.RN_MAX_K, L.RD_MAX_H))


def running_reference(reference) -> Optional[Running]:
    """The reference.Running — as a tuple (K, W) — of a causal running reference: "expanding[:W]" (K = 0: window n is normalised with
    windows 0..n), "trailing:K[:W]" (with the last K, 1 <= K <= RN_MAX_K) or "decayed:H[:W]" (K = 0, .H = H, .decay = exp2(-1 / H):
    every window so far, a half-life of H windows, 1 <= H <= RD_MAX_H); W >= 0 leading windows are flagged `warmup` (default 6).
    None for anything that is not spelled as one; ValueError for one that is spelled wrongly.  The grammar is reference.parse_running."""
    try:
        return parse_running(reference)
    except ValueError:
        raise ValueError(f"reference must be {REFERENCE_FORMS}, got {reference!r}") from None


def run_norm_reference(run_dir, config_name: Optional[str] = None) -> str:
    """NORM_REFERENCE of the run's cv_summary.txt (the file run_channels reads); "subject" where the line is absent."""
    base = Path(run_dir) / config_name if config_name else Path(run_dir)
    for path in (base / "cv_summary.txt", Path(run_dir) / "cv_summary.txt"):
        if path.exists():
            for line in path.read_text(encoding="utf-8").splitlines():
                if line.startswith("NORM_REFERENCE:"):
                    return line.split(":", 1)[1].strip()
            return "subject"
    return "subject"


def resolve_reference(trained: str, live: bool = False) -> str:
    """--reference auto: the monitor's counterpart of the --norm-reference a run was trained under.  subject -> recording (live:
    refused, it is not causal), baseline:K -> head:K, a running reference -> itself with the default warm-up; baseline (every
    baseline window, wherever it lies) has no counterpart on a recording."""
    from .dataset import parse_reference as parse_norm_reference          # training's grammar: None, 0, K or a Running
    try:
        k = parse_norm_reference(trained)
    except ValueError as e:
        raise ValueError(f"--reference auto: the run's NORM_REFERENCE is not one this monitor knows: {e}") from None
    if k is None:
        if live:
            raise ValueError("--reference auto: the run was trained under 'subject', whose counterpart 'recording' is not causal; a live "
                             "monitor can take 'expanding', best with a run trained under --norm-reference expanding")
        return "recording"
    if isinstance(k, Running):
        return f"{k.spelling}:{RUNNING_WARMUP}"
    if k == 0:
        raise ValueError("--reference auto: the run was trained under 'baseline' (every baseline window of a subject), which no reference "
                         "of a recording matches; train under baseline:K and monitor under 'head:K'")
    return f"head:{k}"


def parse_recording_reference(reference, n: int):
    """Which windows supply a recording's mean and std: "recording" (all of them: the counterpart of training's --norm-reference
    subject), "head:K" (the first K >= 1: the counterpart of baseline:K, 60 + 10 (K - 1) seconds at the default window and
    stride) or a pair (w0, w1) of window indices, 0 <= w0 < w1 <= n.  Returns (w0, w1, warm-up windows) — the warm-up count is K
    for "head:K" and 0 otherwise.  A running reference (running_reference: "expanding[:W]", "trailing:K[:W]", "decayed:H[:W]") has statistics per
    window: it returns (0, n, W), the windows any row may draw on and the number flagged.  A tensor of statistics is not parsed here
    (RecordingWindows takes it as it is)."""
    if reference == "recording":
        return 0, int(n), 0
    run = running_reference(reference)
    if run is not None:
        return 0, int(n), run[1]
    if isinstance(reference, str) and reference.startswith("head:"):
        k = reference[len("head:"):]
        if k.isascii() and k.isdigit() and int(k) >= 1:
            if int(k) > n:
                raise ValueError(f"reference {reference!r} needs {int(k)} windows; the recording has {n}")
            return 0, int(k), int(k)
        raise ValueError(f"reference must be {REFERENCE_FORMS}, got {reference!r}")
    if isinstance(reference, (tuple, list)) and len(reference) == 2 and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool)
                                                                             for v in reference):
        w0, w1 = int(reference[0]), int(reference[1])
        if not 0 <= w0 < w1 <= n:
            raise ValueError(f"reference windows must satisfy 0 <= w0 < w1 <= {n}, got {reference!r}")
        return w0, w1, 0
    raise ValueError(f"reference must be {REFERENCE_FORMS}, got {reference!r}")


def ema(score, halflife: float) -> np.ndarray:
    """The causal exponential moving average in float64: s_0 = score_0, s_n = s_{n-1} + a (score_n - s_{n-1}) with
    a = 1 - 2^(-1 / halflife) — after `halflife` windows a step has covered half its height.  halflife 0: the score itself."""
    x = np.asarray(score, dtype=np.float64).reshape(-1)
    if not halflife >= 0:
        raise ValueError(f"halflife must be >= 0 windows, got {halflife!r}")
    a = 1.0 if halflife == 0 else 1.0 - 2.0 ** (-1.0 / float(halflife))
    out = np.empty_like(x)
    s = 0.0
    for n, v in enumerate(x):
        s = float(v) if n == 0 else s + a * (float(v) - s)
        out[n] = s
    return out


def hysteresis(smoothed, on: float, off: float, min_on: int = 1) -> np.ndarray:
    """The state machine over a smoothed score: off at the start, on from the window where smoothed >= `on`, off again from the
    window where smoothed <= `off` (off < on: between the two the state holds).  An episode — a maximal run of on windows — shorter
    than `min_on` windows is dropped.  Returns (N,) bool."""
    if not off < on:
        raise ValueError(f"hysteresis needs off < on, got off = {off!r}, on = {on!r}")
    if isinstance(min_on, bool) or int(min_on) < 1:
        raise ValueError(f"min_on must be an integer >= 1, got {min_on!r}")
    x = np.asarray(smoothed, dtype=np.float64).reshape(-1)
    state = np.zeros(x.size, dtype=bool)
    cur = False
    for n, v in enumerate(x):
        if not cur and v >= on:
            cur = True
        elif cur and v <= off:
            cur = False
        state[n] = cur
    for a, b in _runs(state):
        if b - a < int(min_on):
            state[a:b] = False
    return state


def lost_windows(valid, lost_after: int) -> np.ndarray:
    """(N,) bool: window n is lost when it is invalid and the run of invalid windows it belongs to has reached `lost_after` windows
    at n — from the lost_after-th window of the run to its last."""
    if isinstance(lost_after, bool) or int(lost_after) < 1:
        raise ValueError(f"lost_after must be an integer >= 1, got {lost_after!r}")
    ok = np.asarray(valid, dtype=bool).reshape(-1)
    out = np.zeros(ok.size, dtype=bool)
    run = 0
    for n, v in enumerate(ok):
        run = 0 if v else run + 1
        out[n] = run >= int(lost_after)
    return out


def ema_gaps(score, valid, halflife: float, lost_after: int) -> np.ndarray:
    """`ema` over the valid windows only: an invalid window leaves s where it is (its own score is reported, it does not move the
    smoother), and after a lost stretch (lost_windows) the smoother restarts, s = score, at the next valid window, as at window 0.
    Before the first valid window s = 0.0.  With every window valid these are ema's operations in ema's order: the same bits."""
    x = np.asarray(score, dtype=np.float64).reshape(-1)
    ok = np.asarray(valid, dtype=bool).reshape(-1)
    if ok.size != x.size:
        raise ValueError(f"{x.size} scores and {ok.size} validity flags")
    if not halflife >= 0:
        raise ValueError(f"halflife must be >= 0 windows, got {halflife!r}")
    lost = lost_windows(ok, lost_after)
    a = 1.0 if halflife == 0 else 1.0 - 2.0 ** (-1.0 / float(halflife))
    out = np.empty_like(x)
    s, fresh = 0.0, True
    for n, v in enumerate(x):
        if ok[n]:
            s = float(v) if fresh else s + a * (float(v) - s)
            fresh = False
        elif lost[n]:
            fresh = True
        out[n] = s
    return out


def hysteresis_gaps(smoothed, valid, on: float, off: float, min_on: int = 1, lost_after: int = 6) -> np.ndarray:
    """`hysteresis` that an invalid window does not move: the state holds through it, and from the window where a run of invalid
    windows reaches `lost_after` (lost_windows) it is forced off until a valid window raises it again.  min_on acts on the resulting
    state sequence.  With every window valid this is hysteresis' array."""
    if not off < on:
        raise ValueError(f"hysteresis needs off < on, got off = {off!r}, on = {on!r}")
    if isinstance(min_on, bool) or int(min_on) < 1:
        raise ValueError(f"min_on must be an integer >= 1, got {min_on!r}")
    x = np.asarray(smoothed, dtype=np.float64).reshape(-1)
    ok = np.asarray(valid, dtype=bool).reshape(-1)
    if ok.size != x.size:
        raise ValueError(f"{x.size} smoothed scores and {ok.size} validity flags")
    lost = lost_windows(ok, lost_after)
    state = np.zeros(x.size, dtype=bool)
    cur = False
    for n, v in enumerate(x):
        if ok[n]:
            if not cur and v >= on:
                cur = True
            elif cur and v <= off:
                cur = False
        elif lost[n]:
            cur = False
        state[n] = cur
    for a, b in _runs(state):
        if b - a < int(min_on):
            state[a:b] = False
    return state


def _runs(state) -> List[Tuple[int, int]]:
    """The maximal runs of True in a bool vector as (first, one past last)."""
    s = np.concatenate(([False], np.asarray(state, dtype=bool), [False]))
    edges = np.flatnonzero(s[1:] != s[:-1])
    return [(int(a), int(b)) for a, b in zip(edges[0::2], edges[1::2])]


def find_events(state, smoothed, t_end) -> List[Tuple[float, float, float, float]]:
    """(start_s, end_s, peak, mean) of every episode of `state`: the end time of its first and of its last window (an episode is
    known from the moment its first window is complete), and the maximum and the mean of the smoothed score over it."""
    x, t = np.asarray(smoothed, dtype=np.float64), np.asarray(t_end, dtype=np.float64)
    return [(float(t[a]), float(t[b - 1]), float(x[a:b].max()), float(x[a:b].mean())) for a, b in _runs(state)]


@dataclass
class Timeline:
    """What Monitor.run returns, on the host: per window its end time t_end = (n S + T) / fs in seconds, the ensemble's mean_p and
    std_p (N, K), pred, entropy, mutual_info (N,), votes (N, K), score = mean_p[:, positive], smoothed (float64), state (bool),
    warmup (bool: the window supplied the statistics of a "head:K" reference, or is one of a running reference's first W); `events`
    as find_events lists them; `meta` the settings (under a running reference also reference_window_counts: per window the number
    of windows its statistics were taken over — integers, under "decayed:H" the real effective counts c_n; where the reference was
    resolved from the run, reference_requested = "auto" beside the resolved `reference`).  Only a monitor with `gaps` fills coverage
    (N, C) float64 — per selected channel the share of the window's samples that were valid —, valid and lost (N,) bool; its meta
    holds gaps = "MIN_COVERAGE:LOST_AFTER", invalid_windows and lost_windows, and its CSV the columns valid, coverage_min, lost."""
    t_end: np.ndarray
    mean_p: np.ndarray
    std_p: np.ndarray
    pred: np.ndarray
    entropy: np.ndarray
    mutual_info: np.ndarray
    votes: np.ndarray
    score: np.ndarray
    smoothed: np.ndarray
    state: np.ndarray
    warmup: np.ndarray
    events: List[Tuple[float, float, float, float]]
    meta: dict = field(default_factory=dict)
    coverage: Optional[np.ndarray] = None
    valid: Optional[np.ndarray] = None
    lost: Optional[np.ndarray] = None

    def to_csv(self, path) -> Path:
        path = Path(path)
        gaps = "gaps" in self.meta and self.coverage is not None
        lines = ["window,t_end_s,score,std,smoothed,state,pred,entropy,mutual_info,warmup" + (",valid,coverage_min,lost" if gaps else "")]
        pos = int(self.meta.get("positive", 1))
        for n in range(len(self.t_end)):
            lines.append(f"{n},{self.t_end[n]:.6f},{self.score[n]:.9g},{self.std_p[n, pos]:.9g},{self.smoothed[n]:.9g},{int(self.state[n])},"
                         f"{int(self.pred[n])},{self.entropy[n]:.9g},{self.mutual_info[n]:.9g},{int(self.warmup[n])}"
                         + (f",{int(self.valid[n])},{float(self.coverage[n].min()):.9g},{int(self.lost[n])}" if gaps else ""))
        path.write_text("\n".join(lines) + "\n")
        return path

    def to_json(self, path) -> Path:
        path = Path(path)
        doc = dict(self.meta, windows=int(len(self.t_end)), flagged_windows=int(self.state.sum()),
                   events=[dict(start_s=a, end_s=b, peak=p, mean=m) for a, b, p, m in self.events])
        path.write_text(json.dumps(doc, indent=1))
        return path


def phase_shares(timeline: Timeline, table, T: int, S: int) -> dict:
    """Of the windows that lie wholly inside a phase of a synthetic recording's phase table, the share flagged per raw label."""
    out = {}
    for row in table:
        n = np.arange(len(timeline.t_end))
        inside = (n * S >= row["start"]) & (n * S + T <= row["end"])
        tot, hit = out.get(row["label"], (0, 0))
        out[row["label"]] = (tot + int(inside.sum()), hit + int(timeline.state[inside].sum()))
    return {str(k): {"windows": t, "flagged": h, "share": (h / t if t else None)} for k, (t, h) in sorted(out.items())}


# ---- the recording on the GPU ------------------------------------------------------------------------------------------------------
class RecordingWindows:
    """The windows [n * stride, n * stride + T) of a (L, C_all) float64 recording (a numpy array, uploaded, or a GPU tensor), columns
    `names`, of which `channels` are selected in that order; the channel literally named 'chest_EDA' is log1p-transformed first, as
    in dataset.normalise_subject_device.  `reference`: parse_recording_reference, or a float64 tensor of 2 * MAX_C + 1 statistics
    (msig_nr.h's layout) taken as it is.  `.n` windows, `.shape` = (n, C, T), `.stats` the statistics on the device, `.warmup` the
    number of leading windows that supplied them ("head:K").  Under a running reference (running_reference) `.stats` is the
    (n, 2 * MAX_C + 1) table of one record per window, `.running` = (K, W) and `.warmup` = W, the windows flagged.
    `gaps` (a reference.Gaps; include/msig_gp.h): samples may be missing.  pivot -> window records -> statistics and coverage -> rows
    go through msig_gp_*; `.stats` is a table of one record per window also for a statistics tensor (the one record, broadcast) and
    `.coverage` the (n, MAX_C) table of every window's share of valid samples per selected channel.  Any other reference is refused."""

    def __init__(self, sig, names: Sequence[str], channels: Sequence[str], T: int, stride: int,
                 reference: Union[str, tuple, torch.Tensor] = "recording", device="cuda", gaps: Optional[Gaps] = None):
        if isinstance(sig, np.ndarray):
            sig = torch.from_numpy(np.ascontiguousarray(sig, dtype=np.float64)).to(device)
        if not isinstance(sig, torch.Tensor) or not sig.is_cuda or sig.dtype != torch.float64 or sig.dim() != 2:
            raise ValueError("a recording is a (L, C_all) float64 array: numpy, or a tensor on the GPU (there is no CPU fallback)")
        names, channels = list(names), list(channels)
        if len(names) != sig.shape[1]:
            raise ValueError(f"{len(names)} channel names for a recording of {sig.shape[1]} columns")
        if not 1 <= len(channels) <= L.MAX_C:
            raise ValueError(f"1..{L.MAX_C} channels can be selected, got {len(channels)}")
        missing = [c for c in channels if c not in names]
        if missing:
            raise ValueError(f"the recording has no channel {missing}; it has {names}")
        self.sig, self.device = sig.contiguous(), sig.device
        self.L, self.C_all = int(sig.shape[0]), int(sig.shape[1])
        self.T, self.S, self.C = int(T), int(stride), len(channels)
        self.n = count_windows(self.L, self.T, self.S)
        if self.n < 1:
            raise ValueError(f"the recording has {self.L} samples: shorter than one window of {self.T}")
        self.shape = (self.n, self.C, self.T)
        self.cols = (C.c_int32 * self.C)(*[names.index(c) for c in channels])
        self.mask = sum(1 << c for c, name in enumerate(channels) if name == "chest_EDA")
        self.running = running_reference(reference)
        self.gaps, self.coverage = gaps, None
        if gaps is not None:
            self._gap_tables(reference)
        elif self.running is not None:            # a record per window: the windows' own sums, then their ordered sums (msig_rn.h)
            self.reference_windows, self.warmup = None, self.running[1]
            sums = torch.empty((self.n, 2 * L.MAX_C), dtype=torch.float64, device=self.device)
            self.stats = torch.zeros((self.n, 2 * L.MAX_C + 1), dtype=torch.float64, device=self.device)
            L.check(L.lib().msig_rn_sums(*self._head(), 0, self.n, sums.data_ptr(), self._stream()), "msig_rn_sums")
            if self.running.kind == "decayed":
                L.check(L.lib().msig_rd_stats(*self._head(), sums.data_ptr(), self.n, self.running.decay, self.stats.data_ptr(), self._stream()),
                        "msig_rd_stats")
            else:
                L.check(L.lib().msig_rn_stats(*self._head(), sums.data_ptr(), self.n, self.running[0], self.stats.data_ptr(), self._stream()),
                        "msig_rn_stats")
        elif isinstance(reference, torch.Tensor):
            if reference.dtype != torch.float64 or reference.numel() < 2 * L.MAX_C + 1:
                raise ValueError(f"a statistics tensor holds 2 * {L.MAX_C} + 1 float64 values")
            self.stats, self.reference_windows, self.warmup = reference.to(self.device).contiguous().clone(), None, 0
        else:
            w0, w1, self.warmup = parse_recording_reference(reference, self.n)
            self.reference_windows = (w0, w1)
            self.stats = torch.empty(2 * L.MAX_C + 1, dtype=torch.float64, device=self.device)
            scratch = torch.empty(L.lib().msig_rec_scratch_bytes(), dtype=torch.uint8, device=self.device)
            L.check(L.lib().msig_rec_stats(*self._head(), w0, w1, self.stats.data_ptr(), scratch.data_ptr(), self._stream()), "msig_rec_stats")

    def _gap_tables(self, reference):
        """The gap-tolerant tables (msig_gp.h): the pivot record, the window records, then a statistics and a coverage record per window."""
        if not isinstance(self.gaps, Gaps):
            raise ValueError(f"gaps is a Gaps(min_coverage, lost_after) or None, got {self.gaps!r}")
        given = isinstance(reference, torch.Tensor)
        if self.running is None and not given:
            raise ValueError(f"{GAPS_REFERENCES}; got {reference!r}")
        if given and (reference.dtype != torch.float64 or reference.numel() < 2 * L.MAX_C + 1):
            raise ValueError(f"a statistics tensor holds 2 * {L.MAX_C} + 1 float64 values")
        self.reference_windows, self.warmup = None, (0 if given else self.running[1])
        lib, z = L.lib(), dict(dtype=torch.float64, device=self.device)
        self.pivot = torch.zeros(2 * L.MAX_C, **z)
        self.sums = torch.zeros((self.n, 3 * L.MAX_C), **z)
        self.stats = torch.zeros((self.n, 2 * L.MAX_C + 1), **z)
        self.coverage = torch.zeros((self.n, L.MAX_C), **z)
        mode = L.GpMode(*gp_mode_fields(self.running))
        L.check(lib.msig_gp_pivot(*self._head(), self.n, self.pivot.data_ptr(), self._stream()), "msig_gp_pivot")
        L.check(lib.msig_gp_sums(*self._head(), self.pivot.data_ptr(), 0, self.n, self.sums.data_ptr(), self._stream()), "msig_gp_sums")
        L.check(lib.msig_gp_stats(*self._head(), self.pivot.data_ptr(), self.sums.data_ptr(), self.n, C.byref(mode), self.stats.data_ptr(),
                                  self.coverage.data_ptr(), self._stream()), "msig_gp_stats")
        if given:                                # the coverage is the windows' own; every row takes the one given record
            self.stats = reference.to(self.device).reshape(-1)[:2 * L.MAX_C + 1][None, :].repeat(self.n, 1).contiguous()

    def _head(self):
        return self.sig.data_ptr(), self.L, self.C_all, self.cols, self.C, self.mask, self.T, self.S

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _rows(self, n0: int, B: int):
        if not (0 <= int(n0) and int(B) >= 1 and int(n0) + int(B) <= self.n):          # the table's row is addressed before the library checks
            raise ValueError(f"windows {n0} .. {int(n0) + int(B) - 1} are not all among the recording's {self.n}")

    def batch(self, n0: int, B: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Windows n0 .. n0 + B - 1 as a (B, C, T) float32 tensor (msig_rec_windows)."""
        if out is None:
            out = torch.empty((int(B), self.C, self.T), dtype=torch.float32, device=self.device)
        elif out.dtype != torch.float32 or tuple(out.shape) != (int(B), self.C, self.T) or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"out must be a contiguous float32 ({B}, {self.C}, {self.T}) tensor on {self.device}")
        if self.gaps is not None:
            self._rows(n0, B)
            L.check(L.lib().msig_gp_windows(*self._head(), int(n0), int(B), self.stats[int(n0)].data_ptr(), out.data_ptr(), self._stream()),
                    "msig_gp_windows")
            return out
        if self.running is not None:
            self._rows(n0, B)
            L.check(L.lib().msig_rn_windows(*self._head(), int(n0), int(B), self.stats[int(n0)].data_ptr(), out.data_ptr(), self._stream()),
                    "msig_rn_windows")
            return out
        L.check(L.lib().msig_rec_windows(*self._head(), int(n0), int(B), self.stats.data_ptr(), out.data_ptr(), self._stream()),
                "msig_rec_windows")
        return out

    def fill(self, x0: int, multi: L.Multi, n0: int, B: int):
        """Windows n0 .. n0 + B - 1 into the x buffer of every arena slot of `multi`; x0 is arena 0's (msig_rec_windows_multi)."""
        if self.gaps is not None:
            self._rows(n0, B)
            L.check(L.lib().msig_gp_windows_multi(*self._head(), int(n0), int(B), self.stats[int(n0)].data_ptr(), x0, C.byref(multi),
                                                  self._stream()), "msig_gp_windows_multi")
            return
        if self.running is not None:
            self._rows(n0, B)
            L.check(L.lib().msig_rn_windows_multi(*self._head(), int(n0), int(B), self.stats[int(n0)].data_ptr(), x0, C.byref(multi),
                                                  self._stream()), "msig_rn_windows_multi")
            return
        L.check(L.lib().msig_rec_windows_multi(*self._head(), int(n0), int(B), self.stats.data_ptr(), x0, C.byref(multi), self._stream()),
                "msig_rec_windows_multi")

    def materialise(self) -> torch.Tensor:
        """Every window, (n, C, T) float32, in one msig_rec_windows call.  For tests: it is the copy a monitor avoids."""
        return self.batch(0, self.n)


class RecordingEnsemble(Ensemble):
    """An Ensemble whose input is a RecordingWindows: predict(rw) runs Ensemble's own pieces, forwards and reduction; only the
    filling of the arenas differs — one msig_rec_windows_multi per piece instead of a copy per member."""

    def _check_x(self, x):
        if not isinstance(x, RecordingWindows):
            return super()._check_x(x)
        if x.device != self.device or x.C != self.C or x.T < 16:
            raise ValueError(f"expected windows of {self.C} channels and T >= 16 on {self.device}, got {x.C} channels, T = {x.T} on {x.device}")
        return x

    def _fill(self, x, i: int, b: int, n: int):
        if not isinstance(x, RecordingWindows):
            return super()._fill(x, i, b, n)
        x.fill(self.arenas.ptr("x"), self.arenas.multi(range(n)), i, b)


class Monitor:
    """An ensemble of 1..256 trained models (M = 1: one model) over continuous recordings sampled at `fs` Hz: windows of `window_s`
    seconds every `stride_s`, normalised by `reference` (parse_recording_reference), `eval_batch` windows per piece.  `channels`: the
    names of the models' input channels in their order (None: the recording's columns as they come).  score = the probability of
    class `positive`; smoothed = ema(score, halflife) (in windows); state = hysteresis(smoothed, on, off, min_on).
    `gaps` (a Gaps; None: every sample is taken as a number, as ever): samples may be missing (module docstring) — the timeline
    gains coverage, valid and lost, and smoothed and state are ema_gaps' and hysteresis_gaps'."""

    def __init__(self, models: Sequence, fs: float, window_s: float = 60, stride_s: float = 10, reference="recording", eval_batch: int = 256,
                 positive: int = 1, halflife: float = 3, on: float = 0.6, off: float = 0.4, min_on: int = 2,
                 channels: Optional[Sequence[str]] = None, gaps: Optional[Gaps] = None, resampler=None):
        if not float(fs) > 0:
            raise ValueError(f"fs must be > 0, got {fs!r}")
        self.fs = float(fs)
        if resampler is not None and (not isinstance(resampler, (FirResampler, MixedResampler)) or resampler.fs_out != self.fs):
            raise ValueError(f"resampler is a FirResampler or a MixedResampler whose fs_out is the monitor's fs = {self.fs:g}, or None; got {resampler!r}")
        self.resampler = resampler
        self.T, self.S = int(round(float(window_s) * self.fs)), int(round(float(stride_s) * self.fs))
        if self.T < 16 or self.S < 1:
            raise ValueError(f"a window needs >= 16 samples and a stride >= 1, got {self.T} and {self.S}")
        hysteresis([], on, off, min_on)
        ema([], halflife)
        if gaps is not None and not isinstance(gaps, Gaps):
            raise ValueError(f"gaps is a Gaps(min_coverage, lost_after) or None, got {gaps!r}")
        if gaps is not None and running_reference(reference) is None and not isinstance(reference, torch.Tensor):
            raise ValueError(f"{GAPS_REFERENCES}; got {reference!r}")
        self.gaps = gaps
        self.ensemble = RecordingEnsemble(models, eval_batch=eval_batch)
        if not 0 <= int(positive) < self.ensemble.K:
            raise ValueError(f"positive must be a class in 0..{self.ensemble.K - 1}, got {positive!r}")
        self.reference, self.positive, self.halflife, self.on, self.off, self.min_on = reference, int(positive), float(halflife), float(on), float(off), int(min_on)
        self.reference_requested = None          # "auto" where from_run resolved the reference from the run
        self.channels = None if channels is None else list(channels)
        if self.channels is not None and len(self.channels) != self.ensemble.C:
            raise ValueError(f"the models take {self.ensemble.C} channels, got {len(self.channels)} names")
        self.files: List[Path] = []

    @staticmethod
    def run_files(run_dir, subject: Optional[str] = None, config_name: Optional[str] = None) -> List[Path]:
        """The checkpoints from_run loads.  `subject` given: that fold's members by Ensemble.from_run's rule (ensemble.member_files).
        None — the recording is of a person no fold held out: replica 0 of every fold, fold_test_on_*/best_model.pt in natural order
        of the subject names (S2 before S10)."""
        if subject is not None:
            return member_files(run_dir, subject, config_name)
        base = Path(run_dir) / config_name if config_name else Path(run_dir)
        files = [d / "best_model.pt" for d in base.glob("fold_test_on_*") if (d / "best_model.pt").exists()]
        if not files:
            raise FileNotFoundError(f"no fold_test_on_*/best_model.pt below {base}")
        return sorted(files, key=lambda f: [int(p) if p.isdigit() else p for p in re.split(r"(\d+)", f.parent.name)])

    @staticmethod
    def run_channels(run_dir, config_name: Optional[str] = None) -> Optional[List[str]]:
        """CHANNELS_TO_USE of the run's cv_summary.txt, or None where there is none."""
        base = Path(run_dir) / config_name if config_name else Path(run_dir)
        for path in (base / "cv_summary.txt", Path(run_dir) / "cv_summary.txt"):
            if path.exists():
                for line in path.read_text(encoding="utf-8").splitlines():
                    if line.startswith("CHANNELS_TO_USE:"):
                        return [str(c) for c in ast.literal_eval(line.split(":", 1)[1].strip())]
        return None

    @classmethod
    def from_run(cls, run_dir, subject: Optional[str] = None, config_name: Optional[str] = None, fs: float = 64.0, device="cuda", **kw) -> "Monitor":
        """reference="auto": the counterpart of the run's NORM_REFERENCE (resolve_reference), resolved before anything is loaded."""
        auto = isinstance(kw.get("reference"), str) and kw["reference"] == "auto"
        if auto:
            kw["reference"] = resolve_reference(run_norm_reference(run_dir, config_name))
        files = cls.run_files(run_dir, subject, config_name)
        kw.setdefault("channels", cls.run_channels(run_dir, config_name))
        self = cls(load_members(files, device), fs, **kw)
        self.files = files
        self.reference_requested = "auto" if auto else None
        return self

    def windows(self, sig, names: Sequence[str]) -> RecordingWindows:
        names = list(names)
        return RecordingWindows(sig, names, self.channels if self.channels is not None else names, self.T, self.S, self.reference,
                                device=self.ensemble.device, gaps=self.gaps)

    @torch.no_grad()
    def run(self, sig, names: Optional[Sequence[str]] = None) -> Timeline:
        """The timeline of the recording `sig` with the columns `names`.  With a MixedResampler `sig` is {stream: array}, each at its
        stream's rate, and the columns are the resampler's (`names`, if given, must equal them)."""
        raw = None
        if isinstance(self.resampler, MixedResampler):      # every stream at its own rate: the rows all of them have delivered are monitored
            if names is not None and list(names) != self.resampler.names:
                raise ValueError(f"the resampler's streams have the columns {self.resampler.names}, got {list(names)}")
            if not isinstance(sig, dict):
                raise ValueError("with a MixedResampler a recording is {stream: array}, each array at its stream's rate")
            names, y = self.resampler.names, self.resampler.apply(sig)
            raw, sig = {g.name: int(sig[g.name].shape[0]) for g in self.resampler.streams}, y
        elif names is None:
            raise ValueError("run(sig, names) takes the names of the recording's columns")
        elif self.resampler is not None:           # the recording is at the resampler's fs_in: its causal outputs are what is monitored
            if not isinstance(sig, (np.ndarray, torch.Tensor)) or sig.ndim != 2:
                raise ValueError("a recording is a (L, C_all) float64 array: numpy, or a tensor on the GPU (there is no CPU fallback)")
            raw, sig = int(sig.shape[0]), self.resampler.apply(sig)
        rw = self.windows(sig, names)
        p = self.ensemble.predict(rw)
        host = lambda t: t.cpu().numpy()      # noqa: E731
        mean_p = host(p.mean_p)
        score = mean_p[:, self.positive].astype(np.float64)
        t_end = (np.arange(rw.n, dtype=np.float64) * self.S + self.T) / self.fs
        extra = {}
        if self.gaps is None:
            smoothed = ema(score, self.halflife)
            state = hysteresis(smoothed, self.on, self.off, self.min_on)
        else:
            coverage = np.ascontiguousarray(host(rw.coverage)[:, :rw.C])
            valid = self.gaps.valid(coverage)
            smoothed = ema_gaps(score, valid, self.halflife, self.gaps.lost_after)
            state = hysteresis_gaps(smoothed, valid, self.on, self.off, self.min_on, self.gaps.lost_after)
            extra = dict(coverage=coverage, valid=valid, lost=lost_windows(valid, self.gaps.lost_after))
        warmup = np.arange(rw.n) < rw.warmup
        meta = dict(fs=self.fs, window_samples=self.T, stride_samples=self.S, members=self.ensemble.M, positive=self.positive,
                    halflife=self.halflife, on=self.on, off=self.off, min_on=self.min_on, samples=rw.L,
                    reference=self.reference if isinstance(self.reference, str) else ("statistics" if rw.reference_windows is None
                                                                                      else list(rw.reference_windows)),
                    warmup_windows=int(rw.warmup), files=[str(f) for f in self.files])
        if rw.running is not None:
            counts = rw.stats[:, 2 * L.MAX_C].cpu().numpy()          # decayed: c_n, the effective number of windows, a real number
            meta["reference_window_counts"] = [float(v) if rw.running.kind == "decayed" else int(v) for v in counts]
        if self.reference_requested is not None:
            meta["reference_requested"] = self.reference_requested
        if self.gaps is not None:
            meta.update(gaps=self.gaps.spelling, invalid_windows=int((~extra["valid"]).sum()), lost_windows=int(extra["lost"].sum()))
        if self.resampler is not None:
            meta.update(resampler=self.resampler.spelling, resampler_latency_s=self.resampler.latency_s, raw_samples=raw)
        return Timeline(t_end=t_end, mean_p=mean_p, std_p=host(p.std_p), pred=host(p.pred), entropy=host(p.entropy),
                        mutual_info=host(p.mutual_info), votes=host(p.votes), score=score, smoothed=smoothed, state=state, warmup=warmup,
                        events=find_events(state, smoothed, t_end), meta=meta, **extra)


# ---- the command line ----------------------------------------------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m multimodalsignal_amd.monitor",
                                 description="The stress timeline of a continuous recording from a trained run: timeline.csv and timeline.json.")
    ap.add_argument("--run", type=Path, required=True, help="the run directory (the one that holds fold_test_on_*/)")
    ap.add_argument("--subject", default=None, help="use the members of the fold that tested this subject (default: replica 0 of every fold)")
    ap.add_argument("--config", default=None, help="configuration name of a --model / sweep run")
    ap.add_argument("--recording", type=Path, default=None, help="(L, C_all) float64 .npy")
    ap.add_argument("--names", type=Path, default=None, help="the recording's channel names, one per line")
    ap.add_argument("--synthetic-recording", action="store_true", help="a seeded 40-minute recording with planted stress phases")
    ap.add_argument("--fs", type=float, default=64.0, help="sampling rate the models were trained at")
    ap.add_argument("--resample-from", type=float, default=None, help="the recording's own sampling rate: it is resampled to --fs first")
    ap.add_argument("--resampler", choices=("fft", "fir"), default="fft",
                    help="how --resample-from is resampled: fft — the whole recording at once (scipy.signal.resample's method); fir — the causal "
                         "polyphase FIR resampler a live monitor runs (with it, --synthetic-recording is built at the --resample-from rate)")
    ap.add_argument("--streams", default=None, metavar="SPEC",
                    help="mixed-rate streams, NAME=RATE:COLUMN,...;NAME=RATE:COLUMN,... — every stream is resampled to --fs by the causal FIR "
                         "resampler (a stream at --fs is copied); --recording is then an .npz keyed by stream name, --synthetic-recording is "
                         "built per stream at its rate; excludes --resample-from")
    ap.add_argument("--reference", default="recording", help="recording | head:K | expanding[:W] | trailing:K[:W] | decayed:H[:W] | auto (the counterpart of the run's NORM_REFERENCE)")
    ap.add_argument("--window-s", type=float, default=60.0)
    ap.add_argument("--stride-s", type=float, default=10.0)
    ap.add_argument("--seed", type=int, default=42, help="seed of --synthetic-recording")
    ap.add_argument("--difficulty", type=float, default=1.0, help="difficulty of --synthetic-recording")
    ap.add_argument("--gaps", nargs="?", const="", default=None, metavar="MIN_COVERAGE[:LOST_AFTER]",
                    help="samples may be missing (NaN, +-Inf): a window whose smallest channel coverage is below MIN_COVERAGE (0.75) is "
                         "invalid and holds the smoother and the state; after LOST_AFTER (6) invalid windows in a row the state is off")
    ap.add_argument("--synthetic-gaps", default=None, metavar="SPEC",
                    help="plant gaps into --synthetic-recording: drop=RATE,channel=INDEX:START_S:SECONDS,all=START_S:SECONDS")
    ap.add_argument("--out", type=Path, required=True)
    return ap


def check_gap_args(ap, a):
    """--gaps and --synthetic-gaps, checked before anything touches the GPU; a.gaps becomes a Gaps or None."""
    try:
        a.gaps = None if a.gaps is None else parse_gaps(a.gaps)
        if a.synthetic_gaps is not None:
            if not a.synthetic_recording:
                ap.error("--synthetic-gaps goes with --synthetic-recording")
            from .synth import parse_synthetic_gaps
            spec = parse_synthetic_gaps(a.synthetic_gaps)
            known = [st.name for st in a.streams] if getattr(a, "streams", None) else []
            if any(name not in known for name, _a, _d in spec["stream"]):
                ap.error(f"--synthetic-gaps stream=NAME:START_S:SECONDS names one of the --streams {known}")
        if a.gaps is not None and a.reference != "auto" and running_reference(a.reference) is None:
            ap.error(GAPS_REFERENCES + f"; got {a.reference!r}")
    except ValueError as e:
        ap.error(str(e))


def check_source_args(ap, a):
    """--recording / --synthetic-recording, --names, --fs, --resample-from, --resampler and --streams, checked before anything touches
    the GPU; a.streams becomes a list of Stream or None."""
    if a.synthetic_recording == (a.recording is not None):
        ap.error("give exactly one of --recording X.npy and --synthetic-recording")
    if a.streams is not None:
        if a.resample_from is not None:
            ap.error("--streams excludes --resample-from: every stream has its own rate")
        if a.names is not None:
            ap.error("--streams names the columns itself: it takes no --names")
        if not a.fs > 0:
            ap.error("--fs must be > 0")
        try:
            a.streams = parse_streams(a.streams)
            MixedResampler(a.streams, a.fs, device="cpu")          # the ratios and the column sets, on the host
            if a.synthetic_recording:
                from .synth import CHANNELS6
                unknown = [c for st in a.streams for c in st.columns if c not in CHANNELS6]
                if unknown:
                    raise ValueError(f"--synthetic-recording has the channels {CHANNELS6}; --streams names {unknown}")
        except ValueError as e:
            ap.error(str(e))
        return
    if a.recording is not None and a.names is None:
        ap.error("--recording needs --names FILE (one channel name per line)")
    if a.synthetic_recording and (a.names is not None or (a.resample_from is not None and a.resampler != "fir")):
        ap.error("--synthetic-recording takes neither --names nor --resample-from (--resampler fir excepted: the recording is built at that rate)")
    if not a.fs > 0 or (a.resample_from is not None and not a.resample_from > 0):
        ap.error("--fs and --resample-from must be > 0")
    if a.resampler == "fir":
        if a.resample_from is None:
            ap.error("--resampler fir needs --resample-from RATE")
        try:
            resample_ratio(a.resample_from, a.fs)
        except ValueError as e:
            ap.error(str(e))


def raw_phase_table(table, fs: float):
    """A synthetic recording's phase table with start and end in samples at `fs` instead of the rate the recording was built at."""
    return [dict(row, start=row["start_s"] * fs, end=row["end_s"] * fs) for row in table]


def parse_args(argv=None) -> argparse.Namespace:
    """The arguments, checked before anything touches the GPU."""
    ap = build_parser()
    a = ap.parse_args(argv)
    check_source_args(ap, a)
    if not a.window_s > 0 or not a.stride_s > 0:
        ap.error("--window-s and --stride-s must be > 0")
    try:
        if a.reference != "auto":
            parse_recording_reference(a.reference, 1 << 62)
    except ValueError as e:
        ap.error(str(e))
    check_gap_args(ap, a)
    return a


def load_streams(a, resampler: MixedResampler):
    """--streams: ({stream: (n, ncols) float64 numpy array}, phase table or None) of --recording X.npz or --synthetic-recording."""
    if a.synthetic_recording:
        from .synth import make_synthetic_streams
        return make_synthetic_streams(SYNTHETIC_PHASES, a.streams, fs=a.fs, seed=a.seed, difficulty=a.difficulty, gaps=a.synthetic_gaps)
    with np.load(a.recording) as z:
        missing = [g.name for g in resampler.streams if g.name not in z.files]
        if missing:
            raise ValueError(f"{a.recording} holds the arrays {z.files}; --streams names {missing} too")
        return {g.name: np.ascontiguousarray(z[g.name], dtype=np.float64) for g in resampler.streams}, None


def main_streams(a) -> Timeline:
    """main with --streams: the recording is a dict of arrays, each at its stream's rate."""
    mx = MixedResampler(a.streams, a.fs)
    mon = Monitor.from_run(a.run, a.subject, a.config, fs=a.fs, window_s=a.window_s, stride_s=a.stride_s, reference=a.reference, gaps=a.gaps,
                           resampler=mx)
    sig, table = load_streams(a, mx)
    tl = mon.run(sig)
    if table is not None:
        tl.meta.update(note=SYNTHETIC_NOTE, phases=table, flagged_by_label=phase_shares(tl, table, mon.T, mon.S))
    a.out.mkdir(parents=True, exist_ok=True)
    tl.to_csv(a.out / "timeline.csv")
    path = tl.to_json(a.out / "timeline.json")
    print(f"{len(tl.t_end)} windows, {int(tl.state.sum())} flagged, {len(tl.events)} events; timeline written to: {path}")
    print(f"resampler {mx.spelling}: {tl.meta['raw_samples']} raw samples -> {tl.meta['samples']}, latency {mx.latency_s:.3f} s")
    if a.gaps is not None:
        print(f"gaps {a.gaps.spelling}: {tl.meta['invalid_windows']} invalid windows, {tl.meta['lost_windows']} lost; "
              f"{int((~np.isfinite(tl.score)).sum())} of {len(tl.score)} scores are not finite")
    if table is not None:
        print("NOTE: " + SYNTHETIC_NOTE + ".")
        print("flagged windows by raw label: " + json.dumps(tl.meta["flagged_by_label"]))
    return tl


def main(argv=None) -> Timeline:
    a = parse_args(argv)
    if a.streams is not None:
        return main_streams(a)
    fir = FirResampler(a.resample_from, a.fs) if a.resampler == "fir" else None      # the recording is monitored at its own rate
    mon = Monitor.from_run(a.run, a.subject, a.config, fs=a.fs, window_s=a.window_s, stride_s=a.stride_s, reference=a.reference, gaps=a.gaps,
                           resampler=fir)
    table = None
    if a.synthetic_recording:
        from .synth import CHANNELS6, make_synthetic_recording
        names = list(CHANNELS6)
        sig, table = make_synthetic_recording(SYNTHETIC_PHASES, fs=a.fs if fir is None else a.resample_from, channels=names, seed=a.seed,
                                              difficulty=a.difficulty, gaps=a.synthetic_gaps)
        if fir is not None:
            table = raw_phase_table(table, a.fs)
    else:
        sig = np.load(a.recording)
        names = [ln.strip() for ln in a.names.read_text().splitlines() if ln.strip()]
    sig = torch.from_numpy(np.ascontiguousarray(sig, dtype=np.float64)).to(mon.ensemble.device)
    if a.resample_from is not None and fir is None:
        from .preprocess import resample_device
        sig = resample_device(sig, int(sig.shape[0] * (a.fs / a.resample_from)))
    tl = mon.run(sig, names)
    if table is not None:
        tl.meta.update(note=SYNTHETIC_NOTE, phases=table, flagged_by_label=phase_shares(tl, table, mon.T, mon.S))
    a.out.mkdir(parents=True, exist_ok=True)
    tl.to_csv(a.out / "timeline.csv")
    path = tl.to_json(a.out / "timeline.json")
    print(f"{len(tl.t_end)} windows, {int(tl.state.sum())} flagged, {len(tl.events)} events; timeline written to: {path}")
    if fir is not None:
        print(f"resampler {fir.spelling}: {tl.meta['raw_samples']} raw samples -> {tl.meta['samples']}, latency {fir.latency_s:.3f} s")
    if a.gaps is not None:
        print(f"gaps {a.gaps.spelling}: {tl.meta['invalid_windows']} invalid windows, {tl.meta['lost_windows']} lost; "
              f"{int((~np.isfinite(tl.score)).sum())} of {len(tl.score)} scores are not finite")
    if table is not None:
        print("NOTE: " + SYNTHETIC_NOTE + ".")
        print("flagged windows by raw label: " + json.dumps(tl.meta["flagged_by_label"]))
    return tl


if __name__ == "__main__":
    main()
