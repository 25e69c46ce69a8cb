"""Causal polyphase FIR resampling by a rational ratio (include/msig_rs.h).

A wearable does not deliver the models' rate: WESAD's chest device samples at 700 Hz, the models take 64 Hz.  `FirResampler` is the
resampler that can run live: the filter and the convention of scipy.signal.resample_poly — a Kaiser-windowed sinc of
2 * half + 1 taps, zero phase — with an output emitted only once its whole support has arrived, so the outputs are a causal function
of the stream with a fixed latency.  `apply` resamples a whole recording (msig_rs_resample); `LiveMonitor(resampler=...)` pushes
raw-rate chunks through the same device function into its rings (msig_rs_lv_push): the same bits, whatever the chunking.

The ratio L / M = fs_out / fs_in in lowest terms, half = half_width * max(L, M),
h = firwin(2 * half + 1, 1 / max(L, M), window=("kaiser", beta)) * L, restated in numpy (`fir_taps`); 700 -> 64 Hz gives L = 16,
M = 175, 3501 taps, 219 of them per output.  `fir_taps`, `ratio` and `out_count` need no GPU.  `apply` has no CPU fallback.

Mixed rates (include/msig_mx.h): a wearer's devices do not share a rate either — WESAD's wrist device delivers
BVP at 64 Hz, ACC at 32 Hz, EDA and TEMP at 4 Hz.  `MixedResampler([Stream(name, fs, columns), ...], fs_out)` groups the columns of
a session into streams, each resampled to fs_out by `FirResampler`'s ratio, half and taps for its rate (a stream already at fs_out
is copied); `apply` and `LiveMonitor(resampler=...)` take a dict of arrays keyed by stream name.
"""
from __future__ import annotations

import ctypes as C
import math
from fractions import Fraction
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L


def ratio(fs_in, fs_out) -> Tuple[int, int]:
    """(L, M) with L / M = fs_out / fs_in exactly, in lowest terms; ValueError where the rates are not positive, are equal or have no
    exact ratio with L and M within RS_MAX_RATIO."""
    try:
        a, b = Fraction(fs_in), Fraction(fs_out)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"sampling rates are positive numbers, got {fs_in!r} and {fs_out!r}") from None
    if not (a > 0 and b > 0):
        raise ValueError(f"sampling rates are positive numbers, got {fs_in!r} and {fs_out!r}")
    if a == b:
        raise ValueError(f"fs_in == fs_out == {fs_in!r}: there is nothing to resample")
    q = b / a
    if q.numerator > L.RS_MAX_RATIO or q.denominator > L.RS_MAX_RATIO:
        raise ValueError(f"{fs_in!r} -> {fs_out!r} Hz is the ratio {q.numerator} / {q.denominator}: not exact within {L.RS_MAX_RATIO}")
    return int(q.numerator), int(q.denominator)


def fir_taps(up: int, down: int, half_width: int = 10, beta: float = 5.0) -> np.ndarray:
    """scipy.signal.firwin(2 * half + 1, 1 / max(up, down), window=("kaiser", beta)) * up with half = half_width * max(up, down), in
    float64: the sinc at the cutoff times the symmetric Kaiser window, normalised to unit sum."""
    big = max(int(up), int(down))
    half = int(half_width) * big
    m = np.arange(-half, half + 1, dtype=np.float64)
    h = np.sinc(m / big) / big * np.kaiser(2 * half + 1, float(beta))
    return np.ascontiguousarray(h / h.sum() * int(up))


def out_count(n_in: int, up: int, down: int, half: int) -> int:
    """msig_rs_out_count: the outputs whose whole support lies inside n_in raw rows."""
    v = int(n_in) * int(up) - int(half) - 1
    return 0 if v < 0 else v // int(down) + 1


class FirResampler:
    """fs_in -> fs_out Hz on `device`.  `.L`, `.M`, `.half`, `.h` (the taps on the device, uploaded once; `.taps` on the host),
    `.tail_rows` — the raw rows a live session keeps —, `.latency_s`, `.spelling`; out_count(n), max_rows(k), apply(sig)."""

    def __init__(self, fs_in, fs_out, device="cuda", half_width: int = 10, beta: float = 5.0):
        self.L, self.M = ratio(fs_in, fs_out)
        if isinstance(half_width, bool) or not isinstance(half_width, (int, np.integer)) or int(half_width) < 1:
            raise ValueError(f"half_width is an integer >= 1 (zero crossings of the sinc on each side), got {half_width!r}")
        if not float(beta) >= 0:
            raise ValueError(f"beta must be >= 0, got {beta!r}")
        self.fs_in, self.fs_out, self.half_width, self.beta = float(fs_in), float(fs_out), int(half_width), float(beta)
        self.half = self.half_width * max(self.L, self.M)
        if self.half > L.RS_MAX_HALF:
            raise ValueError(f"half_width {half_width} at the ratio {self.L} / {self.M} needs {2 * self.half + 1} taps; at most {2 * L.RS_MAX_HALF + 1}")
        self.taps = fir_taps(self.L, self.M, self.half_width, self.beta)
        self.device = torch.device(device)
        self.h = torch.from_numpy(self.taps).to(self.device)
        self.tail_rows = 2 * self.half // self.L + 1
        # output m lies at raw time m M / L; its last raw row, floor((m M + half) / L), has arrived half // L + 1 raw rows later at most
        self.latency_s = (self.half // self.L + 1) / self.fs_in
        self.spelling = f"fir:{self.fs_in:g}->{self.fs_out:g}:{self.L}/{self.M}:half{self.half}:kaiser{self.beta:g}"

    def ratio_args(self):
        """h, L, M, half as msig_rs.h's calls take them."""
        return self.h.data_ptr(), self.L, self.M, self.half

    def out_count(self, n_in: int) -> int:
        return out_count(n_in, self.L, self.M, self.half)

    def max_rows(self, k: int) -> int:
        """The largest n_in with out_count(n_in) <= k."""
        return (int(k) * self.M + self.half) // self.L

    def apply(self, sig) -> torch.Tensor:
        """The out_count(n) rows of a (n,) or (n, cols) float64 recording — numpy, uploaded, or a tensor on the resampler's GPU."""
        if isinstance(sig, np.ndarray):
            sig = torch.from_numpy(np.ascontiguousarray(sig, dtype=np.float64)).to(self.device)
        if not isinstance(sig, torch.Tensor) or not sig.is_cuda or sig.device != self.h.device or sig.dtype != torch.float64 or sig.dim() not in (1, 2):
            raise ValueError("apply takes a (n,) or (n, cols) float64 array: numpy, or a tensor on the resampler's GPU (there is no CPU fallback)")
        x = sig.reshape(sig.shape[0], -1).contiguous()
        n = self.out_count(x.shape[0])
        y = torch.empty((n, x.shape[1]), dtype=torch.float64, device=x.device)
        if x.shape[1] > 0:
            stream = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
            L.check(L.lib().msig_rs_resample(x.data_ptr(), x.shape[0], x.shape[1], *self.ratio_args(), y.data_ptr(), n, stream), "msig_rs_resample")
        return y.reshape((n,) + tuple(sig.shape[1:]))


class Stream:
    """The columns `columns` of a session, delivered together at `fs` Hz under the name `name`."""

    def __init__(self, name: str, fs, columns: Sequence[str]):
        if not isinstance(name, str) or not name:
            raise ValueError(f"a stream's name is a non-empty string, got {name!r}")
        if isinstance(columns, str) or len(list(columns)) < 1 or not all(isinstance(c, str) and c for c in columns):
            raise ValueError(f"stream {name!r}: columns is a non-empty sequence of column names, got {columns!r}")
        try:
            ok = Fraction(fs) > 0
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not ok:
            raise ValueError(f"stream {name!r}: fs is a positive number, got {fs!r}")
        self.name, self.fs, self.columns = name, float(fs), [str(c) for c in columns]

    def __repr__(self):
        return f"Stream({self.name!r}, {self.fs:g}, {self.columns!r})"


STREAMS_FORM = "NAME=RATE:COLUMN[,COLUMN...] per stream, the streams separated by ';' (chest=700:chest_ECG,chest_EDA;eda=4:wrist_EDA)"


def parse_streams(spec) -> List[Stream]:
    """--streams SPEC -> [Stream, ...]."""
    out = []
    try:
        for item in str(spec).split(";"):
            name, eq, rest = item.strip().partition("=")
            rate, colon, cols = rest.partition(":")
            if not (eq and colon and name.strip()):
                raise ValueError
            out.append(Stream(name.strip(), float(rate), [c.strip() for c in cols.split(",")]))
    except ValueError:
        raise ValueError(f"--streams takes {STREAMS_FORM}, got {spec!r}") from None
    return out


class _MixedStream:
    """A stream inside a MixedResampler: `.name`, `.fs`, `.columns`, its ratio `.L`, `.M`, `.half` (1, 1, 0: the identity, copied),
    `.col0`, `.ncols` — its columns of a ring row —, `.h_off` and `.tail_off` (doubles into the tap table and into a session's tail
    block), `.tail_rows`, `.latency_s`, `.spelling`; out_count(n), max_rows(k)."""

    def __init__(self, st: Stream, fs_out: float, col0: int, h_off: int, tail_off: int, half_width: int, beta: float):
        self.name, self.fs, self.columns, self.col0, self.ncols = st.name, st.fs, list(st.columns), col0, len(st.columns)
        self.identity = Fraction(st.fs) == Fraction(fs_out)
        if self.identity:
            self.L, self.M, self.half, self.taps, self.tail_rows, self.latency = 1, 1, 0, np.zeros(0, dtype=np.float64), 0, Fraction(0)
            self.spelling = f"{self.name}=copy:{self.fs:g}"
        else:
            self.L, self.M = ratio(st.fs, fs_out)
            self.half = half_width * max(self.L, self.M)
            if self.half > L.RS_MAX_HALF:
                raise ValueError(f"stream {self.name!r}: half_width {half_width} at the ratio {self.L} / {self.M} needs {2 * self.half + 1} taps; "
                                 f"at most {2 * L.RS_MAX_HALF + 1}")
            self.taps = fir_taps(self.L, self.M, half_width, beta)
            self.tail_rows = 2 * self.half // self.L + 1
            self.latency = Fraction(self.half // self.L + 1) / Fraction(st.fs)      # FirResampler.latency_s, exactly
            self.spelling = f"{self.name}=fir:{self.fs:g}->{fs_out:g}:{self.L}/{self.M}:half{self.half}"
        self.latency_s = (self.half // self.L + 1) / self.fs if not self.identity else 0.0
        self.h_off, self.tail_off = h_off, tail_off

    def out_count(self, n_in: int) -> int:
        return out_count(n_in, self.L, self.M, self.half)

    def max_rows(self, k: int) -> int:
        """The largest n_in with out_count(n_in) <= k."""
        return (int(k) * self.M + self.half) // self.L

    def group(self) -> "L.MxGroup":
        return L.MxGroup(self.L, self.M, self.half, self.col0, self.ncols, 0, self.h_off, self.tail_rows, self.tail_off)


class MixedResampler:
    """1..MX_MAX_GROUPS streams, each at its own rate, resampled to fs_out Hz on `device`.  The session's column order is the
    resampler's: `.names` is the streams' columns concatenated in stream order, so stream g owns the columns [col0, col0 + ncols) of
    every ring row.  `.streams` (per stream L, M, half, tail_rows, latency_s, ...), `.stream[name]`, `.h` — one device table of
    every stream's taps —, `.tail_doubles` — the size of a session's tail block —, `.latency_s` (the largest stream latency),
    `.latency_spread_rows` = ceil((max latency - min latency) * fs_out), `.spelling`; out_count({name: n_raw}) is the minimum over
    the streams; apply({name: array}).  All streams start at the same instant: raw row 0 of every stream is t = 0."""

    def __init__(self, streams: Sequence[Stream], fs_out, device="cuda", half_width: int = 10, beta: float = 5.0):
        streams = list(streams)
        if not 1 <= len(streams) <= L.MX_MAX_GROUPS or not all(isinstance(s, Stream) for s in streams):
            raise ValueError(f"a mixed resampler takes 1..{L.MX_MAX_GROUPS} Stream objects, got {len(streams)}")
        if isinstance(half_width, bool) or not isinstance(half_width, (int, np.integer)) or int(half_width) < 1:
            raise ValueError(f"half_width is an integer >= 1 (zero crossings of the sinc on each side), got {half_width!r}")
        if not float(beta) >= 0:
            raise ValueError(f"beta must be >= 0, got {beta!r}")
        if not float(fs_out) > 0:
            raise ValueError(f"fs_out must be > 0, got {fs_out!r}")
        names = [s.name for s in streams]
        if len(set(names)) != len(names):
            raise ValueError(f"stream names are unique, got {names}")
        cols = [c for s in streams for c in s.columns]
        twice = sorted({c for c in cols if cols.count(c) > 1})
        if twice:
            raise ValueError(f"every column belongs to exactly one stream; {twice} appear more than once")
        self.fs_out, self.half_width, self.beta = float(fs_out), int(half_width), float(beta)
        self.streams: List[_MixedStream] = []
        col0 = h_off = tail_off = 0
        for st in streams:
            g = _MixedStream(st, self.fs_out, col0, h_off, tail_off, self.half_width, self.beta)
            self.streams.append(g)
            col0, h_off, tail_off = col0 + g.ncols, h_off + len(g.taps), tail_off + g.tail_rows * g.ncols
        self.stream: Dict[str, _MixedStream] = {g.name: g for g in self.streams}
        self.names, self.C_all, self.tail_doubles = cols, col0, max(tail_off, 1)
        self.taps = np.ascontiguousarray(np.concatenate([g.taps for g in self.streams] + [np.zeros(1)]))      # never empty
        self.device = torch.device(device)
        self.h = torch.from_numpy(self.taps).to(self.device)
        lat = [g.latency for g in self.streams]
        self.latency_s = max(g.latency_s for g in self.streams)
        self.latency_spread_rows = int(math.ceil((max(lat) - min(lat)) * Fraction(self.fs_out)))
        self.spelling = f"mixed->{self.fs_out:g}:kaiser{self.beta:g}[" + ";".join(g.spelling for g in self.streams) + "]"

    def groups(self):
        """The msig_mx_group table, as msig_mx_lv_push takes it (a ctypes array: keep it alive over the call)."""
        return (L.MxGroup * len(self.streams))(*[g.group() for g in self.streams])

    def _per_stream(self, d, what: str) -> dict:
        if not isinstance(d, dict) or set(d) != set(self.stream):
            raise ValueError(f"{what} takes a dict with the streams {[g.name for g in self.streams]}, got {sorted(d) if isinstance(d, dict) else d!r}")
        return d

    def out_count(self, n_raw: Dict[str, int]) -> int:
        """The rows every stream has delivered: the minimum of the streams' output counts."""
        n_raw = self._per_stream(n_raw, "out_count")
        return min(g.out_count(n_raw[g.name]) for g in self.streams)

    def samples(self, g: _MixedStream, x, device=None):
        """A stream's chunk as a contiguous (n, ncols) float64 array of its kind (numpy, or a tensor on the GPU); a one-column stream
        may be 1-D."""
        device = self.h.device if device is None else device
        if isinstance(x, np.ndarray):
            x = np.ascontiguousarray(x, dtype=np.float64)
        elif not isinstance(x, torch.Tensor) or not x.is_cuda or x.device != device or x.dtype != torch.float64:
            raise ValueError(f"stream {g.name!r}: samples are a float64 array, numpy or a tensor on the GPU {device} (there is no CPU fallback)")
        if x.ndim == 1 and g.ncols == 1:
            x = x.reshape(-1, 1)
        if x.ndim != 2 or x.shape[1] != g.ncols:
            raise ValueError(f"stream {g.name!r}: samples are (n, {g.ncols}) — the columns {g.columns} — got {tuple(x.shape)}")
        return x if isinstance(x, np.ndarray) else x.contiguous()

    def apply(self, streams) -> torch.Tensor:
        """(n_out, C_all) of {name: (n_g,) | (n_g, ncols_g)}: n_out = min over the streams of out_count_g(n_g), stream g's columns
        the first n_out outputs of its own stream (msig_mx_resample, one call per stream)."""
        streams = self._per_stream(streams, "apply")
        if self.h.device.type != "cuda":
            raise ValueError("apply runs on the resampler's GPU (there is no CPU fallback); this resampler was built on " + str(self.h.device))
        xs = []
        for g in self.streams:
            x = self.samples(g, streams[g.name])
            xs.append(torch.from_numpy(x).to(self.h.device) if isinstance(x, np.ndarray) else x)
        n = min(g.out_count(x.shape[0]) for g, x in zip(self.streams, xs))
        y = torch.empty((n, self.C_all), dtype=torch.float64, device=self.h.device)
        stream = C.c_void_p(torch.cuda.current_stream(self.h.device).cuda_stream)
        for g, x in zip(self.streams, xs):
            grp = g.group()
            L.check(L.lib().msig_mx_resample(x.data_ptr(), x.shape[0], self.h.data_ptr(), C.byref(grp), y.data_ptr(), n, self.C_all, stream),
                    "msig_mx_resample")
        return y
