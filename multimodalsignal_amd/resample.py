"""Causal polyphase FIR resampling by a rational ratio (include/msig_rs.h).

A wearable does not deliver the models' rate: WESAD's chest device samples at 700 Hz, the models take 64 Hz.  `FirResampler` is the
resampler that can run live: the filter and the convention of scipy.signal.resample_poly — a Kaiser-windowed sinc of
2 * half + 1 taps, zero phase — with an output emitted only once its whole support has arrived, so the outputs are a causal function
of the stream with a fixed latency.  `apply` resamples a whole recording (msig_rs_resample); `LiveMonitor(resampler=...)` pushes
raw-rate chunks through the same device function into its rings (msig_rs_lv_push): the same bits, whatever the chunking.

The ratio L / M = fs_out / fs_in in lowest terms, half = half_width * max(L, M),
h = firwin(2 * half + 1, 1 / max(L, M), window=("kaiser", beta)) * L, restated in numpy (`fir_taps`); 700 -> 64 Hz gives L = 16,
M = 175, 3501 taps, 219 of them per output.  `fir_taps`, `ratio` and `out_count` need no GPU.  `apply` has no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from fractions import Fraction
from typing import Tuple

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
