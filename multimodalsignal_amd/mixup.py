"""Mixup inside the training gather and the criterion (include/msig_st.h).

A training batch never passes through Python, so the blend of every window with its partner (row B-1-b of the same batch) happens in
the gather launch and the loss against both labels in the loss kernels.  `Mixup` is the value object that switches it on — for
`DeviceLoader(..., mixup=...)`, `multifold.LockstepTrainer`, `cfg["mixup"]` / `--mixup ALPHA` of the drivers, and for callers that
build their own batches (`Mixup.apply`).  It also owns the draw of lam ~ Beta(alpha, alpha): one per training batch and fold, a
stateless function of (seed, step, alpha).  Validation, test, calibration and `embed` never mix.

The draw.  base = the msig_dropout_key of (seed, step) on stream MSIG_ST_STREAM_ID = 4; word k (k = 1, 2, ...) of the stream is fmix32(base + k * 0x9E3779B9 mod 2^32);
a uniform u in (0, 1) takes two words: ((w1 >> 6) * 2^26 + (w2 >> 6) + 0.5) / 2^52; a standard normal is
sqrt(-2 ln u1) cos(2 pi u2); Gamma(a >= 1) is Marsaglia and Tsang's method (d = a - 1/3, c = 1 / sqrt(9 d), x normal,
v = (1 + c x)^3, accepted when v > 0 and ln u < x^2 / 2 + d - d v + d ln v, value d v), Gamma(a < 1) = Gamma(a + 1) u^(1/a);
lam = X / (X + Y) with X then Y ~ Gamma(alpha) drawn from the one stream.  All of it in fp64; the result is rounded to fp32 and a
value below 2^-126 is raised to 2^-126, so lam lies in (0, 1].
"""
from __future__ import annotations

import ctypes as C
import math

from . import _lib as L

_M = 0xFFFFFFFF
_TINY = 2.0 ** -126


def _fmix32(h: int) -> int:
    h ^= h >> 16; h = (h * 0x85EBCA6B) & _M
    h ^= h >> 13; h = (h * 0xC2B2AE35) & _M
    return h ^ (h >> 16)


class _Stream:
    __slots__ = ("base", "k")

    def __init__(self, base: int):
        self.base, self.k = int(base), 0

    def word(self) -> int:
        self.k += 1
        return _fmix32((self.base + self.k * 0x9E3779B9) & _M)

    def uniform(self) -> float:
        hi, lo = self.word() >> 6, self.word() >> 6
        return (hi * 67108864 + lo + 0.5) / 4503599627370496.0

    def normal(self) -> float:
        u1, u2 = self.uniform(), self.uniform()
        return math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * math.pi * u2)

    def gamma(self, a: float) -> float:
        if a < 1.0:
            g = self.gamma(a + 1.0)
            return g * self.uniform() ** (1.0 / a)
        d = a - 1.0 / 3.0
        c = 1.0 / math.sqrt(9.0 * d)
        while True:
            x = self.normal()
            v = 1.0 + c * x
            if v <= 0.0:
                continue
            v = v * v * v
            if math.log(self.uniform()) < 0.5 * x * x + d - d * v + d * math.log(v):
                return d * v


def beta_from_key(base: int, alpha: float) -> float:
    """lam ~ Beta(alpha, alpha) of the stream that starts at `base` (see the module docstring), as the fp32 value in (0, 1]."""
    s = _Stream(base)
    x = s.gamma(alpha)
    y = s.gamma(alpha)
    lam = x / (x + y) if x + y > 0.0 else 0.5
    lam = C.c_float(lam).value
    return lam if lam >= _TINY else _TINY


class Mixup:
    """mixup with lam ~ Beta(alpha, alpha), alpha > 0 and finite; immutable."""
    __slots__ = ("alpha",)

    def __init__(self, alpha):
        if isinstance(alpha, (str, bytes, bool)):
            raise ValueError(f"mixup: alpha must be a positive number, got {alpha!r}")
        try:
            a = float(alpha)
        except (TypeError, ValueError):
            raise ValueError(f"mixup: alpha must be a positive number, got {alpha!r}") from None
        if not (a > 0.0 and math.isfinite(a)):
            raise ValueError(f"mixup: alpha must be a positive finite number, got {alpha!r}")
        object.__setattr__(self, "alpha", a)

    def __setattr__(self, name, value):
        raise AttributeError("Mixup is immutable")

    def __eq__(self, other):
        return isinstance(other, Mixup) and self.alpha == other.alpha

    def __hash__(self):
        return hash(self.alpha)

    def __repr__(self):
        return f"Mixup({self.alpha!r})"

    @classmethod
    def coerce(cls, value):
        """None, a Mixup or a number -> None or a Mixup (what cfg["mixup"] may hold)."""
        if value is None or isinstance(value, cls):
            return value
        return cls(value)

    def lam(self, seed: int, step: int) -> float:
        """The lam of training batch `step` (counted from 1) of a loader seeded `seed`: a pure function of (seed, step, alpha)."""
        return beta_from_key(L.dropout_key(seed, step, L.ST_STREAM_ID), self.alpha)

    def lams(self, seed: int, steps):
        """lam(seed, step) for every step of `steps`, as a list (the keys come from one vectorised call)."""
        return [beta_from_key(int(k), self.alpha) for k in L.dropout_keys(seed, list(steps), L.ST_STREAM_ID)]

    def apply(self, x, y, seed: int, step: int, augment=None):
        """Mixes a (B, C, T) fp32 device batch as the training gather of (seed, step) would — one launch with the identity index —
        and returns (x_mixed, y, lam): row b is lam * x[b] + (1 - lam) * x[B-1-b]; `y` is returned as it is (the criterion reads the
        partner's label from y[B-1-b]: pass lam as mix_lambda).  augment: an augment.Augment applied to every row first."""
        import torch
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3):
            raise ValueError("Mixup.apply needs a (B, C, T) float32 GPU tensor")
        x = x.contiguous()
        B, Cn, T = (int(v) for v in x.shape)
        if T < 4 or T % 4:
            raise ValueError(f"mixup: the window length must be a multiple of 4, got {T}")
        lam = self.lam(seed, step)
        out = torch.empty_like(x)
        idx = torch.arange(B, dtype=torch.int64, device=x.device)
        a = None
        if augment is not None and not augment.off:
            augment.check_window(T)
            a = C.byref(augment.struct([L.dropout_key(seed, step, L.AUG_STREAM_ID)]))
        st = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
        L.check(L.lib().msig_st_gather_windows(x.data_ptr(), None, idx.data_ptr(), B, Cn, T, out.data_ptr(), None, a,
                                               (C.c_float * 1)(lam), st), "msig_st_gather_windows")
        return out, y, lam
