"""Window augmentation inside the training gather (include/msig_aug.h).

A training batch never passes through Python: `DeviceLoader` builds it with one gather launch and a fold batch's gather writes
straight into the arenas the next launch trains on.  `Augment` is the value object that switches the augmenting gather on — per
channel magnitude scaling, additive jitter, a time mask and channel dropout, drawn statelessly from (seed, step, row, channel,
sample) — for `DeviceLoader(..., augment=...)`, `multifold.LockstepTrainer`, `cfg["augment"]` / `--augment SPEC` of the drivers, and
for callers that build their own batches (`Augment.apply`).  Validation, test, calibration and `embed` never augment.
"""
from __future__ import annotations

import ctypes as C

from . import _lib as L


def _number(name, value) -> float:
    if isinstance(value, (str, bytes, bool)):
        raise ValueError(f"augment: {name} must be a number, got {value!r}")
    try:
        return float(value)
    except (TypeError, ValueError):
        raise ValueError(f"augment: {name} must be a number, got {value!r}") from None


class Augment:
    """The parameters of the augmenting gather, checked by the rules of the C calls (msig_aug.h); immutable.

    scale      sigma of the per-(window, channel) gain 1 + scale * g           >= 0, 0 = off
    jitter     sigma of the per-sample additive noise jitter * g              >= 0, 0 = off
    mask_prob  probability per window of one zeroed span in all channels      in [0, 1], 0 = off
    mask_max   longest span in samples (its length is uniform in 1..mask_max) 1..T when mask_prob > 0
    chan_drop  probability per (window, channel) of a zeroed channel           in [0, 1), 0 = off
    """
    __slots__ = ("scale", "jitter", "mask_prob", "mask_max", "chan_drop")

    def __init__(self, scale=0.0, jitter=0.0, mask_prob=0.0, mask_max=0, chan_drop=0.0):
        scale, jitter = _number("scale", scale), _number("jitter", jitter)
        mask_prob, chan_drop = _number("mask_prob", mask_prob), _number("chan_drop", chan_drop)
        if isinstance(mask_max, bool) or not isinstance(mask_max, int):
            raise ValueError(f"augment: mask_max must be an integer, got {mask_max!r}")
        if not scale >= 0.0 or not jitter >= 0.0:                      # negative or NaN
            raise ValueError(f"augment: scale and jitter must be >= 0, got {scale!r}, {jitter!r}")
        if not 0.0 <= mask_prob <= 1.0:
            raise ValueError(f"augment: mask_prob must be in [0, 1], got {mask_prob!r}")
        if not 0.0 <= chan_drop < 1.0 or C.c_float(chan_drop).value >= 1.0:          # the C calls see the fp32 value
            raise ValueError(f"augment: chan_drop must be in [0, 1), got {chan_drop!r}")
        if mask_prob > 0.0 and mask_max < 1:
            raise ValueError(f"augment: mask_prob > 0 needs mask_max >= 1 (and <= the window length), got {mask_max!r}")
        for name, v in (("scale", scale), ("jitter", jitter), ("mask_prob", mask_prob), ("mask_max", int(mask_max)), ("chan_drop", chan_drop)):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("Augment is immutable")

    def _tuple(self):
        return (self.scale, self.jitter, self.mask_prob, self.mask_max if self.mask_prob > 0.0 else 0, self.chan_drop)

    def __eq__(self, other):
        return isinstance(other, Augment) and self._tuple() == other._tuple()

    def __hash__(self):
        return hash(self._tuple())

    def __repr__(self):
        return f"Augment({self.spec()!r})"

    @property
    def off(self) -> bool:
        """All four transforms at 0: the augmenting gather is then the plain gather, bit for bit."""
        return self.scale == 0.0 and self.jitter == 0.0 and self.mask_prob == 0.0 and self.chan_drop == 0.0

    def spec(self) -> str:
        """The `parse` form of these parameters (transforms that are off are left out; "none" when all are)."""
        parts = []
        if self.scale:
            parts.append(f"scale={self.scale!r}")
        if self.jitter:
            parts.append(f"jitter={self.jitter!r}")
        if self.mask_prob:
            parts.append(f"mask={self.mask_prob!r}:{self.mask_max}")
        if self.chan_drop:
            parts.append(f"chandrop={self.chan_drop!r}")
        return ",".join(parts) or "none"

    @classmethod
    def parse(cls, spec: str) -> "Augment":
        """"scale=0.1,jitter=0.05,mask=0.5:320,chandrop=0.1": any subset, in any order; mask is PROB:MAX_SAMPLES; "none" = all off."""
        if not isinstance(spec, str):
            raise ValueError(f"augment: the specification must be a string, got {spec!r}")
        kw = {}
        if spec.strip() in ("", "none"):
            return cls()
        for item in spec.split(","):
            name, eq, val = item.strip().partition("=")
            if not eq or name not in ("scale", "jitter", "mask", "chandrop") or name in kw or (name == "mask" and "mask_prob" in kw):
                raise ValueError(f"augment: expected scale=S,jitter=S,mask=P:N,chandrop=P (each at most once), got {item!r} in {spec!r}")
            try:
                if name == "mask":
                    prob, colon, n = val.partition(":")
                    if not colon:
                        raise ValueError("mask takes PROB:MAX_SAMPLES")
                    kw["mask_prob"], kw["mask_max"] = float(prob), int(n)
                else:
                    kw["chan_drop" if name == "chandrop" else name] = float(val)
            except ValueError as e:
                raise ValueError(f"augment: cannot read {item!r} in {spec!r}: {e}") from None
        return cls(**kw)

    @classmethod
    def coerce(cls, value):
        """None, an Augment or a `parse` string -> None or an Augment (what cfg["augment"] may hold)."""
        if value is None or isinstance(value, cls):
            return value
        return cls.parse(value)

    def check_window(self, T: int):
        """The checks that need the window length: raises ValueError by the C calls' rules."""
        if T < 4 or T % 4:
            raise ValueError(f"augment: the window length must be a multiple of 4, got {T}")
        if self.mask_prob > 0.0 and self.mask_max > T:
            raise ValueError(f"augment: mask_max {self.mask_max} exceeds the window length {T}")

    def struct(self, keys=()) -> "L.Aug":
        """msig_aug with these parameters and the given per-fold keys."""
        a = L.Aug(self.scale, self.jitter, self.mask_prob, self.chan_drop, self.mask_max if self.mask_prob > 0.0 else 0, 0)
        for i, k in enumerate(keys):
            a.key[i] = int(k)
        return a

    def apply(self, x, seed: int, step: int):
        """Augments a (B, C, T) fp32 device tensor as the training gather of (seed, step) would — one launch with the identity index —
        and returns a new tensor; `x` is left as it is."""
        import torch
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3):
            raise ValueError("Augment.apply needs a (B, C, T) float32 GPU tensor")
        x = x.contiguous()
        B, Cn, T = (int(v) for v in x.shape)
        self.check_window(T)
        out = torch.empty_like(x)
        idx = torch.arange(B, dtype=torch.int64, device=x.device)
        a = self.struct([L.dropout_key(seed, step, L.AUG_STREAM_ID)])
        st = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
        L.check(L.lib().msig_aug_gather_windows(x.data_ptr(), None, idx.data_ptr(), B, Cn, T, out.data_ptr(), None, C.byref(a), st),
                "msig_aug_gather_windows")
        return out
