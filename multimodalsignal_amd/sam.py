"""Sharpness-aware minimisation (include/msig_sam.h): the host side of a SAM / ASAM train step.

A ``Sam`` is the setting of one run — rho, SAM or ASAM, and ASAM's eta.  The arithmetic is the library's:
``runtime.Engine.train_step(..., sam=)`` hands it to the one train-step call (``msig_sc_train_step``) as its ``msig_sam`` with the engine's SAM
state, a fold batch to its ``_multi`` form (``runtime.FoldArena(..., sam=True)`` owns every fold's state as one more arena region).  Nothing here
is part of a model's ``state_dict``.
"""
from __future__ import annotations

import ctypes as C
import math

from . import _lib as L

DEFAULT_ETA = 0.01            # Kwon et al. 2021


def _number(name: str, value, what: str) -> float:
    if isinstance(value, (str, bytes, bool)):
        raise ValueError(f"SAM's {name} must be {what}, got {value!r}")
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"SAM's {name} must be {what}, got {value!r}") from None
    if math.isnan(v) or math.isinf(v) or v < 0.0:
        raise ValueError(f"SAM's {name} must be {what}, got {value!r}")
    return C.c_float(v).value          # the fp32 value the calls will see


class Sam:
    def __init__(self, rho, adaptive: bool = False, eta=DEFAULT_ETA):
        """rho >= 0 (0 = off: the step without SAM, bit for bit); adaptive: ASAM, whose T_w = |w| + eta with eta >= 0."""
        self.rho = _number("rho", rho, "a finite number >= 0")
        if not isinstance(adaptive, (bool, int)) or adaptive not in (0, 1, False, True):
            raise ValueError(f"SAM's adaptive must be True or False, got {adaptive!r}")
        self.adaptive = bool(adaptive)
        self.eta = _number("eta", eta, "a finite number >= 0")

    @classmethod
    def parse(cls, text) -> "Sam":
        """"RHO[:adaptive[:ETA]]" — the value of --sam and of config['trainer']['sam']; a Sam passes through."""
        if isinstance(text, cls):
            return text
        if isinstance(text, (int, float)) and not isinstance(text, bool):
            return cls(text)
        if not isinstance(text, str) or not text:
            raise ValueError(f"--sam takes RHO[:adaptive[:ETA]], got {text!r}")
        parts = text.split(":")
        if len(parts) > 3 or (len(parts) >= 2 and parts[1] != "adaptive"):
            raise ValueError(f"--sam takes RHO[:adaptive[:ETA]], got {text!r}")
        try:
            rho = float(parts[0])
            eta = float(parts[2]) if len(parts) == 3 else DEFAULT_ETA
        except ValueError:
            raise ValueError(f"--sam takes RHO[:adaptive[:ETA]] with numbers for RHO and ETA, got {text!r}") from None
        return cls(rho, len(parts) >= 2, eta)

    def spec(self) -> str:
        if not self.adaptive:
            return f"{self.rho:g}"
        return f"{self.rho:g}:adaptive:{self.eta:g}"

    @property
    def on(self) -> bool:
        return self.rho != 0.0

    def __repr__(self):
        return f"Sam(rho={self.rho:g}, adaptive={self.adaptive}, eta={self.eta:g})"

    def __eq__(self, other):
        return isinstance(other, Sam) and (self.rho, self.adaptive, self.eta) == (other.rho, other.adaptive, other.eta)

    def __hash__(self):
        return hash((self.rho, self.adaptive, self.eta))

    def descriptor(self, kind: str, state_ptr: int, state_bytes: int) -> L.Sam:
        """msig_sam of a launch on models of `kind` whose state (fold slot 0's in a fold batch) is at `state_ptr`."""
        s = L.Sam()
        s.kind, s.adaptive, s.rho, s.eta = L.GC_KINDS[L.check_kind(kind)], int(self.adaptive), self.rho, self.eta
        s.state, s.state_bytes = state_ptr, int(state_bytes)
        return s


def setting(value):
    """config['trainer']['sam']: None (off) or RHO[:adaptive[:ETA]] / a number / a Sam (ValueError otherwise).  A rho of 0 is kept: it
    runs the SAM call, which is then the plain step."""
    return None if value is None else Sam.parse(value)


def summary(stats, steps: int) -> dict:
    """The history entries of an epoch from a SAM state's statistics (a sequence of L.SAM_NSTAT numbers) over `steps` steps."""
    n = max(int(steps), 1)
    return dict(sam_grad_norm=stats[L.SAM_NORM_SUM] / n, sam_grad_norm_max=stats[L.SAM_NORM_MAX], sam_sharpness=stats[L.SAM_SHARP_SUM] / n)
