"""The one grammar of the causal running references (include/msig_rn.h, include/msig_rd.h; DESIGN.md sections 36 and 37), shared by the
monitors' --reference (monitor.running_reference: with an optional warm-up count W) and training's --norm-reference
(dataset.parse_reference: without one — W is a monitor flag).  Needs no GPU and imports nothing of the package but the limits.

    expanding[:W]      window n is normalised with windows 0..n
    trailing:K[:W]     with the last K, 1 <= K <= RN_MAX_K
    decayed:H[:W]      with every window so far, window n - k weighted 2^(-k / H): a half-life of H windows, 1 <= H <= RD_MAX_H
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from ._lib import RD_MAX_H, RN_MAX_K

RUNNING_KINDS = ("expanding", "trailing", "decayed")
RUNNING_WARMUP = 6          # windows a running reference flags `warmup` by default: head:6's count


class Running(tuple):
    """A parsed running reference.  As a tuple it is (K, W) — K the windows of a trailing reference, 0 for expanding and decayed (the
    size of msig_rn_state_bytes(K)'s state block), W the leading windows flagged `warmup`; `.kind` is one of RUNNING_KINDS, `.H` the
    half-life in windows of a decayed reference (0 otherwise) and `.decay` its lambda = exp2(-1 / H) (None otherwise)."""

    def __new__(cls, kind: str, K: int, W: int, H: int = 0):
        self = super().__new__(cls, (int(K), int(W)))
        self.kind, self.H = kind, int(H)
        self.decay = float(np.exp2(-1.0 / self.H)) if kind == "decayed" else None
        return self

    def __repr__(self) -> str:
        return f"Running({self.spelling!r}, W={self[1]})"

    @property
    def K(self) -> int:
        return self[0]

    @property
    def W(self) -> int:
        return self[1]

    @property
    def spelling(self) -> str:
        """The reference without its warm-up count: what --norm-reference takes."""
        return self.kind + ("" if self.kind == "expanding" else f":{self.K if self.kind == 'trailing' else self.H}")

    def counts(self, n: int) -> list:
        """Per window 0 .. n - 1 the number of windows its statistics were taken over, where that is an integer the host knows
        (expanding, trailing); under decayed it is the real c_n of the device's records and is read from them."""
        if self.kind == "decayed":
            raise ValueError("a decayed reference's window counts are the device's c_n: read them from the statistics records")
        return [k + 1 if self.kind == "expanding" else min(k + 1, self.K) for k in range(n)]


def parse_running(reference, warmup: bool = True) -> Optional[Running]:
    """The Running of a reference spelled "expanding[:W]", "trailing:K[:W]" or "decayed:H[:W]" (W >= 0, default RUNNING_WARMUP).
    None for anything whose first field is not one of the three kinds; ValueError for one that is spelled wrongly.
    warmup=False (training): a `:W` is refused too."""
    if not isinstance(reference, str) or reference.split(":")[0] not in RUNNING_KINDS:
        return None
    kind, *rest = reference.split(":")
    want = 0 if kind == "expanding" else 1
    ok = want <= len(rest) <= want + (1 if warmup else 0) and all(v.isascii() and v.isdigit() for v in rest)
    if ok:
        n = int(rest[0]) if want else 0
        W = int(rest[want]) if len(rest) > want else RUNNING_WARMUP
        if kind == "expanding":
            return Running(kind, 0, W)
        if kind == "trailing" and 1 <= n <= RN_MAX_K:
            return Running(kind, n, W)
        if kind == "decayed" and 1 <= n <= RD_MAX_H:
            return Running(kind, 0, W, H=n)
    raise ValueError(f"a running reference is {RUNNING_FORMS}" + ("" if warmup else " (without ':W': the warm-up count is a flag of the monitors)")
                     + f", got {reference!r}")


RUNNING_FORMS = "'expanding[:W]', 'trailing:K[:W]' with K in 1..%d, 'decayed:H[:W]' with H in 1..%d windows, and W >= 0" % (RN_MAX_K, RD_MAX_H)
