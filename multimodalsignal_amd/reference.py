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


# ---- missing samples (include/msig_gp.h) ---------------------------------------------------------------------
class Gaps:
    """The policy of a gap-tolerant monitor, `Monitor(..., gaps=Gaps(...))`: a window is VALID when the smallest coverage (share of
    valid samples) over its selected channels is >= `min_coverage` (0 never invalidates); a run of `lost_after` invalid windows means
    the wearer is LOST: the state is forced off and the smoother restarts at the next valid window.  Both are policy, not measurements."""

    def __init__(self, min_coverage: float = 0.75, lost_after: int = 6):
        if isinstance(min_coverage, bool) or not isinstance(min_coverage, (int, float)) or not 0.0 <= float(min_coverage) <= 1.0:
            raise ValueError(f"min_coverage must be a number in [0, 1], got {min_coverage!r}")
        if isinstance(lost_after, bool) or not isinstance(lost_after, (int, np.integer)) or int(lost_after) < 1:
            raise ValueError(f"lost_after must be an integer >= 1 windows, got {lost_after!r}")
        self.min_coverage, self.lost_after = float(min_coverage), int(lost_after)

    def __repr__(self) -> str:
        return f"Gaps(min_coverage={self.min_coverage!r}, lost_after={self.lost_after!r})"

    def __eq__(self, other) -> bool:
        return isinstance(other, Gaps) and (self.min_coverage, self.lost_after) == (other.min_coverage, other.lost_after)

    def __hash__(self) -> int:
        return hash((self.min_coverage, self.lost_after))

    @property
    def spelling(self) -> str:
        """What --gaps takes."""
        return f"{self.min_coverage!r}:{self.lost_after}"

    def valid(self, coverage) -> np.ndarray:
        """(N,) bool from the (N, C) coverage of the selected channels."""
        return np.asarray(coverage, dtype=np.float64).min(axis=1) >= self.min_coverage


GAPS_FORMS = "MIN_COVERAGE[:LOST_AFTER] with MIN_COVERAGE in [0, 1] and LOST_AFTER >= 1 windows, or nothing (0.75:6)"


def parse_gaps(text) -> Gaps:
    """--gaps [MIN_COVERAGE[:LOST_AFTER]]: "" or None is Gaps(); ValueError for anything spelled wrongly."""
    if text is None or text == "":
        return Gaps()
    parts = str(text).split(":")
    try:
        if len(parts) > 2 or (len(parts) == 2 and not (parts[1].isascii() and parts[1].isdigit())):
            raise ValueError
        cov = float(parts[0])
        if not np.isfinite(cov):
            raise ValueError
        return Gaps(cov, int(parts[1])) if len(parts) == 2 else Gaps(cov)
    except ValueError:
        raise ValueError(f"--gaps takes {GAPS_FORMS}, got {text!r}") from None


GAPS_REFERENCES = ("gaps need a running reference ('expanding', 'trailing:K', 'decayed:H') or a statistics tensor: the statistics of "
                   "'recording', 'head:K' and a window range weight samples and have no per-channel count of valid ones")


def gp_mode_fields(running: Optional[Running]):
    """(kind, K, decay) of msig_gp_mode for a Running; a statistics tensor's rows need none (expanding serves for the coverage)."""
    if running is None or running.kind == "expanding":
        return 0, 0, 0.0
    return (1, running.K, 0.0) if running.kind == "trailing" else (2, 0, running.decay)
