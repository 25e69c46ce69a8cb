"""Supervised contrastive loss on the classifier's feature (include/msig_sc.h): the host side.

A ``SupCon`` is the term of ONE model: its weight, temperature and which rows count as positives — every window of the anchor's
class, or (``cross-subject``) only those of its class from another person —, the int32 table that maps a store position to the
subject of the window there, the scratch its two launches pass their row statistics through, and the epoch's statistics.  The term
has no parameters and no state that outlives a step.  The arithmetic is the library's: ``runtime.Engine.train_step(..., supcon=)``
and ``multifold.LockstepTrainer`` hand these buffers to ``msig_sc_train_step[_multi]``, which adds the term's gradient to the
feature gradient between the head's launch and the GRU backward.  What a step reports stays the criterion's.
"""
from __future__ import annotations

import json
import math
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from . import _lib as L

POSITIVES = tuple(L.SC_POSITIVES)
STATS = L.SC_STATS
DEFAULT_WEIGHT, DEFAULT_TAU = 0.1, 0.1
TAU_RANGE = (1e-3, 1e3)


def check_batch_size(batch_size: int) -> None:
    """The term's launches take at most MSIG_SC_MAX_BATCH rows: larger training batches are refused before training."""
    if int(batch_size) > L.SC_MAX_BATCH:
        raise ValueError(f"supcon takes training batches of at most {L.SC_MAX_BATCH} windows, got batch size {batch_size}")


def _number(v, what, lo, hi=None):
    if isinstance(v, (str, bytes, bool)) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < lo or (hi is not None and v > hi):
        raise ValueError(f"supcon {what} must be a finite number in [{lo:g}, {'inf' if hi is None else format(hi, 'g')}], got {v!r}")
    return float(v)


def settings(value) -> Optional[dict]:
    """config['trainer']['supcon']: None (off), a number (the weight) or a dict with any of weight / tau / positives — checked,
    defaults filled in."""
    if value is None:
        return None
    if isinstance(value, dict):
        unknown = set(value) - {"weight", "tau", "positives"}
        if unknown:
            raise ValueError(f"supcon has unknown keys {sorted(unknown)}")
        out = dict(weight=DEFAULT_WEIGHT, tau=DEFAULT_TAU, positives="class")
        out.update(value)
    else:
        out = dict(weight=value, tau=DEFAULT_TAU, positives="class")
    out["weight"] = _number(out["weight"], "weight", 0.0)
    out["tau"] = _number(out["tau"], "tau", *TAU_RANGE)
    if out["positives"] not in POSITIVES:
        raise ValueError(f"supcon positives must be one of {POSITIVES}, got {out['positives']!r}")
    return out


def parse(spec, positives=None) -> dict:
    """--supcon [WEIGHT[:TAU]] --supcon-positives P as a setting (ValueError for a bad value).  spec None or "": the defaults."""
    weight, tau = DEFAULT_WEIGHT, DEFAULT_TAU
    if spec not in (None, ""):
        parts = str(spec).split(":")
        if len(parts) > 2:
            raise ValueError(f"supcon takes WEIGHT or WEIGHT:TAU, got {spec!r}")
        try:
            weight = float(parts[0])
            if len(parts) == 2:
                tau = float(parts[1])
        except ValueError:
            raise ValueError(f"supcon takes WEIGHT or WEIGHT:TAU, got {spec!r}") from None
    return settings(dict(weight=weight, tau=tau, positives=positives or "class"))


def settings_line(cfg) -> str:
    c = settings(cfg)
    return f"SUPCON: weight={c['weight']:g} tau={c['tau']:g} positives={c['positives']}"


def subject_table(dataset) -> np.ndarray:
    """The int32 store-position -> subject table of a fold whose TRAINING set is `dataset` (dro.group_table(dataset, "subject", K)
    without the limit on the number of groups: the term compares subjects, it keeps nothing per subject)."""
    ordinals = np.asarray(dataset.subject_ordinals, dtype=np.int32)
    index = getattr(dataset, "index_host", None)
    if index is None:
        return ordinals.copy()
    table = np.full(int(dataset.store.x.shape[0]), -1, dtype=np.int32)
    table[index] = ordinals
    return table


class SupCon:
    def __init__(self, weight: float = DEFAULT_WEIGHT, tau: float = DEFAULT_TAU, positives: str = "class"):
        cfg = settings(dict(weight=weight, tau=tau, positives=positives))
        self.weight, self.tau, self.positives = cfg["weight"], cfg["tau"], cfg["positives"]
        self.grp: Optional[torch.Tensor] = None               # int32 store-position -> subject (cross-subject mode)
        self.scratch: Optional[torch.Tensor] = None
        self.stats = torch.zeros(STATS, dtype=torch.float64)
        self.max_batch = 0

    @property
    def cross_subject(self) -> bool:
        return self.positives == "cross-subject"

    def set_subjects(self, table) -> "SupCon":
        """The fold's subject table (subject_table), before bind(); needed in cross-subject mode only."""
        self.grp = torch.as_tensor(np.asarray(table, dtype=np.int32))
        return self

    def bind(self, device, storage: Optional[dict] = None, max_batch: int = L.SC_MAX_BATCH) -> "SupCon":
        """Moves the buffers to `device` with a scratch for batches of up to `max_batch` rows, or with `storage`
        (runtime.FoldArena.side_storage("supcon", slot)) into one fold's regions of an arena: int32 "grp", uint8 "scratch", float64 "stats"."""
        if self.cross_subject and self.grp is None:
            raise RuntimeError("cross-subject positives need a subject table: call set_subjects first")
        if storage is None:
            if not 1 <= int(max_batch) <= L.SC_MAX_BATCH:
                raise ValueError(f"supcon takes batches of 1..{L.SC_MAX_BATCH} windows, got {max_batch}")
            self.grp = None if self.grp is None else self.grp.to(device)
            self.stats = self.stats.to(device)
            self.scratch = torch.empty(int(L.lib().msig_sc_scratch_bytes(int(max_batch))), dtype=torch.uint8, device=device)
            self.max_batch = int(max_batch)
            return self
        if self.grp is not None:
            if storage["grp"].numel() < self.grp.numel():
                raise ValueError("the arena's subject table is smaller than the fold's")
            storage["grp"].fill_(-1)
            storage["grp"][:self.grp.numel()].copy_(self.grp)
        storage["stats"].copy_(self.stats)
        self.grp, self.scratch, self.stats = storage["grp"], storage["scratch"], storage["stats"]
        self.max_batch = min(L.SC_MAX_BATCH, self.scratch.numel() // int(L.lib().msig_sc_scratch_bytes(L.SC_MAX_BATCH) // L.SC_MAX_BATCH))
        return self

    def descriptor(self, idx: Optional[int] = None, idx_row_stride: int = 0, stride_bytes: int = 0, stats: bool = True,
                   weights=None) -> L.Sc:
        """msig_sc over this term's buffers (a fold batch: arena 0's, `stride_bytes` apart, one weight per fold)."""
        if self.scratch is None or not self.scratch.is_cuda:
            raise RuntimeError("the supcon term is not bound to a device: bind first")
        d = L.Sc()
        d.positives, d.tau = L.SC_POSITIVES[self.positives], self.tau
        d.grp = self.grp.data_ptr() if self.cross_subject else None
        d.idx, d.idx_row_stride = (idx if self.cross_subject else None), int(idx_row_stride)
        d.scratch, d.stats, d.stride_bytes = self.scratch.data_ptr(), self.stats.data_ptr() if stats else None, int(stride_bytes)
        for i, w in enumerate([self.weight] if weights is None else weights):
            d.weight[i] = float(w)
        return d

    @staticmethod
    def epoch_summary(stats) -> dict:
        """History entries of an epoch from its statistics: the mean loss over anchors, the share of anchors whose nearest row in
        A(i) is a positive, and the mean number of anchors per step (None where nothing was counted)."""
        s = np.asarray(stats, dtype=np.float64)
        return dict(supcon_loss=float(s[0] / s[1]) if s[1] > 0 else None, supcon_top1=float(s[2] / s[1]) if s[1] > 0 else None,
                    supcon_anchors=float(s[1] / s[3]) if s[3] > 0 else None)


def fold_info(sc: SupCon) -> dict:
    """What a fold trained with the term adds to its result (multifold.fold_result): the setting."""
    return dict(weight=sc.weight, tau=sc.tau, positives=sc.positives)


def fold_record(info: dict) -> Optional[dict]:
    """The record of one trained fold from its fold_result: the last epoch's three numbers beside the fold's test accuracy; None for a
    fold trained without the term."""
    hist = [h for h in info.get("history", []) if "supcon_loss" in h]
    s = info.get("supcon")
    if s is None or not hist:
        return None
    last = hist[-1]
    return dict(subject=info["subject"], weight=s["weight"], tau=s["tau"], positives=s["positives"], supcon_loss=last["supcon_loss"],
                supcon_top1=last["supcon_top1"], supcon_anchors=last["supcon_anchors"], train_loss=last.get("train_loss"),
                epochs=len(hist), test_accuracy=info.get("accuracy"))


def write_supcon(out_dir, folds, cfg: dict, synthetic: bool = False, stem: str = "supcon"):
    """supcon.txt / supcon.json of a run: per fold the last epoch's contrastive loss, top-1 share and anchors per step beside the
    test accuracy, and their means over the folds.  stem: the files' name (the hierarchical run writes one pair per model)."""
    out_dir = Path(out_dir)
    cfg = settings(cfg)
    mean = lambda key: (lambda v: float(np.mean(v)) if v else None)([f[key] for f in folds if f.get(key) is not None])
    pooled = {k: mean(k) for k in ("supcon_loss", "supcon_top1", "supcon_anchors", "test_accuracy")}
    doc = dict(settings=cfg, probe=cfg["weight"] == 0.0, synthetic=bool(synthetic), folds=folds, pooled=pooled)
    (out_dir / f"{stem}.json").write_text(json.dumps(doc, indent=1))
    lines = [settings_line(cfg) + (" (probe: the loss is measured, the model trains as without it)" if cfg["weight"] == 0.0 else "")]
    if synthetic:
        lines.append("NOTE: the synthetic set draws every subject from one distribution: there is no subject shift for the term to "
                     "remove, so these numbers say nothing about WESAD accuracy.")
    fmt = lambda v: "     n/a" if v is None else f"{v:8.4f}"
    lines.append("")
    lines.append(f"{'fold':10s} {'loss':>8s} {'top-1':>8s} {'anchors':>8s} {'test acc':>8s}")
    for f in folds:
        lines.append(f"{str(f['subject']):10s} {fmt(f['supcon_loss'])} {fmt(f['supcon_top1'])} {fmt(f['supcon_anchors'])} {fmt(f['test_accuracy'])}")
    lines.append(f"{'mean':10s} {fmt(pooled['supcon_loss'])} {fmt(pooled['supcon_top1'])} {fmt(pooled['supcon_anchors'])} {fmt(pooled['test_accuracy'])}")
    path = out_dir / f"{stem}.txt"
    path.write_text("\n".join(lines) + "\n", encoding="utf-8")
    return path
