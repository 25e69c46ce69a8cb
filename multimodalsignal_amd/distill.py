"""Knowledge distillation (include/msig_kd.h): the host side of the distillation term.

A ``Distillation`` is the setting of ONE student — the weight alpha of the teacher's term and the temperature T — together with
what the term reads and writes on the device: the fp32 teacher table (K tempered probabilities per store position, built by
``ensemble.Ensemble.teacher`` or ``teacher_table``) and three float64 statistics.  The arithmetic is the library's:
``runtime.Engine.train_step(..., distill=)`` hands these buffers to the one train-step call (``msig_sc_train_step``) as its
``msig_kd``, a fold batch to its ``_multi`` form (``runtime.FoldArena(..., distill=positions)`` owns the tables in a side block).  Nothing here is part
of a model's ``state_dict``.
"""
from __future__ import annotations

import ctypes as C
import json
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from . import _lib as L

DEFAULT_ALPHA, DEFAULT_T = 0.5, 2.0
STATS = 3                     # msig_kd.stats: [sum of B * L_kd, rows whose argmax is the teacher's, rows]
STUDENT_SUFFIX = "/distilled"


class Distillation:
    def __init__(self, alpha: float = DEFAULT_ALPHA, temperature: float = DEFAULT_T):
        self.alpha, self.temperature = L.check_distill(alpha, temperature)
        self.q: Optional[torch.Tensor] = None                 # (positions, K) float32 teacher table (set_teacher)
        self.stats = torch.zeros(STATS, dtype=torch.float64)

    @classmethod
    def parse(cls, text) -> "Distillation":
        """"ALPHA[:T]" — the value of --distill; None or "" = 0.5:2, the default T is 2."""
        if text is None or text == "" or text is True:
            return cls()
        if isinstance(text, cls):
            return text
        parts = str(text).split(":")
        if len(parts) > 2:
            raise ValueError(f"--distill takes ALPHA[:T], got {text!r}")
        try:
            alpha = float(parts[0])
            temperature = float(parts[1]) if len(parts) == 2 else DEFAULT_T
        except ValueError:
            raise ValueError(f"--distill takes ALPHA[:T] with two numbers, got {text!r}") from None
        return cls(alpha, temperature)

    def spec(self) -> str:
        return f"{self.alpha:g}:{self.temperature:g}"

    def __repr__(self):
        return f"Distillation(alpha={self.alpha:g}, temperature={self.temperature:g})"

    # ---- buffers -----------------------------------------------------------------------------------------------------------------
    def set_teacher(self, table) -> None:
        """The (positions, K) teacher table: rows of probabilities, float32 (teacher_table / Ensemble.teacher), before bind()."""
        t = torch.as_tensor(table)
        if t.dim() != 2 or t.dtype != torch.float32 or not 2 <= t.shape[1] <= L.MAX_K:
            raise ValueError(f"a teacher table is a float32 (positions, K) array with 2 <= K <= {L.MAX_K}, got {t.dtype} {tuple(t.shape)}")
        self.q = t.contiguous()

    def bind(self, device, storage: Optional[dict] = None) -> "Distillation":
        """Moves the buffers to `device`, or with `storage` (runtime.FoldArena.side_storage("distill", slot)) into one fold's regions of an arena:
        float32 "q" (positions * K), float64 "stats"."""
        if storage is None:
            self.stats = self.stats.to(device)
            if self.q is not None:
                self.q = self.q.to(device)
            return self
        storage["stats"].copy_(self.stats)
        self.stats = storage["stats"]
        if self.q is not None:
            if storage["q"].numel() < self.q.numel():
                raise ValueError("the arena's teacher table is shorter than the fold's")
            dst = storage["q"][:self.q.numel()].view(self.q.shape)
            dst.copy_(self.q)
            self.q = dst
        return self

    def descriptor(self, idx: Optional[int] = None, idx_row_stride: int = 0, stride_bytes: int = 0) -> L.Kd:
        """msig_kd over this student's buffers (a fold batch: arena 0's, `stride_bytes` apart)."""
        if self.q is None:
            raise RuntimeError("the distillation has no teacher table: call set_teacher first")
        k = L.Kd()
        k.alpha, k.temperature = self.alpha, self.temperature
        k.q, k.idx, k.idx_row_stride = self.q.data_ptr(), idx, int(idx_row_stride)
        k.stats, k.stride_bytes = self.stats.data_ptr(), int(stride_bytes)
        return k

    @staticmethod
    def epoch_summary(stats) -> dict:
        """History entries of an epoch from its statistics (three numbers): the mean L_kd and the share of training rows whose
        argmax is the teacher's; None for both when no row was distilled (alpha = 0: the term is never launched)."""
        s0, s1, s2 = (float(v) for v in stats)
        return dict(kd_loss=s0 / s2 if s2 > 0 else None, kd_agreement=s1 / s2 if s2 > 0 else None)


def student_name(fold_name: str) -> str:
    """Configuration name of the student of the fold whose replica 0 is `fold_name` (ensemble.replica_name(n, 0))."""
    return fold_name + STUDENT_SUFFIX


def teacher_table(logits: torch.Tensor, temperature: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(N, K) float32 teacher rows of an (M, N, K) float32 device stack of members' logits (msig_kd_teacher): the mean over the
    members of softmax(logits / T), in fp64, summed in member order and rounded once.  At T = 1 the bits are msig_en_reduce's mean_p."""
    if logits.dim() != 3 or logits.dtype != torch.float32 or not logits.is_cuda:
        raise ValueError(f"teacher_table takes a float32 (M, N, K) device tensor, got {logits.dtype} {tuple(logits.shape)} on {logits.device}")
    _, temperature = L.check_distill(0.0, temperature)
    logits = logits.contiguous()
    M, N, K = logits.shape
    if out is None:
        out = torch.empty((N, K), dtype=torch.float32, device=logits.device)
    st = C.c_void_p(torch.cuda.current_stream(logits.device).cuda_stream)
    L.check(L.lib().msig_kd_teacher(logits.data_ptr(), N * K, M, N, K, temperature, out.data_ptr(), st), "msig_kd_teacher")
    return out


# ---- the report of a run -------------------------------------------------------------------------------------------------------------
SYSTEMS = ("ensemble", "mean_member", "replica0", "student")
METRICS = ("accuracy", "f1", "nll", "brier", "ece")


def fidelity(pred, ensemble_pred) -> float:
    """The share of windows predicted as the ensemble predicts them."""
    pred, ensemble_pred = np.asarray(pred), np.asarray(ensemble_pred)
    if pred.shape != ensemble_pred.shape or pred.size == 0:
        raise ValueError(f"fidelity takes two equally long, non-empty prediction vectors, got {pred.shape} and {ensemble_pred.shape}")
    return float(np.mean(pred == ensemble_pred))


def paired(student, replica0) -> dict:
    """student - replica 0 over paired folds: the mean difference and the wins / ties / losses of the student (higher = win)."""
    s, r = np.asarray(student, dtype=np.float64), np.asarray(replica0, dtype=np.float64)
    if s.shape != r.shape or s.size == 0:
        raise ValueError(f"paired takes two equally long, non-empty vectors, got {s.shape} and {r.shape}")
    d = s - r
    return dict(mean_difference=float(d.mean()), wins=int((d > 0).sum()), ties=int((d == 0).sum()), losses=int((d < 0).sum()))


def format_table(doc: dict) -> str:
    """distillation.txt from the document of write_distillation."""
    lines = [f"DISTILLATION: alpha={doc['alpha']:g} T={doc['temperature']:g} members={doc['members']}"]
    if doc.get("synthetic"):
        lines.append("NOTE: the synthetic set shows the machinery, not what WESAD would give: these numbers say nothing about "
                     "WESAD accuracy.")
    head = f"{'fold':8s} {'system':12s} " + " ".join(f"{m:>9s}" for m in METRICS) + f" {'fidelity':>9s}"
    for block in list(doc["folds"]) + ([dict(subject="pooled", **doc["pooled"])] if doc.get("pooled") else []):
        lines += ["", head]
        for name in SYSTEMS:
            row = block.get(name)
            if row is None:
                continue
            cells = " ".join("      n/a" if row.get(m) is None else f"{row[m]:9.4f}" for m in METRICS)
            fid = "      n/a" if row.get("fidelity") is None else f"{row['fidelity']:9.4f}"
            lines.append(f"{block['subject']:8s} {name:12s} {cells} {fid}")
        if block.get("kd_loss") is not None:
            lines.append(f"{block['subject']:8s} last epoch: kd_loss={block['kd_loss']:.4f} kd_agreement={block['kd_agreement']:.4f}")
    if doc.get("paired"):
        lines.append("")
        for m, p in doc["paired"].items():
            lines.append(f"student - replica0 {m:9s} mean {p['mean_difference']:+.4f}  wins/ties/losses {p['wins']}/{p['ties']}/{p['losses']}")
    return "\n".join(lines) + "\n"


def write_distillation(out_dir, folds, setting: Distillation, members: int, pooled: Optional[dict] = None, synthetic: bool = False,
                       stem: str = "distillation"):
    """distillation.txt / distillation.json of a run.  folds: one dict per fold with "subject", a metric row (accuracy, f1, nll,
    brier, ece, fidelity) under each of SYSTEMS it has, and the last epoch's kd_loss / kd_agreement.  pooled: the same rows over the
    pooled test windows.  The paired student - replica 0 differences are taken here, over the folds that have both."""
    out_dir = Path(out_dir)
    both = [f for f in folds if f.get("student") and f.get("replica0")]
    pairs = {}
    for m in ("accuracy", "f1"):
        rows = [f for f in both if f["student"].get(m) is not None and f["replica0"].get(m) is not None]
        if rows:
            pairs[m] = paired([f["student"][m] for f in rows], [f["replica0"][m] for f in rows])
    for m in ("nll", "brier", "ece"):                          # lower is better: the sign is turned so that a win is a win
        rows = [f for f in both if f["student"].get(m) is not None and f["replica0"].get(m) is not None]
        if rows:
            p = paired([-f["student"][m] for f in rows], [-f["replica0"][m] for f in rows])
            p["mean_difference"] = -p["mean_difference"]
            pairs[m] = p
    doc = dict(alpha=setting.alpha, temperature=setting.temperature, members=int(members), synthetic=bool(synthetic), folds=list(folds),
               pooled=pooled, paired=pairs)
    (out_dir / f"{stem}.json").write_text(json.dumps(doc, indent=1))
    path = out_dir / f"{stem}.txt"
    path.write_text(format_table(doc), encoding="utf-8")
    return path
