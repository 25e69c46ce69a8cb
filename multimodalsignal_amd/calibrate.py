"""Few-shot subject calibration after LOSO: how much does a model trained on the other subjects gain from a minute or two of
labelled data of the new wearer?

The feature extractor (CNN + GRU) is frozen and runs in eval mode, so a window's 128-dimensional feature never changes: it is
computed once (``model.embed`` / ``Engine.features``, include/msig_ft.h msig_ft_features) and the classifier is re-fitted on the
cached rows by ``msig_ft_head_epoch`` — an epoch of Adam steps on the 128 -> 64 -> K head in ONE launch, for all folds of a rank at
once in the fold-batched form.  ``Trainer.train`` cannot do this: the fused train step updates every tensor whatever
``requires_grad`` says.  This module is the supported way to train the classifier alone.

Nothing of the run is touched: the calibrator works on a COPY of the model's flat parameter buffer; the model, its BatchNorm
buffers, ``best_model.pt`` and every other output stay as they are.

``calibration_split`` decides which windows of the new subject are seen: the first ``n_per_class`` windows of every class in
recording order, a guard gap around them (windows overlap), the rest for evaluation.
"""
from __future__ import annotations

import ctypes as C
import json
from pathlib import Path
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .runtime import Arenas
from .trainer import accuracy_and_weighted_f1

DEFAULT_GAP = 5          # real WESAD windows are 60 s at a 10 s stride: windows up to 5 apart share samples
DEFAULT_EPOCHS = 30
SYNTHETIC_NOTE = ("WESAD is absent: on the synthetic set this table shows that the calibration machinery works, "
                  "not how much calibration helps on real subjects")


def calibration_split(labels, n_per_class: int, gap: int = DEFAULT_GAP):
    """(cal_idx, eval_idx), int64 arrays of positions in dataset (recording) order.  The first `n_per_class` windows of every class
    present are the calibration set; every window within `gap` positions of a calibration window is dropped; the rest is the
    evaluation remainder.  ValueError — nothing is silently skipped — when a class has fewer than n_per_class + 1 windows, or when
    the remainder misses a class that is present in the subject."""
    y = np.asarray(labels).astype(np.int64).reshape(-1)
    n_per_class, gap = int(n_per_class), int(gap)
    if n_per_class < 1 or gap < 0:
        raise ValueError(f"calibration_split needs n_per_class >= 1 and gap >= 0, got {n_per_class}, {gap}")
    classes = np.unique(y)
    cal = []
    for c in classes:
        pos = np.flatnonzero(y == c)
        if pos.size < n_per_class + 1:
            raise ValueError(f"class {int(c)} has {pos.size} windows: calibration on {n_per_class} per class needs at least {n_per_class + 1}")
        cal.append(pos[:n_per_class])
    cal_idx = np.sort(np.concatenate(cal)) if cal else np.zeros(0, np.int64)
    blocked = np.zeros(y.size, dtype=bool)
    for p in cal_idx:
        blocked[max(0, p - gap):p + gap + 1] = True
    eval_idx = np.flatnonzero(~blocked).astype(np.int64)
    missing = [int(c) for c in classes if not np.any(y[eval_idx] == c)]
    if missing:
        raise ValueError(f"the evaluation remainder misses class(es) {missing}: too few windows are left after {n_per_class} per class "
                         f"and a gap of {gap}")
    return cal_idx.astype(np.int64), eval_idx


def epoch_orders(n: int, epochs: int, seed: int) -> np.ndarray:
    """(epochs, n) int32: the permutation of every epoch, from the calibrator's own shuffle seed."""
    rs = np.random.RandomState(int(seed) & 0x7FFFFFFF)
    return np.stack([rs.permutation(n) for _ in range(epochs)]).astype(np.int32) if epochs else np.zeros((0, n), np.int32)


class HeadCalibrator(Arenas):
    """Calibrates the classifier of one model, or of several (a fold batch: one launch per epoch for all of them).

    jobs: dicts with
        model        the fold's model (CnnGruAttentionModel / CnnGruModel, either depth), on the GPU
        x_cal, y_cal (N, C, T) float32 / (N,) int64 device tensors: the calibration windows
        x_eval, y_eval  the evaluation remainder
        lr, seed, shuffle_seed, class_weight (K numbers or None)      per fold
    epochs, batch_size (<= 256), weight_decay, dropout (None = the model's), betas, eps are shared by the folds of a calibrator.
    batched=False runs one msig_ft_head_epoch per fold and epoch instead of one msig_ft_head_epoch_multi per epoch: the same bits.

    run() returns one dict per job: before / after {accuracy, f1_score} on the remainder, n_cal, n_eval, the per-epoch training
    loss.  `before` is the model as it stands, `after` the same extractor with the tuned head.  tuned_state(i) gives the tuned
    classifier tensors of job i (reference shapes)."""

    def __init__(self, jobs: Sequence[dict], epochs: int = DEFAULT_EPOCHS, batch_size: int = 64, weight_decay: float = 0.0,
                 dropout: Optional[float] = None, betas=(0.9, 0.999), eps: float = 1e-8, batched: bool = True, eval_batch: int = 1024):
        if not (1 <= len(jobs) <= L.MAX_FOLDS):
            raise ValueError(f"1..{L.MAX_FOLDS} folds per calibrator")
        self.jobs, self.epochs, self.batched = list(jobs), int(epochs), bool(batched)
        self.batch = max(1, min(int(batch_size), L.FT_MAX_BATCH))
        self.weight_decay, self.betas, self.eps, self.eval_batch = float(weight_decay), betas, float(eps), int(eval_batch)
        m0 = self.jobs[0]["model"]
        self.engines = [j["model"].engine() for j in self.jobs]
        e0 = self.engines[0]
        for e in self.engines:
            if (e.K, e.n_flat, e.layout[L.P_CLS0_W]) != (e0.K, e0.n_flat, e0.layout[L.P_CLS0_W]):
                raise ValueError("the folds of a calibrator share K and the parameter layout")
        self.K, self.n_flat, self.cls_offset = e0.K, e0.n_flat, e0.layout[L.P_CLS0_W]
        self.dropout_p = float(m0.dropout_p if dropout is None else dropout)
        self.n_cal = [int(j["y_cal"].numel()) for j in self.jobs]
        if min(self.n_cal) < 1:
            raise ValueError("a calibration set is empty")
        n_max = max(self.n_cal)
        super().__init__(len(self.jobs), e0.device,
                         [("params", self.n_flat * 4), ("exp_avg", self.n_flat * 4), ("exp_avg_sq", self.n_flat * 4), ("feat", n_max * 512),
                          ("labels", n_max * 8), ("order", max(1, self.epochs) * n_max * 4), ("cw", self.K * 4), ("acc", max(1, self.epochs) * 16)])
        self.weighted = any(j.get("class_weight") is not None for j in self.jobs)
        self._ran = False

    # ---- the frozen extractor -------------------------------------------------------------------------------------------
    def _features(self, eng, x):
        return torch.cat([eng.features(x[i:i + self.eval_batch], padded=True) for i in range(0, x.shape[0], self.eval_batch)])

    def _predict(self, eng, flat, x, y):
        """Predictions of an eval-mode forward with the parameters in `flat` (the engine's own buffer or the tuned copy) — the
        extractor's tensors are the same bits in both."""
        out = []
        for i in range(0, x.shape[0], self.eval_batch):
            xb, yb = x[i:i + self.eval_batch], y[i:i + self.eval_batch]
            b = eng._batch(xb, yb, False, 0.0, 0, 0)
            b.params = flat.data_ptr()
            b.loss_acc = None
            eng.forward_desc(b)
            out.append(eng.region("PRED", torch.int32, (xb.shape[0],)).clone())
        return torch.cat(out).cpu().numpy().astype(np.int64)

    # ---- the head epochs ------------------------------------------------------------------------------------------------------
    def _head(self, n_cal: int, epoch: int, slot: int = 0) -> L.FtHead:
        h = L.FtHead()
        h.K, h.N, h.n_order, h.batch = self.K, n_cal, n_cal, self.batch
        h.first_step, h.n_steps = 0, (n_cal + self.batch - 1) // self.batch
        h.dropout_thr = L.dropout_threshold(self.dropout_p)
        h.cls_offset = self.cls_offset
        h.beta1, h.beta2, h.eps, h.weight_decay = self.betas[0], self.betas[1], self.eps, self.weight_decay
        h.feat, h.labels = self.ptr("feat", slot), self.ptr("labels", slot)
        h.order = self.ptr("order", slot, epoch * n_cal * 4)
        h.params, h.exp_avg, h.exp_avg_sq = self.ptr("params", slot), self.ptr("exp_avg", slot), self.ptr("exp_avg_sq", slot)
        h.class_weight = self.ptr("cw", slot) if self.weighted else None
        h.loss_acc = self.ptr("acc", slot, epoch * 16)
        return h

    def run(self) -> List[dict]:
        if self._ran:
            raise RuntimeError("a HeadCalibrator runs once (its Adam state and step counts are those of one calibration)")
        self._ran = True
        lib, st = L.lib(), self.stream()
        before = []
        for s, (j, eng) in enumerate(zip(self.jobs, self.engines)):
            if getattr(eng, "scatter", None) is not None:
                eng.scatter()                                       # the one-layer model: its parameters into the padded layout
            self.view(s, "params", torch.float32).copy_(eng.params)
            feat = self._features(eng, j["x_cal"])                   # cached once: the extractor is frozen and in eval mode
            self.view(s, "feat", torch.float32)[:feat.numel()].copy_(feat.reshape(-1))
            self.view(s, "labels", torch.int64)[:self.n_cal[s]].copy_(j["y_cal"].to(torch.int64))
            lab = j["y_cal"].cpu().numpy()
            if lab.min() < 0 or lab.max() >= self.K:
                raise ValueError(f"calibration label outside [0, {self.K})")
            orders = epoch_orders(self.n_cal[s], self.epochs, j.get("shuffle_seed", 0))
            if orders.size:
                self.view(s, "order", torch.int32)[:orders.size].copy_(torch.from_numpy(orders.reshape(-1)))
            w = np.ones(self.K) if j.get("class_weight") is None else L.check_class_weight(j["class_weight"], self.K)
            self.view(s, "cw", torch.float32).copy_(torch.as_tensor(w, dtype=torch.float32))
            before.append(self._predict(eng, eng.params, j["x_eval"], j["y_eval"]))
        steps = [(n + self.batch - 1) // self.batch for n in self.n_cal]
        groups = {}
        for s, n in enumerate(self.n_cal):                          # folds of one launch share N (a class absent from a subject)
            groups.setdefault(n, []).append(s)
        for e in range(self.epochs):
            if self.batched:
                for n_cal, slots in groups.items():
                    h, m = self._head(n_cal, e), L.FtMulti()
                    m.n, m.stride_bytes = len(slots), self.stride
                    for i, s in enumerate(slots):
                        m.slot[i], m.lr[i], m.step0[i] = s, float(self.jobs[s]["lr"]), e * steps[s] + 1
                        m.seed[i] = int(self.jobs[s].get("seed", 0)) & (2 ** 64 - 1)
                    L.check(lib.msig_ft_head_epoch_multi(C.byref(h), C.byref(m), st), "msig_ft_head_epoch_multi")
            else:
                for s, n_cal in enumerate(self.n_cal):
                    h = self._head(n_cal, e, s)
                    h.lr, h.step0, h.seed = float(self.jobs[s]["lr"]), e * steps[s] + 1, int(self.jobs[s].get("seed", 0)) & (2 ** 64 - 1)
                    L.check(lib.msig_ft_head_epoch(C.byref(h), st), "msig_ft_head_epoch")
        out = []
        for s, (j, eng) in enumerate(zip(self.jobs, self.engines)):
            y = j["y_eval"].cpu().numpy().astype(np.int64)
            after = self._predict(eng, self.view(s, "params", torch.float32), j["x_eval"], j["y_eval"])
            acc0, f0 = accuracy_and_weighted_f1(y, before[s])
            acc1, f1 = accuracy_and_weighted_f1(y, after)
            sums = self.view(s, "acc", torch.float64)[:2 * self.epochs].view(-1, 2).cpu().numpy()
            out.append({"n_cal": self.n_cal[s], "n_eval": int(y.size),
                        "before": {"accuracy": acc0, "f1_score": f0}, "after": {"accuracy": acc1, "f1_score": f1},
                        "train_loss": [float(v) / self.n_cal[s] for v in sums[:, 0]]})
        return out

    def tuned_flat(self, slot: int) -> torch.Tensor:
        """The working copy of job `slot`'s flat parameter buffer: the model's tensors with the tuned classifier."""
        return self.view(slot, "params", torch.float32)

    def tuned_state(self, slot: int) -> dict:
        eng = self.engines[slot]
        flat = self.tuned_flat(slot)
        views = eng.named_param_views(flat)
        out = {k: views[k].clone() for k in ("classifier.0.bias", "classifier.3.weight", "classifier.3.bias")}
        w0 = views["classifier.0.weight"]
        if getattr(eng, "hidden", None):                            # the one-layer model: its real columns
            w0 = torch.cat([w0[:, :eng.hidden], w0[:, 64:64 + eng.hidden]], dim=1)
        out["classifier.0.weight"] = w0.clone()
        return out


# ---- the calibration table of a run ---------------------------------------------------------------------------------------------
def summarise(folds: Sequence[dict]) -> dict:
    """folds: per-fold dicts with subject, before / after {accuracy, f1_score} (and n_cal, n_eval).  Mean and population std
    (np.std, as cv_summary.txt) of both, the mean paired difference after - before, wins / ties / losses of the calibrated head."""
    out = {"n_folds": len(folds), "folds": list(folds), "summary": {}, "wins": {}, "ties": {}, "losses": {}}
    for m in ("accuracy", "f1_score"):
        b = np.array([f["before"][m] for f in folds], dtype=np.float64)
        a = np.array([f["after"][m] for f in folds], dtype=np.float64)
        d = a - b
        stat = lambda v: {"mean": float(v.mean()) if v.size else float("nan"), "std": float(v.std()) if v.size else float("nan")}
        out["summary"][m] = {"before": stat(b), "after": stat(a), "difference": stat(d)}
        out["wins"][m], out["ties"][m], out["losses"][m] = int((d > 0).sum()), int((d == 0).sum()), int((d < 0).sum())
    return out


def format_calibration(table: dict, settings: Optional[dict] = None, synthetic: bool = False) -> str:
    lines = ["Few-shot subject calibration: frozen extractor, classifier re-fitted on the test subject's first windows; "
             "both columns on the SAME evaluation remainder; difference = calibrated - LOSO"]
    if settings:
        lines.append("settings: " + ", ".join(f"{k} = {v}" for k, v in settings.items()))
    if synthetic:
        lines.append("NOTE: " + SYNTHETIC_NOTE + ".")
    lines += ["", f"  {'subject':<10} {'n_cal':>6} {'n_eval':>7} {'LOSO acc':>10} {'calib acc':>10} {'diff':>9}   {'LOSO F1':>9} {'calib F1':>9} {'diff':>9}"]
    for f in table["folds"]:
        b, a = f["before"], f["after"]
        lines.append(f"  {f['subject']:<10} {f.get('n_cal', 0):>6} {f.get('n_eval', 0):>7} {b['accuracy']:>10.4f} {a['accuracy']:>10.4f} "
                     f"{a['accuracy'] - b['accuracy']:>+9.4f}   {b['f1_score']:>9.4f} {a['f1_score']:>9.4f} {a['f1_score'] - b['f1_score']:>+9.4f}")
    lines.append("")
    for m, label in (("accuracy", "accuracy"), ("f1_score", "weighted F1")):
        sm = table["summary"][m]
        lines.append(f"  {label}: LOSO {sm['before']['mean']:.4f} ± {sm['before']['std']:.4f}   calibrated {sm['after']['mean']:.4f} ± "
                     f"{sm['after']['std']:.4f}   mean paired difference {sm['difference']['mean']:+.4f} ± {sm['difference']['std']:.4f}   "
                     f"calibrated wins {table['wins'][m]} of {table['n_folds']} folds, ties {table['ties'][m]}, losses {table['losses'][m]}")
    return "\n".join(lines) + "\n"


def write_calibration(run_output_dir, folds: Sequence[dict], settings: Optional[dict] = None, synthetic: bool = False) -> Path:
    """calibration.json (summarise + settings) and calibration.txt in `run_output_dir`."""
    run_output_dir = Path(run_output_dir)
    table = summarise(folds)
    doc = dict(table, settings=dict(settings or {}))
    if synthetic:
        doc["note"] = SYNTHETIC_NOTE
    (run_output_dir / "calibration.json").write_text(json.dumps(doc, indent=1))
    path = run_output_dir / "calibration.txt"
    path.write_text(format_calibration(table, settings, synthetic), encoding="utf-8")
    return path
