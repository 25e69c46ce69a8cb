"""Label-free BatchNorm adaptation to the test subject after LOSO (AdaBN; include/msig_ab.h).

``--calibrate`` answers how to fit a model to a new wearer who has labelled a few windows.  The common case for a wearable is the
other one: the new subject's recording is there, nobody has annotated it.  Every weight stays as trained; the running statistics
of the two BatchNorm layers are replaced by (``alpha`` = 1) or blended with the statistics of the new subject's own windows —
stage 1 first, then stage 2 under the ADAPTED stage 1 in its eval form, the way the model will be used.  The statistics are those
of the whole set however it is cut into batches (fp64 sums carried from batch to batch), not a moving average.

The method reads the test subject's unlabelled windows: it is transductive, as the pipeline's per-subject z-score already is.

Nothing of the run is touched: the adapter works on a COPY of each model's BatchNorm state; the model, its parameters,
``num_batches_tracked``, ``best_model.pt`` and every other output stay as they are (``model.adapt_bn(x, inplace=True)`` is the one
call that loads the result into a model).
"""
from __future__ import annotations

import ctypes as C
import json
from pathlib import Path
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .calibrate import summarise
from .multifold import launch_plan
from .runtime import Arenas, make_batch, workspace_need
from .trainer import accuracy_and_weighted_f1

SYNTHETIC_NOTE = ("WESAD is absent: the synthetic set has no subject shift by construction, so this table shows that the adaptation "
                  "machinery works, not whether adaptation helps on real subjects")
BN_KEYS = (("cnn_encoder.1.running_mean", 0, 16), ("cnn_encoder.1.running_var", 16, 32),
           ("cnn_encoder.5.running_mean", 32, 64), ("cnn_encoder.5.running_var", 64, 96))


def check_alpha(value) -> float:
    """The blend of an adaptation, a finite number in [0, 1]: ValueError otherwise."""
    try:
        a = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"adapt_bn alpha must be a number in [0, 1], got {value!r}") from None
    if not (0.0 <= a <= 1.0):          # NaN fails both comparisons
        raise ValueError(f"adapt_bn alpha must be in [0, 1], got {value!r}")
    return a


def batch_plan(sizes: Sequence[int], batch: int):
    """The launches of one pass over sets of `sizes` windows (any order) in batches of `batch`: (first window, batch size, jobs)
    records in launch order, `jobs` the indices into `sizes` that share the launch.  Sets whose batch sizes agree share a launch —
    the full batches, and ragged last batches of equal size; every window of every set is covered exactly once, in order."""
    if batch < 1 or any(int(n) < 1 for n in sizes):
        raise ValueError(f"batch_plan needs batch >= 1 and non-empty sets, got batch {batch}, sizes {list(sizes)}")
    order = sorted(range(len(sizes)), key=lambda j: (-int(sizes[j]), j))
    return [(i, b, [order[r] for r in range(r0, r0 + nr)]) for i, b, r0, nr in launch_plan([int(sizes[j]) for j in order], int(batch))]


class BnAdapter(Arenas):
    """Adapts the BatchNorm statistics of one model, or of several as a fold batch (one set of launches per batch for all of them).

    jobs: dicts with
        model   the fold's model (CnnGruAttentionModel / CnnGruModel, either depth), on the GPU
        x       (N, C, T) float32 device tensor: the new subject's windows, unlabelled
        y       optional (N,) labels: run() then also reports the model before and after on the same windows
    The jobs of an adapter share the model kind, depth, C, K and T (a fold batch is uniform in them); N is per job.
    alpha: 1 replaces the statistics, 0 keeps them, in between blends.  batched=False runs one msig_ab_accumulate / msig_ab_commit
    per job instead of one *_multi per group: the same bits.

    run() returns one dict per job: n, and with `y` before / after {accuracy, f1_score} — `before` is the model as it stands.
    adapted_state(i) is job i's adapted bn_state (96 floats), adapted_buffers(i) its four running_* tensors under the reference's
    names."""

    def __init__(self, jobs: Sequence[dict], alpha: float = 1.0, batched: bool = True, eval_batch: int = 1024):
        if not (1 <= len(jobs) <= L.MAX_FOLDS):
            raise ValueError(f"1..{L.MAX_FOLDS} folds per adapter")
        self.jobs, self.alpha, self.batched = list(jobs), check_alpha(alpha), bool(batched)
        self.engines = [j["model"].engine() for j in self.jobs]
        e0, x0 = self.engines[0], self.jobs[0]["x"]
        for j, e in zip(self.jobs, self.engines):
            x = j["x"]
            if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 3 or x.shape[1] != e.C or x.shape[0] < 1:
                raise ValueError(f"expected a non-empty float32 (N, {e.C}, T) GPU tensor, got {x.dtype} {tuple(x.shape)} on {x.device}")
            if (e.kind, e.gru_layers, e.C, e.K, e.n_flat, x.shape[2]) != (e0.kind, e0.gru_layers, e0.C, e0.K, e0.n_flat, x0.shape[2]):
                raise ValueError("the folds of an adapter share the model kind, depth, channels, classes and window length")
        self.kind, self.C, self.K, self.T = e0.kind, e0.C, e0.K, int(x0.shape[2])
        self.sizes = [int(j["x"].shape[0]) for j in self.jobs]
        self.batch = max(1, min(int(eval_batch), max(self.sizes)))
        self.eval_batch = max(1, int(eval_batch))
        self.ws_bytes = workspace_need([self.batch], self.C, self.T, self.K, False)        # the EVALUATION layout is all the calls need
        super().__init__(len(self.jobs), e0.device, [("params", e0.n_flat * 4), ("bn_state", L.BN_STATE_FLOATS * 4), ("bn_count", 16),
                                                     ("x", self.batch * self.C * self.T * 4), ("ws", self.ws_bytes), ("ab", L.AB_ACC_DOUBLES * 8)])
        self._ran = False

    def _desc(self, B: int, slot: int = 0) -> L.Batch:
        """The eval descriptor of a batch of B windows in arena `slot` (the *_multi calls are given arena 0's)."""
        return make_batch(B, self.C, self.T, self.K, *(self.ptr(r, slot) for r in ("x", "params", "bn_state", "bn_count", "ws")), self.ws_bytes,
                          self.engines[0].gru_layers)

    def _stage(self, stage: int):
        lib, st, kind = L.lib(), self.stream(), L.FT_KINDS[self.kind]
        for i, b, slots in batch_plan(self.sizes, self.batch):
            for s in slots:
                self.view(s, "x", torch.float32)[:b * self.C * self.T].copy_(self.jobs[s]["x"][i:i + b].reshape(-1))
            if self.batched:
                L.check(lib.msig_ab_accumulate_multi(C.byref(self._desc(b)), C.byref(self.multi(slots)), kind, stage, self.ptr("ab"), st),
                        "msig_ab_accumulate_multi")
            else:
                for s in slots:
                    L.check(lib.msig_ab_accumulate(C.byref(self._desc(b, s)), kind, stage, self.ptr("ab", s), st), "msig_ab_accumulate")
        if self.batched:
            L.check(lib.msig_ab_commit_multi(self.ptr("ab"), stage, self.alpha, self.ptr("bn_state"), self.ptr("bn_state"),
                                             C.byref(self.multi(range(self.n))), st), "msig_ab_commit_multi")
        else:
            for s in range(self.n):
                L.check(lib.msig_ab_commit(self.ptr("ab", s), stage, self.alpha, self.ptr("bn_state", s), self.ptr("bn_state", s), st),
                        "msig_ab_commit")

    def adapt(self):
        """Stage 1 over all batches, commit, stage 2 over all batches, commit — on copies of the models' parameters and state."""
        for s, eng in enumerate(self.engines):
            if getattr(eng, "scatter", None) is not None:
                eng.scatter()                                       # the one-layer model: its parameters into the padded layout
            self.view(s, "params", torch.float32).copy_(eng.params)
            self.view(s, "bn_state", torch.float32).copy_(eng.bn_state)
            self.view(s, "bn_count", torch.int64)[:2].copy_(eng.bn_count)
            self.view(s, "ab").zero_()
        self._stage(1)
        self._stage(2)
        self._ran = True

    def _predict(self, eng, bn_state: torch.Tensor, x, y):
        """Predictions of an eval-mode forward of the model with `bn_state` (its own or the adapted copy) as running statistics."""
        out = []
        for i in range(0, x.shape[0], self.eval_batch):
            xb = x[i:i + self.eval_batch]
            b = eng._batch(xb, None, False, 0.0, 0, 0)
            b.bn_state = bn_state.data_ptr()
            b.loss_acc = None
            eng.forward_desc(b)
            out.append(eng.region("PRED", torch.int32, (xb.shape[0],)).clone())
        return torch.cat(out).cpu().numpy().astype(np.int64)

    def run(self) -> List[dict]:
        if not self._ran:
            self.adapt()
        out = []
        for s, (j, eng) in enumerate(zip(self.jobs, self.engines)):
            r = {"n": self.sizes[s]}
            if j.get("y") is not None:
                y = j["y"].cpu().numpy().astype(np.int64)
                acc0, f0 = accuracy_and_weighted_f1(y, self._predict(eng, eng.bn_state, j["x"], j["y"]))
                acc1, f1 = accuracy_and_weighted_f1(y, self._predict(eng, self.adapted_state(s), j["x"], j["y"]))
                r.update(before={"accuracy": acc0, "f1_score": f0}, after={"accuracy": acc1, "f1_score": f1})
            out.append(r)
        return out

    def adapted_state(self, slot: int) -> torch.Tensor:
        """Job `slot`'s adapted bn_state: rm1 rv1 rm2 rv2, 96 floats (a view of the adapter's working copy)."""
        if not self._ran:
            self.adapt()
        return self.view(slot, "bn_state", torch.float32)

    def adapted_buffers(self, slot: int) -> dict:
        s = self.adapted_state(slot)
        return {k: s[a:b].clone() for k, a, b in BN_KEYS}


# ---- the adaptation table of a run --------------------------------------------------------------------------------------------------
def format_adaptation(table: dict, settings: Optional[dict] = None, synthetic: bool = False) -> str:
    lines = ["Label-free BatchNorm adaptation (AdaBN): every weight as trained, the BatchNorm running statistics from the test subject's "
             "own unlabelled windows (transductive, as the per-subject z-score is); both columns on the SAME windows; "
             "difference = adapted - LOSO"]
    if settings:
        lines.append("settings: " + ", ".join(f"{k} = {v}" for k, v in settings.items()))
    if synthetic:
        lines.append("NOTE: " + SYNTHETIC_NOTE + ".")
    lines += ["", f"  {'subject':<10} {'n':>6} {'LOSO acc':>10} {'adapt acc':>10} {'diff':>9}   {'LOSO F1':>9} {'adapt F1':>9} {'diff':>9}"]
    for f in table["folds"]:
        b, a = f["before"], f["after"]
        lines.append(f"  {f['subject']:<10} {f.get('n', 0):>6} {b['accuracy']:>10.4f} {a['accuracy']:>10.4f} "
                     f"{a['accuracy'] - b['accuracy']:>+9.4f}   {b['f1_score']:>9.4f} {a['f1_score']:>9.4f} {a['f1_score'] - b['f1_score']:>+9.4f}")
    lines.append("")
    for m, label in (("accuracy", "accuracy"), ("f1_score", "weighted F1")):
        sm = table["summary"][m]
        lines.append(f"  {label}: LOSO {sm['before']['mean']:.4f} ± {sm['before']['std']:.4f}   adapted {sm['after']['mean']:.4f} ± "
                     f"{sm['after']['std']:.4f}   mean paired difference {sm['difference']['mean']:+.4f} ± {sm['difference']['std']:.4f}   "
                     f"adapted wins {table['wins'][m]} of {table['n_folds']} folds, ties {table['ties'][m]}, losses {table['losses'][m]}")
    return "\n".join(lines) + "\n"


def write_adaptation(run_output_dir, folds: Sequence[dict], settings: Optional[dict] = None, synthetic: bool = False) -> Path:
    """adaptation.json (calibrate.summarise of the folds' before / after + settings) and adaptation.txt in `run_output_dir`."""
    run_output_dir = Path(run_output_dir)
    table = summarise(folds)
    doc = dict(table, settings=dict(settings or {}))
    if synthetic:
        doc["note"] = SYNTHETIC_NOTE
    (run_output_dir / "adaptation.json").write_text(json.dumps(doc, indent=1))
    path = run_output_dir / "adaptation.txt"
    path.write_text(format_adaptation(table, settings, synthetic), encoding="utf-8")
    return path
