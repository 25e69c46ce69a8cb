"""Subject-adversarial training (include/msig_da.h): the host side of the subject discriminator.

A ``SubjectAdversary`` is the discriminator D = Linear(128, 64) -> ReLU -> Linear(64, S) of ONE model: its flat parameter and Adam
moment buffers, its own optimiser step count, the schedule of the reversal weight lambda and the int32 table that maps a store
position to the domain (training subject) of the window there.  The arithmetic is the library's: ``runtime.Engine.train_step(...,
adversary=)`` and ``multifold.LockstepTrainer`` hand these buffers to the one train-step call (``msig_sc_train_step[_multi]``) as its ``msig_da``.  The buffers are no part of
the model's ``state_dict``: ``best_model.pt`` is what it is without the adversary.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _lib as L

SCHEDULES = ("ganin", "constant")
MAX_DOMAINS = L.MAX_K
STATS = 3                     # msig_da.stats: [sum of n * L_dom, rows whose argmax is their domain, labelled rows]


def flat_layout(S: int):
    """Offsets (floats) of W0 (64,128), b0 (64), W3 (S,64), b3 (S) in the flat buffer; last entry = msig_da_param_floats(S)."""
    if not 2 <= int(S) <= MAX_DOMAINS:
        raise ValueError(f"a subject adversary takes 2..{MAX_DOMAINS} domains, got {S}")
    o, out = 0, []
    for n in (64 * 128, 64, S * 64, S):
        out.append(o)
        o += (n + 3) // 4 * 4
    return out + [o]


def check_batch_size(batch_size: int) -> None:
    """The discriminator's step is one workgroup over at most MSIG_DA_MAX_BATCH rows: larger training batches are refused before training."""
    if int(batch_size) > L.DA_MAX_BATCH:
        raise ValueError(f"subject-adversarial training takes training batches of at most {L.DA_MAX_BATCH} windows, got batch size {batch_size}")


def settings(value) -> Optional[dict]:
    """config['adversary']: None (off) or a dict with any of lam / schedule / gamma / lr_mult / seed — checked, defaults filled in.
    The discriminator's Adam has no settings of its own beyond lr_mult: it shares the model's betas, eps and weight decay."""
    if value is None:
        return None
    if not isinstance(value, dict):
        raise ValueError(f"config['adversary'] must be None or a dict, got {value!r}")
    unknown = set(value) - {"lam", "schedule", "gamma", "lr_mult", "seed"}
    if unknown:
        raise ValueError(f"config['adversary'] has unknown keys {sorted(unknown)}")
    out = dict(lam=0.1, schedule="ganin", gamma=10.0, lr_mult=1.0, seed=None)
    out.update(value)
    for k in ("lam", "gamma", "lr_mult"):
        v = out[k]
        if isinstance(v, (str, bytes, bool)) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"adversary {k} must be a finite number >= 0, got {v!r}")
        out[k] = float(v)
    if out["schedule"] not in SCHEDULES:
        raise ValueError(f"adversary schedule must be one of {SCHEDULES}, got {out['schedule']!r}")
    return out


def subject_ordinals(lengths) -> np.ndarray:
    """Per-window subject ordinal of a dataset that concatenates subjects of `lengths` windows each: 0..len(lengths)-1."""
    return np.repeat(np.arange(len(lengths), dtype=np.int32), np.asarray(lengths, dtype=np.int64))


def domain_table(dataset) -> np.ndarray:
    """The int32 store-position -> domain table of a fold whose TRAINING set is `dataset` (WesadDataset or StoreView): the dataset's
    subjects map to 0..S-1 in dataset order, every other position of the store it draws from to -1."""
    ordinals = np.asarray(dataset.subject_ordinals, dtype=np.int32)
    index = getattr(dataset, "index_host", None)
    if index is None:                                        # a WesadDataset is its own store: position = row
        return ordinals.copy()
    table = np.full(int(dataset.store.x.shape[0]), -1, dtype=np.int32)
    table[index] = ordinals
    return table


class SubjectAdversary:
    def __init__(self, n_domains: int, lam: float = 0.1, schedule: str = "ganin", gamma: float = 10.0, lr_mult: float = 1.0, seed: int = 0):
        cfg = settings(dict(lam=lam, schedule=schedule, gamma=gamma, lr_mult=lr_mult))
        self.S = int(n_domains)
        self.layout = flat_layout(self.S)
        self.lam, self.schedule, self.gamma, self.lr_mult = cfg["lam"], cfg["schedule"], cfg["gamma"], cfg["lr_mult"]
        self.seed = int(seed)
        self.step = 0                                         # D's own optimiser step count
        self.total_steps = 1                                  # of the configured epoch budget (Trainer sets it)
        self.last_lambda = 0.0
        self.params = self.initial_parameters(self.S, self.seed)
        self.exp_avg = torch.zeros_like(self.params)
        self.exp_avg_sq = torch.zeros_like(self.params)
        self.stats = torch.zeros(STATS, dtype=torch.float64)
        self.dom: Optional[torch.Tensor] = None               # int32 domain table (set_domains)
        self.restricted_to: Optional[int] = None              # hidden size of an embedded model whose padded columns W0 leaves alone

    @staticmethod
    def initial_parameters(S: int, seed: int) -> torch.Tensor:
        """torch's default nn.Linear initialisation — weight and bias U(-1/sqrt(fan_in), 1/sqrt(fan_in)) — of both layers into the
        flat layout, drawn from a generator of its own: torch's global RNG is neither read nor advanced."""
        lay = flat_layout(S)
        gen = torch.Generator(device="cpu")
        gen.manual_seed(int(seed) & (2 ** 63 - 1))
        flat = torch.zeros(lay[-1], dtype=torch.float32)
        for o, n, fan_in in ((lay[0], 64 * 128, 128), (lay[1], 64, 128), (lay[2], S * 64, 64), (lay[3], S, 64)):
            bound = 1.0 / math.sqrt(fan_in)
            flat[o:o + n] = (torch.rand(n, generator=gen, dtype=torch.float64) * 2.0 - 1.0).mul_(bound).to(torch.float32)
        return flat

    # ---- schedule ----------------------------------------------------------------------------------------------------------------
    def lam_at(self, step: int, total_steps: int) -> float:
        """The reversal weight of optimiser step `step` (from 1): Ganin & Lempitsky's lam * (2 / (1 + exp(-gamma p)) - 1) with
        p = (step - 1) / total_steps — 0 at the first step, rising to lam — or lam itself for the constant schedule."""
        if self.schedule == "constant":
            return self.lam
        p = (int(step) - 1) / max(int(total_steps), 1)
        return self.lam * (2.0 / (1.0 + math.exp(-self.gamma * p)) - 1.0)

    def next_lambda(self) -> float:
        return self.lam_at(self.step + 1, self.total_steps)

    # ---- buffers -----------------------------------------------------------------------------------------------------------------
    def views(self, flat: Optional[torch.Tensor] = None) -> dict:
        flat = self.params if flat is None else flat
        lay, S = self.layout, self.S
        return {"0.weight": flat[lay[0]:lay[0] + 8192].view(64, 128), "0.bias": flat[lay[1]:lay[1] + 64],
                "2.weight": flat[lay[2]:lay[2] + S * 64].view(S, 64), "2.bias": flat[lay[3]:lay[3] + S]}

    def bind(self, device, storage: Optional[dict] = None) -> "SubjectAdversary":
        """Moves the buffers to `device`, or with `storage` (runtime.FoldArena.side_storage("adversary", slot)) into one fold's regions of an arena:
        float32 "params" / "exp_avg" / "exp_avg_sq", float64 "stats", int32 "dom"."""
        if storage is None:
            for name in ("params", "exp_avg", "exp_avg_sq", "stats", "dom"):
                t = getattr(self, name)
                if t is not None:
                    setattr(self, name, t.to(device))
            return self
        for name in ("params", "exp_avg", "exp_avg_sq", "stats"):
            dst = storage[name][:getattr(self, name).numel()]
            dst.copy_(getattr(self, name))
            setattr(self, name, dst)
        if self.dom is not None:
            if storage["dom"].numel() < self.dom.numel():
                raise ValueError("the arena's domain table is shorter than the fold's")
            storage["dom"].fill_(-1)
            storage["dom"][:self.dom.numel()].copy_(self.dom)
        self.dom = storage["dom"]
        return self

    def set_domains(self, table) -> None:
        """The fold's int32 store-position -> domain table (domain_table), before bind()."""
        t = torch.as_tensor(np.asarray(table, dtype=np.int32))
        if t.numel() and int(t.max()) >= self.S:
            raise ValueError(f"domain table names domain {int(t.max())} but the adversary has {self.S}")
        self.dom = t.to(self.params.device)

    def restrict_features(self, hidden: int) -> None:
        """For the embedded one-layer model (runtime.EmbeddedEngine): its feature row has real values at columns 0..hidden-1 and
        64..64+hidden-1 and exact zeros elsewhere, and the padded GRU units stay exactly zero only while they receive exactly zero
        gradient.  D's first layer is therefore zeroed on the padded input columns: the reversed gradient g = dpre W0 is then exactly
        zero there, and those weights stay zero (their gradient is dpre x 0, their decay wd x 0, Adam of zero moments moves nothing)."""
        if self.restricted_to == int(hidden):
            return
        w0 = self.views()["0.weight"]
        w0[:, hidden:64] = 0.0
        w0[:, 64 + hidden:] = 0.0
        self.restricted_to = int(hidden)

    def descriptor(self, lambdas, lrs, steps, idx: Optional[int] = None, idx_row_stride: int = 0, stride_bytes: int = 0,
                   betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0) -> L.Da:
        """msig_da over this adversary's buffers (a fold batch: arena 0's, `stride_bytes` apart) with per-fold lambda, lr and step."""
        if self.dom is None:
            raise RuntimeError("the adversary has no domain table: call set_domains first")
        a = L.Da()
        a.S, a.weight_decay, a.beta1, a.beta2, a.eps = self.S, weight_decay, betas[0], betas[1], eps
        a.dom, a.idx, a.idx_row_stride = self.dom.data_ptr(), idx, int(idx_row_stride)
        a.params, a.exp_avg, a.exp_avg_sq = self.params.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr()
        a.stats, a.stride_bytes = self.stats.data_ptr(), int(stride_bytes)
        for i, (lm, lr, st) in enumerate(zip(lambdas, lrs, steps)):
            getattr(a, "lambda")[i], a.lr[i], a.step[i] = float(lm), float(lr), int(st)
        return a

    def epoch_summary(self, stats) -> dict:
        """History entries of an epoch from its statistics (three numbers): mean domain loss, domain accuracy, the lambda in force."""
        s0, s1, s2 = (float(v) for v in stats)
        return dict(domain_loss=s0 / s2 if s2 > 0 else float("nan"), domain_acc=s1 / s2 if s2 > 0 else float("nan"),
                    adversary_lambda=self.last_lambda)

    # ---- persistence -------------------------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        out = {k: v.detach().cpu().clone() for k, v in self.views().items()}
        out.update({"exp_avg": self.exp_avg.detach().cpu().clone(), "exp_avg_sq": self.exp_avg_sq.detach().cpu().clone(),
                    "step": self.step, "n_domains": self.S})
        return out

    def load_state_dict(self, state: dict) -> None:
        if int(state["n_domains"]) != self.S:
            raise ValueError(f"state is of an adversary with {state['n_domains']} domains, this one has {self.S}")
        for k, v in self.views().items():
            v.copy_(torch.as_tensor(state[k]).to(v.dtype).reshape(v.shape))
        self.exp_avg.copy_(torch.as_tensor(state["exp_avg"]))
        self.exp_avg_sq.copy_(torch.as_tensor(state["exp_avg_sq"]))
        self.step = int(state["step"])



def fold_record(info: dict) -> Optional[dict]:
    """The adversary's record of one trained fold from its fold_result (multifold.fold_result): S, chance 1 / S, the first and the last
    epoch's domain accuracy and loss, the final lambda and the fold's test accuracy; None for a fold trained without an adversary."""
    hist = [h for h in info.get("history", []) if "domain_acc" in h]
    if "adversary_domains" not in info or not hist:
        return None
    S = int(info["adversary_domains"])
    return dict(subject=info["subject"], S=S, chance=1.0 / S, first_domain_acc=hist[0]["domain_acc"], last_domain_acc=hist[-1]["domain_acc"],
                first_domain_loss=hist[0]["domain_loss"], last_domain_loss=hist[-1]["domain_loss"], final_lambda=hist[-1]["adversary_lambda"],
                epochs=len(hist), test_accuracy=info.get("accuracy"))


def write_adversary(out_dir, folds, cfg: dict, synthetic: bool = False, stem: str = "adversary"):
    """adversary.txt / adversary.json of a run: per fold how subject-identifiable the feature was when training began and ended
    (domain accuracy against chance 1 / S), and the pooled means.  lam = 0 is the probe mode: D only measures.  stem: the files'
    name (the hierarchical run writes one pair per model)."""
    from pathlib import Path
    import json
    out_dir = Path(out_dir)
    keys = ("chance", "first_domain_acc", "last_domain_acc", "first_domain_loss", "last_domain_loss", "final_lambda", "test_accuracy")
    pooled = {k: float(np.mean([f[k] for f in folds if f[k] is not None])) for k in keys if any(f[k] is not None for f in folds)}
    doc = dict(settings=dict(cfg), probe=cfg["lam"] == 0.0, synthetic=bool(synthetic), folds=folds, pooled=pooled)
    (out_dir / f"{stem}.json").write_text(json.dumps(doc, indent=1))
    lines = [f"SUBJECT ADVERSARY: lambda={cfg['lam']:g} schedule={cfg['schedule']} gamma={cfg['gamma']:g} lr_mult={cfg['lr_mult']:g}"
             + (" (probe: the discriminator measures, nothing is reversed)" if cfg["lam"] == 0.0 else "")]
    if synthetic:
        lines.append("NOTE: the synthetic set draws every subject from one distribution: it has no subject shift to remove, so these "
                     "numbers say nothing about WESAD accuracy.")
    lines.append("")
    lines.append(f"{'fold':8s} {'S':>3s} {'chance':>7s} {'acc first':>10s} {'acc last':>9s} {'loss first':>11s} {'loss last':>10s} {'lambda':>7s} {'test acc':>9s}")
    for f in folds:
        ta = "      n/a" if f["test_accuracy"] is None else f"{f['test_accuracy']:9.4f}"
        lines.append(f"{f['subject']:8s} {f['S']:3d} {f['chance']:7.4f} {f['first_domain_acc']:10.4f} {f['last_domain_acc']:9.4f} "
                     f"{f['first_domain_loss']:11.4f} {f['last_domain_loss']:10.4f} {f['final_lambda']:7.4f} {ta}")
    if pooled:
        lines.append("")
        lines.append("pooled mean: " + " ".join(f"{k}={v:.4f}" for k, v in pooled.items()))
    path = out_dir / f"{stem}.txt"
    path.write_text("\n".join(lines) + "\n", encoding="utf-8")
    return path
