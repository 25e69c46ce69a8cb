"""Group-DRO over training subjects (include/msig_dro.h): the host side of the group weights.

A ``GroupDro`` is the state of ONE model's robust objective: the G adversarial weights ``q`` (uniform at 1 / G when training starts,
never reset — not by a learning-rate reduction either), the int32 table that maps a store position to the group of the window
there, and the epoch's statistics.  The arithmetic is the library's: ``runtime.Engine.train_step(..., dro=)`` and
``multifold.LockstepTrainer`` hand these buffers to the one train-step call (``msig_sc_train_step[_multi]``) as its ``msig_dro``, whose one extra launch moves ``q`` with the
groups' losses and rescales the logits' gradient so that the step descends sum_g q_g L_g instead of the pooled mean.  What a step
reports stays the criterion's; the buffers are no part of the model's ``state_dict``.
"""
from __future__ import annotations

import json
import math
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from . import _lib as L

GROUPS = ("subject", "subject-class")
MAX_GROUPS = L.DRO_MAX_GROUPS
STATS = L.DRO_STATS
DEFAULT_ETA = 0.01


def check_batch_size(batch_size: int) -> None:
    """The term's launch keeps a row's loss, mass and group in LDS: larger training batches are refused before training."""
    if int(batch_size) > L.DRO_MAX_BATCH:
        raise ValueError(f"group-DRO takes training batches of at most {L.DRO_MAX_BATCH} windows, got batch size {batch_size}")


def settings(value) -> Optional[dict]:
    """config['trainer']['group_dro']: None (off), a number (eta) or a dict with any of eta / groups — checked, defaults filled in."""
    if value is None:
        return None
    if isinstance(value, dict):
        unknown = set(value) - {"eta", "groups"}
        if unknown:
            raise ValueError(f"group_dro has unknown keys {sorted(unknown)}")
        out = dict(eta=DEFAULT_ETA, groups="subject")
        out.update(value)
    else:
        out = dict(eta=value, groups="subject")
    v = out["eta"]
    if isinstance(v, (str, bytes, bool)) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
        raise ValueError(f"group_dro eta must be a finite number >= 0, got {v!r}")
    out["eta"] = float(v)
    if out["groups"] not in GROUPS:
        raise ValueError(f"group_dro groups must be one of {GROUPS}, got {out['groups']!r}")
    return out


def parse(eta, groups=None) -> dict:
    """--group-dro [ETA] --dro-groups G as a setting (ValueError for a bad value)."""
    return settings(dict(eta=DEFAULT_ETA if eta is None else eta, groups=groups or "subject"))


def settings_line(cfg) -> str:
    c = settings(cfg)
    return f"GROUP DRO: eta={c['eta']:g} groups={c['groups']}"


def group_count(dataset, groups: str, K: int) -> int:
    """G of a fold whose training set is `dataset`: its subjects, or its subjects times the K classes."""
    S = int(np.max(dataset.subject_ordinals)) + 1
    G = S if groups == "subject" else S * int(K)
    if groups not in GROUPS:
        raise ValueError(f"group_dro groups must be one of {GROUPS}, got {groups!r}")
    if not 1 <= G <= MAX_GROUPS:
        raise ValueError(f"group-DRO takes 1..{MAX_GROUPS} groups, got {G} ({S} training subjects, groups={groups!r})")
    return G


def group_table(dataset, groups: str, K: int) -> np.ndarray:
    """The int32 store-position -> group table of a fold whose TRAINING set is `dataset` (WesadDataset or StoreView): the window's
    subject ordinal, or ordinal * K + label (the dataset's mapped labels) for "subject-class"; every other position of the store the
    dataset draws from is -1 (in no group)."""
    group_count(dataset, groups, K)
    ordinals = np.asarray(dataset.subject_ordinals, dtype=np.int64)
    if groups == "subject-class":
        labels = np.asarray(dataset.labels, dtype=np.int64)
        if labels.size and (labels.min() < 0 or labels.max() >= K):
            raise ValueError(f"a label outside [0, {K}) has no (subject, class) group")
        ordinals = ordinals * int(K) + labels
    ordinals = ordinals.astype(np.int32)
    index = getattr(dataset, "index_host", None)
    if index is None:                                        # a WesadDataset is its own store: position = row
        return ordinals.copy()
    table = np.full(int(dataset.store.x.shape[0]), -1, dtype=np.int32)
    table[index] = ordinals
    return table


def worst_subject_accuracy(preds, labels, ordinals):
    """(ordinal, accuracy) of the subject with the lowest accuracy among windows with per-window subject `ordinals` (the first of
    equals); (None, None) without windows."""
    preds, labels, ordinals = np.asarray(preds), np.asarray(labels), np.asarray(ordinals)
    worst = (None, None)
    for s in np.unique(ordinals):
        m = ordinals == s
        acc = float(np.mean(preds[m] == labels[m]))
        if worst[1] is None or acc < worst[1]:
            worst = (int(s), acc)
    return worst


class GroupDro:
    def __init__(self, eta: float = DEFAULT_ETA, groups: str = "subject"):
        cfg = settings(dict(eta=eta, groups=groups))
        self.eta, self.groups = cfg["eta"], cfg["groups"]
        self.G: Optional[int] = None
        self.K = 1                                            # classes per subject of the group index ("subject-class": the model's K)
        self.q: Optional[torch.Tensor] = None                 # float32 (G,)
        self.grp: Optional[torch.Tensor] = None               # int32 store-position -> group
        self.stats = torch.zeros(STATS, dtype=torch.float64)

    def set_groups(self, table, G: int, K: int = 1) -> "GroupDro":
        """The fold's group table (group_table) and count, before bind(); q starts uniform at 1 / G."""
        if not 1 <= int(G) <= MAX_GROUPS:
            raise ValueError(f"group-DRO takes 1..{MAX_GROUPS} groups, got {G}")
        t = torch.as_tensor(np.asarray(table, dtype=np.int32))
        if t.numel() and int(t.max()) >= int(G):
            raise ValueError(f"group table names group {int(t.max())} but there are {G}")
        self.G, self.K = int(G), int(K) if self.groups == "subject-class" else 1
        self.grp = t
        self.q = torch.full((self.G,), 1.0 / self.G, dtype=torch.float32)
        return self

    def bind(self, device, storage: Optional[dict] = None) -> "GroupDro":
        """Moves the buffers to `device`, or with `storage` (runtime.FoldArena.side_storage("dro", slot)) into one fold's regions of an arena:
        float32 "q", float64 "stats", int32 "grp"."""
        if self.q is None:
            raise RuntimeError("the group-DRO state has no groups: call set_groups first")
        if storage is None:
            self.q, self.grp, self.stats = self.q.to(device), self.grp.to(device), self.stats.to(device)
            return self
        if storage["grp"].numel() < self.grp.numel() or storage["q"].numel() < self.G:
            raise ValueError("the arena's group-DRO region is smaller than the fold's")
        storage["grp"].fill_(-1)
        storage["grp"][:self.grp.numel()].copy_(self.grp)
        storage["q"].zero_()
        storage["q"][:self.G].copy_(self.q)
        storage["stats"].copy_(self.stats)
        self.q, self.grp, self.stats = storage["q"][:self.G], storage["grp"], storage["stats"]
        return self

    def descriptor(self, idx: Optional[int] = None, idx_row_stride: int = 0, stride_bytes: int = 0, frozen: bool = False,
                   stats: bool = True) -> L.Dro:
        """msig_dro over this state's buffers (a fold batch: arena 0's, `stride_bytes` apart)."""
        if self.q is None or not self.q.is_cuda:
            raise RuntimeError("the group-DRO state is not bound to a device: set_groups, then bind")
        d = L.Dro()
        d.G, d.eta, d.frozen = self.G, self.eta, int(bool(frozen))
        d.grp, d.idx, d.idx_row_stride = self.grp.data_ptr(), idx, int(idx_row_stride)
        d.q, d.stats, d.stride_bytes = self.q.data_ptr(), self.stats.data_ptr() if stats else None, int(stride_bytes)
        return d

    def epoch_summary(self, stats, q) -> dict:
        """History entries of an epoch from its statistics (STATS numbers) and the weights as the epoch left them: the mean robust
        loss of its steps, the worst group's mean loss (sum of T_g over sum of W_g) and which group and subject that is, max and
        entropy of q, and per subject the mean training loss and the weight (summed over the subject's groups)."""
        s = np.asarray(stats, dtype=np.float64)
        qv = np.asarray(q, dtype=np.float64)[:self.G]
        T, W = s[:self.G], s[MAX_GROUPS:MAX_GROUPS + self.G]
        steps = float(s[3 * MAX_GROUPS + 1])
        loss = [float(T[g] / W[g]) if W[g] > 0 else None for g in range(self.G)]
        seen = [g for g in range(self.G) if loss[g] is not None]
        worst = max(seen, key=lambda g: loss[g]) if seen else None
        S = self.G // self.K
        Ts, Ws = T.reshape(S, self.K).sum(axis=1), W.reshape(S, self.K).sum(axis=1)
        nz = qv[qv > 0]
        return dict(dro_robust_loss=float(s[3 * MAX_GROUPS] / steps) if steps > 0 else None,
                    dro_worst_group_loss=None if worst is None else loss[worst], dro_worst_group=worst,
                    dro_worst_subject=None if worst is None else worst // self.K,
                    dro_q_max=float(qv.max()), dro_q_entropy=float(-(nz * np.log(nz)).sum()),
                    dro_subject_loss=[float(Ts[i] / Ws[i]) if Ws[i] > 0 else None for i in range(S)],
                    dro_subject_q=[float(v) for v in qv.reshape(S, self.K).sum(axis=1)], dro_q=[float(v) for v in qv])


def fold_info(dro: GroupDro, subjects=None) -> dict:
    """What a fold trained with group-DRO adds to its result (multifold.fold_result): the setting, the group count, the training
    subjects' names in ordinal order and the final q."""
    S = dro.G // dro.K
    names = [str(s) for s in subjects] if subjects is not None and len(subjects) == S else [f"#{i}" for i in range(S)]
    return dict(eta=dro.eta, groups=dro.groups, G=dro.G, K=dro.K, subjects=names, q=[float(v) for v in dro.q.detach().cpu().tolist()])


def fold_record(info: dict) -> Optional[dict]:
    """The record of one trained fold from its fold_result: the training subjects ordered by their final weight with their mean
    training loss of the last epoch, the last epoch's robust and mean losses, the worst validation subject and the fold's test
    accuracy; None for a fold trained without group-DRO."""
    hist = [h for h in info.get("history", []) if "dro_q" in h]
    g = info.get("group_dro")
    if g is None or not hist:
        return None
    last, K, names = hist[-1], int(g["K"]), g["subjects"]
    qs = np.asarray(g["q"], dtype=np.float64).reshape(len(names), K).sum(axis=1)
    order = sorted(range(len(names)), key=lambda i: (-qs[i], i))
    return dict(subject=info["subject"], G=int(g["G"]), groups=g["groups"], eta=g["eta"], q=[float(v) for v in g["q"]],
                subjects=[dict(subject=names[i], q=float(qs[i]), loss=last["dro_subject_loss"][i]) for i in order],
                heaviest=names[order[0]], robust_loss=last["dro_robust_loss"], mean_loss=last["train_loss"],
                worst_val_subject=last.get("val_worst_subject"), worst_val_acc=last.get("val_worst_subject_acc"), epochs=len(hist),
                test_accuracy=info.get("accuracy"))


def write_dro(out_dir, folds, cfg: dict, synthetic: bool = False, stem: str = "dro"):
    """dro.txt / dro.json of a run: per fold the training subjects ordered by final q with their last-epoch losses, the robust and
    mean losses and the worst validation subject; pooled over folds, how often each subject was the heaviest.  stem: the files' name
    (the hierarchical run writes one pair per model)."""
    out_dir = Path(out_dir)
    cfg = settings(cfg)
    heaviest = {}
    for f in folds:
        heaviest[f["heaviest"]] = heaviest.get(f["heaviest"], 0) + 1
    ranked = sorted(heaviest.items(), key=lambda kv: (-kv[1], kv[0]))
    doc = dict(settings=cfg, probe=cfg["eta"] == 0.0, synthetic=bool(synthetic), folds=folds,
               pooled=dict(heaviest=[dict(subject=s, folds=n) for s, n in ranked]))
    (out_dir / f"{stem}.json").write_text(json.dumps(doc, indent=1))
    lines = [settings_line(cfg) + (" (probe: q stays uniform, the per-subject losses are measured)" if cfg["eta"] == 0.0 else "")]
    if synthetic:
        lines.append("NOTE: the synthetic set draws every subject from one distribution: it has no hard subject to protect, so these "
                     "numbers say nothing about WESAD accuracy.")
    fmt = lambda v: "     n/a" if v is None else f"{v:8.4f}"
    for f in folds:
        lines.append("")
        lines.append(f"fold {f['subject']}: G={f['G']} robust loss {fmt(f['robust_loss'])} mean loss {fmt(f['mean_loss'])} "
                     f"worst val subject {f['worst_val_subject']} acc {fmt(f['worst_val_acc'])} test acc {fmt(f['test_accuracy'])}")
        lines.append(f"  {'subject':10s} {'q':>8s} {'loss':>8s}")
        for s in f["subjects"]:
            lines.append(f"  {s['subject']:10s} {s['q']:8.4f} {fmt(s['loss'])}")
    if ranked:
        lines.append("")
        lines.append("heaviest subject over folds: " + " ".join(f"{s}={n}" for s, n in ranked))
    path = out_dir / f"{stem}.txt"
    path.write_text("\n".join(lines) + "\n", encoding="utf-8")
    return path
