"""Drop-in for the reference's ``trainer.py`` driving the fused HIP train step.

Public surface kept (reference ``trainer.py:12-273``): ``EarlyStopping(patience, delta,
checkpoint_path, verbose, log_func)``; ``Trainer(model, fold_output_dir, config)`` with
``.train(train_loader, val_loader)`` and ``.evaluate(loader, is_test, is_val)`` returning
``(loss, acc, f1)`` / ``(loss, acc, f1, preds, labels)``; the same ``config['trainer']``
keys; the same artefacts (``training_log.txt``, ``best_model.pt``,
``test_confusion_matrix.png``) and log line format (plus a windows/s figure).

What differs is where the work happens: one ``msig_train_step`` launch sequence per
mini-batch (zero_grad + forward + CE + backward + Adam, trainer.py:144-149) with no
``.item()`` in the loop — the epoch loss is accumulated on the device and read once per
epoch — and evaluation reads predictions back once per call.

Reference behaviours reproduced on purpose: EarlyStopping treats a
HIGHER monitored value as better although it is fed the validation loss; the class-weight
option is accepted and ignored (the reference's branch is unreachable, trainer.py:81).
The class-weighted loss that branch would build is opted into through a key of this repo's
own, ``config['trainer']['class_weights']`` (include/msig_cw.h).
``config['trainer']['max_grad_norm']``, another key of this repo's own, puts
``torch.nn.utils.clip_grad_norm_`` between the backward pass and Adam inside the fused step
(include/msig_gc.h) and adds the epoch's gradient norms to ``history`` and the log.
``config['trainer']['label_smoothing']`` is ``CrossEntropyLoss(label_smoothing=...)`` of the training, validation and test
losses alike (include/msig_st.h); a training loader built with ``mixup=`` has its batches' lam passed on to the step.
``config['adversary']`` (None or a dict of lam / schedule / gamma / lr_mult / seed) trains a subject discriminator on the feature
inside every TRAINING step and reverses its gradient into the extractor (include/msig_da.h); validation and test
never run it; ``history`` and the log gain the epoch's domain loss, domain accuracy and lambda.
``config['averaging']`` (None or a dict with a mode, ``averaging.settings``) keeps an EMA or SWA shadow of the weights — one more launch
after every train step (EMA) or at the end of an epoch (SWA); it steers nothing (include/msig_wa.h).
``config['trainer']['sam']`` (None, or ``RHO[:adaptive[:ETA]]``) makes every TRAINING step a sharpness-aware one (include/msig_sam.h,
DESIGN.md §28): ``history`` and the log gain the epoch's ``sam_grad_norm`` (mean and max) and ``sam_sharpness``; a rho of 0 is the
run without the key; not with ``config['adversary']``.
``config['trainer']['group_dro']`` (None, a number — eta — or a dict with eta / groups, ``dro.settings``) makes every TRAINING step
descend the group-DRO objective over the training subjects (include/msig_dro.h): ``history`` and the log gain
``dro_robust_loss``, ``dro_worst_group_loss`` (and its subject), ``dro_q_max``, ``dro_q_entropy`` and the worst validation subject's
accuracy; the reported losses, the scheduler, early stopping and ``best_model.pt`` keep following the criterion; not with mixup.
"""
from __future__ import annotations

import os
import threading
import time
from pathlib import Path

import numpy as np
import torch
from torch.optim.lr_scheduler import ReduceLROnPlateau

from . import _lib as L
from . import adversary as A
from . import dro as DRO
from . import supcon as SC
from . import averaging as AV
from . import sam as SAM
from .models import CnnGruAttentionModel


_PLOT_LOCK = threading.Lock()      # pyplot is not thread-safe; folds may run concurrently


class EarlyStopping:
    """trainer.py:12-39.  `score >= best + delta` counts as an improvement (checkpoint, reset
    the counter); anything lower increments the counter."""

    def __init__(self, patience=7, delta=0, checkpoint_path="checkpoint.pt", verbose=False, log_func=None):
        self.patience, self.delta, self.checkpoint_path = patience, delta, checkpoint_path
        self.verbose, self.log_func = verbose, log_func
        self.counter, self.best_score, self.early_stop = 0, None, False

    def __call__(self, score, model):
        improved = self.best_score is None or not (score < self.best_score + self.delta)
        if improved:
            self.best_score = score
            self.save_checkpoint(model)
            self.counter = 0
            return
        self.counter += 1
        if self.verbose and self.log_func:
            self.log_func(f"EarlyStopping counter: {self.counter}/{self.patience}")
        if self.counter >= self.patience:
            self.early_stop = True

    def save_checkpoint(self, model):
        # the parameters are views into larger flat buffers (one per model, or one arena for a whole fold batch): save
        # copies, not the buffers behind them
        torch.save({k: v.detach().clone() for k, v in model.state_dict().items()}, self.checkpoint_path)


class MsigAdam(torch.optim.Optimizer):
    """torch.optim.Adam(lr, weight_decay) semantics on the model's flat buffers via
    msig_adam_step.  Exists so that `trainer.optimizer` / ReduceLROnPlateau keep working."""

    def __init__(self, model: CnnGruAttentionModel, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__([p for p in model.parameters()], dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.model = model
        self.step_count = 0

    def add_param_group(self, param_group):
        """torch decorates Optimizer.add_param_group with torch._disable_dynamo, whose wrapper imports torch._dynamo at its first
        call: ~0.9 s of interpreter time in front of the first train step of a run whose 15 folds take 6 s (profiles/
        r04_loso_profile.log), for a compiler this path never uses.  The undecorated function does the same bookkeeping."""
        plain = getattr(torch.optim.Optimizer.add_param_group, "__wrapped__", None)
        return plain(self, param_group) if plain is not None else super().add_param_group(param_group)

    @property
    def hyper(self):
        return self.param_groups[0]

    @torch.no_grad()
    def step(self, closure=None):
        """Un-fused use (after loss.backward()): gathers p.grad into the flat gradient buffer."""
        eng = self.model.engine()
        for p, gv in zip(self.model._named(), self.model._grad_views()):
            if p.numel() and p.grad is not None:
                gv.copy_(p.grad)
        self.step_count += 1
        h = self.hyper
        eng.adam_step(h["lr"], h["betas"], h["eps"], h["weight_decay"], self.step_count)


def accuracy_and_weighted_f1(y_true: np.ndarray, y_pred: np.ndarray):
    """sklearn accuracy_score and f1_score(average='weighted') (trainer.py:234-235): per-class
    F1 weighted by true support; a class with no predicted and no true samples scores 0."""
    y_true, y_pred = np.asarray(y_true).astype(np.int64), np.asarray(y_pred).astype(np.int64)
    n = y_true.size
    acc = float((y_true == y_pred).mean()) if n else 0.0
    f1 = 0.0
    for c in np.unique(y_true):
        tp = float(np.sum((y_true == c) & (y_pred == c)))
        fp = float(np.sum((y_true != c) & (y_pred == c)))
        fn = float(np.sum((y_true == c) & (y_pred != c)))
        denom = 2 * tp + fp + fn
        f1 += (np.sum(y_true == c) / n) * (2 * tp / denom if denom > 0 else 0.0)
    return acc, float(f1)


def balanced_class_weights(labels, num_classes: int) -> np.ndarray:
    """sklearn's compute_class_weight('balanced', classes=range(K), y=labels) (trainer.py:85-89): N / (K * count_c), float64.
    A class of [0, K) with no window in `labels` has no such weight: ValueError naming it."""
    y = np.asarray(labels).astype(np.int64).reshape(-1)
    counts = np.bincount(y, minlength=num_classes)[:num_classes] if y.size else np.zeros(num_classes, np.int64)
    missing = [c for c in range(num_classes) if counts[c] == 0]
    if missing:
        raise ValueError(f"class_weights='balanced': class(es) {missing} of [0, {num_classes}) are absent from the training set")
    return y.size / (num_classes * counts.astype(np.float64))


def class_weight_setting(value, num_classes: int):
    """config['trainer']['class_weights']: None (the unweighted criterion), 'balanced', or K numbers (checked: ValueError)."""
    if value is None or (isinstance(value, str) and value == "balanced"):
        return value
    if isinstance(value, str):
        raise ValueError(f"class_weights must be None, 'balanced' or {num_classes} numbers, got {value!r}")
    return L.check_class_weight(value, num_classes)


def grad_clip_setting(value):
    """config['trainer']['max_grad_norm']: None (no clipping: the unclipped train step) or a positive finite number (ValueError
    otherwise), returned as a float."""
    if value is None:
        return None
    v = L.check_max_grad_norm(value)          # a number > 0; the binding also takes inf ("measure, do not clip"), a configuration does not
    if v == float("inf"):
        raise ValueError(f"max_grad_norm must be None or a positive finite number, got {value!r}")
    return v


def label_smoothing_setting(value):
    """config['trainer']['label_smoothing']: None (the hard-label criterion) or a number with 0 <= eps < 1 (ValueError otherwise)."""
    return None if value is None else L.check_label_smoothing(value)


def grad_norm_summary(stats, steps: int) -> dict:
    """The history entries of an epoch's gradient norms from a clip state's statistics (runtime.Engine.grad_stats) over `steps` steps."""
    return dict(grad_norm_mean=stats["sum"] / max(steps, 1), grad_norm_max=stats["max"], clipped_steps=int(stats["clipped"]))


class Trainer:
    def __init__(self, model, fold_output_dir: Path, config):
        self.model, self.fold_dir, self.config = model, Path(fold_output_dir), config
        self.fold_dir.mkdir(parents=True, exist_ok=True)
        self.log_file = self.fold_dir / "training_log.txt"
        with open(self.log_file, "w") as f:
            f.write(f"Training log for run starting at {time.strftime('%Y-%m-%d %H:%M:%S')}\n" + "=" * 50 + "\n")
        if not torch.cuda.is_available():
            raise RuntimeError("Trainer needs an AMD GPU: the multimodalsignal_amd path has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.model.to(self.device)
        cfg = config["trainer"]
        self.epochs, self.learning_rate = cfg["epochs"], cfg["learning_rate"]
        self.patience, self.weight_decay = cfg["early_stopping"]["patience"], cfg["weight_decay"]
        self.use_class_weights = cfg.get("use_class_weights", False)      # accepted, inert (trainer.py:81)
        # CrossEntropyLoss(weight=...) of the train steps and of the validation / test losses (trainer.py:96-97): None, 'balanced'
        # (from the training loader's labels, when training starts) or K numbers.  class_weight: the (K,) fp32 device vector once set
        self.class_weights = class_weight_setting(cfg.get("class_weights"), self.model.num_classes)
        self.class_weight = None
        # clip_grad_norm_(model.parameters(), max_grad_norm) inside the fused step (include/msig_gc.h); None: the unclipped step
        self.max_grad_norm = grad_clip_setting(cfg.get("max_grad_norm"))
        # CrossEntropyLoss(label_smoothing=eps) of every loss this trainer takes (include/msig_st.h); None / 0: the hard-label calls
        self.label_smoothing = label_smoothing_setting(cfg.get("label_smoothing")) or 0.0
        # subject-adversarial training (include/msig_da.h): the settings now, the discriminator when the training set is known
        self.adversary_cfg = A.settings(config.get("adversary"))
        self.adversary = None
        # distillation (include/msig_kd.h): a distill.Distillation with its teacher table, bound by set_distillation; None: off
        self.distill = None
        # weight averaging (include/msig_wa.h): the fold's averager (settings and counters); the shadow itself is the engine's
        # sharpness-aware minimisation (include/msig_sam.h): a sam.Sam, or None (also for rho = 0: the run without it)
        self.sam = SAM.setting(cfg.get("sam"))
        if self.sam is not None and not self.sam.on:
            self.sam = None
        if self.sam is not None and self.adversary_cfg is not None:
            raise ValueError("config['trainer']['sam'] cannot be combined with config['adversary']: the discriminator's own Adam would "
                             "advance in both passes of a step")
        # group-DRO (include/msig_dro.h): the settings now, the group weights when the training set is known
        self.dro_cfg = DRO.settings(cfg.get("group_dro"))
        self.dro = None
        # supervised contrastive term on the feature (include/msig_sc.h): the settings now, the buffers when the training set is known
        self.supcon_cfg = SC.settings(cfg.get("supcon"))
        self.supcon = None
        self.subject_names = (None, None)        # (training, validation) subjects in ordinal order, when the driver knows them
        self.averaging_cfg = AV.settings(config.get("averaging"))
        self.averager = AV.WeightAverager(self.averaging_cfg) if self.averaging_cfg is not None else None
        self.verbose = cfg.get("verbose", True)
        self.optimizer = MsigAdam(self.model, lr=self.learning_rate, weight_decay=self.weight_decay)   # trainer.py:68
        self.scheduler = ReduceLROnPlateau(self.optimizer, mode="min", factor=0.1, patience=3)         # trainer.py:72-77
        self.early_stopping = None
        if cfg["early_stopping"]["enabled"]:
            self.early_stopping = EarlyStopping(patience=self.patience, delta=cfg["early_stopping"]["delta"],
                                                checkpoint_path=self.fold_dir / "best_model.pt", verbose=True, log_func=self._log)
        self.history = []
        self._labels_ok = set()
        self.total_start_time = time.time()
        self.train_windows = 0
        self.train_seconds = 0.0

    def _log(self, message):
        if self.verbose:
            print(message)
        with open(self.log_file, "a") as f:
            f.write(message + "\n")

    def _to_device(self, inputs, labels):
        if isinstance(inputs, (list, tuple)):
            raise TypeError("list/tuple inputs (the reference's retired HybridDataset, trainer.py:135-140) are not supported")
        return inputs.to(self.device, non_blocking=True), labels.to(self.device, non_blocking=True)

    def _check_labels(self, loader):
        """A class id outside [0, num_classes) would index past the logits row in the loss kernel (torch's
        CrossEntropyLoss raises for it, trainer.py:147); checked once per dataset, on its host-side label vector —
        e.g. CLASSIFICATION_MODE 'ternary' with NUM_CLASSES left at 2 (main.py:22-23)."""
        ds = getattr(loader, "dataset", None)
        labels = getattr(ds, "labels", None)
        if labels is None or id(ds) in self._labels_ok:
            return
        lab = np.asarray(labels)
        if lab.size and (lab.min() < 0 or lab.max() >= self.model.num_classes):
            raise ValueError(f"label {int(lab.max() if lab.max() >= self.model.num_classes else lab.min())} is outside "
                             f"[0, {self.model.num_classes}): dataset labels do not match the model's num_classes")
        self._labels_ok.add(id(ds))

    def prepare_class_weights(self, train_loader):
        """Resolves config['trainer']['class_weights'] once (trainer.py:80-97): 'balanced' from the training loader's dataset labels.
        Logs the vector as the reference does.  Returns the host values (float32) or None."""
        if self.class_weights is None:
            return None
        if self.class_weight is None:
            if isinstance(self.class_weights, str):
                labels = getattr(getattr(train_loader, "dataset", None), "labels", None)
                if labels is None:
                    raise ValueError("class_weights='balanced' needs a training dataset with a `labels` array")
                w = balanced_class_weights(labels, self.model.num_classes)
            else:
                w = self.class_weights
            self.class_weight = torch.tensor(np.asarray(w, dtype=np.float32), device=self.device)
            self._log(f"已启用类别加权损失，权重为: {np.asarray(w, dtype=np.float32)}")
        return self.class_weight.cpu().numpy()

    def prepare_adversary(self, train_loader, storage=None):
        """Builds the fold's subject discriminator once, when config['adversary'] is set: one domain per subject of the training
        set, its domain table over the store the loader gathers from, its schedule over the configured epoch budget.  Its seed is
        the setting's, else the model's dropout seed (per fold).  Its Adam shares the model's betas, eps and weight decay; its learning
        rate is the model's (schedule included) times lr_mult.  storage: one fold's adversary buffers of a FoldArena.  ValueError
        before any training for a batch size the discriminator's step cannot take."""
        if self.adversary_cfg is None or self.adversary is not None:
            return self.adversary
        A.check_batch_size(train_loader.batch_size)
        ds = train_loader.dataset
        if getattr(ds, "subject_ordinals", None) is None:
            raise ValueError("config['adversary'] needs a training dataset with per-window `subject_ordinals`")
        c = self.adversary_cfg
        seed = c["seed"] if c["seed"] is not None else getattr(self.model, "_seed", 0)
        adv = A.SubjectAdversary(int(np.max(ds.subject_ordinals)) + 1, c["lam"], c["schedule"], c["gamma"], c["lr_mult"], seed)
        adv.total_steps = self.epochs * len(train_loader)
        adv.set_domains(A.domain_table(ds))
        if int(getattr(self.model, "gru_num_layers", 2)) == 1:      # the embedded one-layer model: D leaves the padded feature columns alone
            adv.restrict_features(int(self.model.gru_hidden_size))
        self.adversary = adv.bind(self.device, storage)
        self._log(f"subject adversary: {adv.S} domains, lambda {adv.lam:g} ({adv.schedule}), lr x {adv.lr_mult:g}")
        return adv

    def prepare_dro(self, train_loader, storage=None):
        """Builds the fold's group-DRO state once, when config['trainer']['group_dro'] is set: one group per subject of the training
        set (or per (subject, class) pair), its group table over the store the loader gathers from, q uniform at 1 / G.  storage: one
        fold's group-DRO buffers of a FoldArena.  ValueError before any training for a batch size the term's launch cannot take, for
        a loader that mixes, and for more than 64 groups."""
        if self.dro_cfg is None or self.dro is not None:
            return self.dro
        DRO.check_batch_size(train_loader.batch_size)
        if getattr(train_loader, "mixup", None) is not None:
            raise ValueError("group_dro cannot be combined with mixup: a row blended from two subjects has no group")
        ds = train_loader.dataset
        if getattr(ds, "subject_ordinals", None) is None:
            raise ValueError("config['trainer']['group_dro'] needs a training dataset with per-window `subject_ordinals`")
        c, K = self.dro_cfg, int(self.model.num_classes)
        d = DRO.GroupDro(c["eta"], c["groups"])
        d.set_groups(DRO.group_table(ds, c["groups"], K), DRO.group_count(ds, c["groups"], K), K)
        self.dro = d.bind(self.device, storage)
        self._log(f"group-DRO: {d.G} groups ({d.groups}), eta {d.eta:g}")
        return d

    def prepare_supcon(self, train_loader, storage=None):
        """Builds the fold's supervised contrastive term once, when config['trainer']['supcon'] is set: in cross-subject mode its
        subject table over the store the loader gathers from.  storage: one fold's supcon buffers of a FoldArena.  ValueError before
        any training for a batch size the term's launches cannot take and for a loader that mixes."""
        if self.supcon_cfg is None or self.supcon is not None:
            return self.supcon
        SC.check_batch_size(train_loader.batch_size)
        if getattr(train_loader, "mixup", None) is not None:
            raise ValueError("supcon cannot be combined with mixup: a row blended from two windows has no label to contrast")
        c = self.supcon_cfg
        sc = SC.SupCon(c["weight"], c["tau"], c["positives"])
        if sc.cross_subject:
            ds = train_loader.dataset
            if getattr(ds, "subject_ordinals", None) is None:
                raise ValueError("supcon positives 'cross-subject' need a training dataset with per-window `subject_ordinals`")
            sc.set_subjects(SC.subject_table(ds))
        self.supcon = sc.bind(self.device, storage, max_batch=int(train_loader.batch_size))
        self._log(f"supcon: weight {sc.weight:g}, tau {sc.tau:g}, positives {sc.positives}")
        return sc

    def val_worst_subject(self, val_loader, preds, labels) -> "dict | None":
        """With group-DRO on: the validation subject with the lowest accuracy, from the predictions of the epoch's validation pass
        (host side; the validation loader serves its windows in dataset order)."""
        ords = getattr(getattr(val_loader, "dataset", None), "subject_ordinals", None)
        if self.dro_cfg is None or ords is None or len(ords) != len(preds):
            return None
        s, acc = DRO.worst_subject_accuracy(preds, labels, ords)
        names = self.subject_names[1]
        return dict(val_worst_subject=None if s is None else (str(names[s]) if names is not None and s < len(names) else f"#{s}"),
                    val_worst_subject_acc=acc)

    def dro_epoch(self, stats, q, worst=None) -> dict:
        """The epoch's group-DRO entries of history and the log line: GroupDro.epoch_summary, the worst group's subject by name, and
        the worst validation subject."""
        out = self.dro.epoch_summary(stats, q)
        names, s = self.subject_names[0], out["dro_worst_subject"]
        out["dro_worst_subject"] = None if s is None else (str(names[s]) if names is not None and s < len(names) else f"#{s}")
        out.update(worst or dict(val_worst_subject=None, val_worst_subject_acc=None))
        return out

    def set_distillation(self, distillation, storage=None):
        """Turns the fold into a student: `distillation` is a distill.Distillation whose teacher table covers the
        store positions the training loader gathers from (the loader must serve `last_index`).  Every train step then carries the
        distillation term; history and the epoch line gain kd_loss and kd_agreement; validation, the scheduler, early stopping and
        best_model.pt keep following the criterion against the labels.  storage: one fold's distillation buffers of a FoldArena."""
        if distillation.q is None:
            raise ValueError("the distillation has no teacher table: call set_teacher first")
        if int(distillation.q.shape[1]) != int(self.model.num_classes):
            raise ValueError(f"the teacher table has {int(distillation.q.shape[1])} classes, the model {self.model.num_classes}")
        self.distill = distillation.bind(self.device, storage)
        self._log(f"distillation: alpha {distillation.alpha:g}, temperature {distillation.temperature:g}, "
                  f"teacher table of {int(distillation.q.shape[0])} positions")
        return self.distill

    # ---- trainer.py:119-191 -------------------------------------------------------------------
    def train(self, train_loader, val_loader):
        eng = self.model.engine()
        self._check_labels(train_loader)
        self._check_labels(val_loader)
        self.prepare_class_weights(train_loader)
        adv = self.prepare_adversary(train_loader)
        dro = self.prepare_dro(train_loader)
        sc = self.prepare_supcon(train_loader)
        kd = self.distill
        if kd is not None and not hasattr(train_loader, "last_index"):
            raise ValueError("distillation needs a training loader that serves the store positions of its batches (last_index)")
        av = self.averager
        if av is not None:
            eng.average_update(av.bind(eng).start_coef())      # EMA: the shadow starts as a copy of the initial model; SWA: no launch
        n_train = len(train_loader.dataset)
        for epoch in range(self.epochs):
            t0 = time.time()
            self.model.train()
            eng.loss_acc.zero_()
            if self.max_grad_norm is not None:
                eng.zero_grad_stats()
            if adv is not None:
                adv.stats.zero_()
            if kd is not None:
                kd.stats.zero_()
            if dro is not None:
                dro.stats.zero_()
            if sc is not None:
                sc.stats.zero_()
            if self.sam is not None:
                eng.ensure_sam_state()
                eng.zero_sam_stats()
            n_steps = 0
            for inputs, labels in train_loader:
                n_steps += 1
                x, y = self._to_device(inputs, labels)
                h = self.optimizer.hyper
                self.optimizer.step_count += 1
                eng.train_step(x, y, lr=h["lr"], betas=h["betas"], eps=h["eps"], weight_decay=h["weight_decay"],
                               step=self.optimizer.step_count, dropout_p=self.model.dropout_p, seed=self.model._seed,
                               class_weight=self.class_weight, max_grad_norm=self.max_grad_norm, label_smoothing=self.label_smoothing,
                               mix_lambda=getattr(train_loader, "last_lam", None),      # the lam of the batch a mixup loader just served
                               adversary=adv, distill=kd, sam=self.sam, dro=dro,
                               batch_index=getattr(train_loader, "last_index", None) if adv is not None or kd is not None or dro is not None
                               or sc is not None else None, supcon=sc)
                if av is not None and av.mode == "ema":
                    eng.average_update(av.step_coef())
                # running_loss += loss.item() * batch (trainer.py:152) happens inside the step: the loss kernel adds to eng.loss_acc
            sam = None
            if self.sam is not None:                                                     # the same sync: one read-back for all three
                acc, stats, ss = eng.epoch_stats(self.max_grad_norm is not None, True)
                train_loss, sam = acc[0] / n_train, SAM.summary(ss, n_steps)
                grad = grad_norm_summary(stats, n_steps) if stats is not None else None
            elif self.max_grad_norm is None:
                train_loss, grad = float(eng.loss_acc[0].item()) / n_train, None         # the epoch's only sync
            else:                                                                        # the same sync: one read-back for both
                acc, stats = eng.loss_and_grad_stats()
                train_loss, grad = acc[0] / n_train, grad_norm_summary(stats, n_steps)
            dom = adv.epoch_summary(adv.stats.cpu().tolist()) if adv is not None else None
            kds = kd.epoch_summary(kd.stats.cpu().tolist()) if kd is not None else None
            dt = time.time() - t0
            self.train_windows += n_train
            self.train_seconds += dt
            if av is not None and av.mode == "swa":
                eng.average_update(av.epoch_coef(epoch + 1))     # the epoch-end iterate, from start_epoch on (before: no launch)
            val_loss, val_acc, val_f1, vp, vl = self.evaluate(val_loader, is_val=True)
            avg = self.validate_averaged(val_loader) if av is not None and av.validate else None
            drs = None
            if dro is not None:
                drs = self.dro_epoch(dro.stats.cpu().tolist(), dro.q.cpu().tolist(), self.val_worst_subject(val_loader, vp, vl))
            scs = sc.epoch_summary(sc.stats.cpu().tolist()) if sc is not None else None
            if self._end_of_epoch(epoch, train_loss, dt, n_train, val_loss, val_acc, val_f1, grad, dom, avg, kds, sam, drs, scs):
                break
        self.finish_averaging([train_loader])
        self._finish_training()

    def validate_averaged(self, val_loader) -> dict:
        """config['averaging']['validate']: the epoch's validation pass once more under the shadow — its own accumulator zeroing and
        read-back — as the three history entries; None values while an SWA shadow has no iterate yet."""
        if not self.averager.ready:
            return dict(val_loss_avg=None, val_acc_avg=None, val_f1_avg=None)
        loss, acc, f1 = self.evaluate_averaged(val_loader)
        return dict(val_loss_avg=loss, val_acc_avg=acc, val_f1_avg=f1)

    def finish_averaging(self, train_loaders, recompute=True):
        """End of training, BEFORE the early-stopping checkpoint is restored: an SWA fold without an iterate takes the weights the
        last step left as its single one; bn = "recompute" re-estimates the shadow's BatchNorm statistics on the training windows
        (recompute False: the caller does that for a whole fold batch with one adapter)."""
        av = self.averager
        if av is None or av.finished:
            return
        eng = self.model.engine()
        eng.average_update(av.bind(eng).final_coef())
        if recompute and av.bn == "recompute":
            AV.recompute_bn([eng], train_loaders)

    def _end_of_epoch(self, epoch, train_loss, dt, n_train, val_loss, val_acc, val_f1, grad=None, dom=None, avg=None, kd=None, sam=None,
                      dro=None, supcon=None) -> bool:
        """Scheduler step, history, log line, early stopping (trainer.py:160-185); True = stop training.  grad: grad_norm_summary of
        the epoch when max_grad_norm is set — three more history keys and a suffix of the log line; None leaves both as they were.
        dom: SubjectAdversary.epoch_summary of the epoch when config['adversary'] is set, likewise.  avg: the validation pass under
        the averaging shadow when config['averaging']['validate'] is set (three more history keys; it steers nothing).  kd:
        Distillation.epoch_summary of the epoch for a student (set_distillation): kd_loss and kd_agreement, likewise.  sam:
        sam.summary of the epoch when config['trainer']['sam'] is set: sam_grad_norm, sam_grad_norm_max and sam_sharpness, likewise.
        dro: dro_epoch of the epoch when config['trainer']['group_dro'] is set: the robust loss, the worst group's loss and subject,
        max and entropy of q, the per-subject losses and weights and the worst validation subject, likewise (it steers nothing).
        supcon: SupCon.epoch_summary of the epoch when config['trainer']['supcon'] is set: supcon_loss, supcon_top1 and
        supcon_anchors, likewise."""
        self.scheduler.step(val_loss)
        self.history.append(dict(epoch=epoch + 1, train_loss=train_loss, val_loss=val_loss, val_acc=val_acc, val_f1=val_f1,
                                 lr=self.optimizer.hyper["lr"], seconds=dt))
        suffix = ""
        if grad is not None:
            self.history[-1].update(grad)
            suffix = (f" | 梯度范数: {grad['grad_norm_mean']:.4f} (max {grad['grad_norm_max']:.4f}) | "
                      f"裁剪步数: {grad['clipped_steps']} (max_grad_norm={self.max_grad_norm:g})")
        if dom is not None:
            self.history[-1].update(dom)
            suffix += f" | domain loss: {dom['domain_loss']:.4f} | domain acc: {dom['domain_acc']:.4f} | lambda: {dom['adversary_lambda']:.4f}"
        if kd is not None:
            self.history[-1].update(kd)
            if kd["kd_loss"] is not None:
                suffix += f" | kd loss: {kd['kd_loss']:.4f} | kd agreement: {kd['kd_agreement']:.4f}"
        if sam is not None:
            self.history[-1].update(sam)
            suffix += (f" | sam grad norm: {sam['sam_grad_norm']:.4f} (max {sam['sam_grad_norm_max']:.4f}) | "
                       f"sam sharpness: {sam['sam_sharpness']:.6f} (sam={self.sam.spec()})")
        if dro is not None:
            self.history[-1].update(dro)
            if dro["dro_robust_loss"] is not None:
                suffix += (f" | dro robust loss: {dro['dro_robust_loss']:.4f} | worst group loss: {dro['dro_worst_group_loss']:.4f} "
                           f"({dro['dro_worst_subject']}) | q max: {dro['dro_q_max']:.4f} | q entropy: {dro['dro_q_entropy']:.4f}")
            if dro["val_worst_subject_acc"] is not None:
                suffix += f" | worst val subject: {dro['val_worst_subject']} acc {dro['val_worst_subject_acc']:.4f}"
        if supcon is not None:
            self.history[-1].update(supcon)
            if supcon["supcon_loss"] is not None:
                suffix += (f" | supcon loss: {supcon['supcon_loss']:.4f} | top-1: {supcon['supcon_top1']:.4f} | "
                           f"anchors: {supcon['supcon_anchors']:.1f}")
        if avg is not None:
            self.history[-1].update(avg)
            if avg["val_loss_avg"] is not None:
                suffix += f" | averaged: val loss {avg['val_loss_avg']:.4f} acc {avg['val_acc_avg']:.4f} F1 {avg['val_f1_avg']:.4f}"
        self._log(f"Epoch {epoch + 1}/{self.epochs} | 耗时: {dt:.2f}s | 训练损失: {train_loss:.4f} | 验证损失: {val_loss:.4f} | "
                  f"验证Acc: {val_acc:.4f} | 验证F1: {val_f1:.4f} | {n_train / max(dt, 1e-9):.0f} windows/s" + suffix)
        if self.early_stopping:
            self.early_stopping(val_loss, self.model)
            if self.early_stopping.early_stop:
                self._log("触发早停")
                return True
        return False

    def _finish_training(self):
        if self.early_stopping and self.early_stopping.early_stop:
            self._log(f"加载性能最佳的模型权重从: {self.early_stopping.checkpoint_path}")
            self.model.load_state_dict(torch.load(self.early_stopping.checkpoint_path, weights_only=True))
        self._log(f"--- 训练完成 --- 总训练时长: {time.time() - self.total_start_time:.2f}秒")

    # ---- trainer.py:193-247 -------------------------------------------------------------------
    def _eval_pass(self, data_loader, shadow=False):
        """One eval-mode pass over a loader: (loss, predictions, labels).  shadow: under the weight-averaging shadow."""
        eng = self.model.engine()
        self._check_labels(data_loader)
        self.model.eval()
        eng.loss_acc.zero_()
        preds, labs = [], []
        for inputs, labels in data_loader:
            x, y = self._to_device(inputs, labels)
            eng.forward(x, y, training=False, class_weight=self.class_weight, label_smoothing=self.label_smoothing, shadow=shadow)   # the loss kernel adds loss * batch to eng.loss_acc (trainer.py:221)
            preds.append(eng.region("PRED", torch.int32, (y.shape[0],)).clone())
            labs.append(y.clone())          # DeviceLoader reuses its batch buffers
        all_preds = torch.cat(preds).cpu().numpy().astype(np.int64)
        all_labels = torch.cat(labs).cpu().numpy().astype(np.int64)
        loss = float(eng.loss_acc[0].item()) / len(data_loader.dataset)
        return loss, all_preds, all_labels

    def evaluate_averaged(self, data_loader):
        """(loss, acc, f1) of the averaged model — the shadow — on a loader: the same eval forward with the descriptor pointing at
        the shadow.  No plot, no log line; the model is not touched."""
        loss, all_preds, all_labels = self._eval_pass(data_loader, shadow=True)
        return (loss,) + accuracy_and_weighted_f1(all_labels, all_preds)

    def evaluate(self, data_loader, is_test=False, is_val=False):
        loss, all_preds, all_labels = self._eval_pass(data_loader)
        acc, f1 = accuracy_and_weighted_f1(all_labels, all_preds)
        if is_test:
            self.plot_confusion_matrix(all_labels, all_preds, filename="test_confusion_matrix.png")
            self._log("\n--- 最终测试结果 (模型原始输出) ---")
            self._log(f"测试损失: {loss:.4f} | 测试Acc: {acc:.4f} | 测试F1: {f1:.4f}")
            return loss, acc, f1
        if is_val:
            return loss, acc, f1, list(all_preds), list(all_labels)
        return loss, acc, f1

    def plot_confusion_matrix(self, true_labels, pred_labels, filename="confusion_matrix.png"):
        if os.environ.get("MSIG_NO_PLOT") == "1":          # diagnostic only (tools/profile_loso.py): what the PNGs cost the LOSO wall-clock
            return
        try:
            _PLOT_LOCK.acquire()
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
            classes = np.unique(np.concatenate([true_labels, pred_labels]))
            cm = np.zeros((classes.size, classes.size), dtype=np.int64)
            for t, p in zip(true_labels, pred_labels):
                cm[np.searchsorted(classes, t), np.searchsorted(classes, p)] += 1
            names = ["Non-Stress", "Stress"] if len(np.unique(true_labels)) == 2 else ["Neutral/Baseline", "Amusement", "Stress/TSST"]
            fig, ax = plt.subplots(figsize=(8, 6))
            ax.imshow(cm, cmap="Blues")
            for i in range(cm.shape[0]):
                for j in range(cm.shape[1]):
                    ax.text(j, i, str(cm[i, j]), ha="center", va="center")
            ax.set_xticks(range(classes.size)); ax.set_yticks(range(classes.size))
            ax.set_xticklabels(names[:classes.size]); ax.set_yticklabels(names[:classes.size])
            ax.set_xlabel("Predicted Label"); ax.set_ylabel("True Label"); ax.set_title("Confusion Matrix")
            path = self.fold_dir / filename
            fig.savefig(path)
            plt.close(fig)
            self._log(f"混淆矩阵已保存至: {path}")
        except Exception as e:   # plotting must never fail a fold (trainer.py:272-273)
            self._log(f"保存混淆矩阵失败: {e}")
        finally:
            _PLOT_LOCK.release()
