"""Lockstep training of several LOSO folds as ONE fold batch (include/msig.h msig_*_multi).

The reference trains its 15 folds one after the other (main.py:98-125); each is a fresh model with its own
data split, optimiser, scheduler and early stopping.  At its batch size (64 windows) a fold's train step is ~30
launches that each occupy a few CUs, and fifteen folds on fifteen streams are bound by the command processor's
dispatch rate, not by the CUs.  Here the folds of a rank advance in lockstep: every launch of the step covers all
active folds (blockIdx.z = fold, per-fold arenas — runtime.FoldArena), one gather builds all their batches, one
device op accumulates all their losses, and there is one host sync per epoch.  Everything that is per fold in the
reference stays per fold — weights, BatchNorm statistics, shuffling order, dropout stream, learning-rate schedule,
early stopping, checkpoints, logs.  The forward GRU forms are bit-identical, so the library picks them per launch (layer 0
wave-specialised, layer 1 from 32 tiles per launch on); the BACKWARD form of a launch is by default the one a stand-alone fold of
the same batch size gets (runtime.FoldArena.multi pins msig_multi.form_folds = 1), so each fold's numbers are bit-identical to its
stand-alone run whatever its companions, the grouping or the rank count
(tests/test_trainer_gpu.py::test_lockstep_folds_equal_sequential, ::test_fold_results_do_not_depend_on_sharding); with
`adaptive_forms` the backward form follows the folds still active in a launch (a fold's last bits then depend, reproducibly, on
when its companions stop).  Folds may differ in train / val set size; folds that
stop early leave the batch.  Every train launch is msig_sc_train_step_multi, with NULL for each optional term that is off, and every
evaluation launch msig_st_forward_multi, whatever the folds have switched on: runtime's module docstring says why that is bit-safe.
With config['averaging'] every train launch is followed by one msig_wa_update_multi over the same folds (EMA; SWA: one per epoch),
each fold at its own coefficient: the shadows live in the arenas, where msig_st_forward_multi can evaluate them (include/msig_wa.h,
DESIGN.md §22).  With config['trainer']['sam'] the same launch runs two passes of all its folds, each fold's SAM state one more
region of its arena (include/msig_sam.h).  The buffers of the adversary, distillation, group-DRO and supervised
contrastive terms are side blocks of the arena set, one table (runtime.FoldArena.side).
"""
from __future__ import annotations

import ctypes as C
import json
import time
from typing import List

import numpy as np
import torch

from . import _lib as L
from . import adversary as A
from . import dro as DRO
from . import supcon as SC
from . import averaging as AV
from . import sam as SAM
from .runtime import FoldArena, _ref
from .trainer import Trainer, accuracy_and_weighted_f1, grad_clip_setting, grad_norm_summary, label_smoothing_setting


def _depth(model):
    """(gru_hidden_size, gru_num_layers) of a model: the arena form it takes (runtime.FoldArena)."""
    return int(getattr(model, "gru_hidden_size", 64)), int(getattr(model, "gru_num_layers", 2))


def _kind(model):
    """Model kind of a fold: "cnn_gru_attention" or "cnn_gru" (runtime.Engine)."""
    return getattr(model, "kind", None) or "cnn_gru_attention"


def averaged_result(prep, trainer):
    """What a fold trained with config['averaging'] adds to its result, whichever mode trained it; None without averaging.  Writes
    averaged_model.pt beside best_model.pt and evaluates the averaged model — the shadow at the end of training — on the fold's
    validation set and (when the fold has a test pass) its test set: the windows the LOSO model is evaluated on.  `loso_val_loss` is
    the LOSO model's loss (the model as `_finish_training` left it) on the same validation windows."""
    av = getattr(trainer, "averager", None)
    if av is None:
        return None
    av.bind(trainer.model.engine()).save(prep["fold_dir"] / "averaged_model.pt")
    out = av.summary()
    out["val_loss"], out["val_acc"], out["val_f1"] = trainer.evaluate_averaged(prep["loaders"][1])
    out["loso_val_loss"] = trainer.evaluate(prep["loaders"][1])[0]
    out["test_loss"], out["accuracy"], out["f1_score"] = trainer.evaluate_averaged(prep["loaders"][2]) if prep.get("test_pass", True) else (None,) * 3
    return out


def fold_result(prep, trainer, accuracy, f1_score, seconds, averaging=None):
    """The result dict of one trained fold, whichever mode trained it (main.train_fold, LockstepTrainer.run); a fold with a test
    pass of its own leaves it in fold_result.json as soon as it has finished (it survives a crash of another fold).  averaging:
    `averaged_result` of a fold trained with config['averaging'] — one more key; None adds nothing."""
    info = dict(subject=prep["subject"], accuracy=accuracy, f1_score=f1_score, seconds=seconds, epochs=len(trainer.history),
                train_windows_per_s=trainer.train_windows / max(trainer.train_seconds, 1e-9), history=trainer.history)
    if getattr(trainer, "adversary", None) is not None:      # config['adversary']: what main.write_adversary tabulates
        info["adversary_domains"] = trainer.adversary.S
    if getattr(trainer, "distill", None) is not None:        # a student (prep["distill"]): its setting beside the history's kd_* entries
        info["distillation"] = dict(alpha=trainer.distill.alpha, temperature=trainer.distill.temperature)
    if getattr(trainer, "dro", None) is not None:            # config['trainer']['group_dro']: what main's dro tables tabulate
        info["group_dro"] = DRO.fold_info(trainer.dro, prep.get("train_subjects"))
        hist = [h for h in trainer.history if h.get("dro_subject_loss") is not None]
        info["group_dro"]["subject_loss"] = hist[-1]["dro_subject_loss"] if hist else None      # per-subject mean training loss, last epoch
    if getattr(trainer, "supcon", None) is not None:         # config['trainer']['supcon']: what main's supcon tables tabulate
        info["supcon"] = SC.fold_info(trainer.supcon)
    if averaging is not None:
        info["averaging"] = averaging
    if prep.get("test_pass", True):
        (prep["fold_dir"] / "fold_result.json").write_text(json.dumps(info))
    return info


def _domains(prep):
    """Domains of a fold's subject adversary — the subjects of its training set — or None when config['adversary'] is not set."""
    if A.settings(prep["config"].get("adversary")) is None:
        return None
    return int(np.max(prep["loaders"][0].dataset.subject_ordinals)) + 1


def _dro_groups(prep):
    """(setting, G) of a fold's group-DRO term, or None when config['trainer']['group_dro'] is not set."""
    c = DRO.settings(prep["config"]["trainer"].get("group_dro"))
    if c is None:
        return None
    return (c["eta"], c["groups"], DRO.group_count(prep["loaders"][0].dataset, c["groups"], prep["model"].num_classes))


def _supcon(prep):
    """(weight, tau, positives) of a fold's supervised contrastive term, or None when config['trainer']['supcon'] is not set."""
    c = SC.settings(prep["config"]["trainer"].get("supcon"))
    return None if c is None else (c["weight"], c["tau"], c["positives"])


def _shared(values, what, show=None):
    """The one value a launch-wide setting has in every fold of a batch, else ValueError naming the values found."""
    if any(v != values[0] for v in values):
        raise ValueError(f"lockstep folds must share one {what}, got {sorted(set(values) if show is None else {show(v) for v in values})}")
    return values[0]


def lockstep_compatible(preps) -> bool:
    """Folds can share launches when they draw from one SubjectStore with one model kind and configuration and one batch size.  Their
    train / val sets may differ in size (WESAD subjects differ by a few windows, dataset.py:17-27): full batches run as one fold
    batch, the folds' ragged last batches as launches over the folds whose batch sizes agree (`launch_plan`).  The one-layer
    32-unit model has an arena form (padded, as runtime.EmbeddedEngine); a batch is uniform in depth — msig_batch.gru_layers is
    one value per launch, and so is the kind (msig_multi has no per-slot flag: msig_st.kind is the launch's)."""
    if not (1 <= len(preps) <= L.MAX_FOLDS):       # a batch of ONE fold is a fold batch too (a window's last fold, a rank's only one)
        return False
    tr0, va0, _ = preps[0]["loaders"]
    d0, k0 = _depth(preps[0]["model"]), _kind(preps[0]["model"])
    for p in preps:
        tr, va, _ = p["loaders"]
        if (_depth(p["model"]) != d0 or _kind(p["model"]) != k0
                or tr.batch_size != tr0.batch_size or va.batch_size != va0.batch_size or tr.store.data_ptr() != tr0.store.data_ptr()
                or p["model"].in_channels != preps[0]["model"].in_channels or p["model"].num_classes != preps[0]["model"].num_classes
                or p["model"].dropout_p != preps[0]["model"].dropout_p
                or _domains(p) != _domains(preps[0])         # msig_da.S is one value per launch
                or _dro_groups(p) != _dro_groups(preps[0])   # and so are msig_dro.G and eta
                or _supcon(p) != _supcon(preps[0])):          # and msig_sc.tau and positives
            return False
    return True


def launch_plan(sizes, bs):
    """The launches of one pass over datasets of `sizes` windows (non-increasing) in batches of `bs`, as (first window, batch
    size, first row, row count) records: at every step the rows that still have a batch form a prefix and their batch sizes are
    non-increasing, so the rows of equal batch size are contiguous runs — each run is one launch over those folds."""
    assert all(sizes[i] >= sizes[i + 1] for i in range(len(sizes) - 1))
    plan, k = [], 0
    while sizes and k * bs < sizes[0]:
        i, r = k * bs, 0
        while r < len(sizes) and sizes[r] > i:
            b, r1 = min(bs, sizes[r] - i), r + 1
            while r1 < len(sizes) and sizes[r1] > i and min(bs, sizes[r1] - i) == b:
                r1 += 1
            plan.append((i, b, r, r1 - r))
            r = r1
        k += 1
    return plan


class LockstepTrainer:
    def __init__(self, preps: List[dict], device, adaptive_forms: bool = False):
        self.preps, self.device = preps, torch.device(device)
        tr0, va0, te0 = preps[0]["loaders"]
        m0 = preps[0]["model"]
        self.n = len(preps)
        self.C, self.K, self.T = m0.in_channels, m0.num_classes, int(tr0.store.shape[2])
        hidden, layers = _depth(m0)
        if any(_depth(p["model"]) != (hidden, layers) for p in preps):
            raise ValueError("a fold batch is uniform in depth: msig_batch.gru_layers is one value per launch")
        self.kind = _kind(m0)
        if any(_kind(p["model"]) != self.kind for p in preps):
            raise ValueError("a fold batch is uniform in model kind: msig_multi has no per-slot kind")
        self.embedded = layers == 1
        # gradient-norm clipping (config['trainer']['max_grad_norm'], include/msig_gc.h): the arenas get a clip state only when a
        # fold asks for it; a fold of such a batch that does not is run with max_norm = inf, which is the unclipped step bit for bit
        norms = [grad_clip_setting(p["config"]["trainer"].get("max_grad_norm")) for p in preps]
        self.clip = any(v is not None for v in norms)
        # subject-adversarial training (config['adversary'], include/msig_da.h): every fold's discriminator lives in the arena set's
        # adversary block; S is the launch's, so the folds of a batch have equally many training subjects
        self.adv_S = _shared([_domains(p) for p in preps], "adversary setting and domain count", str)
        if self.adv_S is not None:
            A.check_batch_size(tr0.batch_size)
        self.dom_stats = {}
        # distillation (prep["distill"]: a distill.Distillation with the fold's teacher table, include/msig_kd.h): alpha and the
        # temperature are the launch's, so the folds of a batch share them; every fold's table lives in the arena set's own block
        self.kd_cfg = _shared([None if p.get("distill") is None else (p["distill"].alpha, p["distill"].temperature) for p in preps],
                              "distillation setting", str)
        self.kd_stats = {}
        # weight averaging (config['averaging'], include/msig_wa.h): the folds of a batch share one setting (the launches after a
        # step and the per-epoch passes are the batch's); coefficients and counters are per fold.  The shadows are arena regions.
        self.avg_cfg = _shared([AV.settings(p["config"].get("averaging")) for p in preps], "averaging setting", repr)
        self._wa_started = False
        # sharpness-aware minimisation (config['trainer']['sam'], include/msig_sam.h): rho, the form and eta are the launch's, so the
        # folds of a batch share them; every fold's state is one more region of its arena
        self.sam_cfg = _shared([SAM.setting(p["config"]["trainer"].get("sam")) for p in preps], "sam setting", repr)
        if self.sam_cfg is not None and not self.sam_cfg.on:
            self.sam_cfg = None
        if self.sam_cfg is not None and self.adv_S is not None:
            raise ValueError("config['trainer']['sam'] cannot be combined with config['adversary']")
        self.sam_stats = {}
        # group-DRO (config['trainer']['group_dro'], include/msig_dro.h): eta and G are the launch's, so the folds of a batch share
        # them; every fold's q, group table and statistics live in the arena set's own block
        self.dro_cfg = _shared([_dro_groups(p) for p in preps], "group_dro setting and group count", str)
        if self.dro_cfg is not None:
            DRO.check_batch_size(tr0.batch_size)
        self.dro_stats, self.val_worst = {}, {}
        # supervised contrastive term (config['trainer']['supcon'], include/msig_sc.h): tau and the positives are the launch's, so the
        # folds of a batch share them (and, with one configuration, the weight); every fold's subject table, scratch and statistics
        # live in the arena set's own block
        self.sc_cfg = _shared([_supcon(p) for p in preps], "supcon setting", str)
        if self.sc_cfg is not None:
            SC.check_batch_size(tr0.batch_size)
        self.sc_stats = {}
        self.arena = FoldArena(self.C, self.K, self.device, self.n, tr0.batch_size, self.T, eval_batch=max(va0.batch_size, te0.batch_size),
                               adaptive_forms=adaptive_forms, gru_hidden=hidden, gru_layers=layers, kind=self.kind, grad_clip=self.clip,
                               adversary=None if self.adv_S is None else (self.adv_S, int(tr0.store.shape[0])),
                               averaging=self.avg_cfg is not None,
                               distill=None if self.kd_cfg is None else int(tr0.store.shape[0]), sam=self.sam_cfg is not None,
                               dro=None if self.dro_cfg is None else (self.dro_cfg[2], int(tr0.store.shape[0])),
                               supcon=None if self.sc_cfg is None else int(tr0.store.shape[0]))
        if self.clip:
            for slot, v in enumerate(norms):
                self.arena.set_max_norm(slot, float("inf") if v is None else v)
        self.grad_stats = {}
        # window augmentation inside the gather (include/msig_aug.h): the training loaders carry it; a launch has ONE set of
        # parameters, so the folds of a batch must agree on them — their keys are per fold (each loader's own seed and batch count)
        self.augment = _shared([getattr(p["loaders"][0], "augment", None) for p in preps], "augmentation", repr)
        # soft targets (include/msig_st.h): label smoothing is the launch's and mixup's alpha decides how every fold's lam is drawn,
        # so the folds of a batch must agree on both; lam itself is per fold, from each loader's own seed and batch count
        self.mixup = _shared([getattr(p["loaders"][0], "mixup", None) for p in preps], "mixup alpha", repr)
        self.smoothing = _shared([label_smoothing_setting(p["config"]["trainer"].get("label_smoothing")) or 0.0 for p in preps], "label_smoothing")
        self.trainers: List[Trainer] = []
        for slot, p in enumerate(preps):
            model = p["model"]
            model._engine = self.arena.engine(slot)            # zeroed storage of arena `slot`: the model's parameters become views into it
            t = p["trainer"] = Trainer(model, p["fold_dir"], p["config"])
            model.engine()
            if self.embedded:
                model._engine.scatter()                        # into the padded layout, once: the steps train it in place
            if self.adv_S is not None:
                t.prepare_adversary(p["loaders"][0], self.arena.side_storage("adversary", slot))
            if self.kd_cfg is not None:
                t.set_distillation(p["distill"], self.arena.side_storage("distill", slot))
            t.subject_names = (p.get("train_subjects"), p.get("val_subjects"))
            if self.dro_cfg is not None:
                t.prepare_dro(p["loaders"][0], self.arena.side_storage("dro", slot))
            if self.sc_cfg is not None:
                t.prepare_supcon(p["loaders"][0], self.arena.side_storage("supcon", slot))
            self.trainers.append(t)
        # class-weighted CrossEntropy (config['trainer']['class_weights'], include/msig_cw.h): each fold's own vector — 'balanced'
        # from its own training set — in its arena; a fold without one gets all ones, which is the unweighted criterion bit for bit
        cws = [t.prepare_class_weights(p["loaders"][0]) for t, p in zip(self.trainers, preps)]
        self.cw = None
        if any(w is not None for w in cws):
            for slot, w in enumerate(cws):
                self.arena.set_class_weight(slot, np.ones(self.K) if w is None else w)
            self.cw = self.arena.ptr("cw")
        h0 = self.trainers[0].optimizer.hyper
        for t in self.trainers:
            h = t.optimizer.hyper
            if (h["betas"], h["eps"], h["weight_decay"]) != (h0["betas"], h0["eps"], h0["weight_decay"]) or t.epochs != self.trainers[0].epochs:
                raise ValueError("lockstep folds must share betas / eps / weight decay / epoch budget")
        # per-fold running sums of a pass ([sum of CE, #correct], float64): msig_batch.loss_acc of every arena, added to by the
        # loss kernel of each launch a fold takes part in — no accumulation op per launch on this side
        self.acc = self.arena.across("acc", 0, torch.float64, 2)                       # (folds, 2) strided view
        self._layouts, self._eval_orders, self._idx = {}, {}, {}

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ---- host-side bookkeeping is kept off the per-step path: descriptors, layouts and dropout keys are prepared per epoch ----
    def _layout(self, B, training, shadow=False):
        key = (B, bool(training)) + ((True,) if shadow else ())
        if key not in self._layouts:
            off = L.workspace_layout(B, self.C, self.T, self.K, training)
            self._layouts[key] = (off, self.arena.batch(B, training, self.trainers[0].model.dropout_p if training else 0.0, shadow=shadow))
        return self._layouts[key]

    def _wa_update(self, slots, coefs):
        """One msig_wa_update_multi over arenas `slots`, each fold at its own coefficient (all zero: no launch)."""
        if any(c != 0.0 for c in coefs):
            L.check(L.lib().msig_wa_update_multi(C.byref(self.arena.wa(slots, coefs)), C.byref(self.arena.multi(slots)), self._stream()),
                    "msig_wa_update_multi")

    def _gather(self, loader, order_mat, row0, i, b, m, aug=None, lam=None):
        """order_mat: (folds, n_max) int64 store positions of the pass; gathers columns i .. i+b of rows row0 .. row0+m.n.
        lam: the folds' mixup weights (a C float array; include/msig_st.h) of a training launch whose loaders augment or mix — all
        ones without mixup, which is the augmented gather itself; aug: its msig_aug (keys filled for the folds of `m`) or None.
        lam None: the plain gather, which takes any window length (C * T a multiple of 4: the float4 copy; otherwise element by
        element).  The augmenting / mixing gather needs T % 4 == 0 and refuses any other before a launch."""
        store, idx = loader.store, order_mat.data_ptr() + 8 * (row0 * order_mat.shape[1] + i)
        if lam is None:
            L.check(L.lib().msig_gather_windows_multi(store.data_ptr(), loader.store_y.data_ptr(), idx, order_mat.shape[1], b,
                                                      store.shape[1] * store.shape[2], self.arena.ptr("x"), self.arena.ptr("y"), C.byref(m),
                                                      self._stream()), "msig_gather_windows_multi")
            return
        L.check(L.lib().msig_st_gather_windows_multi(store.data_ptr(), loader.store_y.data_ptr(), idx, order_mat.shape[1], b, store.shape[1],
                                                     store.shape[2], self.arena.ptr("x"), self.arena.ptr("y"), C.byref(m),
                                                     C.byref(aug) if aug is not None else None, lam, self._stream()),
                "msig_st_gather_windows_multi")

    @staticmethod
    def _stack(rows):
        """(folds, n_max) matrix of the folds' visiting orders; short rows are padded with their own first entry (never gathered:
        a launch only covers columns every one of its rows has)."""
        n_max = max(int(r.numel()) for r in rows)
        if all(int(r.numel()) == n_max for r in rows):
            return torch.stack(rows).contiguous()
        return torch.stack([torch.cat([r, r[:1].expand(n_max - int(r.numel()))]) for r in rows]).contiguous()

    def _zero_acc(self, slots):
        """Zeroes the running sums of the given arenas only: a fold that has stopped runs its test pass on a side stream with its
        own arena's accumulator."""
        key = tuple(slots)
        if key not in self._idx:
            self._idx[key] = torch.tensor(list(slots), dtype=torch.int64, device=self.device)
        self.acc.index_fill_(0, self._idx[key], 0.0)

    def _train_epoch(self, active):
        """One epoch of every active fold.  Folds are visited in order of decreasing training-set size so that the folds of a
        launch are consecutive rows of the order matrix (`launch_plan`); which folds share a launch has no influence on any
        fold's numbers.  Returns per-arena loss sums (indexed by slot) — the epoch's only sync."""
        arena, lib = self.arena, L.lib()
        if self.clip:
            arena.zero_grad_stats(sorted(active))
        if self.sam_cfg is not None:
            arena.zero_sam_stats(sorted(active))
        act = sorted(active, key=lambda f: -len(self.preps[f]["loaders"][0].dataset))
        trs = [self.trainers[f] for f in act]
        loaders = [self.preps[f]["loaders"][0] for f in act]
        order = self._stack([ld.epoch_order() for ld in loaders])                     # (folds, n_max): one stack per epoch
        sizes, bs = [len(ld.dataset) for ld in loaders], loaders[0].batch_size
        for t in trs:
            t.model.train()
        thr = L.dropout_threshold(trs[0].model.dropout_p)
        step0 = [t.optimizer.step_count for t in trs]                                  # folds of unequal size drift apart in step count
        n_steps = [(n + bs - 1) // bs for n in sizes]
        steps = [np.arange(s0 + 1, s0 + 1 + ns) for s0, ns in zip(step0, n_steps)]
        kg = [L.dropout_keys(t.model._seed, st, 1) if thr else np.zeros(len(st), np.uint32) for t, st in zip(trs, steps)]
        kh = [L.dropout_keys(t.model._seed, st, 2) if thr else np.zeros(len(st), np.uint32) for t, st in zip(trs, steps)]
        # augmentation keys: per fold from its own loader's (seed, batches served so far), as its sequential iteration draws them
        aug = self.augment.struct() if self.augment is not None else None
        ka = [L.dropout_keys(ld.aug_seed, np.arange(ld.aug_step + 1, ld.aug_step + 1 + ns), L.AUG_STREAM_ID)
              for ld, ns in zip(loaders, n_steps)] if aug is not None else None
        # mixup weights: every fold's lam of every step of the epoch at once, keyed like the augmentation (the same counter)
        mix = self.mixup
        la = [mix.lams(ld.aug_seed, range(ld.aug_step + 1, ld.aug_step + 1 + ns)) for ld, ns in zip(loaders, n_steps)] if mix is not None else None
        # subject adversaries: every fold's lambda of every step of the epoch from its own schedule and step count
        advs = [t.adversary for t in trs] if self.adv_S is not None else None
        if advs is not None:
            dl = [[a.lam_at(a.step + 1 + k, a.total_steps) for k in range(ns)] for a, ns in zip(advs, n_steps)]
        # the optional terms that are on, by their name in the arena's table of side blocks: statistics zeroed here, read back below
        terms = [t for t, on in (("adversary", advs), ("distill", self.kd_cfg), ("dro", self.dro_cfg), ("supcon", self.sc_cfg)) if on is not None]
        for t in terms:
            arena.zero_side_stats(t, act)
        # weight averaging: EMA's coefficient of every step of the epoch per fold, from the fold's own update count
        avs = [t.averager for t in trs] if self.avg_cfg is not None else None
        ema = avs is not None and self.avg_cfg["mode"] == "ema"
        if avs is not None and not self._wa_started:          # EMA: every shadow starts as a copy of its initial model
            self._wa_started = True
            self._wa_update(act, [av.start_coef() for av in avs])
        wc = [av.peek_step_coefs(ns) for av, ns in zip(avs, n_steps)] if ema else None
        lrs = [t.optimizer.hyper["lr"] for t in trs]
        h0 = trs[0].optimizer.hyper
        b1, b2, eps, wd = h0["betas"][0], h0["betas"][1], h0["eps"], h0["weight_decay"]
        ea, eas, st = arena.ptr("exp_avg"), arena.ptr("exp_avg_sq"), self._stream()
        # per row run (r0, nr) and epoch: its msig_multi (slots, learning rates), its msig_st (smoothing, class weights, the clip)
        # and its msig_da or None; the step loop only fills keys, steps, lams, lambdas and idx.  Every launch is the widest call
        # (runtime's module docstring): with everything off it is msig_train_step_multi, bit for bit.
        runs = {}
        self._zero_acc(act)
        for i, b, r0, nr in launch_plan(sizes, bs):
            k = i // bs
            if (r0, nr) not in runs:
                sl = act[r0:r0 + nr]
                runs[(r0, nr)] = (arena.multi(sl, lr=lrs[r0:r0 + nr]),
                                  arena.soft(sl, self.smoothing, None, self.cw, arena.clip(sl, self.cw) if self.clip else None),
                                  None if advs is None else arena.da(sl, self.adv_S, [0.0] * nr, [lrs[r0 + j] * advs[r0 + j].lr_mult for j in range(nr)],
                                                                     [1] * nr, h0["betas"], eps, wd),
                                  arena.wa(sl, [0.0] * nr) if ema else None,
                                  None if self.kd_cfg is None else arena.kd(*self.kd_cfg),
                                  None if self.sam_cfg is None else arena.sam(self.sam_cfg),
                                  None if self.dro_cfg is None else arena.dro(self.dro_cfg[0]),
                                  None if self.sc_cfg is None else arena.sc(self.sc_cfg[2], self.sc_cfg[1], [self.sc_cfg[0]] * nr))
            m, s, a, w, kd, sm, dr, sc = runs[(r0, nr)]
            for j in range(nr):
                m.key_gru[j] = int(kg[r0 + j][k]); m.key_head[j] = int(kh[r0 + j][k]); m.step[j] = int(steps[r0 + j][k])
                if aug is not None:
                    aug.key[j] = int(ka[r0 + j][k])
                if mix is not None:
                    s.lam[j] = la[r0 + j][k]
                if a is not None:
                    getattr(a, "lambda")[j], a.step[j] = dl[r0 + j][k], advs[r0 + j].step + 1 + k
            self._gather(loaders[0], order, r0, i, b, m, aug, s.lam if aug is not None or mix is not None else None)
            _, desc = self._layout(b, True)
            for d in (a, kd, dr, sc if sc is not None and sc.positives else None):      # the descriptors that read by store position
                if d is not None:
                    d.idx, d.idx_row_stride = order.data_ptr() + 8 * (r0 * order.shape[1] + i), order.shape[1]
            L.check(lib.msig_sc_train_step_multi(C.byref(desc), C.byref(m), C.byref(s), _ref(a), _ref(kd), _ref(sm), _ref(dr), _ref(sc), ea, eas,
                                                 b1, b2, eps, wd, int(steps[r0][k]), st), "msig_sc_train_step_multi")
            if w is not None:                  # EMA: one launch over the same folds, each at its own coefficient
                for j in range(nr):
                    w.coef[j] = wc[r0 + j][k]
                L.check(lib.msig_wa_update_multi(C.byref(w), C.byref(m), st), "msig_wa_update_multi")
        for t, s0, ns in zip(trs, step0, n_steps):
            t.optimizer.step_count = s0 + ns
        if ema:
            for av, ns in zip(avs, n_steps):
                av.advance(ns)
        elif avs is not None:                  # SWA: the epoch-end iterate of every active fold that has reached start_epoch, one launch
            self._wa_update(act, [av.epoch_coef(len(t.history) + 1) for av, t in zip(avs, trs)])
        if aug is not None or mix is not None:
            for ld, ns in zip(loaders, n_steps):
                ld.aug_step += ns
        # the epoch's statistics of each term that is on: one more small read-back per term
        stats = {t: (arena.dro_stats() if t == "dro" else arena.side_stats(t)).cpu().numpy() for t in terms}
        if advs is not None:
            for f, a, ns, lams in zip(act, advs, n_steps, dl):
                a.step += ns
                a.last_lambda = lams[-1] if lams else a.last_lambda
                self.dom_stats[f] = a.epoch_summary(stats["adversary"][f])
        if self.kd_cfg is not None:
            for f, t in zip(act, trs):
                self.kd_stats[f] = t.distill.epoch_summary(stats["distill"][f])
        if self.dro_cfg is not None:       # every fold's statistics and weights
            self.dro_stats = {f: (stats["dro"][f, :L.DRO_STATS], stats["dro"][f, L.DRO_STATS:]) for f in act}
        if self.sc_cfg is not None:
            self.sc_stats = {f: SC.SupCon.epoch_summary(stats["supcon"][f]) for f in act}
        # the epoch's only other sync: the loss sums, with the SAM statistics and the folds' gradient-norm statistics when they are on
        parts = [self.acc[:, :1]]
        if self.sam_cfg is not None:
            parts.append(arena.across("sam", 0, torch.float64, L.SAM_NSTAT))
        if self.clip:
            parts.append(arena.across("gc", 0, torch.float64, L.GC_NSTAT))
        both = (torch.cat(parts, dim=1) if len(parts) > 1 else parts[0]).cpu().numpy()
        if self.sam_cfg is not None:
            self.sam_stats = {f: SAM.summary(both[f, 1:1 + L.SAM_NSTAT].tolist(), ns) for f, ns in zip(act, n_steps)}
        if self.clip:
            st4 = both[:, -L.GC_NSTAT:]
            self.grad_stats = {f: grad_norm_summary(dict(sum=float(st4[f, L.GC_SUM]), max=float(st4[f, L.GC_MAX]),
                                                         clipped=int(st4[f, L.GC_CLIPPED])), ns)
                               for f, ns in zip(act, n_steps) if self.trainers[f].max_grad_norm is not None}
        return both[:, 0]

    def _evaluate(self, active, which, shadow=False):
        """Validation pass of every active fold (loader index `which`): per fold (loss, acc, f1), in the order of `active`.  shadow:
        the same pass under the folds' weight-averaging shadows (the descriptor points at the "avg_*" regions), with its own
        accumulator zeroing and read-back."""
        arena, lib = self.arena, L.lib()
        act = sorted(active, key=lambda f: -len(self.preps[f]["loaders"][which].dataset))
        loaders = [self.preps[f]["loaders"][which] for f in act]
        for f in act:
            self.trainers[f].model.eval()
        key = (which, tuple(act))
        if key not in self._eval_orders:                   # validation order is fixed (no shuffling): stack it once per active set
            self._eval_orders = {key: self._stack([ld.epoch_order() for ld in loaders])}
        order = self._eval_orders[key]
        sizes, bs = [len(ld.dataset) for ld in loaders], loaders[0].batch_size
        st = self._stream()
        runs = {}
        self._zero_acc(act)
        preds = [[] for _ in act]
        for i, b, r0, nr in launch_plan(sizes, bs):
            if (r0, nr) not in runs:           # the criterion's label smoothing applies to validation losses too; evaluation never mixes
                runs[(r0, nr)] = (arena.multi(act[r0:r0 + nr]), arena.soft(act[r0:r0 + nr], self.smoothing, None, self.cw))
            m, s = runs[(r0, nr)]
            self._gather(loaders[0], order, r0, i, b, m)
            off, desc = self._layout(b, False, shadow)
            L.check(lib.msig_st_forward_multi(C.byref(desc), C.byref(m), C.byref(s), st), "msig_st_forward_multi")
            got = arena.across("ws", off[L.WS["PRED"]], torch.int32, b)[act[r0:r0 + nr]]      # (folds of the launch, b) copy
            for j in range(nr):
                preds[r0 + j].append(got[j])
        sums = self.acc[:, 0].cpu().numpy()
        out = {}
        for j, f in enumerate(act):
            ds = loaders[j].dataset
            pred = torch.cat(preds[j]).cpu().numpy().astype(np.int64)
            acc, f1 = accuracy_and_weighted_f1(np.asarray(ds.labels).astype(np.int64), pred)
            out[f] = (float(sums[f]) / len(ds), acc, f1)
            if which == 1 and not shadow and self.dro_cfg is not None:
                self.val_worst[f] = self.trainers[f].val_worst_subject(loaders[j], pred, np.asarray(ds.labels).astype(np.int64))
        return [out[f] for f in active]

    def run(self, t_start: float = None):
        """Trains every fold to its early stop (or the epoch budget), then evaluates each on its test subject; returns the folds'
        `fold_result` dicts in position order.  A budget of 0 epochs takes every fold straight to its test pass."""
        from concurrent.futures import ThreadPoolExecutor
        for t, p in zip(self.trainers, self.preps):
            for ld in p["loaders"]:
                t._check_labels(ld)
        t_start = time.time() if t_start is None else t_start
        dev = self.device

        def finish(f):
            """Checkpoint restore, test pass, confusion matrix, fold_result.json of one fold — on a side stream, off the
            lockstep loop's critical path (a stopped fold's arena is no longer touched by the batch)."""
            t, p = self.trainers[f], self.preps[f]
            torch.cuda.set_device(dev)
            test = p.get("test_pass", True)       # False: the caller evaluates the model itself (main.run_hierarchical_experiment)
            with torch.cuda.stream(torch.cuda.Stream(dev)):
                if self.embedded:
                    t.model._engine.gather()       # the trained padded layout -> the model's reference-shaped parameters
                t._finish_training()
                acc, f1 = t.evaluate(p["loaders"][2], is_test=True)[1:] if test else (None, None)
                torch.cuda.current_stream(dev).synchronize()
            return fold_result(p, t, acc, f1, getattr(t, "finished_at", time.time() - t_start))

        active = list(range(self.n))
        n_train = [len(p["loaders"][0].dataset) for p in self.preps]
        pending = {}
        with ThreadPoolExecutor(max_workers=2) as side:
            for epoch in range(self.trainers[0].epochs):               # the batch's budget: its folds share it (__init__)
                if not active:
                    break
                t0 = time.time()
                sums = self._train_epoch(active)
                dt = time.time() - t0
                vals = self._evaluate(active, 1)
                avg_vals = self._validate_averaged(active)
                still = []
                for (vl, va, vf), f in zip(vals, active):
                    t = self.trainers[f]
                    if self.embedded:
                        t.model._engine.gather()   # once per epoch, for the checkpoint early stopping may write (best_model.pt)
                    t.train_windows += n_train[f]
                    t.train_seconds += dt
                    if not t._end_of_epoch(epoch, float(sums[f]) / n_train[f], dt, n_train[f], vl, va, vf, self.grad_stats.get(f), self.dom_stats.get(f),
                                           avg_vals.get(f), self.kd_stats.get(f), self.sam_stats.get(f),
                                           None if self.dro_cfg is None else t.dro_epoch(*self.dro_stats[f], self.val_worst.get(f)),
                                           self.sc_stats.get(f)):
                        still.append(f)
                    else:
                        t.finished_at = time.time() - t_start
                        self._finish_averaging([f])
                        torch.cuda.current_stream(dev).synchronize()       # its last launches are done before the side stream reads
                        pending[f] = side.submit(finish, f)
                active = still
            torch.cuda.current_stream(dev).synchronize()
            self._finish_averaging(active)
            torch.cuda.current_stream(dev).synchronize()
            for f in active:                                               # ran out of epochs without an early stop
                pending[f] = side.submit(finish, f)
            results = [pending[f].result() for f in range(self.n)]
        return self._averaged_results(results)

    # ---- weight averaging (config['averaging']) ------------------------------------------------------------------------------------
    def _validate_averaged(self, active) -> dict:
        """config['averaging']['validate']: {fold: the three history entries of the epoch's validation pass under the shadow};
        None values for an SWA fold that has no iterate yet.  Empty without it."""
        if self.avg_cfg is None or not self.avg_cfg["validate"]:
            return {}
        ready = [f for f in active if self.trainers[f].averager.ready]
        out = {f: dict(val_loss_avg=None, val_acc_avg=None, val_f1_avg=None) for f in active}
        if ready:
            for f, (vl, va, vf) in zip(ready, self._evaluate(ready, 1, shadow=True)):
                out[f] = dict(val_loss_avg=vl, val_acc_avg=va, val_f1_avg=vf)
        return out

    def _finish_averaging(self, folds):
        """End of training of `folds`, before their checkpoints are restored: an SWA fold without an iterate takes the weights the
        last step left as its single one (one launch over those folds)."""
        if self.avg_cfg is None or not folds:
            return
        self._wa_update(list(folds), [self.trainers[f].averager.final_coef() for f in folds])

    def _averaged_results(self, results):
        """After every fold has finished: bn = "recompute" for all folds of the batch as ONE adapter, then each fold's averaged
        model — averaged_model.pt, its validation and test passes — into its result (and its fold_result.json)."""
        if self.avg_cfg is None:
            return results
        if self.avg_cfg["bn"] == "recompute":
            AV.recompute_bn([t.model.engine() for t in self.trainers], [p["loaders"][0] for p in self.preps])
        for p, t, info in zip(self.preps, self.trainers, results):
            info["averaging"] = averaged_result(p, t)
            if p.get("test_pass", True):
                (p["fold_dir"] / "fold_result.json").write_text(json.dumps(info))
        return results
