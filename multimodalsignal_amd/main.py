"""LOSO experiment driver — the reference's ``main.py`` (run_simple_experiment,
main.py:91-156) with the 15 folds sharded over the GPUs of one node.

    python -m multimodalsignal_amd.main --data ./data/chest_raw                 # 1 GPU
    python -m torch.distributed.run --nproc-per-node 8 -m multimodalsignal_amd.main --data ...
    python -m multimodalsignal_amd.main --synthetic /tmp/wesad_synth             # no dataset needed

Same module-level constants as the reference (edit them or use the flags), same fold
directories / ``cv_summary.txt``.  Differences, all deliberate: every fold gets an explicit
seed (SEED + fold index) because a sharded run cannot share one global RNG stream
(SURVEY.md §5.1-7); data live in HBM (DeviceLoader); rank 0 writes the summary after one
RCCL all_gather of the per-fold metrics.  The hierarchical experiment (main.py:159-247), which the
reference cannot run itself, is run_hierarchical_experiment / --hierarchical.
"""
from __future__ import annotations

import argparse
import json
import os
import threading
import time
import warnings
from datetime import datetime
from operator import itemgetter
from pathlib import Path

import numpy as np
import torch

from . import _lib as L
from .augment import Augment
from .mixup import Mixup
from . import adversary as adversary_mod
from . import dro as dro_mod
from . import supcon as supcon_mod
from . import averaging as averaging_mod
from .dataset import DeviceLoader, SubjectStore, WesadDataset, parse_reference, reference_mask, running_norm_reference
from . import distill as distill_mod
from . import sam as sam_mod
from . import ensemble as ensemble_mod
from .loso import folds_for_rank, gather_fold_metrics, split_train_val
from .models import CnnGruAttentionModel, CnnGruModel
from .multifold import averaged_result, fold_result, lockstep_compatible
from .trainer import Trainer, grad_clip_setting, label_smoothing_setting
from .waves import MAX_TRAIN_STREAMS, cap_waves, chunk_schedule, deal, on_streams, run_wave  # noqa: F401  (the first three: importable from here)

warnings.filterwarnings("ignore", message="Initializing zero-element tensors is a no-op")

# ---- configuration (main.py:20-67) -------------------------------------------------------------
RUN_NAME = "simple_binary"
CLASSIFICATION_MODE = "stress_binary"
NUM_CLASSES = 2
MODEL_TO_USE = "cnn_gru_attention"
CHANNELS_TO_USE = ["chest_ECG", "chest_EDA", "chest_Resp"]
# 'cnn_gru': the baseline the reference's README names (README.md:13,81) and its models.py never defines (models.CnnGruModel)
MODEL_PARAMS = {"cnn_gru_attention": {"cnn_out_channels": 32, "gru_hidden_size": 64, "gru_num_layers": 2, "dropout": 0.5},
                "cnn_gru": {"cnn_out_channels": 32, "gru_hidden_size": 64, "gru_num_layers": 2, "dropout": 0.5}}
MODEL_CLASSES = {"cnn_gru_attention": CnnGruAttentionModel, "cnn_gru": CnnGruModel}
PROCESSED_DATA_PATH = Path("./data")
EARLY_DATA_PATH = PROCESSED_DATA_PATH / "chest_raw"
SEED = 42
NUM_WORKERS = 0
EPOCHS = 100
BATCH_SIZE = 64
LEARNING_RATE = 0.001
PATIENCE = 20
WEIGHTS_DECAY = 1e-4
ALL_SUBJECTS = [f"S{i}" for i in range(2, 18) if i != 12]
# Batch size of the validation / test passes.  The reference evaluates in batches of BATCH_SIZE (main.py:113-114); evaluation runs in
# eval mode (running BatchNorm statistics, no dropout), so every window's logits — and with them accuracy, F1 and the confusion matrix —
# are the same whatever the batching; only the summation order of the reported loss changes (~1e-7 relative).  One launch sequence
# over a subject's ~270 windows instead of five is what the latency-bound B = 64 regime wants (0 = BATCH_SIZE, the reference's loaders).
EVAL_BATCH_SIZE = 1024
# Class-weighted CrossEntropyLoss (include/msig_cw.h): "none" (the reference's effective criterion — its use_class_weights branch
# cannot run, trainer.py:81) or "balanced" (compute_class_weight('balanced') over each model's own training labels, trainer.py:85-89).
CLASS_WEIGHTS = "none"


def model_kind(cfg):
    """cfg["model"]: the model kind of a configuration ("cnn_gru_attention" when absent)."""
    return cfg.get("model", MODEL_TO_USE)


def make_model(cfg, in_channels, num_classes, params):
    return MODEL_CLASSES[model_kind(cfg)](in_channels=in_channels, num_classes=num_classes, **params)


def trainer_class_weights(cfg):
    """cfg["class_weights"] as config['trainer']['class_weights']: None for "none"."""
    v = cfg.get("class_weights", CLASS_WEIGHTS)
    return None if v is None or (isinstance(v, str) and v == "none") else v


def trainer_config(cfg, fold_idx):
    """config['trainer'] of the Trainer of fold `fold_idx` (main.py:60-67), every experiment's."""
    pat = cfg["patience"]
    if isinstance(pat, (list, tuple)):       # a per-fold cycle of patiences (tests: folds that stop at different epochs); an int as in main.py:66
        pat = int(pat[fold_idx % len(pat)])
    tc = {"trainer": {"epochs": cfg["epochs"], "learning_rate": cfg["lr"],
                      "early_stopping": {"enabled": True, "patience": pat, "delta": 0},
                      "weight_decay": cfg["weight_decay"], "verbose": cfg.get("verbose", False)}}
    if trainer_class_weights(cfg) is not None:      # each model's from its own training labels (M1's stress_binary, M2's amusement_binary)
        tc["trainer"]["class_weights"] = trainer_class_weights(cfg)
    if cfg.get("max_grad_norm") is not None:        # clip_grad_norm_ inside the fused step (include/msig_gc.h); absent = the unclipped step
        tc["trainer"]["max_grad_norm"] = grad_clip_setting(cfg["max_grad_norm"])
    if cfg.get("label_smoothing") is not None:      # CrossEntropyLoss(label_smoothing=) of every loss (include/msig_st.h); absent = hard labels
        tc["trainer"]["label_smoothing"] = label_smoothing_setting(cfg["label_smoothing"])
    if cfg.get("sam") is not None:                  # sharpness-aware train steps (include/msig_sam.h); absent = the plain step
        tc["trainer"]["sam"] = sam_mod.setting(cfg["sam"]).spec()
    if cfg.get("group_dro") is not None:            # group-DRO over the training subjects (include/msig_dro.h); absent = the pooled mean
        tc["trainer"]["group_dro"] = dro_mod.settings(cfg["group_dro"])
    if cfg.get("supcon") is not None:               # supervised contrastive loss on the feature (include/msig_sc.h); absent = none
        tc["trainer"]["supcon"] = supcon_mod.settings(cfg["supcon"])
    if cfg.get("adversary") is not None:            # a subject discriminator inside every training step (include/msig_da.h); absent = none
        tc["adversary"] = adversary_mod.settings(cfg["adversary"])
    if cfg.get("averaging") is not None:            # an EMA / SWA shadow of the weights (include/msig_wa.h); absent = none
        tc["averaging"] = averaging_mod.settings(cfg["averaging"])
    return tc


def adversary_line(cfg):
    """The SUBJECT ADVERSARY line of a summary, or None when the configuration has none."""
    a = adversary_mod.settings(cfg.get("adversary"))
    if a is None:
        return None
    return f"SUBJECT ADVERSARY: lambda={a['lam']:g} schedule={a['schedule']} gamma={a['gamma']:g} lr_mult={a['lr_mult']:g}\n"


def soft_targets_line(cfg):
    """The SOFT TARGETS line of a summary, or None when neither label smoothing nor mixup is set."""
    ls, mix = cfg.get("label_smoothing"), Mixup.coerce(cfg.get("mixup"))
    if ls is None and mix is None:
        return None
    parts = ([f"label_smoothing={ls:g}"] if ls is not None else []) + ([f"mixup_alpha={mix.alpha:g}"] if mix is not None else [])
    return "SOFT TARGETS: " + " ".join(parts) + "\n"


def norm_reference(cfg):
    """cfg["norm_reference"]: which windows supply each subject's normalisation statistics ("subject" when absent)."""
    return cfg.get("norm_reference", "subject")


def host_datasets(cfg, all_channel_names, cache, channels, mode):
    """The dataset factory over host arrays: subjects -> WesadDataset (`cache`: one dict shared by the datasets of a run)."""
    return lambda subjects: WesadDataset(cfg["data_path"], subjects, channels, all_channel_names, classification_mode=mode, cache=cache,
                                         reference=norm_reference(cfg))


def make_unit(fold_idx, subject, fold_dir, datasets, in_channels, num_classes, params, seed, cfg, device, shuffle=True, test_pass=True,
              skip_empty=False):
    """One training unit — a fold's model with its loaders and trainer configuration — as the `prep` dict train_fold and
    multifold.LockstepTrainer consume.  Everything of a unit that touches global state (RNG seeding, model initialisation, host
    data) happens here: the drivers call it sequentially, in the main thread, so that concurrent units stay deterministic.
    `datasets(subjects)` is the dataset factory (host_datasets, or SubjectStore.view: index subsets of one HBM-resident store);
    `seed` seeds torch for the model's initialisation, the model's dropout stream and the training loader's shuffler.
    test_pass False: whoever trains the unit leaves the test subject to the caller.  skip_empty: None for a unit whose training
    or validation set is empty (main.py:187-189)."""
    train_subjects, val_subjects = split_train_val(cfg["subjects"], subject, cfg["seed"])
    if cfg.get("adversary") is not None:            # before any data is loaded: the discriminator's step takes at most 256 rows
        adversary_mod.check_batch_size(cfg["batch_size"])
    if cfg.get("group_dro") is not None:            # likewise: the term's launch takes at most 2048 rows, and a blended row has no group
        dro_mod.check_batch_size(cfg["batch_size"])
        if Mixup.coerce(cfg.get("mixup")) is not None:
            raise ValueError("group_dro cannot be combined with mixup: a row blended from two subjects has no group")
    if cfg.get("supcon") is not None:               # likewise: at most 2048 rows, and a blended row has no label to contrast
        supcon_mod.check_batch_size(cfg["batch_size"])
        if Mixup.coerce(cfg.get("mixup")) is not None:
            raise ValueError("supcon cannot be combined with mixup: a row blended from two windows has no label to contrast")
    train_ds, val_ds = datasets(train_subjects), datasets(val_subjects)
    if skip_empty and (len(train_ds) == 0 or len(val_ds) == 0):
        return None
    fold_dir.mkdir(parents=True, exist_ok=True)
    torch.manual_seed(seed)
    # Evaluation runs in eval mode (running BN statistics, no dropout), so its predictions do not depend on how the
    # windows are batched; only the summation order of the reported loss does (~1e-7 relative).
    ebs = int(cfg.get("eval_batch_size") or cfg["batch_size"])
    # cfg["augment"] (--augment SPEC, include/msig_aug.h): the TRAINING loader's gather augments; validation and test never do
    # cfg["mixup"] (--mixup ALPHA, include/msig_st.h): likewise the training loader's gather alone mixes
    loaders = (DeviceLoader(train_ds, cfg["batch_size"], shuffle, device, seed=seed, augment=Augment.coerce(cfg.get("augment")),
                            mixup=Mixup.coerce(cfg.get("mixup"))),
               DeviceLoader(val_ds, ebs, False, device), DeviceLoader(datasets([subject]), ebs, False, device))
    model = make_model(cfg, in_channels, num_classes, params)
    model.set_dropout_seed(seed * 0x9E3779B97F4A7C15 + 12345)
    return dict(fold=fold_idx, subject=subject, fold_dir=fold_dir, loaders=loaders, model=model, config=trainer_config(cfg, fold_idx),
                test_pass=test_pass, train_subjects=list(train_subjects), val_subjects=list(val_subjects))


def prepare_fold(fold_idx, subject_to_test, run_output_dir, device, all_channel_names, cfg, cache=None):
    """The unit of fold `fold_idx` of the simple experiment (make_unit): seed SEED + fold index — seed replica cfg["replica"] of a
    --seeds run: ensemble.replica_seed, the split stays SEED's — `cache` a SubjectStore (one HBM-resident store for the whole run) or
    the host cache of WesadDataset."""
    datasets = cache.view if isinstance(cache, SubjectStore) else host_datasets(cfg, all_channel_names, cache, cfg["channels"], cfg["mode"])
    # cfg["shuffle"] = False: training batches in dataset order (with dropout 0 the run is deterministic up to rounding — the
    # setting tests/test_accuracy_parity_gpu.py compares fold by fold with the reference's CPU run); default as main.py:112
    return make_unit(fold_idx, subject_to_test, Path(run_output_dir) / f"fold_test_on_{subject_to_test}", datasets, len(cfg["channels"]),
                     cfg["num_classes"], cfg["model_params"], ensemble_mod.replica_seed(cfg["seed"], fold_idx, cfg.get("replica", 0)), cfg, device,
                     shuffle=bool(cfg.get("shuffle", True)))


def train_fold(prep, device):
    """The reference's per-fold body (main.py:116-125) on the current HIP stream.  prep["test_pass"] False: no test pass — the
    caller evaluates the trained model itself (run_hierarchical_experiment).  prep["distill"]: a distill.Distillation with the
    fold's teacher table — the fold trains as a student, as a fold batch of such preps does."""
    train_loader, val_loader, test_loader = prep["loaders"]
    trainer = prep["trainer"] = Trainer(prep["model"], prep["fold_dir"], prep["config"])
    if prep.get("distill") is not None:
        trainer.set_distillation(prep["distill"])
    trainer.subject_names = (prep.get("train_subjects"), prep.get("val_subjects"))      # named in the group-DRO log entries
    t0 = time.time()
    trainer.train(train_loader, val_loader)
    acc, f1 = trainer.evaluate(test_loader, is_test=True)[1:] if prep.get("test_pass", True) else (None, None)
    seconds = time.time() - t0
    return fold_result(prep, trainer, acc, f1, seconds, averaged_result(prep, trainer))      # config['averaging']: the averaged model's passes


def run_fold(fold_idx, subject_to_test, run_output_dir, device, all_channel_names, cfg, cache=None):
    """One iteration of the reference's fold loop (main.py:99-125)."""
    return train_fold(prepare_fold(fold_idx, subject_to_test, run_output_dir, device, all_channel_names, cfg, cache), device)


def write_summary(run_output_dir, results, cfg, wall_s, world):
    accs = [r["accuracy"] for r in results]
    f1s = [r["f1_score"] for r in results]
    path = Path(run_output_dir) / "cv_summary.txt"
    with open(path, "w", encoding="utf-8") as f:
        f.write("实验配置:\n")
        kind = model_kind(cfg)
        for k, v in (("MODEL_TO_USE", kind), ("RUN_NAME", RUN_NAME), ("SEED", cfg["seed"]), ("CHANNELS_TO_USE", cfg["channels"]),
                     ("EPOCHS", cfg["epochs"]), ("BATCH_SIZE", cfg["batch_size"]), ("LEARNING_RATE", cfg["lr"]),
                     ("NUM_WORKERS", NUM_WORKERS), ("PATIENCE", cfg["patience"]), ("NUM_CLASSES", cfg["num_classes"]),
                     ("MODEL_PARAMS", {kind: cfg["model_params"]})):
            f.write(f"{k}: {v}\n")
        if trainer_class_weights(cfg) is not None:                  # named only when set: summaries of unweighted runs are unchanged
            f.write(f"CLASS_WEIGHTS: {trainer_class_weights(cfg)}\n")
        if cfg.get("max_grad_norm") is not None:                    # likewise
            f.write(f"MAX_GRAD_NORM: {cfg['max_grad_norm']:g}\n")
        if cfg.get("sam") is not None:                              # likewise
            f.write(f"SAM: {cfg['sam']}\n")
        if cfg.get("augment") is not None:                          # likewise
            f.write(f"AUGMENT: {Augment.coerce(cfg['augment']).spec()}\n")
        if soft_targets_line(cfg) is not None:                      # likewise
            f.write(soft_targets_line(cfg))
        if adversary_line(cfg) is not None:                         # likewise
            f.write(adversary_line(cfg))
        if cfg.get("group_dro") is not None:                        # likewise
            f.write(dro_mod.settings_line(cfg["group_dro"]) + "\n")
        if cfg.get("supcon") is not None:                           # likewise
            f.write(supcon_mod.settings_line(cfg["supcon"]) + "\n")
        if cfg.get("averaging") is not None:                        # likewise
            f.write(averaging_mod.settings_line(cfg["averaging"]) + "\n")
        if cfg.get("norm_reference") is not None:                   # likewise
            f.write(f"NORM_REFERENCE: {cfg['norm_reference']}\n")
        f.write("\n每个折叠的详细结果:\n")
        for r in results:
            f.write(f"  - 测试 {r['subject']}: Accuracy = {r['accuracy']:.4f}, F1-score = {r['f1_score']:.4f}\n")
        f.write("\n最终平均性能:\n")
        f.write(f"平均准确率 (Accuracy): {np.mean(accs):.4f} ± {np.std(accs):.4f}\n")
        f.write(f"平均 F1 分数 (Weighted F1-score): {np.mean(f1s):.4f} ± {np.std(f1s):.4f}\n")
        f.write(f"\nLOSO wall-clock: {wall_s:.1f} s on {world} GPU(s)\n")
    return path


def _windows(prep, loader=2, idx=None, labels=True):
    """(x, y, pos) of one of a prep's loaders — 2, the TEST subject's, or 0, the training subjects' — on the device, in store order;
    pos their store positions.  idx: positions within that order to take instead of all of them.  labels=False: y is None."""
    ld = prep["loaders"][loader]
    pos = ld.index if ld.index is not None else torch.arange(len(ld.dataset), device=ld.store.device)
    if idx is not None:
        pos = pos[torch.as_tensor(idx, device=pos.device)]
    return ld.store.index_select(0, pos), ld.store_y.index_select(0, pos) if labels else None, pos


def _tag(name):
    """What a unit's printed lines put before "fold": the configuration's name and a slash, nothing for the unnamed one."""
    return f"{name}/" if name else ""


def _fold_batches(kept, units, cfgs):
    """(configuration name, its cfg, chunk of at most MAX_FOLDS units) over the kept units in unit order, grouped by configuration in
    order of first appearance: what calibrates or adapts as one fold batch."""
    by_cfg = {}
    for u in sorted(kept):
        by_cfg.setdefault(units[u][0], []).append(u)
    for n, us in by_cfg.items():
        for c0 in range(0, len(us), L.MAX_FOLDS):
            yield n, cfgs[n], us[c0:c0 + L.MAX_FOLDS]


def calibration_settings(cfg):
    """The calibration settings of a configuration (--calibrate ...), as calibration.txt / calibration.json name them."""
    from .calibrate import DEFAULT_EPOCHS, DEFAULT_GAP
    lr = cfg.get("calibration_lr")
    return {"windows_per_class": int(cfg.get("calibrate") or 0), "gap": int(cfg.get("calibration_gap", DEFAULT_GAP)),
            "epochs": int(cfg.get("calibration_epochs", DEFAULT_EPOCHS)), "lr": float(cfg["lr"] if lr is None else lr),
            "batch_size": int(cfg["batch_size"]), "weight_decay": float(cfg["weight_decay"])}


def calibrate_units(kept, units, cfgs, device, rank=0):
    """Few-shot subject calibration of the rank's finished folds (calibrate.HeadCalibrator): per fold the first --calibrate windows
    per class of the TEST subject re-fit the classifier of the fold's model (the one its test pass evaluated) on frozen features; the
    LOSO model and the calibrated head are then evaluated on the same remainder.  All folds of a configuration calibrate as one
    fold batch — one launch per epoch (cfg["calibration_batched"] False: one launch per fold and epoch, the same bits).  The models,
    best_model.pt, fold_result.json and the LOSO summary are untouched; each fold directory gets calibration_result.json.
    Returns {unit: ((acc, f1) before, (acc, f1) after, (n_cal, n_eval))}."""
    from .calibrate import HeadCalibrator, calibration_split
    out = {}
    for n, cfg, chunk in _fold_batches(kept, units, cfgs):
        st, jobs = calibration_settings(cfg), []
        for u in chunk:
            p = kept[u]
            loader, model = p["loaders"][2], p["model"]
            labels = np.asarray(loader.dataset.labels).astype(np.int64)
            try:
                cal_idx, eval_idx = calibration_split(labels, st["windows_per_class"], st["gap"])
            except ValueError as e:
                raise ValueError(f"--calibrate {st['windows_per_class']}: test subject {p['subject']}: {e}") from None
            (xc, yc, _), (xe, ye, _) = _windows(p, idx=cal_idx), _windows(p, idx=eval_idx)
            cw = p["trainer"].class_weight if p.get("trainer") is not None else None
            fold_seed = cfg["seed"] + p["fold"]
            jobs.append(dict(model=model, x_cal=xc, y_cal=yc, x_eval=xe, y_eval=ye, lr=st["lr"],
                             seed=(model._seed ^ 0xCA11B8A7E) % (1 << 64), shuffle_seed=fold_seed + 7919,
                             class_weight=None if cw is None else cw.cpu().numpy()))
        cal = HeadCalibrator(jobs, epochs=st["epochs"], batch_size=st["batch_size"], weight_decay=st["weight_decay"],
                             batched=bool(cfg.get("calibration_batched", True)), eval_batch=kept[chunk[0]]["loaders"][2].batch_size)
        for u, r in zip(chunk, cal.run()):
            p = kept[u]
            r = dict(subject=p["subject"], settings=st, **r)
            (p["fold_dir"] / "calibration_result.json").write_text(json.dumps(r))
            print(f"[rank {rank}] {_tag(n)}fold {p['fold']} ({p['subject']}) calibration on {r['n_cal']} windows, remainder {r['n_eval']}: "
                  f"acc {r['before']['accuracy']:.4f} -> {r['after']['accuracy']:.4f}  f1 {r['before']['f1_score']:.4f} -> "
                  f"{r['after']['f1_score']:.4f}", flush=True)
            out[u] = ((r["before"]["accuracy"], r["before"]["f1_score"]), (r["after"]["accuracy"], r["after"]["f1_score"]),
                      (float(r["n_cal"]), float(r["n_eval"])))
    return out


def adaptation_settings(cfg):
    """The adaptation settings of a configuration (--adapt-bn ...), as adaptation.txt / adaptation.json name them."""
    return {"alpha": float(cfg.get("adapt_bn", 1.0))}


def adapt_units(kept, units, cfgs, device, rank=0):
    """Label-free BatchNorm adaptation of the rank's finished folds (adapt.BnAdapter): per fold the running statistics of the fold's
    model (the one its test pass evaluated) are re-estimated on the TEST subject's windows, labels unread, and the LOSO model and the
    adapted one are evaluated on those same windows.  All folds of a configuration adapt as one fold batch
    (cfg["adapt_bn_batched"] False: single calls, the same bits).  The models, best_model.pt, fold_result.json and the LOSO summary
    are untouched; each fold directory gets adaptation_result.json.
    Returns {unit: ((acc, f1) before, (acc, f1) after, (n, 0.0))}."""
    from .adapt import BnAdapter
    out = {}
    for n, cfg, chunk in _fold_batches(kept, units, cfgs):
        st, jobs = adaptation_settings(cfg), []
        for u in chunk:
            x, y, _ = _windows(kept[u])
            jobs.append(dict(model=kept[u]["model"], x=x, y=y))
        ad = BnAdapter(jobs, alpha=st["alpha"], batched=bool(cfg.get("adapt_bn_batched", True)),
                       eval_batch=kept[chunk[0]]["loaders"][2].batch_size)
        for u, r in zip(chunk, ad.run()):
            p = kept[u]
            r = dict(subject=p["subject"], settings=st, **r)
            (p["fold_dir"] / "adaptation_result.json").write_text(json.dumps(r))
            print(f"[rank {rank}] {_tag(n)}fold {p['fold']} ({p['subject']}) BatchNorm adaptation on {r['n']} unlabelled windows: "
                  f"acc {r['before']['accuracy']:.4f} -> {r['after']['accuracy']:.4f}  f1 {r['before']['f1_score']:.4f} -> "
                  f"{r['after']['f1_score']:.4f}", flush=True)
            out[u] = ((r["before"]["accuracy"], r["before"]["f1_score"]), (r["after"]["accuracy"], r["after"]["f1_score"]),
                      (float(r["n"]), 0.0))
    return out


def entropy_units(kept, units, cfgs, device, rank=0):
    """Label-free entropy-minimisation adaptation of the rank's finished folds (tta.EntropyAdapter): per fold the selected tensors of
    a COPY of the fold's model (the one its test pass evaluated) descend the entropy of its own predictions on the TEST subject's
    windows, labels unread by the objective, and the LOSO model and the adapted one are evaluated on those same windows.  With
    --adapt-bn also given the adaptation starts from the AdaBN statistics (an adapt.BnAdapter of its own, the flag's alpha) and the
    record has the AdaBN column too.  All folds of a configuration adapt as one fold batch (cfg["adapt_entropy_batched"] False:
    single calls, the same bits).  The models, best_model.pt, fold_result.json and the LOSO summary are untouched; each fold
    directory gets entropy_adaptation_result.json.  Returns the units adapted."""
    from . import tta
    from .adapt import BnAdapter
    done = []
    for n, cfg, chunk in _fold_batches(kept, units, cfgs):
        st, jobs = tta.settings_of(cfg), []
        for u in chunk:
            x, y, _ = _windows(kept[u])
            jobs.append(dict(model=kept[u]["model"], x=x, y=y))
        eval_batch = kept[chunk[0]]["loaders"][2].batch_size
        bn = None
        if cfg.get("adapt_bn") is not None:
            bn = BnAdapter([dict(model=j["model"], x=j["x"]) for j in jobs], alpha=float(cfg["adapt_bn"]), eval_batch=eval_batch)
            for i, j in enumerate(jobs):
                j["bn_state"] = bn.adapted_state(i).clone()
        ad = tta.EntropyAdapter(jobs, lr=st["lr"], epochs=st["epochs"], diversity=st["diversity"], batch=st["batch"], params=st["params"],
                                seed=st["seed"], order=st["order"], batched=bool(cfg.get("adapt_entropy_batched", True)), eval_batch=eval_batch)
        for u, r in zip(chunk, ad.run()):
            p = kept[u]
            r = dict(subject=p["subject"], settings=st, **r)
            (p["fold_dir"] / "entropy_adaptation_result.json").write_text(json.dumps(r))
            mid = f" -> {r['start']['accuracy']:.4f} (AdaBN)" if "start" in r else ""
            print(f"[rank {rank}] {_tag(n)}fold {p['fold']} ({p['subject']}) entropy adaptation on {r['n']} unlabelled windows: "
                  f"acc {r['before']['accuracy']:.4f}{mid} -> {r['after']['accuracy']:.4f}  entropy {r['entropy']['before']:.4f} -> "
                  f"{r['entropy']['after']:.4f}  {r['flipped']} predictions flipped", flush=True)
            done.append(u)
    return done


def attribution_settings(cfg):
    """The attribution settings of a configuration (--attribute ...), as attribution.txt / attribution.json name them; the bin is
    the flag's, else one second of a 60-second window of T samples (None while T is not known)."""
    out = {"steps": int(cfg["attribute"]), "baseline": "zero", "target": "predicted"}
    if cfg.get("attribute_bin") is not None:
        out["bin"] = int(cfg["attribute_bin"])
    return out


def attribute_units(kept, units, cfgs, device, rank=0):
    """Integrated-gradients attribution of the rank's finished folds (attribute.fold_attribution): per fold, from the model the fold
    trained (the one its test pass evaluated) and the TEST subject's windows — which channels and which seconds of the window the
    predicted class rests on, the gate's values and the forward-only channel-occlusion drops.  One model at a time: a path batch
    fills the chip on its own.  The models, best_model.pt, fold_result.json and the LOSO summary are untouched; each fold directory
    gets attribution_result.json.  Returns the units attributed."""
    from .attribute import fold_attribution
    from .runtime import Engine
    done = []
    for u in sorted(kept):
        n, _ = units[u]
        cfg, p = cfgs[n], kept[u]
        model = p["model"]
        x, y, _ = _windows(p)
        r = fold_attribution(model, x, y, steps=int(cfg["attribute"]), bin=cfg.get("attribute_bin"), channels=cfg["channels"],
                             num_classes=cfg["num_classes"])
        model.engine().drop_workspaces(Engine.EVAL_KEEP)           # the kept-evaluation workspace of a path batch: not needed again
        r = dict(subject=p["subject"], **r)
        (p["fold_dir"] / "attribution_result.json").write_text(json.dumps(r))
        order = np.argsort(-np.asarray(r["share"]), kind="stable")
        print(f"[rank {rank}] {_tag(n)}fold {p['fold']} ({p['subject']}) attribution over {r['n']} windows, {r['steps']} path points: "
              + ", ".join(f"{r['channels'][i]} {r['share'][i]:.3f}" for i in order)
              + f" | completeness gap mean {r['gap_rel_mean']:.2e} max {r['gap_rel_max']:.2e}", flush=True)
        done.append(u)
    return done


def uncertainty_settings(cfg):
    """The Monte-Carlo dropout settings of a configuration (--mc-dropout ...), as uncertainty.txt / uncertainty.json name them."""
    return {"samples": int(cfg["mc_dropout"]), "seed": int(cfg.get("mc_seed", 0)), "dropout": float(cfg["model_params"]["dropout"])}


def uncertainty_units(kept, units, cfgs, device, rank=0):
    """Monte-Carlo dropout of the rank's finished folds (uncertainty.fold_uncertainty): per fold, from the model the fold trained
    (the one its test pass evaluated) and the TEST subject's windows — how sure the model is of each window and what refusing the
    least certain ones buys.  One model at a time: a wide batch fills the chip on its own.  The models, best_model.pt,
    fold_result.json and the LOSO summary are untouched; each fold directory gets uncertainty_result.json.  Returns the units done."""
    from .uncertainty import fold_uncertainty
    done = []
    for u in sorted(kept):
        n, _ = units[u]
        cfg, p = cfgs[n], kept[u]
        model = p["model"]
        x, y, _ = _windows(p)
        r = fold_uncertainty(model, x, y, samples=int(cfg["mc_dropout"]), seed=int(cfg.get("mc_seed", 0)))
        r = dict(subject=p["subject"], **r)
        (p["fold_dir"] / "uncertainty_result.json").write_text(json.dumps(r))
        au = r["auroc_entropy"]
        print(f"[rank {rank}] {_tag(n)}fold {p['fold']} ({p['subject']}) Monte-Carlo dropout over {r['n']} windows, {r['samples']} samples: "
              f"acc eval {r['accuracy_eval']:.4f} mc {r['accuracy_mc']:.4f} | AUROC of entropy {'n/a' if au is None else format(au, '.4f')} | "
              f"ECE eval {r['ece_eval']:.4f} mc {r['ece_mc']:.4f}", flush=True)
        done.append(u)
    return done


def ensemble_units(members, local, epochs, units, cfgs, seeds, rank=0):
    """The deep ensembles of a --seeds run (ensemble.fold_ensemble): per (configuration, fold) of the rank, its `seeds` replicas' models
    — the ones their test passes evaluated — on the TEST subject's windows.  Unit u * seeds + r is replica r of base unit u
    (ensemble.deal_replicas).  The models, best_model.pt, fold_result.json and the LOSO summary are untouched; replica 0's fold
    directory gets ensemble_result.json, which also records the members' test-pass metrics and stop epochs."""
    for u0 in sorted(u for u in members if u % seeds == 0):
        us = [u0 + r for r in range(seeds)]
        n, k = units[u0]
        p = members[u0]
        x, y, _ = _windows(p)
        t0 = time.time()
        r = ensemble_mod.fold_ensemble([members[u]["model"] for u in us], x, y, eval_batch=p["loaders"][2].batch_size)
        r = dict(subject=p["subject"], fold=k, seeds=[ensemble_mod.replica_seed(cfgs[n]["seed"], k, i) for i in range(seeds)],
                 member_accuracy=[local[u][0] for u in us], member_f1=[local[u][1] for u in us], epochs=[epochs[u] for u in us],
                 seconds=time.time() - t0, **r)
        (p["fold_dir"] / "ensemble_result.json").write_text(json.dumps(r))
        print(f"[rank {rank}] {_tag(n)}fold {k} ({p['subject']}) ensemble of {seeds} seeds over {r['n']} windows: members "
              + " ".join(f"{a:.4f}" for a in r["member_accuracy"])
              + f" | ensemble acc {r['ensemble']['accuracy']:.4f} f1 {r['ensemble']['f1_score']:.4f} | disagreement "
              f"{r['ensemble']['mean_disagreement']:.4f}", flush=True)


def distill_units(members, units, cfgs, out_dir, stores, seeds, kd, train_cfg, device, all_channel_names, rank=0):
    """--distill: per (configuration, fold) of the rank, once its `seeds` replicas have finished, the fold's
    teacher table — its test-pass models as an ensemble.Ensemble in eval mode, ensemble.Ensemble.teacher at the setting's
    temperature, on the store positions of the fold's TRAINING subjects (every other row stays zero and is never read) — and then
    the fold's student: one more unit of configuration replica_name(n, 0) + "/distilled" with replica 0's unit seed, split and
    every training option, trained like any unit (train_units: fold batches per configuration, or sequentially) with the
    distillation term on.  The students write the usual per-fold files under distilled/fold_test_on_<sid>/; replica 0's fold
    directory gets distilled_result.json: ensemble, mean member, replica 0 and student on the test subject's windows."""
    from .ensemble import Ensemble, ensemble_metrics
    base_units = sorted(u for u in members if u % seeds == 0)
    sunits, preps, teachers = {}, {}, {}
    for u0 in base_units:
        n, k = units[u0]
        models = [members[u0 + r]["model"] for r in range(seeds)]
        store = members[u0]["loaders"][0].store
        t0 = time.time()
        x, _, pos = _windows(members[u0], loader=0, labels=False)
        table = torch.zeros((int(store.shape[0]), int(cfgs[n]["num_classes"])), dtype=torch.float32, device=store.device)
        table.index_copy_(0, pos, Ensemble(models, eval_batch=members[u0]["loaders"][2].batch_size).teacher(x, kd.temperature))
        torch.cuda.synchronize(device)
        teachers[u0] = (table, time.time() - t0)
        sunits[u0] = (distill_mod.student_name(n), k)
    groups = {}
    for u0 in base_units:
        groups.setdefault(sunits[u0][0], []).append(u0)

    def make(u0):
        n, k = units[u0]
        p = prepare_fold(k, cfgs[n]["subjects"][k], out_dir[n] / "distilled", device, all_channel_names, dict(cfgs[n], replica=0), stores[n])
        p["distill"] = distill_mod.Distillation(kd.alpha, kd.temperature)
        p["distill"].set_teacher(teachers[u0][0])
        preps[u0] = p
        return p

    infos = dict(train_units(base_units, list(groups.values()), make, train_cfg, device))
    for u0 in base_units:
        n, k = units[u0]
        p0, info = members[u0], infos[u0]
        x, y, _ = _windows(p0)
        r = ensemble_mod.fold_ensemble([members[u0 + r]["model"] for r in range(seeds)], x, y, eval_batch=p0["loaders"][2].batch_size)
        sp = Ensemble([preps[u0]["model"]], eval_batch=p0["loaders"][2].batch_size).predict(x)
        win, mem = r["windows"], r["member_windows"]
        yy = np.asarray(win["y"], dtype=np.int64)
        student = {"mean_p": sp.mean_p.double().cpu().tolist(), "entropy": sp.entropy.double().cpu().tolist(),
                   "mutual_info": sp.mutual_info.double().cpu().tolist()}
        en_pred = np.asarray(win["mean_p"]).argmax(axis=1)

        def row(w):
            m = ensemble_metrics(w["mean_p"], yy, w["entropy"], w["mutual_info"])
            return dict(accuracy=m["accuracy"], f1=m["f1_score"], nll=m["nll"], brier=m["brier"], ece=m["ece"],
                        fidelity=distill_mod.fidelity(np.asarray(w["mean_p"]).argmax(axis=1), en_pred))
        rows = [row(w) for w in mem]
        last = info["history"][-1] if info["history"] else {}
        doc = dict(subject=p0["subject"], fold=k, members=seeds, alpha=kd.alpha, temperature=kd.temperature, n=int(yy.size),
                   ensemble=row(win), mean_member={m: float(np.mean([rw[m] for rw in rows])) for m in rows[0]}, replica0=rows[0],
                   student=row(student), kd_loss=last.get("kd_loss"), kd_agreement=last.get("kd_agreement"), student_epochs=info["epochs"],
                   teacher_seconds=teachers[u0][1], student_seconds=info["seconds"],
                   windows=dict(y=win["y"], ensemble=win, members=mem, student=student))
        (p0["fold_dir"] / "distilled_result.json").write_text(json.dumps(doc))
        print(f"[rank {rank}] {_tag(n)}fold {k} ({p0['subject']}) distilled from {seeds} member(s): student acc {doc['student']['accuracy']:.4f} "
              f"fidelity {doc['student']['fidelity']:.4f} | replica 0 acc {doc['replica0']['accuracy']:.4f} | ensemble acc "
              f"{doc['ensemble']['accuracy']:.4f}", flush=True)


def write_distillation_tables(base, out_dir, results, kd, seeds):
    """distillation.txt / distillation.json of every configuration of a --distill run, from the folds' distilled_result.json, which
    every rank has written before the fold metrics were gathered: per fold and pooled over all test windows."""
    from .ensemble import ensemble_metrics
    paths = []
    for n, cfg in base.items():
        files = [out_dir[n] / f"fold_test_on_{r['subject']}" / "distilled_result.json" for r in results[n]]
        docs = [json.loads(f.read_text()) for f in files if f.exists()]
        if not docs:
            continue
        y = np.concatenate([np.asarray(d["windows"]["y"], dtype=np.int64) for d in docs])
        cat = lambda pick, key: np.concatenate([np.asarray(pick(d)[key], dtype=np.float64) for d in docs])
        en_pred = cat(lambda d: d["windows"]["ensemble"], "mean_p").argmax(axis=1)

        def row(pick):
            p = cat(pick, "mean_p")
            m = ensemble_metrics(p, y, cat(pick, "entropy"), cat(pick, "mutual_info"))
            return dict(accuracy=m["accuracy"], f1=m["f1_score"], nll=m["nll"], brier=m["brier"], ece=m["ece"],
                        fidelity=distill_mod.fidelity(p.argmax(axis=1), en_pred))
        rows = [row(lambda d, i=i: d["windows"]["members"][i]) for i in range(seeds)]
        pooled = dict(ensemble=row(lambda d: d["windows"]["ensemble"]), mean_member={m: float(np.mean([rw[m] for rw in rows])) for m in rows[0]},
                      replica0=rows[0], student=row(lambda d: d["windows"]["student"]))
        kdl = [d["kd_loss"] for d in docs if d.get("kd_loss") is not None]
        if kdl:
            pooled.update(kd_loss=float(np.mean(kdl)), kd_agreement=float(np.mean([d["kd_agreement"] for d in docs if d.get("kd_agreement") is not None])))
        folds = [{k: v for k, v in d.items() if k not in ("windows", "teacher_seconds", "student_seconds")} for d in docs]
        paths.append(distill_mod.write_distillation(out_dir[n], folds, kd, seeds, pooled=pooled, synthetic=bool(cfg.get("synthetic"))))
    return paths


def write_seed_tables(run_output_dir, base, out_dir, results, seeds):
    """seeds.txt / seeds.json of a --seeds run, from the gathered per-replica results and the folds' ensemble_result.json, which
    every rank has written before the fold metrics were gathered."""
    tables = {}
    for n, cfg in base.items():
        per = {m: [[r[m] for r in results[ensemble_mod.replica_name(n, i)]] for i in range(seeds)] for m in ("accuracy", "f1_score")}
        files = [out_dir[n] / f"fold_test_on_{r['subject']}" / "ensemble_result.json" for r in results[n]]
        tables[n] = ensemble_mod.summarise_seeds([json.loads(f.read_text()) for f in files], per)
    return ensemble_mod.write_seeds(run_output_dir, tables, seeds, synthetic=bool(next(iter(base.values())).get("synthetic")))


def _warm_imports():
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot  # noqa: F401
    except Exception:
        pass


def subject_stores(cfgs, all_channel_names, device):
    """{configuration name: SubjectStore}, one store per distinct data set: the model kinds of a comparison run read the same windows."""
    stores, by_data = {}, {}
    for n, c in cfgs.items():
        dkey = (str(c["data_path"]), tuple(c["subjects"]), tuple(c["channels"]), c["mode"], c.get("normalise", "host"), norm_reference(c))
        if dkey not in by_data:
            by_data[dkey] = SubjectStore(c["data_path"], c["subjects"], c["channels"], all_channel_names, classification_mode=c["mode"],
                                         device=device, normalise=c.get("normalise", "host"), reference=norm_reference(c))
        stores[n] = by_data[dkey]
    return stores


def rank_units(cfgs, world, rank):
    """The work units of a job — (configuration, fold) pairs, numbered fold-major, configuration-minor, so that neighbouring units of
    one fold index go to different ranks — with this rank's share of them (unit numbers, dealt round-robin) and that share grouped
    by configuration (in order of first appearance).  Returns units, mine, groups."""
    names, cfg0 = list(cfgs), next(iter(cfgs.values()))
    units = [(n, k) for k in range(max(len(c["subjects"]) for c in cfgs.values())) for n in names if k < len(cfgs[n]["subjects"])]
    mine = folds_for_rank(len(units), world, rank)
    if cfg0.get("only_subjects"):       # a subset of the LOSO's folds (tests: the splits stay those of the full subject list)
        keep = set(cfg0["only_subjects"])
        mine = [u for u in mine if cfgs[units[u][0]]["subjects"][units[u][1]] in keep]
    groups = {}
    for u in mine:
        groups.setdefault(units[u][0], []).append(u)
    return units, mine, list(groups.values())


def train_units(mine, groups, make, cfg0, device):
    """Trains the units `mine` of a rank (`groups`: the same units by configuration; make(unit): its prep, see prepare_fold) in
    one of three modes and yields (unit, result dict): sequentially (concurrent_folds 1; a unit is yielded when it finishes), as
    fold batches (the units of a wave when the wave has finished, in batch order then position order), or — with --no-lockstep, or
    for units that cannot share launches — as single folds on concurrent streams (all units, in order, when the last has finished)."""
    conc = max(1, min(int(cfg0.get("concurrent_folds", 1)), len(mine)))
    if conc == 1:
        for u in mine:                                   # a unit is made immediately before it trains: one unit's loaders at a time
            yield u, train_fold(make(u), device)
        return
    preps = {u: make(u) for u in mine}                   # sequential: seeding / initialisation order as in every other mode
    torch.cuda.synchronize(device)                       # uploads were issued on this thread's stream
    # Folds of one configuration advance in LOCKSTEP as one fold batch: every launch of the step covers all of them
    # (multifold.LockstepTrainer, msig_*_multi) — at B = 64 fifteen streams are bound by the command processor, one set of
    # launches is not.  The folds' splits may differ in size (real WESAD): full batches share launches, ragged last batches
    # run over the folds whose batch sizes agree.  At most `concurrent_folds` folds are resident at a time (waves.deal).
    waves = deal(groups, mine, conc, cfg0.get("lockstep_groups", 4), sweep=len(groups) > 1) if cfg0.get("lockstep", True) else []
    if waves and all(lockstep_compatible([preps[u] for u in ch]) for wv in waves for ch in wv):
        t_start = time.time()
        for wv in waves:
            yield from run_wave(wv, preps, device, bool(cfg0.get("adaptive_forms", False)), t_start)
        return
    # At the reference's batch size (64) one fold keeps ~2 % of an MI355X busy (4 batch tiles of a strictly
    # sequential recurrence), so the rank's units run concurrently, each on its own HIP stream.  Seeding,
    # model initialisation and host-side data preparation stay sequential (deterministic); only the
    # training loops overlap (libmsig_hip.so is re-entrant across streams; ctypes releases the GIL).
    # Beyond four streams the device falls off a cliff (MAX_TRAIN_STREAMS).
    yield from zip(mine, on_streams(lambda u: train_fold(preps[u], device), mine, device, workers=min(conc, MAX_TRAIN_STREAMS)))


def write_summaries(cfgs, units, out_dir, results, cal_all, wall, world, t_data, ad_all=None, attributed=False, uncertain=False,
                    entropy=False):
    """cv_summary.txt — and calibration.txt / calibration.json after --calibrate, adaptation.txt / adaptation.json after --adapt-bn,
    attribution.txt / attribution.json after --attribute, uncertainty.txt / uncertainty.json after --mc-dropout (from the folds'
    attribution_result.json / uncertainty_result.json, which every rank has written before the fold metrics were gathered) — of
    every configuration of a job."""
    for n in cfgs:
        out_dir[n].mkdir(parents=True, exist_ok=True)
        path = write_summary(out_dir[n], results[n], cfgs[n], wall, world)
        accs = [r["accuracy"] for r in results[n]]
        print(f"交叉验证汇总结果已保存至: {path}")
        print(f"{(n + ': ') if n else ''}平均准确率 (Accuracy): {np.mean(accs):.4f} ± {np.std(accs):.4f}"
              f" | LOSO wall-clock {wall:.1f}s on {world} GPU(s) ({len(units)} folds in this job; load + normalise + upload {t_data:.1f}s)")
        if cfgs[n].get("adversary") is not None:      # from the folds' fold_result.json, which every rank has written by now
            files = [out_dir[n] / f"fold_test_on_{r['subject']}" / "fold_result.json" for r in results[n]]
            folds = [adversary_mod.fold_record(json.loads(f.read_text())) for f in files if f.exists()]
            folds = [f for f in folds if f is not None]
            if folds:
                path = adversary_mod.write_adversary(out_dir[n], folds, adversary_mod.settings(cfgs[n]["adversary"]),
                                                     synthetic=bool(cfgs[n].get("synthetic")))
                print(f"Subject-adversary table written to: {path}")
        if cfgs[n].get("group_dro") is not None:      # likewise from the folds' fold_result.json
            files = [out_dir[n] / f"fold_test_on_{r['subject']}" / "fold_result.json" for r in results[n]]
            folds = [dro_mod.fold_record(json.loads(f.read_text())) for f in files if f.exists()]
            folds = [f for f in folds if f is not None]
            if folds:
                path = dro_mod.write_dro(out_dir[n], folds, cfgs[n]["group_dro"], synthetic=bool(cfgs[n].get("synthetic")))
                print(f"Group-DRO table written to: {path}")
        if cfgs[n].get("supcon") is not None:         # likewise from the folds' fold_result.json
            files = [out_dir[n] / f"fold_test_on_{r['subject']}" / "fold_result.json" for r in results[n]]
            folds = [supcon_mod.fold_record(json.loads(f.read_text())) for f in files if f.exists()]
            folds = [f for f in folds if f is not None]
            if folds:
                path = supcon_mod.write_supcon(out_dir[n], folds, cfgs[n]["supcon"], synthetic=bool(cfgs[n].get("synthetic")))
                print(f"Supcon table written to: {path}")
        if cfgs[n].get("averaging") is not None:      # likewise from the folds' fold_result.json
            files = [out_dir[n] / f"fold_test_on_{r['subject']}" / "fold_result.json" for r in results[n]]
            folds = [averaging_mod.fold_record(json.loads(f.read_text())) for f in files if f.exists()]
            folds = [f for f in folds if f is not None]
            if folds:
                path = averaging_mod.write_averaging(out_dir[n], folds, cfgs[n]["averaging"], synthetic=bool(cfgs[n].get("synthetic")))
                print(f"Weight-averaging table written to: {path}")
        if cal_all is not None:
            from .calibrate import write_calibration
            folds = [{"subject": cfgs[n]["subjects"][units[u][1]], "n_cal": int(cal_all[u][2][0]), "n_eval": int(cal_all[u][2][1]),
                      "before": {"accuracy": cal_all[u][0][0], "f1_score": cal_all[u][0][1]},
                      "after": {"accuracy": cal_all[u][1][0], "f1_score": cal_all[u][1][1]}}
                     for u in sorted(cal_all) if units[u][0] == n]
            path = write_calibration(out_dir[n], folds, calibration_settings(cfgs[n]), synthetic=bool(cfgs[n].get("synthetic")))
            print(f"校准结果已保存至: {path}")
        if ad_all is not None:
            from .adapt import write_adaptation
            folds = [{"subject": cfgs[n]["subjects"][units[u][1]], "n": int(ad_all[u][2][0]),
                      "before": {"accuracy": ad_all[u][0][0], "f1_score": ad_all[u][0][1]},
                      "after": {"accuracy": ad_all[u][1][0], "f1_score": ad_all[u][1][1]}}
                     for u in sorted(ad_all) if units[u][0] == n]
            path = write_adaptation(out_dir[n], folds, adaptation_settings(cfgs[n]), synthetic=bool(cfgs[n].get("synthetic")))
            print(f"BatchNorm adaptation table written to: {path}")
        if entropy:      # entropy_adaptation.txt / .json after --adapt-entropy, from the folds' entropy_adaptation_result.json
            from .tta import settings_of, write_entropy_adaptation
            files = [out_dir[n] / f"fold_test_on_{r['subject']}" / "entropy_adaptation_result.json" for r in results[n]]
            folds = [json.loads(f.read_text()) for f in files if f.exists()]
            if folds:
                path = write_entropy_adaptation(out_dir[n], folds, settings_of(cfgs[n]), synthetic=bool(cfgs[n].get("synthetic")))
                print(f"Entropy adaptation table written to: {path}")
        if attributed:
            from .attribute import write_attribution
            files = [out_dir[n] / f"fold_test_on_{r['subject']}" / "attribution_result.json" for r in results[n]]
            folds = [json.loads(f.read_text()) for f in files if f.exists()]
            if folds:
                path = write_attribution(out_dir[n], folds, attribution_settings(cfgs[n]), synthetic=bool(cfgs[n].get("synthetic")))
                print(f"Attribution table written to: {path}")
        if uncertain:
            from .uncertainty import write_uncertainty
            files = [out_dir[n] / f"fold_test_on_{r['subject']}" / "uncertainty_result.json" for r in results[n]]
            folds = [json.loads(f.read_text()) for f in files if f.exists()]
            if folds:
                path = write_uncertainty(out_dir[n], folds, uncertainty_settings(cfgs[n]), synthetic=bool(cfgs[n].get("synthetic")))
                print(f"Uncertainty table written to: {path}")


def run_experiments(run_output_dir, device, all_channel_names, cfgs, rank=0, world=1):
    """Runs the LOSO loop of every configuration in `cfgs` ({name: cfg}) as ONE sharded job: the work units
    are (configuration, fold) pairs — 15 for a plain run, 4 x 15 = 60 for the channel-ablation sweep — dealt
    round-robin to the ranks and trained concurrently within a rank.  A configuration named "" writes into
    `run_output_dir` itself, any other into `run_output_dir/<name>`.  Returns {name: results}, wall seconds."""
    cfg0 = next(iter(cfgs.values()))
    t0 = time.time()
    # matplotlib (the confusion-matrix plots) costs ~0.4 s of interpreter time the first time it is imported: started here on a
    # thread, it runs while this thread reads and normalises the subjects' files (numpy, mostly outside the interpreter lock)
    # instead of in front of the first fold's test pass.  (Round 3 also warmed torch._dynamo here, which torch.optim's first
    # Optimizer pulled in — 0.9 s that still ended up in front of the first train step; trainer.MsigAdam no longer triggers it.)
    warm = threading.Thread(target=_warm_imports, daemon=True)
    warm.start()
    # --seeds S (cfg["seeds"] > 1): every (configuration, fold) trains S seed replicas.  Replica r of configuration n is one more
    # configuration, ensemble.replica_name(n, r) — r = 0 the configuration itself, r >= 1 writing to its seed_<r>/ — that shares the
    # SubjectStore; a rank holds all replicas of the folds it holds.  base: the configurations as given (absent or 1: all of this is off)
    S, base = int(cfg0.get("seeds") or 1), cfgs
    # --distill (cfg["distill"]): after a fold's replicas, its student — one more unit, trained against the
    # replicas' ensemble; absent: off, and every unit, arena, launch, file and bit is what it was
    kd = distill_mod.Distillation.parse(cfg0["distill"]) if cfg0.get("distill") is not None else None
    if S > 1:
        cfgs = {ensemble_mod.replica_name(n, r): dict(c, replica=r) for n, c in base.items() for r in range(S)}
    stores = subject_stores(cfgs, all_channel_names, device)
    t_data = time.time() - t0
    units, mine, groups = rank_units(base, world, rank)
    if S > 1:
        units, mine, groups = ensemble_mod.deal_replicas(units, mine, S)
    out_dir = {n: (Path(run_output_dir) / n if n else Path(run_output_dir)) for n in cfgs}
    n_cal = int(cfg0.get("calibrate") or 0)          # --calibrate: windows per class of the test subject; 0 = off
    adapt = cfg0.get("adapt_bn") is not None         # --adapt-bn: label-free BatchNorm adaptation to the test subject; absent = off
    attr = cfg0.get("attribute") is not None         # --attribute: integrated-gradients attribution on the test subject; absent = off
    mc = cfg0.get("mc_dropout") is not None          # --mc-dropout: Monte-Carlo dropout uncertainty on the test subject; absent = off
    tent = cfg0.get("adapt_entropy") is not None     # --adapt-entropy: entropy-minimisation adaptation to the test subject; absent = off
    kept, local = {}, {}                             # unit -> its prep (model, loaders), kept for the calibration / adaptation after the folds; -> its metrics
    members, epochs = {}, {}                         # --seeds: every unit's prep, for the ensembles after the folds; its stop epoch

    def make(u):
        n, k = units[u]
        p = prepare_fold(k, cfgs[n]["subjects"][k], out_dir[n], device, all_channel_names, cfgs[n], stores[n])
        if (n_cal or adapt or attr or mc or tent) and not cfgs[n].get("replica"):      # the post-LOSO passes run on replica 0 only
            kept[u] = p
        if S > 1 or kd is not None:
            members[u] = p
        return p

    # the replicas are what fills the chip: S times the folds are resident (a sweep is one window whatever the width)
    conc = int(cfg0.get("concurrent_folds", 1))      # 1 stays 1: sequential training, unit by unit
    train_cfg = dict(cfg0, concurrent_folds=conc * S) if S > 1 and conc > 1 else cfg0
    for u, info in train_units(mine, groups, make, train_cfg, device):
        n, k = units[u]
        local[u] = (info["accuracy"], info["f1_score"])
        epochs[u] = info["epochs"]
        print(f"[rank {rank}] {n + '/' if n else ''}fold {k} ({cfgs[n]['subjects'][k]}): acc {info['accuracy']:.4f} f1 {info['f1_score']:.4f} "
              f"{info['epochs']} epochs {info['seconds']:.1f}s {info['train_windows_per_s']:.0f} windows/s", flush=True)
    cal_local = calibrate_units(kept, units, cfgs, device, rank) if n_cal and kept else {}
    ad_local = adapt_units(kept, units, cfgs, device, rank) if adapt and kept else {}      # on its own: the LOSO model, not the calibrated one
    if tent and kept:                                # on copies of the LOSO model; its records go to the fold directories
        entropy_units(kept, units, cfgs, device, rank)
    if attr and kept:                                # likewise the LOSO model; its records go to the fold directories
        attribute_units(kept, units, cfgs, device, rank)
    if mc and kept:                                  # likewise
        uncertainty_units(kept, units, cfgs, device, rank)
    # emulate_rank (bench.py --emulate-ranks): this process plays rank `rank` of a `world`-GPU job ALONE on its GPU — exactly what
    # that rank executes on an 8-GPU node, less the one ~100-byte all_gather of the fold metrics
    emulate, gdev = cfg0.get("emulate_rank"), cfg0.get("gather_device", device)
    if S > 1:                                        # each fold's S test-pass models as an ensemble on its test subject, before the gather
        ensemble_units(members, local, epochs, units, cfgs, S, rank)
    if kd is not None:                               # each fold's teacher table and student, likewise before the gather
        distill_units(members, units, cfgs, out_dir, stores, S, kd, cfg0, device, all_channel_names, rank)
    # a rank holds ceil(folds / world) folds with all their replicas: the gather's rows per rank are sized for that
    n_rows = len(units) if S == 1 else -(-(len(units) // S) // world) * S * world
    allm = dict(local) if emulate else gather_fold_metrics(local, n_rows, world, gdev)
    wall = time.time() - t0
    cal_all = None
    if n_cal and emulate:     # after the LOSO wall-clock is taken: the summary's timing line is the LOSO's
        cal_all = dict(cal_local)
    elif n_cal:
        parts = [gather_fold_metrics({u: v[i] for u, v in cal_local.items()}, len(units), world, gdev) for i in range(3)]
        cal_all = {u: (parts[0][u], parts[1][u], parts[2][u]) for u in parts[0]}
    ad_all = None
    if adapt and emulate:
        ad_all = dict(ad_local)
    elif adapt:
        parts = [gather_fold_metrics({u: v[i] for u, v in ad_local.items()}, len(units), world, gdev) for i in range(3)]
        ad_all = {u: (parts[0][u], parts[1][u], parts[2][u]) for u in parts[0]}
    warm.join()            # long done in a real run; a tiny one must not leave an import running at interpreter exit
    results = {n: [] for n in cfgs}
    for u in sorted(allm):
        n, k = units[u]
        results[n].append({"subject": cfgs[n]["subjects"][k], "accuracy": allm[u][0], "f1_score": allm[u][1]})
    if S > 1:                                        # replica 0 is the run: its summaries are those of a run without --seeds
        if rank == 0 or emulate:
            path = write_seed_tables(run_output_dir, base, out_dir, results, S)
            print(f"Seed-replica and ensemble table written to: {path}")
        results = {n: results[n] for n in base}
        cfgs = base
    if kd is not None and (rank == 0 or emulate):
        for path in write_distillation_tables(base, out_dir, results, kd, S):
            print(f"Distillation table written to: {path}")
    if rank == 0 or emulate:
        write_summaries(cfgs, units, out_dir, results, cal_all, wall, world, t_data, ad_all, attributed=attr, uncertain=mc, entropy=tent)
    return results, wall


def comparison(results, kinds, channels):
    """Attention model vs baseline, fold by fold.  results: {set name: {kind: [per-fold dicts with subject, accuracy, f1_score]}};
    channels: {set name: channel list}.  Folds are paired by test subject (the kinds share splits, seeds and loader order).  The
    paired difference is cnn_gru_attention - cnn_gru and the win counts are the attention model's, the baseline's and the ties,
    whatever the order of `kinds`; std is the population std (np.std, as cv_summary.txt).  Returns a JSON-ready dict."""
    a, b = sorted(kinds, key=list(MODEL_PARAMS).index)          # (cnn_gru_attention, cnn_gru)
    out = {"kinds": [a, b], "difference": f"{a} - {b}", "sets": {}}
    for name, per_kind in results.items():
        ra = {r["subject"]: r for r in per_kind[a]}
        rb = {r["subject"]: r for r in per_kind[b]}
        folds = []
        for subj in [r["subject"] for r in per_kind[a] if r["subject"] in rb]:
            row = {"subject": subj}
            for kind, rr in ((a, ra), (b, rb)):
                row[kind] = {"accuracy": float(rr[subj]["accuracy"]), "f1_score": float(rr[subj]["f1_score"])}
            row["difference"] = {m: row[a][m] - row[b][m] for m in ("accuracy", "f1_score")}
            folds.append(row)
        summary = {}
        for key in (a, b, "difference"):
            summary[key] = {}
            for m in ("accuracy", "f1_score"):
                v = np.array([f[key][m] for f in folds], dtype=np.float64)
                summary[key][m] = {"mean": float(v.mean()) if v.size else float("nan"), "std": float(v.std()) if v.size else float("nan")}
        ch = list(channels[name])
        out["sets"][name] = {
            "channels": ch, "gate_hidden_width": len(ch) // 4, "folds": folds, "summary": summary,
            "attention_wins": {m: int(sum(f["difference"][m] > 0 for f in folds)) for m in ("accuracy", "f1_score")},
            "baseline_wins": {m: int(sum(f["difference"][m] < 0 for f in folds)) for m in ("accuracy", "f1_score")},
            "ties": {m: int(sum(f["difference"][m] == 0 for f in folds)) for m in ("accuracy", "f1_score")},
            "n_folds": len(folds)}
    return out


def write_comparison(run_output_dir, cmp):
    """comparison.json (the dict of `comparison`) and comparison.txt beside the configurations' directories."""
    run_output_dir = Path(run_output_dir)
    (run_output_dir / "comparison.json").write_text(json.dumps(cmp, indent=1))
    a, b = cmp["kinds"]
    lines = [f"模型对比 (paired LOSO folds): {a} vs {b}; difference = {cmp['difference']}", ""]
    for name, st in cmp["sets"].items():
        gw = st["gate_hidden_width"]
        lines.append(f"channel set {name or 'default'}: {st['channels']} (C = {len(st['channels'])}), gate hidden width C // 4 = {gw}"
                     + ("  -> the gate is the constant 0.5: the models differ only by that scale before BatchNorm-1" if gw == 0 else ""))
        lines.append(f"  {'subject':<10} {a + ' acc':>24} {b + ' acc':>14} {'diff':>9}   {a + ' F1':>23} {b + ' F1':>13} {'diff':>9}")
        for f in st["folds"]:
            lines.append(f"  {f['subject']:<10} {f[a]['accuracy']:>24.4f} {f[b]['accuracy']:>14.4f} {f['difference']['accuracy']:>+9.4f}   "
                         f"{f[a]['f1_score']:>23.4f} {f[b]['f1_score']:>13.4f} {f['difference']['f1_score']:>+9.4f}")
        sm = st["summary"]
        for key in (a, b, "difference"):
            sg = "+" if key == "difference" else ""
            lines.append(f"  {key:<18} accuracy {sm[key]['accuracy']['mean']:{sg}.4f} ± {sm[key]['accuracy']['std']:.4f}   "
                         f"weighted F1 {sm[key]['f1_score']['mean']:{sg}.4f} ± {sm[key]['f1_score']['std']:.4f}")
        for m, label in (("accuracy", "accuracy"), ("f1_score", "weighted F1")):
            lines.append(f"  {label}: {a} wins {st['attention_wins'][m]} of {st['n_folds']} folds, {b} wins {st['baseline_wins'][m]}, "
                         f"ties {st['ties'][m]}")
        lines.append("")
    path = run_output_dir / "comparison.txt"
    path.write_text("\n".join(lines), encoding="utf-8")
    return path


def reference_dir(reference):
    """The directory name of a reference's configuration in a --norm-reference run of several: "baseline:30" -> "baseline_30"."""
    return reference.replace(":", "_")


def normalisation(results, references, data_path, subjects):
    """The references of a --norm-reference run of several, fold by fold.  results: {set name: {reference: [per-fold dicts with
    subject, accuracy, f1_score]}}.  Folds are paired by test subject (the references share splits, seeds and loader order); the
    paired difference is reference - anchor, the anchor being "subject" or, where that is not among them, the first reference.
    Per subject the number of reference windows used and whether the whole-recording fallback applied (from the raw label files:
    what every store of the run was built from).  std is the population std (np.std, as cv_summary.txt).  Returns a JSON-ready dict."""
    anchor = "subject" if "subject" in references else references[0]
    windows = {}
    for ref in references:
        windows[ref] = {}
        for sid in subjects:
            fy = Path(data_path) / f"{sid}_y.npy"
            if not fy.exists():
                continue
            y_raw = np.load(fy)
            if running_norm_reference(ref) is not None:           # window n is normalised with the windows up to n: no one count
                windows[ref][sid] = {"n_windows": int(len(y_raw)), "reference_windows": "per window", "fallback": False}
                continue
            n = int(reference_mask(y_raw, ref).sum())
            fallback = n == 0
            windows[ref][sid] = {"n_windows": int(len(y_raw)), "reference_windows": int(len(y_raw)) if fallback else n, "fallback": fallback}
    out = {"references": list(references), "anchor": anchor, "difference": f"reference - {anchor}", "reference_windows": windows, "sets": {}}
    for name, per_ref in results.items():
        base = {r["subject"]: r for r in per_ref[anchor]}
        st = {"n_folds": len(base), "references": {}}
        for ref in references:
            rows = {r["subject"]: r for r in per_ref[ref]}
            folds = [{"subject": sid, "accuracy": float(rows[sid]["accuracy"]), "f1_score": float(rows[sid]["f1_score"]),
                      "difference": {m: float(rows[sid][m]) - float(base[sid][m]) for m in ("accuracy", "f1_score")}}
                     for sid in base if sid in rows]
            entry = {"folds": folds, "summary": {}, "difference": {}}
            for m in ("accuracy", "f1_score"):
                v = np.array([f[m] for f in folds], dtype=np.float64)
                d = np.array([f["difference"][m] for f in folds], dtype=np.float64)
                entry["summary"][m] = {"mean": float(v.mean()) if v.size else float("nan"), "std": float(v.std()) if v.size else float("nan")}
                entry["difference"][m] = {"mean": float(d.mean()) if d.size else float("nan"), "std": float(d.std()) if d.size else float("nan"),
                                          "wins": int((d > 0).sum()), "ties": int((d == 0).sum()), "losses": int((d < 0).sum())}
            st["references"][ref] = entry
        out["sets"][name] = st
    return out


def write_normalisation(run_output_dir, table, synthetic=False):
    """normalisation.json (the dict of `normalisation`) and normalisation.txt beside the configurations' directories."""
    run_output_dir = Path(run_output_dir)
    table = dict(table, synthetic=bool(synthetic))
    (run_output_dir / "normalisation.json").write_text(json.dumps(table, indent=1))
    refs, anchor = table["references"], table["anchor"]
    lines = [f"Normalisation references (paired LOSO folds): {', '.join(refs)}; difference = {table['difference']}"]
    if synthetic:
        lines.append("synthetic data: its subject effects are affine, so every reference removes them — this table shows that the "
                     "machinery runs, not what a reference costs or gains on WESAD")
    lines.append("")
    for name, st in table["sets"].items():
        if name:
            lines.append(f"channel set {name}")
        subjects = [f["subject"] for f in st["references"][anchor]["folds"]]
        lines.append(f"  {'subject':<10}" + "".join(f" {r + ' acc':>18} {'F1':>8} {'d acc':>8} {'d F1':>8}" for r in refs))
        for i, sid in enumerate(subjects):
            row = f"  {sid:<10}"
            for r in refs:
                f = st["references"][r]["folds"][i]
                row += f" {f['accuracy']:>18.4f} {f['f1_score']:>8.4f} {f['difference']['accuracy']:>+8.4f} {f['difference']['f1_score']:>+8.4f}"
            lines.append(row)
        for r in refs:
            sm, df = st["references"][r]["summary"], st["references"][r]["difference"]
            lines.append(f"  {r:<14} accuracy {sm['accuracy']['mean']:.4f} ± {sm['accuracy']['std']:.4f}   "
                         f"weighted F1 {sm['f1_score']['mean']:.4f} ± {sm['f1_score']['std']:.4f}")
            if r != anchor:
                for m, label in (("accuracy", "accuracy"), ("f1_score", "weighted F1")):
                    lines.append(f"    {label} vs {anchor}: {df[m]['mean']:+.4f} ± {df[m]['std']:.4f}; wins {df[m]['wins']} ties {df[m]['ties']} "
                                 f"losses {df[m]['losses']} of {st['n_folds']} folds")
        lines.append("")
    lines.append("reference windows used per subject (fallback: no baseline window, the statistics of all windows):")
    for r in refs:
        lines.append(f"  {r}: " + ", ".join((f"{sid} per window" if w["reference_windows"] == "per window" else
                                             f"{sid} {w['reference_windows']}/{w['n_windows']}") + (" fallback" if w["fallback"] else "")
                                            for sid, w in table["reference_windows"][r].items()))
    path = run_output_dir / "normalisation.txt"
    path.write_text("\n".join(lines) + "\n", encoding="utf-8")
    return path


def run_simple_experiment(run_output_dir, device, all_channel_names, cfg=None, rank=0, world=1):
    """The reference's entry point (main.py:91): one configuration, 15 folds."""
    results, wall = run_experiments(run_output_dir, device, all_channel_names, {"": cfg or default_cfg()}, rank, world)
    return results[""], wall


# ---- hierarchical experiment (main.py:20-40, 159-247) ------------------------------------------------------------------
M1_CHANNELS_TO_USE = ["chest_ECG", "chest_EDA", "chest_Resp"]
M1_MODEL_PARAMS = {"cnn_out_channels": 32, "gru_hidden_size": 64, "gru_num_layers": 2, "dropout": 0.5}
M2_CHANNELS_TO_USE = ["chest_ECG", "chest_EDA", "chest_Resp"]
M2_MODEL_PARAMS = {"cnn_out_channels": 32, "gru_hidden_size": 32, "gru_num_layers": 1, "dropout": 0.5}


def hierarchical_units(k, cfg, models, datasets, run_output_dir, device):
    """The (fold, model) units of fold k of the hierarchical experiment, as (tag, prep) pairs — M1, then M2, each made when it is
    asked for (make_unit; seed SEED + 2 k + (M2), loaders that always shuffle, no test pass: the fold's M1 test pass and its
    three-class decision are the driver's `decide`).  `datasets`: {tag: dataset factory}.  Ends, with the reference's warning, at
    the first model whose training or validation set is empty (main.py:187-189): a fold that loses its M2 this way has trained
    its M1 and never decides."""
    sid = cfg["subjects"][k]
    fold_dir = Path(run_output_dir) / f"fold_test_on_{sid}"
    fold_dir.mkdir(parents=True, exist_ok=True)
    for tag, ch, par, mode in models:
        p = make_unit(k, sid, fold_dir / f"model_{tag}", datasets[tag], len(ch), 2, par, cfg["seed"] + 2 * k + (tag == "m2"), cfg, device,
                      test_pass=False, skip_empty=True)
        if p is None:
            print(f"警告: 训练集或验证集在 {mode} 模式下没有数据，跳过此折叠。")
            return
        yield tag, p


def run_hierarchical_experiment(run_output_dir, device, all_channel_names, cfg=None, rank=0, world=1):
    """The reference's run_hierarchical_experiment (main.py:159-247): per LOSO fold a stress-vs-rest model M1 (the reference
    configuration) and an amusement-vs-baseline model M2 (gru_hidden_size 32, gru_num_layers 1: runtime.EmbeddedEngine), then the
    three-class decision `2 if M1 says stress else M2's class` on the test subject.  The reference cannot run this function (its
    dataset.py raises for 'amusement_binary'): the label map is defined in dataset.map_labels, and the
    summary the reference stops short of (overall three-class accuracy / weighted F1, per-fold M1 accuracy) is written to
    hierarchical_summary.txt.  Folds are dealt to the ranks like the simple experiment's, so a fold's M1 and M2 stay on one rank.
    By default the rank's work units — (fold, model) pairs — train as fold batches (multifold.LockstepTrainer): the M1s over the
    stress_binary store, the M2s (the one-layer model: runtime.FoldArena's padded form) over the amusement_binary store — views of one
    store per model (SubjectStore.from_wesad: the same windows, bit for bit) — dealt and run like the simple experiment's
    (waves.deal, waves.run_wave), the two models being the groups that train side by side; each fold's decision runs once both
    its models have finished.  M2's training sets are smaller; folds of unequal size share launches as in the simple experiment,
    and the backward kernel form is pinned per fold (FoldArena.multi), so every fold's bits are those of its sequential run.
    cfg["concurrent_folds"] = 1 (or lockstep False) trains each fold's two models one after the other (train_fold), as the
    reference does; both give the same bits.  Returns (per-fold dicts in subject order, wall seconds)."""
    from .trainer import accuracy_and_weighted_f1
    cfg = dict(cfg or default_cfg())
    m1_ch, m2_ch = list(cfg.get("m1_channels", M1_CHANNELS_TO_USE)), list(cfg.get("m2_channels", M2_CHANNELS_TO_USE))
    m1_par, m2_par = dict(cfg.get("m1_params", M1_MODEL_PARAMS)), dict(cfg.get("m2_params", M2_MODEL_PARAMS))
    subjects, t0, cache = list(cfg["subjects"]), time.time(), {}
    models = (("m1", m1_ch, m1_par, "stress_binary"), ("m2", m2_ch, m2_par, "amusement_binary"))
    ebs = int(cfg.get("eval_batch_size") or cfg["batch_size"])     # validation / test passes (per-window results do not depend on it)
    local, rows = {}, {}
    mine = folds_for_rank(len(subjects), world, rank)

    def decide(k, trainers):
        """M1's test pass and the three-class decision of fold k (main.py:203-247), once both its models have trained."""
        sid = subjects[k]
        m1_test = host_datasets(cfg, all_channel_names, cache, m1_ch, "stress_binary")([sid])
        _, m1_acc, m1_f1 = trainers["m1"].evaluate(DeviceLoader(m1_test, ebs, False, device), is_test=True)   # main.py:203-207
        eval_ch = list(dict.fromkeys(m1_ch + m2_ch))              # main.py:211 (a set there: the order is immaterial, the indices follow it)
        tern = host_datasets(cfg, all_channel_names, cache, eval_ch, "ternary")([sid])
        i1, i2 = [eval_ch.index(c) for c in m1_ch], [eval_ch.index(c) for c in m2_ch]
        m1, m2 = trainers["m1"].model.eval(), trainers["m2"].model.eval()
        preds = []
        with torch.no_grad():
            for xb, _ in DeviceLoader(tern, ebs, False, device):
                p1 = torch.argmax(m1(xb[:, i1, :].contiguous()), dim=1)
                p2 = torch.argmax(m2(xb[:, i2, :].contiguous()), dim=1)
                preds.append(torch.where(p1 == 1, torch.full_like(p2, 2), p2))      # main.py:243
        pred = torch.cat(preds).cpu().numpy()
        acc3, f13 = accuracy_and_weighted_f1(np.asarray(tern.labels), pred)
        rows[k] = dict(subject=sid, m1_accuracy=m1_acc, m1_f1=m1_f1, ternary_accuracy=acc3, ternary_f1=f13, n=int(len(pred)),
                       correct=int((pred == np.asarray(tern.labels)).sum()))
        (Path(run_output_dir) / f"fold_test_on_{sid}" / "fold_result.json").write_text(json.dumps(rows[k]))
        if cfg.get("adversary") is not None:      # each model's adversary record beside its logs; rank 0 tabulates them after the run
            for tag, t in trainers.items():
                rec = adversary_mod.fold_record(dict(subject=sid, history=t.history, adversary_domains=t.adversary.S,
                                                     accuracy=m1_acc if tag == "m1" else None))
                if rec is not None:                 # a model that trained no epoch has no record
                    (Path(run_output_dir) / f"fold_test_on_{sid}" / f"model_{tag}" / "adversary_result.json").write_text(json.dumps(rec))
        if cfg.get("group_dro") is not None:      # likewise each model's group-DRO record
            for tag, t in trainers.items():
                if t.dro is None:
                    continue
                info = dict(subject=sid, history=t.history, accuracy=m1_acc if tag == "m1" else None,
                            group_dro=dro_mod.fold_info(t.dro, t.subject_names[0]))
                rec = dro_mod.fold_record(info)
                if rec is not None:
                    (Path(run_output_dir) / f"fold_test_on_{sid}" / f"model_{tag}" / "dro_result.json").write_text(json.dumps(rec))
        if cfg.get("supcon") is not None:         # likewise each model's supcon record
            for tag, t in trainers.items():
                if t.supcon is None:
                    continue
                rec = supcon_mod.fold_record(dict(subject=sid, history=t.history, accuracy=m1_acc if tag == "m1" else None,
                                                  supcon=supcon_mod.fold_info(t.supcon)))
                if rec is not None:
                    (Path(run_output_dir) / f"fold_test_on_{sid}" / f"model_{tag}" / "supcon_result.json").write_text(json.dumps(rec))
        local[k] = (m1_acc, acc3)
        print(f"[rank {rank}] fold {k} ({sid}): M1 acc {m1_acc:.4f} | three-class acc {acc3:.4f} f1 {f13:.4f}", flush=True)

    if int(cfg.get("concurrent_folds", 1)) > 1 and cfg.get("lockstep", True) and mine:
        stores = {tag: SubjectStore.from_wesad(cfg["data_path"], subjects, ch, all_channel_names, mode, device, cache, norm_reference(cfg))
                  for tag, ch, _, mode in models}
        datasets = {tag: stores[tag].view for tag in stores}
        # sequential: seeding / initialisation order as in the sequential driver
        units = {(k, tag): p for k in mine for tag, p in hierarchical_units(k, cfg, models, datasets, run_output_dir, device)}
        waves = deal([[u for u in units if u[1] == tag] for tag in stores], mine, cfg.get("concurrent_folds", 15), cfg.get("lockstep_groups", 4),
                     fold_of=itemgetter(0))
        if not all(lockstep_compatible([units[u] for u in ch]) for wv in waves for ch in wv):
            raise RuntimeError("hierarchical fold batch: folds of one model do not share a store / batch size")
        torch.cuda.synchronize(device)                  # uploads were issued on this thread's stream
        t_start, finished, undecided = time.time(), set(), list(mine)
        for wv in waves:
            finished.update(u for u, _ in run_wave(wv, units, device, bool(cfg.get("adaptive_forms", False)), t_start))
            for k in [k for k in undecided if all((k, tag) in finished for tag in stores)]:      # both its models have finished
                undecided.remove(k)
                decide(k, {tag: units[(k, tag)]["trainer"] for tag in stores})
    else:
        datasets = {tag: host_datasets(cfg, all_channel_names, cache, ch, mode) for tag, ch, _, mode in models}
        for k in mine:
            trainers = {}
            for tag, p in hierarchical_units(k, cfg, models, datasets, run_output_dir, device):     # made immediately before it trains
                train_fold(p, device)
                trainers[tag] = p["trainer"]
            if len(trainers) == len(models):
                decide(k, trainers)
    allm = gather_fold_metrics(local, len(subjects), world, cfg.get("gather_device", device))
    wall = time.time() - t0
    results = [dict(subject=subjects[k], m1_accuracy=allm[k][0], ternary_accuracy=allm[k][1]) for k in sorted(allm)]
    if rank == 0:
        path = Path(run_output_dir) / "hierarchical_summary.txt"
        with open(path, "w", encoding="utf-8") as f:
            f.write(f"M1 {m1_ch} {m1_par}\nM2 {m2_ch} {m2_par}\n")
            if model_kind(cfg) != MODEL_TO_USE:                      # named only when not the reference's model, like CLASS_WEIGHTS
                f.write(f"MODEL_TO_USE: {model_kind(cfg)}\n")
            if trainer_class_weights(cfg) is not None:
                f.write(f"CLASS_WEIGHTS: {trainer_class_weights(cfg)}\n")
            if cfg.get("max_grad_norm") is not None:
                f.write(f"MAX_GRAD_NORM: {cfg['max_grad_norm']:g}\n")
            if cfg.get("sam") is not None:
                f.write(f"SAM: {cfg['sam']}\n")
            if cfg.get("augment") is not None:
                f.write(f"AUGMENT: {Augment.coerce(cfg['augment']).spec()}\n")
            if soft_targets_line(cfg) is not None:
                f.write(soft_targets_line(cfg))
            if adversary_line(cfg) is not None:
                f.write(adversary_line(cfg))
            if cfg.get("group_dro") is not None:
                f.write(dro_mod.settings_line(cfg["group_dro"]) + "\n")
            if cfg.get("supcon") is not None:
                f.write(supcon_mod.settings_line(cfg["supcon"]) + "\n")
            if cfg.get("norm_reference") is not None:
                f.write(f"NORM_REFERENCE: {cfg['norm_reference']}\n")
            f.write("\n")
            for r in results:
                f.write(f"  - 测试 {r['subject']}: M1 Accuracy = {r['m1_accuracy']:.4f}, 三分类 Accuracy = {r['ternary_accuracy']:.4f}\n")
            if results:
                f.write(f"\n平均 M1 准确率: {np.mean([r['m1_accuracy'] for r in results]):.4f}\n")
                f.write(f"平均三分类准确率: {np.mean([r['ternary_accuracy'] for r in results]):.4f}\n")
            f.write(f"\nwall-clock: {wall:.1f} s on {world} GPU(s)\n")
        print(f"分层分类汇总结果已保存至: {path}")
        if cfg.get("adversary") is not None:
            for tag in ("m1", "m2"):
                files = [Path(run_output_dir) / f"fold_test_on_{r['subject']}" / f"model_{tag}" / "adversary_result.json" for r in results]
                folds = [json.loads(f.read_text()) for f in files if f.exists()]
                if folds:
                    path = adversary_mod.write_adversary(run_output_dir, folds, adversary_mod.settings(cfg["adversary"]),
                                                         synthetic=bool(cfg.get("synthetic")), stem=f"adversary_{tag}")
                    print(f"Subject-adversary table written to: {path}")
        if cfg.get("group_dro") is not None:
            for tag in ("m1", "m2"):
                files = [Path(run_output_dir) / f"fold_test_on_{r['subject']}" / f"model_{tag}" / "dro_result.json" for r in results]
                folds = [json.loads(f.read_text()) for f in files if f.exists()]
                if folds:
                    path = dro_mod.write_dro(run_output_dir, folds, cfg["group_dro"], synthetic=bool(cfg.get("synthetic")), stem=f"dro_{tag}")
                    print(f"Group-DRO table written to: {path}")
        if cfg.get("supcon") is not None:
            for tag in ("m1", "m2"):
                files = [Path(run_output_dir) / f"fold_test_on_{r['subject']}" / f"model_{tag}" / "supcon_result.json" for r in results]
                folds = [json.loads(f.read_text()) for f in files if f.exists()]
                if folds:
                    path = supcon_mod.write_supcon(run_output_dir, folds, cfg["supcon"], synthetic=bool(cfg.get("synthetic")), stem=f"supcon_{tag}")
                    print(f"Supcon table written to: {path}")
    return results, wall


def ablation_sets(all_channel_names):
    """The channel-ablation sweep of BASELINE.json: ECG only, EDA only, every chest channel, every wrist channel
    (sets whose channels the dataset does not have are dropped)."""
    have = list(all_channel_names)
    sets = {"ecg_only": [c for c in have if c == "chest_ECG"], "eda_only": [c for c in have if c == "chest_EDA"],
            "chest_only": [c for c in have if c.startswith("chest_")], "wrist_only": [c for c in have if c.startswith("wrist_")]}
    return {n: ch for n, ch in sets.items() if ch}


def default_cfg():
    return dict(data_path=EARLY_DATA_PATH, channels=list(CHANNELS_TO_USE), mode=CLASSIFICATION_MODE, num_classes=NUM_CLASSES,
                model_params=dict(MODEL_PARAMS[MODEL_TO_USE]), seed=SEED, epochs=EPOCHS, batch_size=BATCH_SIZE, lr=LEARNING_RATE,
                patience=PATIENCE, weight_decay=WEIGHTS_DECAY, subjects=list(ALL_SUBJECTS), verbose=False, concurrent_folds=15,
                eval_batch_size=EVAL_BATCH_SIZE, class_weights=CLASS_WEIGHTS)


def parse_args(ap, argv=None):
    """parse_args plus the checks between flags that need no GPU."""
    args = ap.parse_args(argv)
    if args.calibrate < 0:
        ap.error("--calibrate takes a number of windows per class (>= 1; 0 = off)")
    if args.calibrate and (args.hierarchical or args.ablation or args.sweep):
        ap.error("--calibrate runs with the standard LOSO and the --model comparison run (not --hierarchical, --ablation or --sweep)")
    if not args.calibrate and (args.calibration_sequential
                               or any(v is not None for v in (args.calibration_gap, args.calibration_epochs, args.calibration_lr))):
        ap.error("--calibration-gap / --calibration-epochs / --calibration-lr / --calibration-sequential need --calibrate N")
    if (args.calibration_gap is not None and args.calibration_gap < 0) or (args.calibration_epochs is not None and args.calibration_epochs < 0):
        ap.error("--calibration-gap and --calibration-epochs must be >= 0")
    if args.calibration_lr is not None and not args.calibration_lr > 0:
        ap.error("--calibration-lr must be > 0")
    if args.adapt_bn is not None:
        from .adapt import check_alpha
        try:
            args.adapt_bn = check_alpha(args.adapt_bn)
        except ValueError as e:
            ap.error(f"--adapt-bn: {e}")
        if args.hierarchical or args.ablation or args.sweep:
            ap.error("--adapt-bn runs with the standard LOSO and the --model comparison run (not --hierarchical, --ablation or --sweep)")
    elif args.adapt_bn_sequential:
        ap.error("--adapt-bn-sequential needs --adapt-bn")
    if args.adapt_entropy is not None:
        from . import tta
        try:
            args.adapt_entropy = tta.parse_flag(args.adapt_entropy)
            tta.check_settings(**args.adapt_entropy, params=args.adapt_entropy_params or "bn",
                               batch=64 if args.adapt_entropy_batch is None else args.adapt_entropy_batch)
        except ValueError as e:
            ap.error(f"--adapt-entropy: {e}")
        if args.hierarchical or args.ablation or args.sweep:
            ap.error("--adapt-entropy runs with the standard LOSO and the --model comparison run (not --hierarchical, --ablation or --sweep)")
    elif args.adapt_entropy_sequential or args.adapt_entropy_params is not None or args.adapt_entropy_batch is not None:
        ap.error("--adapt-entropy-params / --adapt-entropy-batch / --adapt-entropy-sequential need --adapt-entropy")
    if args.attribute is not None:
        from .attribute import check_bin, check_steps
        try:
            args.attribute = check_steps(args.attribute)
            args.attribute_bin = check_bin(args.attribute_bin)
        except ValueError as e:
            ap.error(f"--attribute: {e}")
        if args.hierarchical or args.ablation or args.sweep:
            ap.error("--attribute runs with the standard LOSO and the --model comparison run (not --hierarchical, --ablation or --sweep)")
    elif args.attribute_bin is not None:
        ap.error("--attribute-bin needs --attribute")
    if args.mc_dropout is not None:
        from .uncertainty import check_samples, check_seed
        try:
            args.mc_dropout = check_samples(args.mc_dropout)
            args.mc_seed = check_seed(0 if args.mc_seed is None else args.mc_seed)
        except ValueError as e:
            ap.error(f"--mc-dropout: {e}")
        if args.hierarchical or args.ablation or args.sweep:
            ap.error("--mc-dropout runs with the standard LOSO and the --model comparison run (not --hierarchical, --ablation or --sweep)")
    elif args.mc_seed is not None:
        ap.error("--mc-seed needs --mc-dropout")
    try:
        args.seeds = ensemble_mod.check_seeds(args.seeds)
    except ValueError as e:
        ap.error(f"--seeds: {e}")
    if args.seeds > 1 and args.hierarchical:
        ap.error("--seeds runs with the standard LOSO, --model, --ablation and --sweep (not --hierarchical)")
    if args.distill is not None:
        try:
            args.distill = distill_mod.Distillation.parse(args.distill).spec()
        except ValueError as e:
            ap.error(f"--distill: {e}")
        if args.hierarchical:
            ap.error("--distill runs with the standard LOSO, --model, --ablation and --sweep (not --hierarchical)")
    try:
        args.max_grad_norm = grad_clip_setting(args.max_grad_norm)
    except ValueError as e:
        ap.error(f"--max-grad-norm: {e}")
    if args.sam is not None:
        try:
            args.sam = sam_mod.Sam.parse(args.sam)
        except ValueError as e:
            ap.error(f"--sam: {e}")
        if args.subject_adversarial is not None:
            ap.error("--sam cannot be combined with --subject-adversarial: the discriminator's own Adam would advance in both passes of a step")
        args.sam = args.sam.spec() if args.sam.on else None         # --sam 0 is the run without the flag
    if args.augment is not None:
        try:
            args.augment = Augment.parse(args.augment)
            if args.synthetic is not None:          # its window length is known here; a data directory's when the loaders are made
                args.augment.check_window(args.samples)
        except ValueError as e:
            ap.error(f"--augment: {e}")
    try:
        args.label_smoothing = label_smoothing_setting(args.label_smoothing)
    except ValueError as e:
        ap.error(f"--label-smoothing: {e}")
    if args.mixup is not None:
        try:
            args.mixup = Mixup(args.mixup)
        except ValueError as e:
            ap.error(f"--mixup: {e}")
        if args.synthetic is not None and (args.samples < 4 or args.samples % 4):
            ap.error(f"--mixup: the window length must be a multiple of 4, got {args.samples}")
    if args.subject_adversarial is not None:
        try:
            args.subject_adversarial = adversary_mod.settings(dict(lam=args.subject_adversarial, schedule=args.adversary_schedule or "ganin",
                                                                   lr_mult=1.0 if args.adversary_lr_mult is None else args.adversary_lr_mult))
        except ValueError as e:
            ap.error(f"--subject-adversarial: {e}")
    elif args.adversary_schedule is not None or args.adversary_lr_mult is not None:
        ap.error("--adversary-schedule / --adversary-lr-mult need --subject-adversarial")
    if args.group_dro is not None:
        try:
            args.group_dro = dro_mod.parse(args.group_dro, args.dro_groups)
            dro_mod.check_batch_size(args.batch_size)
        except ValueError as e:
            ap.error(f"--group-dro: {e}")
        if args.mixup is not None:
            ap.error("--group-dro cannot be combined with --mixup: a row blended from two subjects has no group")
    elif args.dro_groups is not None:
        ap.error("--dro-groups needs --group-dro")
    if args.supcon is not None:
        try:
            args.supcon = supcon_mod.parse(args.supcon, args.supcon_positives)
        except ValueError as e:
            ap.error(f"--supcon: {e}")
        supcon_mod.check_batch_size(args.batch_size)          # ValueError, before any data or GPU work
        if args.mixup is not None:
            raise ValueError("--supcon cannot be combined with --mixup: a row blended from two windows has no label to contrast")
    elif args.supcon_positives is not None:
        ap.error("--supcon-positives needs --supcon")
    if args.weight_average is not None:
        try:
            spec = averaging_mod.parse_flag(args.weight_average)
            if args.average_bn is not None:
                spec["bn"] = args.average_bn
            if args.average_validate:
                spec["validate"] = True
            args.weight_average = averaging_mod.settings(spec)
        except ValueError as e:
            ap.error(f"--weight-average: {e}")
        if args.hierarchical or args.ablation or args.sweep:
            ap.error("--weight-average runs with the standard LOSO and the --model comparison run (not --hierarchical, --ablation or --sweep)")
    elif args.average_bn is not None or args.average_validate:
        ap.error("--average-bn / --average-validate need --weight-average")
    if args.norm_reference is not None:
        try:
            for ref in args.norm_reference:
                parse_reference(ref)
        except ValueError as e:
            ap.error(f"--norm-reference: {e}")
        if len(set(args.norm_reference)) != len(args.norm_reference):
            ap.error("--norm-reference: every reference once")
        if len(args.norm_reference) > 1:
            if len(set(args.model)) > 1:
                ap.error("--norm-reference with several values takes one --model kind; run the kinds as separate jobs")
            if args.hierarchical:
                ap.error("--norm-reference with several values runs with the standard LOSO, --ablation and --sweep (not --hierarchical)")
            post = [flag for flag, on in (("--calibrate", args.calibrate), ("--adapt-bn", args.adapt_bn is not None),
                                          ("--adapt-entropy", args.adapt_entropy is not None), ("--attribute", args.attribute is not None), ("--mc-dropout", args.mc_dropout is not None),
                                          ("--seeds", args.seeds > 1), ("--weight-average", args.weight_average is not None)) if on]
            if post:
                ap.error(f"--norm-reference with several values does not combine with {', '.join(post)}; give one reference")
    return args


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", type=Path, default=None, help="directory with {sid}_X.npy/_y.npy and _channel_names.txt")
    ap.add_argument("--synthetic", type=Path, default=None, help="generate (if missing) and use a synthetic dataset here")
    ap.add_argument("--synthetic-windows", type=int, default=270)
    ap.add_argument("--samples", type=int, default=3840)
    ap.add_argument("--channels", nargs="+", default=None)
    ap.add_argument("--ablation", action="store_true",
                    help="channel-ablation sweep {ECG-only, EDA-only, chest-only, wrist-only} x all folds as one sharded job")
    ap.add_argument("--sweep", nargs="+", default=None, metavar="NAME=CH1,CH2",
                    help="custom sweep: one LOSO run per named channel set, all folds of all sets sharded together")
    ap.add_argument("--epochs", type=int, default=EPOCHS)
    ap.add_argument("--patience", type=int, nargs="+", default=[PATIENCE], help="early-stopping patience; several values = a per-fold cycle")
    ap.add_argument("--batch-size", type=int, default=BATCH_SIZE)
    ap.add_argument("--eval-batch-size", type=int, default=EVAL_BATCH_SIZE,
                    help="batch size of the validation / test passes (per-window results do not depend on it; 0 = --batch-size, the reference's loaders)")
    ap.add_argument("--subjects", nargs="+", default=None)
    ap.add_argument("--out", type=Path, default=Path("./output"))
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--concurrent-folds", type=int, default=15,
                    help="folds resident per GPU at a time (as lockstep fold batches; with --no-lockstep at most MAX_TRAIN_STREAMS = 4 of them train at once); 1 = sequential")
    ap.add_argument("--lockstep-groups", type=int, default=4, help="fold batches per configuration, each on its own HIP stream")
    ap.add_argument("--hierarchical", action="store_true",
                    help="the reference's hierarchical experiment (main.py:159-247): M1 stress vs rest + M2 amusement vs baseline per fold")
    ap.add_argument("--adaptive-forms", action="store_true",
                    help="let the GRU kernel form of a fold batch follow the folds still active in each launch (faster on one GPU; a "
                         "fold's last bits then depend on its companions — by default they do not depend on grouping or rank count)")
    ap.add_argument("--window-spread", type=int, default=0, help="synthetic set: subjects get --synthetic-windows +- this many windows")
    ap.add_argument("--no-lockstep", action="store_true",
                    help="train concurrent folds on one HIP stream each instead of as one fold batch (msig_*_multi)")
    ap.add_argument("--difficulty", type=float, default=1.0, help="noise scale of the synthetic dataset")
    ap.add_argument("--normalise", choices=["host", "device"], default="host", help="where the per-subject z-score runs")
    ap.add_argument("--norm-reference", nargs="+", default=None, metavar="REF",
                    help="which windows supply each subject's normalisation mean and std (all of its windows are then transformed with "
                         "them): subject = every window (the default, transductive for the test subject), baseline = the windows of the "
                         "baseline phase (raw protocol label 1), baseline:K = the first K of those (60 + 10 (K - 1) seconds of rest).  A "
                         "subject without a baseline window keeps the subject rule, with a warning.  expanding | trailing:K | "
                         "decayed:H = causal: window n is normalised with the windows up to n in file order — all of them, the last K, "
                         "or all at a half-life of H windows — the rows monitor.py / live.py feed the model under the same --reference "
                         "(--reference auto picks it).  One value: that reference in every "
                         "driver and with every option.  Several: one job with one LOSO per reference on shared splits, seeds and fold "
                         "batches, and normalisation.txt / normalisation.json with the paired differences (one --model kind, not "
                         "--hierarchical, no post-LOSO option)")
    ap.add_argument("--class-weights", choices=["none", "balanced"], default=CLASS_WEIGHTS,
                    help="class-weighted CrossEntropyLoss for training, validation and test losses: 'balanced' = N / (K * count_c) over "
                         "each model's own training labels (M1 and M2 separately in --hierarchical)")
    ap.add_argument("--max-grad-norm", type=float, default=None, metavar="X",
                    help="torch.nn.utils.clip_grad_norm_(model.parameters(), X) between backward and Adam inside the fused train step "
                         "(every mode: LOSO, --ablation, --hierarchical, --model, sequential); logs each epoch's gradient norms")
    ap.add_argument("--sam", default=None, metavar="RHO[:adaptive[:ETA]]",
                    help="sharpness-aware minimisation inside the fused train step: per batch the gradient at w, a step of length RHO "
                         "along it, the gradient there (same dropout masks), and Adam at w with that second gradient; ':adaptive' = ASAM "
                         "with T_w = |w| + ETA (default 0.01).  A step costs about two (every mode: LOSO, --ablation, --sweep, "
                         "--hierarchical, --model, --seeds, --distill, sequential; not with --subject-adversarial); logs each epoch's "
                         "sam_grad_norm and sam_sharpness; 0 = off")
    ap.add_argument("--augment", default=None, metavar="SPEC",
                    help="augment every training batch inside its gather launch, e.g. scale=0.1,jitter=0.05,mask=0.5:320,chandrop=0.1: "
                         "per-channel gain 1 + scale * g, additive noise jitter * g per sample, with probability mask=P one zeroed span of "
                         "1..N samples per window, each channel zeroed with probability chandrop (every mode: LOSO, --ablation, "
                         "--hierarchical, --model, sequential; validation, test and --calibrate never augment)")
    ap.add_argument("--label-smoothing", type=float, default=None, metavar="E",
                    help="CrossEntropyLoss(label_smoothing=E), 0 <= E < 1, inside the fused step; like the criterion it is, it applies to "
                         "training, validation and test losses (every mode: LOSO, --ablation, --hierarchical, --model, sequential)")
    ap.add_argument("--mixup", type=float, default=None, metavar="ALPHA",
                    help="mixup of every training batch inside its gather launch: row b is blended with row B-1-b, lam ~ Beta(ALPHA, ALPHA) "
                         "per batch and fold, and the loss is taken against both labels (every mode; composes with --augment: augment, "
                         "then mix; validation, test and --calibrate never mix)")
    ap.add_argument("--subject-adversarial", type=float, nargs="?", const=0.1, default=None, metavar="LAMBDA",
                    help="subject-adversarial training (DANN): a subject discriminator on the 128-d feature, trained inside every training "
                         "step, whose gradient is reversed into the extractor with weight LAMBDA (bare flag: 0.1; 0 = probe mode: the "
                         "discriminator only measures how subject-identifiable the feature is and the model's bits are unchanged).  Every "
                         "mode: LOSO, --ablation, --hierarchical, --model, sequential; batch sizes up to 256; writes adversary.txt / "
                         "adversary.json")
    ap.add_argument("--group-dro", type=float, nargs="?", const=dro_mod.DEFAULT_ETA, default=None, metavar="ETA",
                    help="group-DRO over the training subjects (Sagawa et al., 2020, the online algorithm): every fold keeps one adversarial "
                         "weight per group, raised with that group's loss at step size ETA (default 0.01) inside every training step, "
                         "and the step descends the weighted sum of the groups' losses instead of the pooled mean (include/msig_dro.h); "
                         "ETA 0 is the probe mode: uniform weights, the per-subject losses are measured; every training mode: LOSO, "
                         "--ablation / --sweep, --hierarchical, --model, --seeds, --distill, sequential; batch sizes up to 2048; not "
                         "with --mixup; writes dro.txt / dro.json")
    ap.add_argument("--dro-groups", choices=list(dro_mod.GROUPS), default=None,
                    help="the groups of --group-dro: a fold's training subjects (default) or its (subject, class) pairs")
    ap.add_argument("--supcon", nargs="?", const="", default=None, metavar="WEIGHT[:TAU]",
                    help="supervised contrastive loss (Khosla et al., 2020) on the 128-d feature the classifier sees, added to the "
                         f"criterion with WEIGHT (default {supcon_mod.DEFAULT_WEIGHT:g}) at temperature TAU (default {supcon_mod.DEFAULT_TAU:g}) "
                         "inside every training step (include/msig_sc.h); WEIGHT 0 measures the loss and trains as without it; not with "
                         "--mixup, batches of at most 2048; history and the epoch line gain supcon_loss / supcon_top1 / supcon_anchors; "
                         "writes supcon.txt / supcon.json")
    ap.add_argument("--supcon-positives", choices=list(supcon_mod.POSITIVES), default=None,
                    help="the positives of --supcon: every window of the anchor's class (default), or only those of its class from a "
                         "different subject (windows of the same class and subject are then neither positives nor negatives)")
    ap.add_argument("--adversary-schedule", choices=list(adversary_mod.SCHEDULES), default=None,
                    help="lambda over the training steps: ganin = LAMBDA * (2 / (1 + exp(-10 p)) - 1), p the fraction of the epoch budget "
                         "done (default), or constant")
    ap.add_argument("--adversary-lr-mult", type=float, default=None, metavar="X",
                    help="the discriminator's learning rate as a multiple of the model's (default 1)")
    ap.add_argument("--weight-average", default=None, metavar="ema[:DECAY]|swa[:START_EPOCH]",
                    help="keep an averaged copy of every fold's weights and BatchNorm statistics beside the model: ema = an exponential "
                         "moving average updated after every train step (DECAY in [0, 1), default 0.99, with a 10-update warm-up), swa = "
                         "the mean of the epoch-end weights from epoch START_EPOCH on (default 10).  One more streaming launch per step "
                         "(ema) or epoch (swa); training, early stopping, best_model.pt and every LOSO number are unchanged.  After each "
                         "fold writes averaged_model.pt, evaluates it on the fold's validation and test windows and writes averaging.txt / "
                         "averaging.json (standard LOSO and --model comparison runs; combines with every training-time option and with "
                         "--calibrate, --adapt-bn, --attribute and --mc-dropout, which keep acting on the LOSO model)")
    ap.add_argument("--average-bn", choices=list(averaging_mod.BN_MODES), default=None,
                    help="BatchNorm statistics of the averaged model: average = averaged like the weights (ema's default), recompute = "
                         "re-estimated on the fold's training windows under the averaged weights after training (swa's default)")
    ap.add_argument("--average-validate", action="store_true",
                    help="also run each epoch's validation pass under the averaged model and log it (val_loss_avg / val_acc_avg / "
                         "val_f1_avg in the history); it steers nothing")
    ap.add_argument("--model", nargs="+", choices=list(MODEL_PARAMS), default=[MODEL_TO_USE],
                    help="model kind(s): cnn_gru_attention (the reference's model) and/or cnn_gru (the baseline without ChannelAttention). "
                         "Two kinds run the LOSO (or each sweep set) once per kind as one job, with paired folds, and write "
                         "comparison.txt / comparison.json")
    ap.add_argument("--calibrate", type=int, default=0, metavar="N",
                    help="after each fold's test pass, few-shot subject calibration: re-fit the classifier (frozen CNN + GRU) on the first N "
                         "windows per class of the test subject and evaluate the LOSO model and the calibrated head on the remaining "
                         "windows; writes calibration.txt / calibration.json (0 = off; standard LOSO and --model comparison runs)")
    ap.add_argument("--calibration-gap", type=int, default=None,
                    help="windows dropped on either side of a calibration window (overlapping windows; default 5)")
    ap.add_argument("--calibration-epochs", type=int, default=None, help="head epochs of the calibration (default 30)")
    ap.add_argument("--calibration-lr", type=float, default=None, help="learning rate of the calibration (default: the run's LEARNING_RATE)")
    ap.add_argument("--calibration-sequential", action="store_true",
                    help="calibrate with one launch per fold and epoch instead of one per epoch for all folds of a rank (the same bits)")
    ap.add_argument("--adapt-bn", type=float, nargs="?", const=1.0, default=None, metavar="ALPHA",
                    help="after each fold's test pass, label-free BatchNorm adaptation (AdaBN): every weight as trained, the BatchNorm "
                         "running statistics re-estimated on the test subject's unlabelled windows and blended as (1 - ALPHA) * trained + "
                         "ALPHA * subject (bare flag: 1.0); evaluates the LOSO model and the adapted one on the same windows and writes "
                         "adaptation.txt / adaptation.json (standard LOSO and --model comparison runs; may be combined with --calibrate, "
                         "each on its own against the LOSO model)")
    ap.add_argument("--adapt-bn-sequential", action="store_true",
                    help="adapt with single calls per fold instead of one fold batch for all folds of a rank (the same bits)")
    ap.add_argument("--adapt-entropy", nargs="?", const="", default=None, metavar="LR[:EPOCHS[:DIVERSITY]]",
                    help="after each fold's test pass, label-free entropy-minimisation adaptation (TENT) of a COPY of the fold's model on "
                         "the test subject's unlabelled windows: every weight frozen but the BatchNorm scale and shift (see "
                         "--adapt-entropy-params), which take EPOCHS passes (default 1) of Adam at LR (default 1e-3) down the entropy of the "
                         "model's own eval-mode predictions, less DIVERSITY (default 0) times the entropy of a batch's mean prediction; "
                         "evaluates the LOSO model and the adapted one on the same windows and writes entropy_adaptation.txt / "
                         "entropy_adaptation.json with the prediction entropy, flipped predictions and predicted-class shares; with "
                         "--adapt-bn it starts from the AdaBN statistics and the table has the AdaBN column too (standard LOSO and --model "
                         "comparison runs; replica 0 under --seeds)")
    ap.add_argument("--adapt-entropy-params", choices=("bn", "bn+gate", "all"), default=None,
                    help="the tensors --adapt-entropy lets move: the BatchNorm scale and shift (default), those and ChannelAttention's two "
                         "matrices, or every parameter")
    ap.add_argument("--adapt-entropy-batch", type=int, default=None, metavar="B", help="windows per adaptation step (default 64, at most 2048)")
    ap.add_argument("--adapt-entropy-sequential", action="store_true",
                    help="adapt with single calls per fold instead of one fold batch for all folds of a rank (the same bits)")
    ap.add_argument("--attribute", type=int, nargs="?", const=32, default=None, metavar="STEPS",
                    help="after each fold's test pass, integrated-gradients attribution of the fold's model on the test subject's windows "
                         "(zero baseline, each window's predicted class, STEPS midpoints of the path, 1..256; bare flag: 32): which channels "
                         "and which seconds the decision rests on, the gate's values and a forward-only channel-occlusion column; writes "
                         "attribution.txt / attribution.json (standard LOSO and --model comparison runs; may be combined with --calibrate "
                         "and --adapt-bn, each on its own against the LOSO model)")
    ap.add_argument("--attribute-bin", type=int, default=None, metavar="SAMPLES",
                    help="samples per time bin of the attribution's time profile (default max(1, T // 60): one-second bins of 60-second windows)")
    ap.add_argument("--mc-dropout", type=int, nargs="?", const=32, default=None, metavar="S",
                    help="after each fold's test pass, Monte-Carlo dropout of the fold's model on the test subject's windows: S stochastic "
                         "passes (1..256; bare flag: 32) with both dropout masks on and BatchNorm in its eval form, the deterministic trunk "
                         "run once per window; predictive entropy, mutual information, AUROC of the entropy as an error detector, "
                         "selective accuracy at 100 / 90 / 80 / 50 %% coverage and ECE; writes uncertainty.txt / uncertainty.json (standard "
                         "LOSO and --model comparison runs; may be combined with --calibrate, --adapt-bn and --attribute, each on its own "
                         "against the LOSO model)")
    ap.add_argument("--mc-seed", type=int, default=None, metavar="SEED", help="seed of the Monte-Carlo dropout masks (default 0)")
    ap.add_argument("--distill", nargs="?", const="0.5:2", default=None, metavar="ALPHA[:T]",
                    help="after each fold's --seeds S replicas (S >= 1; S = 1 is born-again self-distillation) train one student of the "
                         "fold against their ensemble's tempered probabilities as well as the labels: weight ALPHA in [0, 1] of the "
                         "teacher's term (T^2 KL at temperature T in [1/64, 64], default 2) and 1 - ALPHA of the criterion; without a "
                         "value 0.5:2.  The student has replica 0's seed, split and every training option (ALPHA 0 reproduces replica 0 "
                         "bit for bit), trains as one more fold-batch unit and writes its per-fold files under distilled/; "
                         "distilled_result.json per fold and distillation.txt / distillation.json compare ensemble, mean member, "
                         "replica 0 and student (not with --hierarchical)")
    ap.add_argument("--seeds", type=int, default=1, metavar="S",
                    help="train S seed replicas (1..64) of every fold as fold-batch units: the same train / validation split, unit seed "
                         "SEED + fold + r * 1000003 for replica r (initialisation, shuffle order, dropout, augmentation and mixup draws). "
                         "Replica 0 is the run without the flag and writes its files; replica r >= 1 writes under seed_<r>/.  After "
                         "training each fold's replicas are evaluated on its test subject as a deep ensemble (ensemble_result.json), "
                         "and seeds.txt / seeds.json hold the LOSO means per seed with their spread, the ensemble and mean-member rows "
                         "and, with several configurations, the paired differences over seeds.  Every training-time option applies to "
                         "all replicas; --calibrate, --adapt-bn, --attribute and --mc-dropout act on replica 0 (not with --hierarchical)")
    return ap


def build_cfg(args, kinds):
    """The configuration of the parsed command line, before the data set is known (no GPU needed); keys of optional features
    (max_grad_norm, augment, calibrate ...) exist only when their flag was given."""
    cfg = default_cfg()
    cfg.update(epochs=args.epochs, patience=args.patience[0] if len(args.patience) == 1 else list(args.patience), batch_size=args.batch_size,
               verbose=args.verbose,
               concurrent_folds=args.concurrent_folds, normalise=args.normalise, eval_batch_size=args.eval_batch_size,
               lockstep=not args.no_lockstep, lockstep_groups=args.lockstep_groups, adaptive_forms=args.adaptive_forms,
               class_weights=args.class_weights, model=kinds[0], model_params=dict(MODEL_PARAMS[kinds[0]]))
    if args.max_grad_norm is not None:      # without the flag the configuration has no such key
        cfg["max_grad_norm"] = args.max_grad_norm
    if args.sam is not None:                # likewise
        cfg["sam"] = args.sam
    if args.augment is not None:            # likewise
        cfg["augment"] = args.augment
    if args.label_smoothing is not None:    # likewise
        cfg["label_smoothing"] = args.label_smoothing
    if args.mixup is not None:              # likewise
        cfg["mixup"] = args.mixup
    if args.subject_adversarial is not None:      # likewise; refused here, before any data or GPU work, for a batch size it cannot take
        adversary_mod.check_batch_size(args.batch_size)
        cfg.update(adversary=args.subject_adversarial, synthetic=args.synthetic is not None)
    if args.group_dro is not None:                # likewise
        cfg.update(group_dro=args.group_dro, synthetic=args.synthetic is not None)
    if args.supcon is not None:                   # likewise
        cfg.update(supcon=args.supcon, synthetic=args.synthetic is not None)
    if args.weight_average is not None:           # likewise
        cfg.update(averaging=args.weight_average, synthetic=args.synthetic is not None)
    if args.calibrate:        # without the flag the configuration — and with it every log, summary and result — is what it was
        cfg.update(calibrate=args.calibrate, synthetic=args.synthetic is not None, calibration_batched=not args.calibration_sequential)
        for key, val in (("calibration_gap", args.calibration_gap), ("calibration_epochs", args.calibration_epochs),
                         ("calibration_lr", args.calibration_lr)):
            if val is not None:
                cfg[key] = val
    if args.adapt_bn is not None:      # likewise: without the flag there is no such key
        cfg.update(adapt_bn=args.adapt_bn, synthetic=args.synthetic is not None, adapt_bn_batched=not args.adapt_bn_sequential)
    if args.adapt_entropy is not None:      # likewise
        cfg.update(adapt_entropy=dict(args.adapt_entropy), synthetic=args.synthetic is not None,
                   adapt_entropy_batched=not args.adapt_entropy_sequential)
        if args.adapt_entropy_params is not None:
            cfg["adapt_entropy_params"] = args.adapt_entropy_params
        if args.adapt_entropy_batch is not None:
            cfg["adapt_entropy_batch"] = args.adapt_entropy_batch
    if args.attribute is not None:     # likewise
        cfg.update(attribute=args.attribute, synthetic=args.synthetic is not None)
        if args.attribute_bin is not None:
            cfg["attribute_bin"] = args.attribute_bin
    if args.mc_dropout is not None:    # likewise
        cfg.update(mc_dropout=args.mc_dropout, mc_seed=args.mc_seed, synthetic=args.synthetic is not None)
    if args.seeds > 1:                 # likewise: --seeds 1 is the run without the flag
        cfg.update(seeds=args.seeds, synthetic=args.synthetic is not None)
    if args.distill is not None:       # likewise
        cfg.update(distill=args.distill, synthetic=args.synthetic is not None)
    if args.norm_reference is not None:      # likewise; several values: the list, which main() turns into one configuration each
        refs = list(args.norm_reference)
        cfg.update(norm_reference=refs[0] if len(refs) == 1 else refs, synthetic=args.synthetic is not None)
    return cfg


def main(argv=None):
    ap = build_parser()
    args = parse_args(ap, argv)
    kinds = [k for k in MODEL_PARAMS if k in args.model]          # attention model first, whatever the order given
    if len(kinds) > 1 and args.hierarchical:
        ap.error("--hierarchical takes one --model kind (M1 and M2 are both of that kind); run the kinds as separate jobs")

    # Concurrent folds need their own hardware queues: with the runtime's default of 4, fifteen streams share four
    # queues and serialise (1649 -> 2914 train steps/s at 15 folds with 16 queues, tools/concurrency_probe.py).
    # Read by the HIP runtime when it initialises, so it has to be set before the first GPU call.
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
    world, rank, local_rank = int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("RANK", 0)), int(os.environ.get("LOCAL_RANK", 0))
    # one process per GPU over RCCL; MSIG_DIST_BACKEND=gloo (and ranks sharing a GPU) only to rehearse on a 1-GPU box
    backend = os.environ.get("MSIG_DIST_BACKEND", "nccl")
    local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world > 1:
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(backend)
    cfg = build_cfg(args, kinds)
    if args.synthetic is not None:
        from .synth import CHANNELS6, make_synthetic_wesad
        if rank == 0 and not (args.synthetic / "_channel_names.txt").exists():
            make_synthetic_wesad(args.synthetic, windows_per_subject=args.synthetic_windows, T=args.samples, difficulty=args.difficulty,
                                 window_spread=args.window_spread)
        if world > 1:
            dist.barrier(device_ids=[local_rank]) if backend == "nccl" else dist.barrier()
        cfg.update(data_path=args.synthetic, channels=list(CHANNELS6))
    elif args.data is not None:
        cfg.update(data_path=args.data)
    if args.channels:
        cfg.update(channels=args.channels)
    if args.subjects:
        cfg.update(subjects=args.subjects)
    torch.manual_seed(cfg["seed"])
    np.random.seed(cfg["seed"])
    stamp = datetime.now().strftime("%Y%m%d_%H%M%S")
    run_output_dir = args.out / RUN_NAME / f"run_{stamp}"
    if rank == 0:
        run_output_dir.mkdir(parents=True, exist_ok=True)
        print(f"====== 运行结果将保存至: {run_output_dir} ====== ({world} GPU(s))")
    if world > 1:
        box = [str(run_output_dir)]
        dist.broadcast_object_list(box, src=0)
        run_output_dir = Path(box[0])
    with open(Path(cfg["data_path"]) / "_channel_names.txt") as f:
        all_channel_names = [ln.strip() for ln in f if ln.strip()]
    cfg["gather_device"] = device if backend == "nccl" else torch.device("cpu")
    sets = None
    if args.ablation:
        sets = ablation_sets(all_channel_names)
    if args.sweep:
        sets = dict(sets or {})
        for item in args.sweep:
            name, _, chans = item.partition("=")
            if not name or not chans:
                ap.error(f"--sweep expects NAME=CH1,CH2,... (got {item!r})")
            sets[name] = chans.split(",")
    refs = cfg.get("norm_reference")
    if args.hierarchical:
        results, wall = run_hierarchical_experiment(run_output_dir, device, all_channel_names, cfg, rank, world)
    elif isinstance(refs, list):
        # one job: every (reference, set) is a configuration of its own — own store and fold batches, shared splits and seeds
        sets_ = sets or {"": list(cfg["channels"])}
        for n, ch in sets_.items():
            if len(ch) > 16:
                ap.error(f"channel set {n!r} has {len(ch)} channels; the HIP path supports at most 16")
        name = lambda ref, n: f"{reference_dir(ref)}/{n}" if n else reference_dir(ref)      # noqa: E731
        cfgs = {name(ref, n): dict(cfg, channels=list(ch), norm_reference=ref) for n, ch in sets_.items() for ref in refs}
        results, wall = run_experiments(run_output_dir, device, all_channel_names, cfgs, rank, world)
        if rank == 0:
            paired = {n: {ref: results[name(ref, n)] for ref in refs} for n in sets_}
            path = write_normalisation(run_output_dir, normalisation(paired, refs, cfg["data_path"], cfg["subjects"]),
                                       synthetic=bool(cfg.get("synthetic")))
            print(f"Normalisation-reference table written to: {path}")
    elif len(kinds) > 1:
        # one job: every (kind, set) is a configuration of its own — own fold batches and streams, shared splits and seeds
        sets_ = sets or {"": list(cfg["channels"])}
        for n, ch in sets_.items():
            if len(ch) > 16:
                ap.error(f"channel set {n!r} has {len(ch)} channels; the HIP path supports at most 16")
        cfgs = {(f"{kd}/{n}" if n else kd): dict(cfg, channels=list(ch), model=kd, model_params=dict(MODEL_PARAMS[kd]))
                for n, ch in sets_.items() for kd in kinds}
        results, wall = run_experiments(run_output_dir, device, all_channel_names, cfgs, rank, world)
        if rank == 0:
            paired = {n: {kd: results[f"{kd}/{n}" if n else kd] for kd in kinds} for n in sets_}
            path = write_comparison(run_output_dir, comparison(paired, kinds, sets_))
            print(f"模型对比已保存至: {path}")
    elif sets:
        for n, ch in sets.items():
            if len(ch) > 16:
                ap.error(f"channel set {n!r} has {len(ch)} channels; the HIP path supports at most 16")
        results, wall = run_experiments(run_output_dir, device, all_channel_names,
                                        {n: dict(cfg, channels=list(ch)) for n, ch in sets.items()}, rank, world)
    else:
        results, wall = run_simple_experiment(run_output_dir, device, all_channel_names, cfg, rank, world)
    if world > 1:
        dist.destroy_process_group()
    return results, wall


if __name__ == "__main__":
    main()
