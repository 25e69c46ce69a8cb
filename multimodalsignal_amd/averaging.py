"""Weight averaging (include/msig_wa.h): the host side of the EMA / SWA shadow of a model.

The model a fold ends with is one noisy iterate — the early-stopping checkpoint, or whatever the last step left behind.  An
averaged model is a second copy of the parameters and the BatchNorm statistics, the SHADOW, moved towards the model by one
streaming launch (``msig_wa_update[_multi]``):

* ``ema``: after every train step, ``shadow += a * (model - shadow)`` with ``a = 1 - d_t``, ``d_t = min(decay, (1 + t) / (warmup + t))``
  (``d_t = decay`` for ``warmup = 0``), t the number of updates so far; the shadow starts as a copy of the initial model.
* ``swa``: at the end of every epoch ``e >= start_epoch`` (1-based), ``a = 1 / (k + 1)`` with k the iterates averaged so far: the
  running mean of the epoch-end iterates (Izmailov et al., "Averaging weights leads to wider optima and better generalization").
  A fold that stops before ``start_epoch`` takes its end-of-training weights as its single iterate and reports ``iterates = 0``.

The coefficients are computed here, in double precision, and rounded ONCE to fp32; the arithmetic is the library's.  A
``WeightAverager`` holds one fold's counters.  The averaged model is the shadow at the END OF TRAINING — after the last train step,
before the early-stopping checkpoint is restored into the model: the restore does not touch it.  It is evaluated by the existing
forward (``runtime.Engine.forward(..., shadow=True)``, ``runtime.FoldArena.batch(..., shadow=True)``).

``bn = "recompute"`` re-estimates the averaged weights' BatchNorm statistics on the fold's own TRAINING windows after training,
with the existing ``adapt.BnAdapter`` at ``alpha = 1`` — whole-set statistics under the averaged weights, the role
``torch.optim.swa_utils.update_bn`` plays for torch's AveragedModel (which also ends with whole-set statistics: its cumulative
moving average over one pass).  ``bn = "average"`` keeps the averaged running statistics.

The averager steers nothing: scheduler, early stopping, checkpoints and every number of the LOSO model are what they are without it.
Whether averaging helps LOSO accuracy on real WESAD is not known; the synthetic set cannot decide it.
"""
from __future__ import annotations

import ctypes
import json
from pathlib import Path
from typing import Optional, Sequence

import numpy as np
import torch

MODES = ("ema", "swa")
BN_MODES = ("average", "recompute")
DEFAULT_DECAY, DEFAULT_WARMUP, DEFAULT_START_EPOCH = 0.99, 10, 10
KEYS = ("mode", "decay", "warmup", "start_epoch", "bn", "validate")
SYNTHETIC_NOTE = ("WESAD is absent: on the synthetic set the LOSO column is the checkpoint the reference's inverted early stopping restores "
                  "and the averaged column the end of a trajectory that separates the classes, so this table shows that the averaging "
                  "machinery works, not whether averaging helps on WESAD")


def _f32(v: float) -> float:
    return ctypes.c_float(v).value


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def settings(value) -> Optional[dict]:
    """config['averaging']: None (off) or a dict with ``mode`` ("ema" / "swa") and any of decay / warmup / start_epoch / bn /
    validate — checked, defaults filled in (ValueError otherwise, before any training).  decay in [0, 1), default 0.99: a horizon of
    100 steps, about two epochs of a LOSO fold (about 47 steps each); 0.999 would span most of a fold's training.  warmup >= 0,
    default 10.  start_epoch >= 1, default 10 (SWA only).  bn: "average" (EMA's default) or "recompute" (SWA's).  validate: a
    second validation pass per epoch under the shadow, reported, steering nothing."""
    if value is None:
        return None
    if not isinstance(value, dict):
        raise ValueError(f"config['averaging'] must be None or a dict, got {value!r}")
    unknown = set(value) - set(KEYS)
    if unknown:
        raise ValueError(f"config['averaging'] has unknown keys {sorted(unknown)}")
    mode = value.get("mode")
    if mode not in MODES:
        raise ValueError(f"averaging mode must be one of {MODES}, got {mode!r}")
    out = dict(mode=mode, decay=DEFAULT_DECAY, warmup=DEFAULT_WARMUP, start_epoch=DEFAULT_START_EPOCH,
               bn="average" if mode == "ema" else "recompute", validate=False)
    out.update({k: v for k, v in value.items() if v is not None})
    d = out["decay"]
    if isinstance(d, (str, bytes, bool)) or not isinstance(d, (int, float, np.floating, np.integer)) or not 0.0 <= float(d) < 1.0:
        raise ValueError(f"averaging decay must be a number in [0, 1), got {d!r}")       # NaN fails the comparison
    out["decay"] = float(d)
    if _f32(out["decay"]) >= 1.0:
        raise ValueError(f"averaging decay must be below 1 as an fp32 number, got {d!r}")
    if not _is_int(out["warmup"]) or out["warmup"] < 0:
        raise ValueError(f"averaging warmup must be an integer >= 0, got {out['warmup']!r}")
    if not _is_int(out["start_epoch"]) or out["start_epoch"] < 1:
        raise ValueError(f"averaging start_epoch must be an integer >= 1, got {out['start_epoch']!r}")
    out["warmup"], out["start_epoch"] = int(out["warmup"]), int(out["start_epoch"])
    if out["bn"] not in BN_MODES:
        raise ValueError(f"averaging bn must be one of {BN_MODES}, got {out['bn']!r}")
    if not isinstance(out["validate"], (bool, np.bool_)):
        raise ValueError(f"averaging validate must be a bool, got {out['validate']!r}")
    out["validate"] = bool(out["validate"])
    return out


def ema_coef(t: int, decay: float = DEFAULT_DECAY, warmup: int = DEFAULT_WARMUP) -> float:
    """The coefficient a = 1 - d_t of EMA update number t (from 0), double arithmetic rounded once to fp32."""
    d = float(decay) if int(warmup) == 0 else min(float(decay), (1.0 + t) / (float(warmup) + t))
    return _f32(1.0 - d)


def swa_coef(k: int) -> float:
    """The coefficient a = 1 / (k + 1) of the SWA update that adds iterate number k + 1 (k iterates already averaged)."""
    return _f32(1.0 / (int(k) + 1.0))


def parse_flag(text: str) -> dict:
    """--weight-average ema[:DECAY] | swa[:START_EPOCH] as a (not yet checked) config['averaging'] dict; ValueError for a bad form."""
    mode, sep, arg = str(text).partition(":")
    if mode not in MODES or (sep and not arg):
        raise ValueError(f"expected ema[:DECAY] or swa[:START_EPOCH], got {text!r}")
    out = {"mode": mode}
    if sep:
        try:
            if mode == "ema":
                out["decay"] = float(arg)
            else:
                out["start_epoch"] = int(arg)
        except ValueError:
            raise ValueError(f"expected ema[:DECAY] (a number) or swa[:START_EPOCH] (an integer), got {text!r}") from None
    return out


class WeightAverager:
    """One fold's averaging state: the settings, the number of updates issued and of iterates averaged, and — once `bind` has
    named it — the engine whose shadow it describes.  It issues nothing itself: a trainer asks it for the next coefficient and
    hands that to runtime.Engine.average_update or, per fold of a launch, to msig_wa_update_multi."""

    def __init__(self, cfg: dict):
        cfg = settings(cfg)
        if cfg is None:
            raise ValueError("WeightAverager needs averaging settings (a dict with a mode)")
        self.cfg = cfg
        self.mode, self.decay, self.warmup, self.start_epoch = cfg["mode"], cfg["decay"], cfg["warmup"], cfg["start_epoch"]
        self.bn, self.validate = cfg["bn"], cfg["validate"]
        self.updates = 0          # EMA: updates after train steps (the initial copy is not one); SWA: launches issued
        self.iterates = 0         # SWA: epoch-end iterates averaged
        self.ready = False        # the shadow holds a model (after the first copy)
        self.finished = False
        self.engine = None

    def bind(self, engine) -> "WeightAverager":
        self.engine = engine
        return self

    # ---- the schedule: each call returns the coefficient of the NEXT update and counts it -------------------------------------
    def start_coef(self) -> float:
        """Before the first train step: 1 (copy the initial model) for EMA, 0 (nothing) for SWA."""
        if self.mode == "ema" and not self.ready:
            self.ready = True
            return 1.0
        return 0.0

    def peek_step_coefs(self, n: int):
        """The coefficients of the next n EMA updates, without counting them (0 for SWA: it has none per step)."""
        if self.mode != "ema":
            return [0.0] * n
        return [ema_coef(self.updates + k, self.decay, self.warmup) for k in range(n)]

    def step_coef(self) -> float:
        """After a train step: EMA's a_t (and t advances); 0 for SWA."""
        if self.mode != "ema":
            return 0.0
        a = ema_coef(self.updates, self.decay, self.warmup)
        self.updates += 1
        return a

    def advance(self, n: int) -> None:
        """Counts n EMA updates issued with peek_step_coefs' coefficients."""
        if self.mode == "ema":
            self.updates += int(n)

    def epoch_coef(self, epoch: int) -> float:
        """At the end of (1-based) epoch `epoch`: SWA's 1 / (k + 1) from start_epoch on (and k advances); else 0."""
        if self.mode != "swa" or epoch < self.start_epoch:
            return 0.0
        a = swa_coef(self.iterates)
        self.iterates += 1
        self.updates += 1
        self.ready = True
        return a

    def final_coef(self) -> float:
        """At the end of training: 1 for an SWA fold that stopped before start_epoch (its end-of-training weights are its single
        iterate; `iterates` stays 0), else 0."""
        self.finished = True
        if not self.ready:
            self.ready = True
            return 1.0
        return 0.0

    def summary(self) -> dict:
        return dict(mode=self.mode, updates=self.updates, iterates=self.iterates, bn=self.bn)

    # ---- the averaged model ---------------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        """The averaged model under the reference's state_dict keys, reference shapes (the one-layer model's gathered from its
        padded shadow): loads into this repo's models and into the reference's."""
        if self.engine is None or not self.ready:
            raise RuntimeError("the averager has no averaged model yet")
        return self.engine.shadow_named()

    def save(self, path) -> Path:
        path = Path(path)
        torch.save({k: v.detach().cpu() for k, v in self.state_dict().items()}, path)
        return path


class _ShadowEngine:
    """What adapt.BnAdapter reads of an engine, over the SHADOW's buffers: the adapter then estimates the statistics of the
    averaged weights.  The padded layout is taken as it is (no scatter)."""

    def __init__(self, eng):
        self.kind, self.gru_layers, self.C, self.K, self.n_flat, self.device = eng.kind, eng.gru_layers, eng.C, eng.K, eng.n_flat, eng.device
        self.params, self.bn_state, self.bn_count = eng.avg_params, eng.avg_bn_state, eng.avg_bn_count


class _ShadowModel:
    def __init__(self, eng):
        self._eng = _ShadowEngine(eng)

    def engine(self):
        return self._eng


def training_windows(loader) -> torch.Tensor:
    """The (N, C, T) windows of a DeviceLoader's dataset, in dataset order."""
    return loader.store if loader.index is None else loader.store.index_select(0, loader.index)


def recompute_bn(engines: Sequence, loaders: Sequence, eval_batch: int = 1024, batched: bool = True):
    """bn = "recompute": the BatchNorm statistics of every engine's averaged weights, re-estimated on its own training windows by ONE
    adapt.BnAdapter (alpha = 1: whole-set statistics, stage 2 under the new stage 1) and written into the shadow's bn_state —
    torch's update_bn for an AveragedModel, with whole-set statistics.  The counts stay the model's.  Returns the adapter."""
    from .adapt import BnAdapter
    ad = BnAdapter([dict(model=_ShadowModel(e), x=training_windows(ld)) for e, ld in zip(engines, loaders)], alpha=1.0, batched=batched,
                   eval_batch=eval_batch)
    ad.adapt()
    for s, e in enumerate(engines):
        e.avg_bn_state.copy_(ad.adapted_state(s))
    return ad


# ---- the averaging table of a run ----------------------------------------------------------------------------------------------------
def fold_record(info: dict) -> Optional[dict]:
    """The averaging record of one trained fold from its fold_result.json: the LOSO model against the averaged one on the same test
    windows, both validation losses and the update / iterate counts; None for a fold trained without averaging."""
    av = info.get("averaging")
    if not av or av.get("accuracy") is None or info.get("accuracy") is None:
        return None
    return dict(subject=info["subject"], updates=av["updates"], iterates=av["iterates"],
                before={"accuracy": info["accuracy"], "f1_score": info["f1_score"]},
                after={"accuracy": av["accuracy"], "f1_score": av["f1_score"]},
                val_loss=av["loso_val_loss"], val_loss_avg=av["val_loss"])


def summarise(folds: Sequence[dict]) -> dict:
    out = {"folds": list(folds), "n_folds": len(folds), "summary": {}, "wins": {}, "ties": {}, "losses": {}}
    for m in ("accuracy", "f1_score"):
        b = np.array([f["before"][m] for f in folds], dtype=np.float64)
        a = np.array([f["after"][m] for f in folds], dtype=np.float64)
        d = a - b
        st = lambda v: {"mean": float(v.mean()) if v.size else float("nan"), "std": float(v.std()) if v.size else float("nan")}
        out["summary"][m] = {"before": st(b), "after": st(a), "difference": st(d)}
        out["wins"][m], out["ties"][m], out["losses"][m] = int((d > 0).sum()), int((d == 0).sum()), int((d < 0).sum())
    return out


def settings_line(cfg: dict) -> str:
    c = settings(cfg)
    core = f"decay={c['decay']:g} warmup={c['warmup']}" if c["mode"] == "ema" else f"start_epoch={c['start_epoch']}"
    return f"WEIGHT AVERAGING: mode={c['mode']} {core} bn={c['bn']}" + (" validate" if c["validate"] else "")


def format_averaging(table: dict, cfg: dict, synthetic: bool = False) -> str:
    lines = [settings_line(cfg),
             "The averaged model is the shadow at the end of training (the early-stopping restore does not touch it); both columns on "
             "the SAME test windows; difference = averaged - LOSO.  Whether averaging helps LOSO accuracy on real WESAD is not known."]
    if synthetic:
        lines.append("NOTE: " + SYNTHETIC_NOTE + ".")
    count = "iterates" if settings(cfg)["mode"] == "swa" else "updates"
    lines += ["", f"  {'subject':<10} {count:>8} {'LOSO acc':>10} {'avg acc':>10} {'diff':>9}   {'LOSO F1':>9} {'avg F1':>9} {'diff':>9}   "
                  f"{'val loss':>9} {'avg val':>9}"]
    for f in table["folds"]:
        b, a = f["before"], f["after"]
        lines.append(f"  {f['subject']:<10} {f[count]:>8d} {b['accuracy']:>10.4f} {a['accuracy']:>10.4f} {a['accuracy'] - b['accuracy']:>+9.4f}   "
                     f"{b['f1_score']:>9.4f} {a['f1_score']:>9.4f} {a['f1_score'] - b['f1_score']:>+9.4f}   "
                     f"{f['val_loss']:>9.4f} {f['val_loss_avg']:>9.4f}")
    lines.append("")
    for m, label in (("accuracy", "accuracy"), ("f1_score", "weighted F1")):
        sm = table["summary"][m]
        lines.append(f"  {label}: LOSO {sm['before']['mean']:.4f} ± {sm['before']['std']:.4f}   averaged {sm['after']['mean']:.4f} ± "
                     f"{sm['after']['std']:.4f}   mean paired difference {sm['difference']['mean']:+.4f} ± {sm['difference']['std']:.4f}   "
                     f"averaged wins {table['wins'][m]} of {table['n_folds']} folds, ties {table['ties'][m]}, losses {table['losses'][m]}")
    return "\n".join(lines) + "\n"


def write_averaging(run_output_dir, folds: Sequence[dict], cfg: dict, synthetic: bool = False) -> Path:
    """averaging.json (the folds' records, the pooled differences and wins, the settings) and averaging.txt in `run_output_dir`."""
    run_output_dir = Path(run_output_dir)
    table = summarise(folds)
    doc = dict(table, settings=settings(cfg))
    if synthetic:
        doc["note"] = SYNTHETIC_NOTE
    (run_output_dir / "averaging.json").write_text(json.dumps(doc, indent=1))
    path = run_output_dir / "averaging.txt"
    path.write_text(format_averaging(table, cfg, synthetic), encoding="utf-8")
    return path
