"""Seed replicas of a LOSO run and their deep-ensemble prediction (include/msig_en.h).

``--seeds S`` trains S seed replicas of every fold as fold-batch units: the same train / validation split, another initialisation,
shuffle order, dropout stream and augmentation / mixup draws (`replica_seed`).  What varies over seeds is reported (`seed_table`,
`pair_table`), and each fold's replicas are evaluated on the test subject as a deep ensemble (Lakshminarayanan et al., 2017): the
members' probabilities averaged, with the spread, the entropies and the members' disagreement per window (`Ensemble`,
msig_en_reduce / msig_en_reduce_multi).

The host helpers at the top need no GPU.  `Ensemble` has no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import json
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .runtime import Arenas, make_batch, workspace_need
from .uncertainty import COVERAGES, ECE_BINS, expected_calibration_error, window_metrics

REPLICA_STRIDE = 1_000_003      # unit seed of replica r = the fold's seed + r * REPLICA_STRIDE (a prime far above any fold index)
MAX_SEEDS = 64
SYNTHETIC_NOTE = ("synthetic data set: the classes are planted and easy, so the table shows that the seed-replica and ensemble "
                  "machinery works, not what the spread over seeds or an ensemble's gain would be on WESAD")
METRIC_KEYS = ("accuracy", "f1_score", "nll", "brier", "ece", "mean_disagreement", "auroc_entropy")


# ---- the parts that need no GPU ---------------------------------------------------------------------------------------------------
def check_seeds(value) -> int:
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 1 <= int(value) <= MAX_SEEDS:
        raise ValueError(f"seeds must be an integer in 1..{MAX_SEEDS}, got {value!r}")
    return int(value)


def replica_seed(seed: int, fold: int, replica: int = 0) -> int:
    """The unit seed of replica `replica` of fold `fold`: replica 0 has the seed every fold has without --seeds (seed + fold).  The
    train / validation split is NOT seeded by it: all replicas of a fold share split_train_val(..., seed)."""
    return int(seed) + int(fold) + int(replica) * REPLICA_STRIDE


def replica_name(name: str, replica: int) -> str:
    """The configuration name replica `replica` of configuration `name` runs under — and, below the run directory, the directory it
    writes to: replica 0 is the configuration itself, replica r >= 1 its seed_<r>/."""
    return name if replica == 0 else (f"{name}/seed_{replica}" if name else f"seed_{replica}")


def deal_replicas(units: Sequence[tuple], mine: Sequence[int], seeds: int):
    """From a job's (configuration, fold) units and a rank's share of them (main.rank_units) to the units with `seeds` replicas
    each: unit u's replica r is unit u * seeds + r, (replica_name(configuration, r), fold), and a rank that holds u holds all its
    replicas.  Returns units, mine, groups — `groups` the rank's share by replica configuration, in order of first appearance, the
    way rank_units groups by configuration.  seeds = 1 returns what went in."""
    S = check_seeds(seeds)
    xunits = [(replica_name(n, r), k) for n, k in units for r in range(S)]
    xmine = [u * S + r for u in mine for r in range(S)]
    groups: Dict[str, List[int]] = {}
    for u in xmine:
        groups.setdefault(xunits[u][0], []).append(u)
    return xunits, xmine, list(groups.values())


def _mean_std(v) -> dict:
    v = np.asarray(v, dtype=np.float64)
    return {"mean": float(v.mean()), "std": float(v.std(ddof=1)) if v.size > 1 else None}


def seed_table(values) -> dict:
    """`values`: (S, F) — seed replica x fold — of one metric.  per_seed = each replica's LOSO mean over the folds, with the mean
    and the SAMPLE standard deviation (ddof = 1; None for S = 1) over the seeds; per_fold = every fold's S values with their mean
    and sample standard deviation."""
    v = np.asarray(values, dtype=np.float64)
    if v.ndim != 2 or v.shape[0] < 1 or v.shape[1] < 1:
        raise ValueError(f"seed_table takes a (seeds, folds) table, got shape {tuple(v.shape)}")
    per_seed = v.mean(axis=1)
    return dict(seeds=int(v.shape[0]), folds=int(v.shape[1]), per_seed=per_seed.tolist(), **_mean_std(per_seed),
                per_fold=[dict(members=v[:, f].tolist(), **_mean_std(v[:, f])) for f in range(v.shape[1])])


def pair_table(per_seed_a, per_seed_b, ensemble_a=None, ensemble_b=None) -> dict:
    """Two configurations over the same seeds: the per-seed difference a - b of their LOSO means, its mean and sample standard
    deviation, the seeds a wins / b wins / ties, and the difference of the two ensembles' values."""
    a, b = np.asarray(per_seed_a, dtype=np.float64), np.asarray(per_seed_b, dtype=np.float64)
    if a.shape != b.shape or a.ndim != 1 or a.size < 1:
        raise ValueError("pair_table takes two per-seed vectors of equal length")
    d = a - b
    return dict(per_seed_difference=d.tolist(), **_mean_std(d), wins=int((d > 0).sum()), losses=int((d < 0).sum()), ties=int((d == 0).sum()),
                seeds=int(d.size), ensemble_difference=None if ensemble_a is None or ensemble_b is None else float(ensemble_a) - float(ensemble_b))


def ensemble_metrics(mean_p, y, entropy, mutual_info, disagreement=None) -> dict:
    """The table row of a set of windows from a (N, K) probability table, the labels and the per-window entropy and mutual
    information: accuracy and weighted F1 of the first argmax, NLL = -mean ln p[y], Brier = mean sum_k (p_k - [k = y])^2, the 15-bin
    ECE of the predicted class's probability, the mean disagreement, and uncertainty.window_metrics' entropy / mutual-information /
    AUROC / selective-accuracy columns."""
    from .trainer import accuracy_and_weighted_f1
    p, y = np.asarray(mean_p, dtype=np.float64), np.asarray(y).astype(np.int64).reshape(-1)
    if p.ndim != 2 or p.shape[0] != y.size or y.size < 1:
        raise ValueError(f"ensemble_metrics takes (N, K) probabilities and N labels, got {tuple(p.shape)} and {y.size}")
    pred = p.argmax(axis=1)
    ok = pred == y
    conf = p[np.arange(y.size), pred]
    acc, f1 = accuracy_and_weighted_f1(y, pred)
    onehot = np.zeros_like(p)
    onehot[np.arange(y.size), y] = 1.0
    w = window_metrics({"correct_eval": ok, "correct_mc": ok, "conf_eval": conf, "conf_mc": conf, "entropy": entropy,
                        "mutual_information": mutual_info})
    return {"n": int(y.size), "accuracy": acc, "f1_score": f1,
            "nll": float(-np.log(np.maximum(p[np.arange(y.size), y], np.finfo(np.float64).tiny)).mean()),
            "brier": float(((p - onehot) ** 2).sum(axis=1).mean()), "ece": expected_calibration_error(conf, ok, ECE_BINS),
            "mean_disagreement": None if disagreement is None else float(np.asarray(disagreement, dtype=np.float64).mean()),
            "entropy_correct": w["entropy_correct"], "entropy_wrong": w["entropy_wrong"],
            "mutual_information_correct": w["mutual_information_correct"], "mutual_information_wrong": w["mutual_information_wrong"],
            "auroc_entropy": w["auroc_entropy"], "selective_accuracy": w["selective_accuracy"]}


def _mean_rows(rows: Sequence[dict]) -> dict:
    """The field-wise mean of metric rows (dicts of numbers, None and nested dicts); None where any row has None."""
    out = {}
    for k, v0 in rows[0].items():
        vs = [r[k] for r in rows]
        if isinstance(v0, dict):
            out[k] = _mean_rows(vs)
        elif any(v is None for v in vs):
            out[k] = None
        elif k == "n":
            out[k] = int(v0)
        else:
            out[k] = float(np.mean(vs))
    return out


def _row_from_windows(w: dict, with_disagreement=True) -> dict:
    return ensemble_metrics(w["mean_p"], w["y"], w["entropy"], w["mutual_info"], w.get("disagreement") if with_disagreement else None)


def summarise_seeds(folds: Sequence[dict], per_seed: dict) -> dict:
    """One configuration's part of seeds.json.  `folds`: the folds' ensemble_result.json records in fold order; `per_seed`:
    {"accuracy": (S, F), "f1_score": (S, F)} — every replica's test-pass metrics.  The ensemble row and the mean-member row hold the
    LOSO mean over the folds (accuracy, F1) and the metrics of all folds' windows pooled."""
    folds = list(folds)
    acc, f1 = seed_table(per_seed["accuracy"]), seed_table(per_seed["f1_score"])
    S = acc["seeds"]
    pool = lambda ws: {k: [v for w in ws for v in w[k]] for k in ws[0]}
    ens_pooled = _row_from_windows(pool([f["windows"] for f in folds]))
    member_pooled = _mean_rows([_row_from_windows(dict(pool([f["member_windows"][r] for f in folds]), y=[v for f in folds for v in f["windows"]["y"]]),
                                                  False) for r in range(S)])
    rows = []
    for i, f in enumerate(folds):
        rows.append(dict(subject=f["subject"], n=f["n"], member_accuracy=f["member_accuracy"], member_f1=f["member_f1"],
                         member_accuracy_mean=acc["per_fold"][i]["mean"], member_accuracy_std=acc["per_fold"][i]["std"],
                         epochs=f["epochs"], ensemble_accuracy=f["ensemble"]["accuracy"], ensemble_f1=f["ensemble"]["f1_score"],
                         mean_disagreement=f["ensemble"]["mean_disagreement"]))
    return {"seeds": S, "n_folds": len(folds), "accuracy": {k: acc[k] for k in ("per_seed", "mean", "std")},
            "f1_score": {k: f1[k] for k in ("per_seed", "mean", "std")}, "folds": rows,
            "ensemble": {"loso_mean": {m: float(np.mean([f["ensemble"][m] for f in folds])) for m in ("accuracy", "f1_score")},
                         "pooled": ens_pooled},
            "mean_member": {"loso_mean": {"accuracy": acc["mean"], "f1_score": f1["mean"]}, "pooled": member_pooled}}


def _f(v, spec=".4f") -> str:
    return "n/a" if v is None else format(v, spec)


def format_seeds(doc: dict) -> str:
    """seeds.txt from the dict of seeds.json."""
    st = doc["settings"]
    lines = [f"Seed replicas: every fold trained {st['seeds']} times as fold-batch units — the same train / validation split, unit seed "
             f"SEED + fold + r * {st['stride']} (initialisation, shuffle order, dropout stream, augmentation and mixup draws); replica 0 "
             "is the run without --seeds.  LOSO mean = a replica's mean over the folds; ± is the SAMPLE standard deviation over the seeds "
             "(ddof = 1).  ensemble = the members' probabilities averaged per window of the fold's test subject (a deep ensemble); mean "
             "member = the same metric computed per member and averaged.  NLL in nats, 15-bin ECE, disagreement = share of member pairs "
             "whose predictions differ, AUROC of the predictive entropy as a detector of errors, selective accuracy with the most "
             "uncertain windows dropped first."]
    if doc.get("note"):
        lines.append("NOTE: " + doc["note"] + ".")
    for name, c in doc["configurations"].items():
        lines += ["", f"configuration {name or 'default'}: {c['seeds']} seeds x {c['n_folds']} folds"]
        for m, label in (("accuracy", "accuracy"), ("f1_score", "weighted F1")):
            lines.append(f"  LOSO mean {label} per seed: " + " ".join(_f(v) for v in c[m]["per_seed"])
                         + f"   over seeds: {_f(c[m]['mean'])} ± {_f(c[m]['std'])}")
        lines.append(f"  {'subject':<10}{'n':>6}  {'member accuracies':<{max(18, 7 * c['seeds'])}} {'mean':>7} {'± std':>8}  {'stop epochs':<{max(12, 4 * c['seeds'])}} "
                     f"{'ens acc':>8} {'ens F1':>8} {'disagree':>9}")
        for f in c["folds"]:
            lines.append(f"  {f['subject']:<10}{f['n']:>6}  {' '.join(_f(v) for v in f['member_accuracy']):<{max(18, 7 * c['seeds'])}} "
                         f"{_f(f['member_accuracy_mean']):>7} {_f(f['member_accuracy_std']):>8}  "
                         f"{' '.join(str(e) for e in f['epochs']):<{max(12, 4 * c['seeds'])}} {_f(f['ensemble_accuracy']):>8} {_f(f['ensemble_f1']):>8} "
                         f"{_f(f['mean_disagreement']):>9}")
        head = (f"  {'':<12}{'LOSO acc':>9}{'LOSO F1':>9}{'pool acc':>9}{'pool F1':>9}{'NLL':>9}{'Brier':>9}{'ECE':>9}{'disagree':>9}{'AUROC':>9}"
                + "".join(f"{'sel@' + str(k):>9}" for k in COVERAGES))
        lines += ["", head]
        for key, label in (("ensemble", "ensemble"), ("mean_member", "mean member")):
            r, p = c[key]["loso_mean"], c[key]["pooled"]
            lines.append(f"  {label:<12}{_f(r['accuracy']):>9}{_f(r['f1_score']):>9}{_f(p['accuracy']):>9}{_f(p['f1_score']):>9}{_f(p['nll']):>9}"
                         f"{_f(p['brier']):>9}{_f(p['ece']):>9}{_f(p['mean_disagreement']):>9}{_f(p['auroc_entropy']):>9}"
                         + "".join(f"{_f(p['selective_accuracy'][str(k)]):>9}" for k in COVERAGES))
        lines.append(f"  pooled windows: {c['ensemble']['pooled']['n']}")
    if doc.get("pairs"):
        lines += ["", "pairs of configurations (difference = first - second, per seed of the LOSO mean accuracy):"]
        for p in doc["pairs"]:
            lines.append(f"  {p['a'] or 'default'} - {p['b'] or 'default'}: " + " ".join(_f(v, '+.4f') for v in p["accuracy"]["per_seed_difference"])
                         + f"   mean {_f(p['accuracy']['mean'], '+.4f')} ± {_f(p['accuracy']['std'])}   first wins {p['accuracy']['wins']} of "
                         f"{p['accuracy']['seeds']} seeds, second {p['accuracy']['losses']}, ties {p['accuracy']['ties']}   "
                         f"ensemble difference {_f(p['accuracy']['ensemble_difference'], '+.4f')}")
    return "\n".join(lines) + "\n"


def write_seeds(run_output_dir, configurations: Dict[str, dict], seeds: int, synthetic: bool = False) -> Path:
    """seeds.json and seeds.txt in `run_output_dir`: `configurations` maps a configuration name to its summarise_seeds dict; with
    several, every pair also gets its pair_table (accuracy and F1)."""
    run_output_dir = Path(run_output_dir)
    doc = {"settings": {"seeds": int(seeds), "stride": REPLICA_STRIDE}, "configurations": configurations, "pairs": []}
    names = list(configurations)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            ca, cb = configurations[a], configurations[b]
            doc["pairs"].append({"a": a, "b": b, **{m: pair_table(ca[m]["per_seed"], cb[m]["per_seed"], ca["ensemble"]["loso_mean"][m],
                                                                  cb["ensemble"]["loso_mean"][m]) for m in ("accuracy", "f1_score")}})
    if synthetic:
        doc["note"] = SYNTHETIC_NOTE
    (run_output_dir / "seeds.json").write_text(json.dumps(doc, indent=1))
    path = run_output_dir / "seeds.txt"
    path.write_text(format_seeds(doc), encoding="utf-8")
    return path


# ---- the ensemble on the GPU ------------------------------------------------------------------------------------------------------
def member_files(run_dir, subject: str, config_name: Optional[str] = None) -> List[Path]:
    """The checkpoints of the fold that tested `subject` in the run at `run_dir` (configuration `config_name`): replica 0's
    fold_test_on_<subject>/best_model.pt, then every seed_<r>/fold_test_on_<subject>/best_model.pt, r = 1, 2, ... while they exist."""
    base = Path(run_dir) / config_name if config_name else Path(run_dir)
    files, r = [base / f"fold_test_on_{subject}" / "best_model.pt"], 1
    while (base / f"seed_{r}" / f"fold_test_on_{subject}" / "best_model.pt").exists():
        files.append(base / f"seed_{r}" / f"fold_test_on_{subject}" / "best_model.pt")
        r += 1
    if not files[0].exists():
        raise FileNotFoundError(files[0])
    return files


def load_members(files: Sequence, device="cuda") -> list:
    """The models of the checkpoints `files`, in eval mode on `device`; the model kind, depth, C and K are read off each checkpoint."""
    from .models import CnnGruAttentionModel, CnnGruModel
    models = []
    for f in files:
        sd = torch.load(f, weights_only=True, map_location="cpu")
        klass = CnnGruAttentionModel if "channel_attention.fc.0.weight" in sd else CnnGruModel
        with torch.random.fork_rng(devices=[]):         # the constructor draws an initialisation: torch's RNG stays where it was
            model = klass(in_channels=int(sd["cnn_encoder.0.weight"].shape[1]), num_classes=int(sd["classifier.3.weight"].shape[0]),
                          gru_hidden_size=int(sd["gru.weight_hh_l0"].shape[1]), gru_num_layers=2 if "gru.weight_ih_l1" in sd else 1)
        model.load_state_dict(sd)
        models.append(model.to(device).eval())
    return models


@dataclass
class EnsemblePrediction:
    """What Ensemble.predict returns, on the input's device — msig_en_reduce's outputs (include/msig_en.h): mean_p and std_p (N, K)
    of the members' softmax vectors (population std), pred (N,) int32 = first argmax of mean_p, entropy (N,) = H(mean_p) in nats,
    expected_entropy (N,) = the members' mean entropy, mutual_info (N,) = their difference (not clamped), votes (N, K) int32,
    member_pred (N, M) int32 = each member's first maximal logit, disagreement (N,) = share of member pairs that differ; n windows,
    `members` members."""
    mean_p: torch.Tensor
    std_p: torch.Tensor
    pred: torch.Tensor
    entropy: torch.Tensor
    expected_entropy: torch.Tensor
    mutual_info: torch.Tensor
    votes: torch.Tensor
    member_pred: torch.Tensor
    disagreement: torch.Tensor
    n: int
    members: int


class Ensemble:
    """A deep ensemble of 1..256 trained models on the GPU that share kind, depth, C and K.

    The members' parameters and BatchNorm state are COPIED at construction (the one-layer model's into its padded layout); the
    models are never written and never run: the forwards run on the ensemble's own arenas (params, bn_state, bn_count, x, ws — the
    way adapt.BnAdapter builds its set), at most MAX_FOLDS members at a time.  batched=True: one eval msig_st_forward_multi per
    chunk of members and piece of windows; with M <= MAX_FOLDS the logits are reduced where that forward left them
    (msig_en_reduce_multi), otherwise they are collected into one (M, N, K) stack and reduced by msig_en_reduce.  batched=False: one
    msig_st_forward per member, the stack, msig_en_reduce.  All routes give the same bits.  `eval_batch`: windows per piece."""

    def __init__(self, models: Sequence, batched: bool = True, eval_batch: int = 1024):
        models = list(models)
        if not 1 <= len(models) <= L.EN_MAX_MEMBERS:
            raise ValueError(f"an ensemble has 1..{L.EN_MAX_MEMBERS} members, got {len(models)}")
        if isinstance(eval_batch, bool) or int(eval_batch) < 1:
            raise ValueError(f"eval_batch must be an integer >= 1, got {eval_batch!r}")
        engines = [m.engine() for m in models]
        e0 = engines[0]
        for e in engines:
            if (e.kind, e.gru_layers, e.C, e.K, e.n_flat, e.device) != (e0.kind, e0.gru_layers, e0.C, e0.K, e0.n_flat, e0.device):
                raise ValueError("the members of an ensemble share the model kind, depth, channels, classes and device")
        self.M, self.batched, self.eval_batch = len(models), bool(batched), int(eval_batch)
        self.kind, self.gru_layers, self.C, self.K, self.n_flat, self.device = e0.kind, e0.gru_layers, e0.C, e0.K, e0.n_flat, e0.device
        self.slots = min(self.M, L.MAX_FOLDS)
        dev = self.device
        self.params = torch.zeros((self.M, self.n_flat), dtype=torch.float32, device=dev)
        self.bn_state = torch.empty((self.M, L.BN_STATE_FLOATS), dtype=torch.float32, device=dev)
        self.bn_count = torch.empty((self.M, 2), dtype=torch.int64, device=dev)
        with torch.no_grad():
            for m, e in enumerate(engines):
                if getattr(e, "index", None) is not None:       # the one-layer model: its parameters into the padded layout
                    self.params[m].index_copy_(0, e.index, e.small.detach())
                else:
                    self.params[m].copy_(e.params.detach())
                self.bn_state[m].copy_(e.bn_state)
                self.bn_count[m].copy_(e.bn_count)
        self._st = L.make_st(self.kind, 0.0)
        self._arena_key, self.arenas, self._loaded = None, None, None

    @classmethod
    def from_run(cls, run_dir, subject: str, config_name: Optional[str] = None, device="cuda", **kw) -> "Ensemble":
        """The ensemble of the fold that tested `subject` in the run at `run_dir` (configuration `config_name` of a --model / sweep
        run): replica 0's fold_test_on_<subject>/best_model.pt and every seed_<r>/fold_test_on_<subject>/best_model.pt, r = 1, 2, ...
        The model kind, depth, C and K are read off the checkpoints."""
        return cls(load_members(member_files(run_dir, subject, config_name), device), **kw)

    # ---- the arenas -------------------------------------------------------------------------------------------------------------
    def _arenas(self, T: int, sizes: Sequence[int]):
        """`slots` arenas for pieces of `sizes` windows of length T (cached: the same call again allocates nothing)."""
        key = (T, tuple(sorted(set(sizes))))
        if key == self._arena_key:
            return
        self.ws_bytes, self.T = workspace_need(key[1], self.C, T, self.K, False), T      # the evaluation layout, for every piece that runs
        self.arenas = Arenas(self.slots, self.device, (("params", self.n_flat * 4), ("bn_state", L.BN_STATE_FLOATS * 4), ("bn_count", 16),
                                                       ("x", max(key[1]) * self.C * T * 4), ("ws", self.ws_bytes)))
        self._arena_key, self._loaded = key, None

    mem, off, stride = (property(lambda self, k=k: getattr(self.arenas, k, None)) for k in ("mem", "off", "stride"))      # the arenas' own

    def _load(self, m0: int, n: int):
        """Members m0 .. m0 + n - 1 into arenas 0 .. n - 1."""
        if self._loaded == (m0, n):
            return
        for s in range(n):
            self.arenas.view(s, "params", torch.float32).copy_(self.params[m0 + s])
            self.arenas.view(s, "bn_state", torch.float32).copy_(self.bn_state[m0 + s])
            self.arenas.view(s, "bn_count", torch.int64)[:2].copy_(self.bn_count[m0 + s])
        self._loaded = (m0, n)

    def _desc(self, B: int, slot: int = 0) -> L.Batch:
        return make_batch(B, self.C, self.T, self.K, *(self.arenas.ptr(r, slot) for r in ("x", "params", "bn_state", "bn_count", "ws")),
                          self.ws_bytes, self.gru_layers)

    def _logits(self, slot: int, B: int) -> torch.Tensor:
        o = L.workspace_layout(B, self.C, self.T, self.K, False)[L.WS["LOGITS"]]
        return self.arenas.view(slot, "ws")[o:o + B * self.K * 4].view(torch.float32).view(B, self.K)

    def _check_x(self, x) -> torch.Tensor:
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.device != self.device:
            raise ValueError("an ensemble predicts on a GPU tensor on its members' device: the MI355X path has no CPU fallback")
        if x.dtype != torch.float32 or x.dim() != 3 or x.shape[1] != self.C or x.shape[0] < 1 or x.shape[2] < 16:
            raise ValueError(f"expected float32 (N, {self.C}, T >= 16) input, got {x.dtype} {tuple(x.shape)}")
        return x.detach().contiguous()

    def _fill(self, x, i: int, b: int, n: int):
        """Windows i .. i + b - 1 of x into the x buffer of arenas 0 .. n - 1 (monitor.RecordingEnsemble fills them from a recording)."""
        for s in range(n):
            self.arenas.view(s, "x", torch.float32)[:b * self.C * self.T].copy_(x[i:i + b].reshape(-1))

    def _reduce(self, x, in_slots, stacked):
        """The members' eval forwards over x in chunks of members and pieces of windows, then the reduction: with batched=True and
        M <= MAX_FOLDS `in_slots(logits0, multi, first window, windows, stream)` per piece, on the logits where
        msig_st_forward_multi left them; otherwise the logits are collected into one (M, N, K) stack for `stacked(stack, stream)`."""
        N, _, T = x.shape
        M, K, lib, st = self.M, self.K, L.lib(), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        pieces = [(i, min(self.eval_batch, N - i)) for i in range(0, N, self.eval_batch)]
        self._arenas(T, [b for _, b in pieces])
        in_place = self.batched and M <= L.MAX_FOLDS
        stack = None if in_place else torch.empty((M, N, K), dtype=torch.float32, device=self.device)
        for m0 in range(0, M, self.slots):
            n = min(self.slots, M - m0)
            self._load(m0, n)
            for i, b in pieces:
                self._fill(x, i, b, n)
                if self.batched:
                    multi = self.arenas.multi(range(n))
                    L.check(lib.msig_st_forward_multi(C.byref(self._desc(b)), C.byref(multi), C.byref(self._st), st), "msig_st_forward_multi")
                    if in_place:
                        in_slots(self._logits(0, b).data_ptr(), multi, i, b, st)
                else:
                    for s in range(n):
                        L.check(lib.msig_st_forward(C.byref(self._desc(b, s)), C.byref(self._st), st), "msig_st_forward")
                if stack is not None:
                    for s in range(n):
                        stack[m0 + s, i:i + b].copy_(self._logits(s, b))
        if stack is not None:
            stacked(stack.data_ptr(), st)

    @torch.no_grad()
    def predict(self, x) -> EnsemblePrediction:
        x = self._check_x(x)
        N, M, K, dev, lib = x.shape[0], self.M, self.K, self.device, L.lib()
        out = EnsemblePrediction(
            mean_p=torch.empty((N, K), dtype=torch.float32, device=dev), std_p=torch.empty((N, K), dtype=torch.float32, device=dev),
            pred=torch.empty((N,), dtype=torch.int32, device=dev), entropy=torch.empty((N,), dtype=torch.float32, device=dev),
            expected_entropy=torch.empty((N,), dtype=torch.float32, device=dev), mutual_info=torch.empty((N,), dtype=torch.float32, device=dev),
            votes=torch.empty((N, K), dtype=torch.int32, device=dev), member_pred=torch.empty((N, M), dtype=torch.int32, device=dev),
            disagreement=torch.empty((N,), dtype=torch.float32, device=dev), n=int(N), members=M)

        def outputs(i):
            return (out.mean_p[i:].data_ptr(), out.std_p[i:].data_ptr(), out.pred[i:].data_ptr(), out.entropy[i:].data_ptr(),
                    out.expected_entropy[i:].data_ptr(), out.mutual_info[i:].data_ptr(), out.votes[i:].data_ptr(),
                    out.member_pred[i:].data_ptr(), out.disagreement[i:].data_ptr())

        self._reduce(x,
                     lambda logits0, multi, i, b, st: L.check(lib.msig_en_reduce_multi(logits0, C.byref(multi), b, K, *outputs(i), st),
                                                              "msig_en_reduce_multi"),
                     lambda stack, st: L.check(lib.msig_en_reduce(stack, N * K, M, N, K, *outputs(0), st), "msig_en_reduce"))
        return out

    @torch.no_grad()
    def teacher(self, x, temperature: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The distillation teacher rows of the windows x (include/msig_kd.h): (N, K) float32, row n the mean over
        the members of softmax(logits / temperature) in fp64, summed in member order and rounded once.  predict()'s chunked eval
        forwards; with batched=True and M <= MAX_FOLDS msig_kd_teacher_multi reads the logits where the forward left them, otherwise
        they are collected into one (M, N, K) stack for msig_kd_teacher.  All routes give the same bits, and at temperature 1 they
        are predict()'s mean_p.  `out`: an (N, K) float32 device tensor to fill (rows of a larger table)."""
        x = self._check_x(x)
        _, temperature = L.check_distill(0.0, temperature)
        N, M, K, dev, lib = x.shape[0], self.M, self.K, self.device, L.lib()
        if out is None:
            out = torch.empty((N, K), dtype=torch.float32, device=dev)
        elif out.dtype != torch.float32 or tuple(out.shape) != (N, K) or not out.is_contiguous() or out.device != dev:
            raise ValueError(f"out must be a contiguous float32 ({N}, {K}) tensor on {dev}, got {out.dtype} {tuple(out.shape)}")
        self._reduce(x,
                     lambda logits0, multi, i, b, st: L.check(lib.msig_kd_teacher_multi(logits0, C.byref(multi), b, K, temperature,
                                                                                        out[i:].data_ptr(), st), "msig_kd_teacher_multi"),
                     lambda stack, st: L.check(lib.msig_kd_teacher(stack, N * K, M, N, K, temperature, out.data_ptr(), st), "msig_kd_teacher"))
        return out


# ---- what the driver does with a fold's replicas ------------------------------------------------------------------------------------
def fold_ensemble(models: Sequence, x, y, eval_batch: int = 1024) -> dict:
    """The record of one fold's replicas on its test subject's windows x (N, C, T) with labels y: ensemble_metrics of the ensemble
    and of the mean member, and the per-window values ("windows", "member_windows") the run's pooled rows are computed from.
    JSON-ready."""
    y = np.asarray(y.cpu() if isinstance(y, torch.Tensor) else y).astype(np.int64)
    p = Ensemble(models, eval_batch=eval_batch).predict(x)
    win = {"y": y.tolist(), "mean_p": p.mean_p.double().cpu().tolist(), "entropy": p.entropy.double().cpu().tolist(),
           "mutual_info": p.mutual_info.double().cpu().tolist(), "disagreement": p.disagreement.double().cpu().tolist()}
    members = []
    for m in models:            # a member alone: its own probabilities and entropy (M = 1: mutual information 0)
        q = Ensemble([m], eval_batch=eval_batch).predict(x)
        members.append({"mean_p": q.mean_p.double().cpu().tolist(), "entropy": q.entropy.double().cpu().tolist(),
                        "mutual_info": q.mutual_info.double().cpu().tolist()})
    return {"n": int(y.size), "members": len(models), "ensemble": _row_from_windows(win),
            "mean_member": _mean_rows([_row_from_windows(dict(w, y=win["y"]), False) for w in members]),
            "windows": win, "member_windows": members}
