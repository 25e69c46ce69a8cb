"""Monte-Carlo dropout uncertainty and selective prediction (include/msig_mc.h).

The model has two dropout sites at p = ``dropout`` — between the GRU layers and in the classifier.  Monte-Carlo dropout runs S
stochastic passes with the masks ON and BatchNorm in its EVAL form and summarises them per window: the mean probability, its
spread, the predictive entropy H(mean), the expected entropy mean_s H(p_s), their difference (the mutual information between the
prediction and the mask) and the vote split.  Everything before the first dropout site is deterministic in eval mode, so
``McDropout`` runs it ONCE per window (msig_mc_trunk), replicates its output S-fold on the device (msig_mc_expand) and runs only
the stochastic tail on the S-times wider batch (msig_mc_tail); msig_mc_reduce turns the (N * S, K) logits into the statistics.

A result is a function of (weights, x, seed, S, chunk) alone: windows are cut into chunks of ``chunk`` windows, chunk j draws its
masks under msig_dropout_key(seed, j, 1) / (seed, j, 2), and window i of the chunk, sample s, is row i * S + s of the wide batch.
Parameters, BatchNorm buffers, ``model.training``, the model's dropout step counter and torch's RNG are untouched.

The tables of a LOSO run (``--mc-dropout``) are at the end.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import json
from dataclasses import dataclass
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L

DEFAULT_SAMPLES = 32
DEFAULT_ROWS = 2048          # rows of the wide batch the default chunk fills: 128 batch tiles, under ~2 GB of workspace at T = 3840
COVERAGES = (100, 90, 80, 50)
ECE_BINS = 15
SYNTHETIC_NOTE = ("synthetic data set: the classes are planted and easy, so the table shows that the uncertainty machinery works, "
                  "not what abstention is worth on WESAD")


# ---- the parts that need no GPU ---------------------------------------------------------------------------------------------------
def check_samples(samples) -> int:
    if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)) or not 1 <= int(samples) <= L.MC_MAX_SAMPLES:
        raise ValueError(f"samples must be an integer in 1..{L.MC_MAX_SAMPLES}, got {samples!r}")
    return int(samples)


def check_seed(seed) -> int:
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"seed must be an integer in 0..2^64-1, got {seed!r}")
    return int(seed)


def default_chunk(samples: int) -> int:
    """The largest number of windows whose samples fill at most DEFAULT_ROWS rows, at least 1."""
    return max(1, DEFAULT_ROWS // check_samples(samples))


def check_chunk(chunk, samples: int) -> int:
    if chunk is None:
        return default_chunk(samples)
    if isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or int(chunk) < 1:
        raise ValueError(f"chunk must be None or an integer >= 1 (windows per wide batch), got {chunk!r}")
    return int(chunk)


def chunk_plan(N: int, samples: int, chunk=None) -> List[Tuple[int, int, int]]:
    """[(j, first window, windows)] of the wide batches: chunk j holds `chunk` windows (the last one the remainder)."""
    if N < 1:
        raise ValueError(f"need at least one window, got {N}")
    per = check_chunk(chunk, samples)
    return [(j, i, min(per, N - i)) for j, i in enumerate(range(0, N, per))]


def chunk_keys(seed: int, j: int) -> Tuple[int, int]:
    """(key_gru, key_head) of chunk j: msig_dropout_key(seed, j, 1) and (seed, j, 2) — the streams of the two dropout sites."""
    return L.dropout_key(seed, j, 1), L.dropout_key(seed, j, 2)


def auroc(score, positive) -> Optional[float]:
    """Area under the ROC curve of `score` as a detector of `positive` (bool): the Mann-Whitney statistic with average ranks for
    ties.  None when there is no positive or no negative."""
    score, positive = np.asarray(score, dtype=np.float64), np.asarray(positive, dtype=bool)
    n_pos, n_neg = int(positive.sum()), int((~positive).sum())
    if n_pos == 0 or n_neg == 0:
        return None
    order = np.argsort(score, kind="stable")
    s = score[order]
    ranks = np.empty(s.size, dtype=np.float64)
    i = 0
    while i < s.size:
        j = i
        while j + 1 < s.size and s[j + 1] == s[i]:
            j += 1
        ranks[order[i:j + 1]] = 0.5 * (i + j) + 1.0          # the average of the 1-based ranks i+1 .. j+1
        i = j + 1
    return float((ranks[positive].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))


def selective_accuracy(correct, uncertainty, coverages: Sequence[int] = COVERAGES) -> dict:
    """{str(coverage in %): accuracy on the kept windows}.  The most uncertain windows are dropped first (among equal
    uncertainties the higher window index first); ceil(coverage * N / 100) windows are kept."""
    correct, uncertainty = np.asarray(correct, dtype=bool), np.asarray(uncertainty, dtype=np.float64)
    order = np.argsort(uncertainty, kind="stable")           # ascending; ties in window order
    out = {}
    for cov in coverages:
        keep = -(-correct.size * int(cov) // 100)
        out[str(int(cov))] = float(correct[order[:keep]].mean()) if keep > 0 else None
    return out


def expected_calibration_error(confidence, correct, bins: int = ECE_BINS) -> float:
    """sum over `bins` equal-width confidence bins (lo, hi] of |accuracy - mean confidence| * share of the windows."""
    confidence, correct = np.asarray(confidence, dtype=np.float64), np.asarray(correct, dtype=np.float64)
    if confidence.size == 0:
        return 0.0
    idx = np.clip(np.ceil(confidence * bins).astype(np.int64) - 1, 0, bins - 1)
    ece = 0.0
    for b in range(bins):
        m = idx == b
        if m.any():
            ece += abs(correct[m].mean() - confidence[m].mean()) * m.sum() / confidence.size
    return float(ece)


def _mean_or_none(v) -> Optional[float]:
    v = np.asarray(v, dtype=np.float64)
    return float(v.mean()) if v.size else None


def window_metrics(w: dict) -> dict:
    """The table row of a set of windows, from their per-window record `w` (lists of equal length: correct_eval, correct_mc,
    conf_eval, conf_mc, entropy, mutual_information)."""
    ok_mc, ok_ev = np.asarray(w["correct_mc"], dtype=bool), np.asarray(w["correct_eval"], dtype=bool)
    ent, mi = np.asarray(w["entropy"], dtype=np.float64), np.asarray(w["mutual_information"], dtype=np.float64)
    return {"n": int(ok_mc.size),
            "accuracy_eval": _mean_or_none(ok_ev), "accuracy_mc": _mean_or_none(ok_mc),
            "entropy_correct": _mean_or_none(ent[ok_mc]), "entropy_wrong": _mean_or_none(ent[~ok_mc]),
            "mutual_information_correct": _mean_or_none(mi[ok_mc]), "mutual_information_wrong": _mean_or_none(mi[~ok_mc]),
            "auroc_entropy": auroc(ent, ~ok_mc),
            "selective_accuracy": selective_accuracy(ok_mc, ent),
            "ece_eval": expected_calibration_error(w["conf_eval"], ok_ev), "ece_mc": expected_calibration_error(w["conf_mc"], ok_mc)}


WINDOW_KEYS = ("correct_eval", "correct_mc", "conf_eval", "conf_mc", "entropy", "mutual_information")


@dataclass
class McPrediction:
    """What predict_mc returns, on the input's device: mean (N, K) and std (N, K) of the S softmax vectors (population std), pred
    (N,) int32 = first argmax of mean, entropy (N,) = H(mean) in nats, expected_entropy (N,) = mean_s H(p_s), mutual_information
    (N,) = their difference (not clamped), votes (N, K) int32 = samples whose first maximal logit is k, and with
    return_samples=True samples (N, S, K), the logits of every pass (else None)."""
    mean: torch.Tensor
    std: torch.Tensor
    pred: torch.Tensor
    entropy: torch.Tensor
    expected_entropy: torch.Tensor
    mutual_information: torch.Tensor
    votes: torch.Tensor
    samples: Optional[torch.Tensor] = None


class McDropout:
    """Monte-Carlo dropout of one model (either kind, either depth).  Holds the staging buffer of the trunk's output; the two
    workspaces — the trunk's, of `chunk` rows, and the tail's, of `chunk * samples` rows — are the engine's evaluation workspaces
    (Engine.workspace), so it bumps ``model._token`` as any later forward does."""

    def __init__(self, model, samples: int = DEFAULT_SAMPLES, seed: int = 0, chunk: Optional[int] = None):
        self.model = model
        self.S = check_samples(samples)
        self.seed = check_seed(seed)
        self.chunk = check_chunk(chunk, self.S)
        self.C, self.K = int(model.in_channels), int(model.num_classes)
        self.thr = L.dropout_threshold(model.dropout_p)
        self._stage = None

    def _check_x(self, x) -> torch.Tensor:
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError("Monte-Carlo dropout needs a GPU tensor: the MI355X path has no CPU fallback")
        if x.dtype != torch.float32 or x.dim() != 3 or x.shape[1] != self.C or x.shape[0] < 1 or x.shape[2] < 16:
            raise ValueError(f"expected float32 (N, {self.C}, T >= 16) input, got {x.dtype} {tuple(x.shape)}")
        return x.detach().contiguous()

    def _windows_per_chunk(self, eng, T: int) -> int:
        """`chunk`, fewer when the engine's workspace is a fold arena's fixed region that so many rows do not fit (a result then
        differs from a stand-alone model's with the same `chunk`: the chunk is part of what a result depends on)."""
        per = self.chunk
        region = getattr(eng, "_ws_region", None)
        if region is not None:
            while per > 1 and L.workspace_layout(per * self.S, self.C, T, self.K, False)[-1] > region.numel():
                per //= 2
        return per

    @torch.no_grad()
    def predict(self, x, return_samples: bool = False) -> McPrediction:
        x = self._check_x(x)
        N, Cc, T = x.shape
        S, K, dev = self.S, self.K, x.device
        model = self.model
        eng = model.engine()
        per = self._windows_per_chunk(eng, T)
        plan = chunk_plan(N, S, per)
        TP = L.stage_lengths(T)[3]
        two = eng.gru_layers != 1
        src_name, row = ("H0", TP * 128) if two else ("FEAT", 128)
        if per * S * TP * 128 > 1 << 31:
            raise ValueError(f"chunk {per} x samples {S}: the wide batch's dropout mask index is 32-bit; use a smaller chunk")
        if getattr(model, "embedded", False):
            eng.scatter()
        last, keep = eng._last, eng._keep
        if self._stage is None or self._stage.numel() < per * row or self._stage.device != dev:
            self._stage = torch.empty(per * row, dtype=torch.float32, device=dev)
        mean = torch.empty((N, K), dtype=torch.float32, device=dev)
        std = torch.empty((N, K), dtype=torch.float32, device=dev)
        pred = torch.empty((N,), dtype=torch.int32, device=dev)
        ent = torch.empty((N,), dtype=torch.float32, device=dev)
        eent = torch.empty((N,), dtype=torch.float32, device=dev)
        mi = torch.empty((N,), dtype=torch.float32, device=dev)
        votes = torch.empty((N, K), dtype=torch.int32, device=dev)
        samples = torch.empty((N, S, K), dtype=torch.float32, device=dev) if return_samples else None
        lib, kind, st = L.lib(), L.MC_KINDS[eng.kind], eng._stream()
        # the wide workspace first: if it grows the engine's evaluation pool, the trunk's layout is made in the grown pool
        eng.workspace(min(per, N) * S, T, False)
        for j, i, nb in plan:
            xb = x[i:i + nb]
            if xb.data_ptr() % 16:
                xb = xb.clone()
            rows = nb * S
            b = eng._batch(xb, None, False, 0.0, 0, 0)
            wbuf, woff = eng.workspace(rows, T, False)
            L.check(lib.msig_mc_trunk(C.byref(b), kind, st), "msig_mc_trunk")
            model._bump_token()
            # the two workspaces are prefixes of one pool: the trunk's output leaves it before the wide layout is written
            stage = self._stage[:nb * row]
            stage.copy_(eng.region(src_name, torch.float32, (nb * row,)))
            wide = wbuf[woff[L.WS[src_name]]:woff[L.WS[src_name] + 1]].view(torch.float32)
            L.check(lib.msig_mc_expand(stage.data_ptr(), wide.data_ptr(), nb, S, row, st), "msig_mc_expand")
            t = L.Batch.from_buffer_copy(b)
            t.shape = L.Shape(rows, Cc, T, K)
            t.x, t.labels = None, None
            t.ws, t.ws_bytes = wbuf.data_ptr(), wbuf.numel()
            t.dropout_thr = self.thr
            t.key_gru, t.key_head = chunk_keys(self.seed, j)
            L.check(lib.msig_mc_tail(C.byref(t), kind, st), "msig_mc_tail")
            logits = wbuf[woff[L.WS["LOGITS"]]:woff[L.WS["LOGITS"] + 1]].view(torch.float32)[:rows * K]
            L.check(lib.msig_mc_reduce(logits.data_ptr(), nb, S, K, mean[i:].data_ptr(), std[i:].data_ptr(), pred[i:].data_ptr(),
                                       ent[i:].data_ptr(), eent[i:].data_ptr(), mi[i:].data_ptr(), votes[i:].data_ptr(), st),
                    "msig_mc_reduce")
            if samples is not None:
                samples[i:i + nb].copy_(logits.view(nb, S, K))
        if last is not None and last in eng._ws:
            eng._last, eng._keep = last, keep
        else:
            eng._keep = None                                          # do not keep the last chunk alive through the engine
        return McPrediction(mean=mean, std=std, pred=pred, entropy=ent, expected_entropy=eent, mutual_information=mi, votes=votes,
                            samples=samples)


# ---- the uncertainty tables of a LOSO run (--mc-dropout) ----------------------------------------------------------------------------
@torch.no_grad()
def eval_logits(model, x, batch: int = 1024) -> torch.Tensor:
    """(N, K) logits of plain eval-mode forwards whatever ``model.training`` is, `batch` windows at a time; a window's logits do not
    depend on the batching.  Model state is untouched."""
    eng = model.engine()
    last, keep = eng._last, eng._keep
    region = getattr(eng, "_ws_region", None)
    while region is not None and batch > 1 and L.workspace_layout(batch, eng.C, x.shape[2], eng.K, False)[-1] > region.numel():
        batch //= 2
    out = []
    for i in range(0, x.shape[0], batch):
        xb = x[i:i + batch]
        eng.forward(xb, None, training=False)
        model._bump_token()
        out.append(eng.region("LOGITS", torch.float32, (xb.shape[0], eng.K)).clone())
    if last is not None and last in eng._ws:
        eng._last, eng._keep = last, keep
    else:
        eng._keep = None
    return torch.cat(out)


def fold_uncertainty(model, x, y, samples: int = DEFAULT_SAMPLES, seed: int = 0, chunk: Optional[int] = None) -> dict:
    """The per-fold record of the driver: the deterministic eval prediction and the Monte-Carlo prediction of the model on the
    windows x (N, C, T) with true labels y — window_metrics of the fold, plus the per-window values ("windows") the pooled row of
    the run is computed from.  JSON-ready."""
    mc = McDropout(model, samples=samples, seed=seed, chunk=chunk)
    p = mc.predict(x)
    y = np.asarray(y.cpu() if isinstance(y, torch.Tensor) else y).astype(np.int64)
    lg = eval_logits(model, x.detach().contiguous()).double().cpu().numpy()
    e = np.exp(lg - lg.max(axis=1, keepdims=True))
    pe = e / e.sum(axis=1, keepdims=True)
    mean = p.mean.double().cpu().numpy()
    pred_mc = p.pred.cpu().numpy().astype(np.int64)
    w = {"correct_eval": (pe.argmax(axis=1) == y).tolist(), "correct_mc": (pred_mc == y).tolist(),
         "conf_eval": pe.max(axis=1).tolist(), "conf_mc": mean[np.arange(mean.shape[0]), pred_mc].tolist(),
         "entropy": p.entropy.double().cpu().tolist(), "mutual_information": p.mutual_information.double().cpu().tolist()}
    return dict(window_metrics(w), samples=mc.S, seed=mc.seed, chunk=mc.chunk, dropout=float(model.dropout_p), windows=w)


def summarise_uncertainty(folds: Sequence[dict]) -> dict:
    """The folds' rows (without their per-window values) and the pooled row: window_metrics of all folds' windows together, in
    fold order."""
    folds = list(folds)
    pooled_w = {k: [v for f in folds for v in f["windows"][k]] for k in WINDOW_KEYS}
    rows = [{k: v for k, v in f.items() if k != "windows"} for f in folds]
    return {"n_folds": len(folds), "folds": rows, "pooled": window_metrics(pooled_w) if folds else None}


def _fmt(v, spec=".4f") -> str:
    return "   n/a" if v is None else format(v, spec)


def format_uncertainty(table: dict, settings: Optional[dict] = None, synthetic: bool = False) -> str:
    lines = ["Monte-Carlo dropout of each fold's model on its TEST subject's windows: S stochastic passes with both dropout masks on "
             "and BatchNorm in its eval form.  acc = accuracy of the deterministic eval prediction / of the argmax of the mean "
             "probability; H = predictive entropy of the mean (nats), MI = H - mean_s H(p_s), each averaged over the correctly / "
             "wrongly classified windows; AUROC of H as a detector of the MC prediction's errors (ties: average ranks; n/a without "
             "errors or without correct windows); selective accuracy with the most uncertain windows dropped first; 15-bin ECE."]
    if settings:
        lines.append("settings: " + ", ".join(f"{k} = {v}" for k, v in settings.items()))
    if synthetic:
        lines.append("NOTE: " + SYNTHETIC_NOTE + ".")
    head = (f"  {'subject':<10}{'n':>6}{'acc eval':>10}{'acc mc':>9}{'H ok':>8}{'H wrong':>9}{'MI ok':>8}{'MI wrong':>9}{'AUROC':>8}"
            + "".join(f"{'sel@' + str(c):>9}" for c in COVERAGES) + f"{'ECE eval':>10}{'ECE mc':>9}")
    lines += ["", head]

    def row(name, r):
        return (f"  {name:<10}{r['n']:>6}{_fmt(r['accuracy_eval']):>10}{_fmt(r['accuracy_mc']):>9}{_fmt(r['entropy_correct']):>8}"
                f"{_fmt(r['entropy_wrong']):>9}{_fmt(r['mutual_information_correct']):>8}{_fmt(r['mutual_information_wrong']):>9}"
                f"{_fmt(r['auroc_entropy']):>8}" + "".join(f"{_fmt(r['selective_accuracy'][str(c)]):>9}" for c in COVERAGES)
                + f"{_fmt(r['ece_eval']):>10}{_fmt(r['ece_mc']):>9}")

    for f in table["folds"]:
        lines.append(row(str(f.get("subject", "?")), f))
    if table.get("pooled"):
        lines += ["", row("pooled", table["pooled"])]
    return "\n".join(lines) + "\n"


def write_uncertainty(run_output_dir, folds: Sequence[dict], settings: Optional[dict] = None, synthetic: bool = False) -> Path:
    """uncertainty.json (summarise_uncertainty of the folds' records + settings) and uncertainty.txt in `run_output_dir`."""
    run_output_dir = Path(run_output_dir)
    table = summarise_uncertainty(folds)
    doc = dict(table, settings=dict(settings or {}))
    if synthetic:
        doc["note"] = SYNTHETIC_NOTE
    (run_output_dir / "uncertainty.json").write_text(json.dumps(doc, indent=1))
    path = run_output_dir / "uncertainty.txt"
    path.write_text(format_uncertainty(table, settings, synthetic), encoding="utf-8")
    return path
