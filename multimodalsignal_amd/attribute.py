"""Integrated-gradients channel and time attribution (include/msig_at.h).

For a trained model F in EVAL mode (running-statistics BatchNorm, no dropout), a window x (C, T), a baseline x0 and a target
vector v over the K logits, with f(x) = sum_k v[k] * logits(x)[k]:

    IG = (x - x0) * sum_p w_p * df/dx (x0 + alpha_p * (x - x0)),     alpha_p = (p + 1/2) / P,  w_p = 1 / P   (the midpoint rule)

and its sums per time bin, per channel and per window; total ~ f(x) - f(x0), the residual (``gap``) being the quadrature error of
P points.  ``Attributor`` builds the path batch (msig_at_path), runs the model's eval-mode forward kept for a backward and its
backward with msig_batch.dx on it — gradients of the parameters go to a scratch buffer of the attributor's own, never to the
engine's — and reduces the (N * P, C, T) gradient in one pass (msig_at_reduce).  ``channel_occlusion`` is the forward-only
cross-check on the same path kernel, ``gate`` reads the ChannelAttention gate's values.  The tables of a LOSO run
(``--attribute``) are at the end.  There is no CPU fallback.
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

DEFAULT_STEPS = 32
DEFAULT_PATH_BATCH = 2048
SYNTHETIC_NOTE = ("synthetic data set: every channel carries a planted class effect, so the table shows that the attribution "
                  "machinery works, not which WESAD channels matter")


# ---- the parts that need no GPU ---------------------------------------------------------------------------------------------------
def check_steps(steps) -> int:
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or not 1 <= int(steps) <= L.AT_MAX_POINTS:
        raise ValueError(f"steps must be an integer in 1..{L.AT_MAX_POINTS}, got {steps!r}")
    return int(steps)


def check_bin(bin) -> Optional[int]:
    if bin is None:
        return None
    if isinstance(bin, bool) or not isinstance(bin, (int, np.integer)) or int(bin) < 1:
        raise ValueError(f"bin must be an integer >= 1 (samples per time bin), got {bin!r}")
    return int(bin)


def default_bin(T: int) -> int:
    """One-second bins for the pipeline's 60-second windows."""
    return max(1, int(T) // 60)


def midpoint_table(P: int) -> Tuple[np.ndarray, np.ndarray]:
    """(alpha, w) of the midpoint rule with P points, float64: alpha_p = (p + 1/2) / P, w_p = 1 / P."""
    P = check_steps(P)
    return (np.arange(P, dtype=np.float64) + 0.5) / P, np.full(P, 1.0 / P, dtype=np.float64)


def occlusion_table(Cin: int) -> np.ndarray:
    """The (C + 1, C) coefficient table of channel occlusion: row c has channel c at its baseline, row C is the window itself."""
    coef = np.ones((Cin + 1, Cin), dtype=np.float64)
    coef[np.arange(Cin), np.arange(Cin)] = 0.0
    return coef


def path_plan(N: int, P: int, path_batch: int) -> List[Tuple[int, int]]:
    """[(first window, windows)] of the path batches: path_batch // P whole windows each, a ragged last one; a window's P points
    are never split."""
    if N < 1:
        raise ValueError(f"need at least one window, got {N}")
    if P < 1 or path_batch < P:
        raise ValueError(f"path_batch ({path_batch}) must hold the {P} path points of at least one window")
    per = path_batch // P
    return [(i, min(per, N - i)) for i in range(0, N, per)]


def class_target(k: int, K: int) -> torch.Tensor:
    """v of a class index: e_k - (1 - e_k) / (K - 1) — logit k against the mean of the others; for K = 2 the log-odds."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= int(k) < K:
        raise ValueError(f"target class must be an integer in 0..{K - 1}, got {k!r}")
    v = torch.full((K,), -1.0 / (K - 1), dtype=torch.float32)
    v[int(k)] = 1.0
    return v


def target_vectors(target, K: int, N: int, logits: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The (N, K) float32 target vectors of a call, on the device of `logits` (else the tensor's own, else the CPU): an int k ->
    class_target(k) for every window; "predicted" -> k = argmax of each window's own eval logits (`logits`, (N, K)); a (K,) or
    (N, K) float tensor -> taken as v itself."""
    dev = logits.device if logits is not None else (target.device if isinstance(target, torch.Tensor) else torch.device("cpu"))
    if isinstance(target, str):
        if target != "predicted":
            raise ValueError(f"target must be a class index, 'predicted' or a ({K},) / ({N}, {K}) float tensor, got {target!r}")
        if logits is None or tuple(logits.shape) != (N, K):
            raise ValueError("target 'predicted' needs the windows' (N, K) eval logits")
        table = torch.stack([class_target(k, K) for k in range(K)]).to(dev)
        return table.index_select(0, torch.argmax(logits, dim=1)).contiguous()
    if isinstance(target, torch.Tensor):
        if not target.is_floating_point() or tuple(target.shape) not in ((K,), (N, K)):
            raise ValueError(f"a target tensor must be float with shape ({K},) or ({N}, {K}), got {target.dtype} {tuple(target.shape)}")
        v = target.detach().to(device=dev, dtype=torch.float32)
        return (v.expand(N, K) if v.dim() == 1 else v).contiguous()
    return class_target(target, K).to(dev).expand(N, K).contiguous()


def target_dot(logits: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """f = sum_k v[k] * logits[k] over the last dimension, added in the order k = 0, 1, ..., K-1 with elementwise fp32 operations:
    the same bits for a window whatever tensor shape it is part of (a library reduction may pick its order by shape)."""
    acc = logits[..., 0] * v[..., 0]
    for k in range(1, logits.shape[-1]):
        acc = acc + logits[..., k] * v[..., k]
    return acc


def baseline_kind(baseline, Cin: int, N: Optional[int] = None, T: Optional[int] = None) -> int:
    """MSIG_AT_BASE_* of a baseline: None -> zero, (C,) -> per channel, (C, T) -> one shared window, (N, C, T) -> one per input.
    N / T None: not known yet (the constructor), checked again with the input.  ValueError for anything else."""
    if baseline is None:
        return L.AT_BASE_ZERO
    if not isinstance(baseline, torch.Tensor) or not baseline.is_floating_point():
        raise ValueError(f"baseline must be None or a float tensor of shape (C,), (C, T) or (N, C, T), got {type(baseline).__name__}")
    s = tuple(baseline.shape)
    if len(s) == 1 and s[0] == Cin:
        return L.AT_BASE_CHANNEL
    if len(s) == 2 and s[0] == Cin and (T is None or s[1] == T):
        return L.AT_BASE_SHARED
    if len(s) == 3 and s[1] == Cin and (T is None or s[2] == T) and (N is None or s[0] == N):
        return L.AT_BASE_OWN
    want = f"({Cin},), ({Cin}, {T if T is not None else 'T'}) or ({N if N is not None else 'N'}, {Cin}, {T if T is not None else 'T'})"
    raise ValueError(f"baseline must have shape {want}, got {s}")


@dataclass
class Attribution:
    """What Attributor.attribute returns, all float32 on the input's device: map (N, C, T) or None, bins (N, C, NB), channel (N, C),
    total (N,), f_x and f_base (N,), gap = total - (f_x - f_base) (the quadrature error of the path points) and target (N, K), the v
    used."""
    map: Optional[torch.Tensor]
    bins: torch.Tensor
    channel: torch.Tensor
    total: torch.Tensor
    f_x: torch.Tensor
    f_base: torch.Tensor
    gap: torch.Tensor
    target: torch.Tensor


class Attributor:
    """Integrated gradients, channel occlusion and the gate's values of one model (either kind, either depth).  Holds its own
    buffers — path points, their gradients, the upstream gradient, the coefficient tables and a scratch of the engine's n_flat
    floats for the parameter gradients the backward writes on its way — and uses the engine's evaluation and kept-evaluation
    workspaces, so it bumps ``model._token`` as any later forward does.  Parameters, BatchNorm buffers, the engine's gradient
    buffer, ``model._step`` and ``model.training`` are untouched."""

    def __init__(self, model, steps: int = DEFAULT_STEPS, baseline: Optional[torch.Tensor] = None, bin: Optional[int] = None,
                 path_batch: int = DEFAULT_PATH_BATCH):
        self.model = model
        self.P = check_steps(steps)
        self.bin = check_bin(bin)
        if isinstance(path_batch, bool) or not isinstance(path_batch, (int, np.integer)) or int(path_batch) < self.P:
            raise ValueError(f"path_batch must be an integer >= steps ({self.P}): a window's path points are never split, got {path_batch!r}")
        self.path_batch = int(path_batch)
        self.C, self.K = int(model.in_channels), int(model.num_classes)
        baseline_kind(baseline, self.C)
        self.baseline = baseline
        self._bufs = {}

    # ---- checks and buffers ------------------------------------------------------------------------------------------------------
    def _check_x(self, x) -> torch.Tensor:
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError("attribution needs a GPU tensor: the MI355X path has no CPU fallback")
        if x.dtype != torch.float32 or x.dim() != 3 or x.shape[1] != self.C or x.shape[0] < 1 or x.shape[2] < 16:
            raise ValueError(f"expected float32 (N, {self.C}, T >= 16) input, got {x.dtype} {tuple(x.shape)}")
        return x.detach().contiguous()

    def _check_target(self, target, N):
        """ValueError for a target that is no class index in range, "predicted" or a (K,) / (N, K) float tensor; launches nothing."""
        if isinstance(target, str):
            if target != "predicted":
                raise ValueError(f"target must be a class index, 'predicted' or a float tensor, got {target!r}")
        elif isinstance(target, torch.Tensor):
            target_vectors(target, self.K, N)
        else:
            class_target(target, self.K)

    @staticmethod
    def _aligned(t: torch.Tensor) -> torch.Tensor:
        """`t`, or a copy when a slice of windows does not start on a 16-byte boundary (only with C * T % 4 != 0)."""
        return t if t.data_ptr() % 16 == 0 else t.clone()

    def _base(self, x):
        """(kind, contiguous float32 device tensor or None) of the baseline for the input x."""
        kind = baseline_kind(self.baseline, self.C, x.shape[0], x.shape[2])
        if kind == L.AT_BASE_ZERO:
            return kind, None
        return kind, self.baseline.detach().to(device=x.device, dtype=torch.float32).contiguous()

    def _base_windows(self, kind, base, x) -> torch.Tensor:
        """The baseline as windows: (1, C, T) for the three shared kinds, (N, C, T) for one per input."""
        _, Cc, T = x.shape
        if kind == L.AT_BASE_ZERO:
            return torch.zeros((1, Cc, T), dtype=torch.float32, device=x.device)
        if kind == L.AT_BASE_CHANNEL:
            return base.view(1, Cc, 1).expand(1, Cc, T).contiguous()
        return base.view(-1, Cc, T)

    def _buf(self, name, numel, dtype, dev) -> torch.Tensor:
        t = self._bufs.get(name)
        if t is None or t.numel() < numel or t.device != dev:
            t = self._bufs[name] = torch.empty(numel, dtype=dtype, device=dev)
        return t[:numel]

    def _table(self, name, values: np.ndarray, dev) -> torch.Tensor:
        key = (name, values.shape)
        t = self._bufs.get(key)
        if t is None or t.device != dev:
            t = self._bufs[key] = torch.as_tensor(values.astype(np.float32)).contiguous().to(dev)
        return t

    def _stream(self, dev):
        return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def _windows_per_batch(self, eng, T: int, rows: int, keep: bool) -> int:
        """Windows of `rows` path rows each per model call: path_batch // rows, fewer when the engine's workspace is a fold
        arena's fixed region (a model still bound to the arena it trained in) that the layout of so many rows does not fit."""
        per = max(1, self.path_batch // rows)
        region = getattr(eng, "_ws_region", None)
        if region is not None:
            while per > 1 and L.workspace_layout(per * rows, self.C, T, self.K, keep)[-1] > region.numel():
                per //= 2
        return per

    def _eval_logits(self, eng, x) -> torch.Tensor:
        """(N, K) logits of plain eval forwards (the evaluation layout), path_batch windows at a time; a window's logits do not
        depend on the batching."""
        out, per = [], self._windows_per_batch(eng, x.shape[2], 1, False)
        for i in range(0, x.shape[0], per):
            xb = x[i:i + per]
            eng.forward(xb, None, training=False)
            self.model._bump_token()
            out.append(eng.region("LOGITS", torch.float32, (xb.shape[0], self.K)).clone())
        return torch.cat(out)

    def _path(self, xb, kind, base_b, coef, v, P, xp, dlogits):
        nb, Cc, T = xb.shape
        L.check(L.lib().msig_at_path(xb.data_ptr(), None if base_b is None else base_b.data_ptr(), kind, coef.data_ptr(),
                                     None if v is None else v.data_ptr(), nb, P, Cc, T, self.K, xp.data_ptr(),
                                     None if dlogits is None else dlogits.data_ptr(), self._stream(xb.device)), "msig_at_path")

    # ---- the calls ---------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def attribute(self, x, target="predicted", return_map: bool = True) -> Attribution:
        x = self._check_x(x)
        N, Cc, T = x.shape
        kind, base = self._base(x)
        self._check_target(target, N)
        bin_ = self.bin if self.bin is not None else default_bin(T)
        NB = -(-T // bin_)
        P, dev = self.P, x.device
        path_plan(N, P, self.path_batch)
        eng = self.model.engine()
        plan = path_plan(N, P, P * self._windows_per_batch(eng, T, P, True))
        last, keep = eng._last, eng._keep
        logits_x = self._eval_logits(eng, x)
        v = target_vectors(target, self.K, N, logits_x)
        logits_b = self._eval_logits(eng, self._base_windows(kind, base, x))
        f_x, f_base = target_dot(logits_x, v), target_dot(logits_b.expand(N, self.K), v)
        alpha, w = midpoint_table(P)
        coef = self._table("ig_coef", np.repeat(alpha[:, None], Cc, axis=1), dev)
        wt = self._table("ig_w", w, dev)
        per = plan[0][1]
        xp_all = self._buf("xp", per * P * Cc * T, torch.float32, dev)
        dx_all = self._buf("dx", per * P * Cc * T, torch.float32, dev)
        dl_all = self._buf("dlogits", per * P * self.K, torch.float32, dev)
        scratch = self._buf("grads", eng.n_flat, torch.float32, dev)
        sums = self._buf("sums", per * Cc, torch.float64, dev)
        amap = torch.empty((N, Cc, T), dtype=torch.float32, device=dev) if return_map else None
        bins = torch.empty((N, Cc, NB), dtype=torch.float32, device=dev)
        chan = torch.empty((N, Cc), dtype=torch.float32, device=dev)
        total = torch.empty((N,), dtype=torch.float32, device=dev)
        lib, backward = L.lib(), ("msig_cg_backward" if eng.kind == "cnn_gru" else "msig_backward")
        for i, nb in plan:
            xb, vb = self._aligned(x[i:i + nb]), v[i:i + nb]
            base_b = self._aligned(base[i:i + nb]) if kind == L.AT_BASE_OWN else base
            mb = None if amap is None else self._aligned(amap[i:i + nb])
            xp = xp_all[:nb * P * Cc * T].view(nb * P, Cc, T)
            dx = dx_all[:nb * P * Cc * T].view(nb * P, Cc, T)
            dl = dl_all[:nb * P * self.K].view(nb * P, self.K)
            self._path(xb, kind, base_b, coef, vb, P, xp, dl)
            b = eng.forward(xp, None, training=False, keep_for_backward=True)
            self.model._bump_token()
            b = L.Batch.from_buffer_copy(b)
            b.grads, b.dx = scratch.data_ptr(), dx.data_ptr()         # the eval-keep layout is the training layout; grads: our scratch
            L.check(getattr(lib, backward)(C.byref(b), dl.data_ptr(), self._stream(dev)), backward)
            L.check(lib.msig_at_reduce(dx.data_ptr(), xb.data_ptr(), None if base_b is None else base_b.data_ptr(), kind, wt.data_ptr(),
                                       nb, P, Cc, T, bin_, None if mb is None else mb.data_ptr(), bins[i:i + nb].data_ptr(),
                                       chan[i:i + nb].data_ptr(), total[i:i + nb].data_ptr(), sums.data_ptr(), self._stream(dev)),
                    "msig_at_reduce")
            if mb is not None and mb.data_ptr() != amap[i:i + nb].data_ptr():
                amap[i:i + nb].copy_(mb)
        if last is not None and last in eng._ws:
            eng._last, eng._keep = last, keep
        else:
            eng._keep = None                                          # do not keep the path batch alive through the engine
        return Attribution(map=amap, bins=bins, channel=chan, total=total, f_x=f_x, f_base=f_base, gap=total - (f_x - f_base), target=v)

    @torch.no_grad()
    def channel_occlusion(self, x, target="predicted") -> torch.Tensor:
        """occ[n][c] = f(x_n) - f(x_n with channel c set to its baseline): forwards only, in the evaluation layout, C + 1 path rows
        per window (msig_at_path with the occlusion table)."""
        x = self._check_x(x)
        N, Cc, T = x.shape
        kind, base = self._base(x)
        self._check_target(target, N)
        P, dev = Cc + 1, x.device
        eng = self.model.engine()
        plan = path_plan(N, P, P * self._windows_per_batch(eng, T, P, False))
        last, keep = eng._last, eng._keep
        v = target_vectors(target, self.K, N, self._eval_logits(eng, x) if isinstance(target, str) else None).to(dev)
        coef = self._table("occ_coef", occlusion_table(Cc), dev)
        xp_all = self._buf("xp", plan[0][1] * P * Cc * T, torch.float32, dev)
        occ = torch.empty((N, Cc), dtype=torch.float32, device=dev)
        for i, nb in plan:
            xb = self._aligned(x[i:i + nb])
            base_b = self._aligned(base[i:i + nb]) if kind == L.AT_BASE_OWN else base
            xp = xp_all[:nb * P * Cc * T].view(nb * P, Cc, T)
            self._path(xb, kind, base_b, coef, None, P, xp, None)
            eng.forward(xp, None, training=False)
            self.model._bump_token()
            f = target_dot(eng.region("LOGITS", torch.float32, (nb * P, self.K)).view(nb, P, self.K), v[i:i + nb, None, :])
            occ[i:i + nb] = f[:, Cc:] - f[:, :Cc]
        if last is not None and last in eng._ws:
            eng._last, eng._keep = last, keep
        else:
            eng._keep = None
        return occ

    @torch.no_grad()
    def gate(self, x) -> Optional[torch.Tensor]:
        """The ChannelAttention gate's values s (N, C) of an eval forward (workspace region GATE_S).  C < 4: the gate's hidden width
        C // 4 is zero and s is the constant 0.5 the reference degenerates to.  cnn_gru has no gate: None."""
        x = self._check_x(x)
        if self.model.kind != "cnn_gru_attention":
            return None
        N = x.shape[0]
        if self.C < 4:
            return torch.full((N, self.C), 0.5, dtype=torch.float32, device=x.device)
        eng = self.model.engine()
        last, keep = eng._last, eng._keep
        out, per = [], self._windows_per_batch(eng, x.shape[2], 1, False)
        for i in range(0, N, per):
            xb = x[i:i + per]
            eng.forward(xb, None, training=False)
            self.model._bump_token()
            out.append(eng.region("GATE_S", torch.float32, (xb.shape[0], self.C)).clone())
        if last is not None and last in eng._ws:
            eng._last, eng._keep = last, keep
        else:
            eng._keep = None
        return torch.cat(out)


# ---- the attribution tables of a LOSO run (--attribute) ----------------------------------------------------------------------------
def fold_attribution(model, x, y, steps: int = DEFAULT_STEPS, bin: Optional[int] = None, channels: Optional[Sequence[str]] = None,
                     num_classes: Optional[int] = None) -> dict:
    """The per-fold record of the driver: integrated gradients towards each window's predicted class, the gate's values and the
    channel-occlusion drops of the model on the windows x (N, C, T) with true labels y — JSON-ready."""
    at = Attributor(model, steps=steps, bin=bin)
    a = at.attribute(x, "predicted", return_map=False)
    occ, gate = at.channel_occlusion(x, a.target), at.gate(x)
    chan = a.channel.double().cpu().numpy()
    y = np.asarray(y.cpu() if isinstance(y, torch.Tensor) else y).astype(np.int64)
    K = int(num_classes or model.num_classes)
    mag = np.abs(chan)
    den = mag.sum(axis=1, keepdims=True)
    share = np.divide(mag, den, out=np.zeros_like(mag), where=den > 0)
    scale = np.maximum(np.abs((a.f_x - a.f_base).double().cpu().numpy()), 1e-12)
    rel_gap = np.abs(a.gap.double().cpu().numpy()) / scale
    T = x.shape[2]
    rec = {"n": int(x.shape[0]), "steps": at.P, "bin": int(at.bin if at.bin is not None else default_bin(T)),
           "channels": list(channels) if channels is not None else [f"ch{c}" for c in range(at.C)],
           "share": share.mean(axis=0).tolist(),
           "signed": chan.mean(axis=0).tolist(),
           "signed_by_class": {str(k): (chan[y == k].mean(axis=0).tolist() if (y == k).any() else None) for k in range(K)},
           "occlusion": occ.double().mean(dim=0).cpu().tolist(),
           "time_profile": a.bins.double().abs().sum(dim=1).mean(dim=0).cpu().tolist(),
           "gap_rel_mean": float(rel_gap.mean()), "gap_rel_max": float(rel_gap.max())}
    if gate is None:
        rec["gate"], rec["gate_note"] = None, "cnn_gru has no gate"
    else:
        rec["gate"] = gate.double().mean(dim=0).cpu().tolist()
        if at.C < 4:
            rec["gate_note"] = "degenerate gate (C // 4 = 0): the constant 0.5"
    return rec


def summarise_attribution(folds: Sequence[dict]) -> dict:
    """Over folds: mean and population std (np.std, as cv_summary.txt) of every per-channel column, and the channel ranking by mean
    share.  A fold whose attribution is all zero has shares 0 (no division by zero) and counts as such."""
    folds = list(folds)
    names = list(folds[0]["channels"]) if folds else []
    out = {"n_folds": len(folds), "channels": names, "folds": folds, "summary": {}}
    for key in ("share", "signed", "occlusion", "gate"):
        rows = [f[key] for f in folds if f.get(key) is not None]
        if rows:
            a = np.asarray(rows, dtype=np.float64)
            out["summary"][key] = {"mean": a.mean(axis=0).tolist(), "std": a.std(axis=0).tolist()}
        else:
            out["summary"][key] = None
    sh = out["summary"]["share"]
    order = np.argsort(-np.asarray(sh["mean"]), kind="stable").tolist() if sh else []
    out["ranking"] = [names[i] for i in order]
    gaps = [f["gap_rel_max"] for f in folds]
    out["gap_rel_max"] = float(max(gaps)) if gaps else None
    out["gap_rel_mean"] = float(np.mean([f["gap_rel_mean"] for f in folds])) if folds else None
    return out


def format_attribution(table: dict, settings: Optional[dict] = None, synthetic: bool = False) -> str:
    names = table["channels"]
    lines = ["Integrated-gradients attribution of each fold's model on its TEST subject's windows, towards each window's predicted "
             "class (zero baseline = the subject's own mean level after the z-score; midpoint rule).  share = mean over windows of "
             "|chan[c]| / sum_c' |chan[c']|; signed = mean chan[c]; occlusion = mean f(x) - f(x with channel c at its baseline), "
             "forward only; gate = mean ChannelAttention value."]
    if settings:
        lines.append("settings: " + ", ".join(f"{k} = {v}" for k, v in settings.items()))
    if synthetic:
        lines.append("NOTE: " + SYNTHETIC_NOTE + ".")
    w = max([12] + [len(n) + 1 for n in names])
    head = f"  {'subject':<10} {'column':<10}" + "".join(f"{n:>{w}}" for n in names)
    for f in table["folds"]:
        lines += ["", head]
        cols = [("share", f["share"]), ("signed", f["signed"])]
        cols += [(f"signed|y={k}", v) for k, v in f.get("signed_by_class", {}).items() if v is not None]
        cols += [("occlusion", f["occlusion"])]
        if f.get("gate") is not None:
            cols.append(("gate", f["gate"]))
        for name, vals in cols:
            lines.append(f"  {f['subject']:<10} {name:<10}" + "".join(f"{v:>{w}.4f}" for v in vals))
        if f.get("gate_note"):
            lines.append(f"  {f['subject']:<10} gate: {f['gate_note']}")
        prof = np.asarray(f.get("time_profile", []), dtype=np.float64)
        if prof.size:
            lines.append(f"  {f['subject']:<10} time profile over {prof.size} bins of {f['bin']} samples: peak at bin {int(prof.argmax())} "
                         f"({prof.max():.4g}), mean {prof.mean():.4g}")
        lines.append(f"  {f['subject']:<10} n = {f['n']}, completeness gap |total - (f(x) - f(x0))| / |f(x) - f(x0)|: mean "
                     f"{f['gap_rel_mean']:.3e}, max {f['gap_rel_max']:.3e}")
    lines += ["", f"  over {table['n_folds']} folds (mean ± population std)", f"  {'':<10} {'column':<10}" + "".join(f"{n:>{w}}" for n in names)]
    for key in ("share", "signed", "occlusion", "gate"):
        sm = table["summary"].get(key)
        if sm is None:
            continue
        lines.append(f"  {'':<10} {key:<10}" + "".join(f"{m:>{w}.4f}" for m in sm["mean"]))
        lines.append(f"  {'':<10} {'  ± std':<10}" + "".join(f"{s:>{w}.4f}" for s in sm["std"]))
    lines.append("  channel ranking by mean share: " + " > ".join(table["ranking"]))
    return "\n".join(lines) + "\n"


def write_attribution(run_output_dir, folds: Sequence[dict], settings: Optional[dict] = None, synthetic: bool = False) -> Path:
    """attribution.json (summarise_attribution of the folds' records + settings) and attribution.txt in `run_output_dir`."""
    run_output_dir = Path(run_output_dir)
    table = summarise_attribution(folds)
    doc = dict(table, settings=dict(settings or {}))
    if synthetic:
        doc["note"] = SYNTHETIC_NOTE
    (run_output_dir / "attribution.json").write_text(json.dumps(doc, indent=1))
    path = run_output_dir / "attribution.txt"
    path.write_text(format_attribution(table, settings, synthetic), encoding="utf-8")
    return path
