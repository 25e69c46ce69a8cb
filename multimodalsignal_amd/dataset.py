"""Drop-in for the reference's ``dataset.py`` plus a GPU-resident batch source.

``WesadDataset`` keeps the reference's constructor, attributes (``.data`` (N,T,C)
float64, ``.labels``) and item format ((C,T) float32, int64 scalar) and applies the same
label maps and per-subject normalisation (reference ``dataset.py:9-65``).  What is new is
``DeviceLoader``: the whole (N,C,T) fp32 store lives in HBM once (≈4 k windows < 1 GB),
shuffling is a device permutation and a batch is one ``msig_gather_windows`` launch —
replacing the per-item cast/permute + DataLoader collate + H2D copy of every step
(``dataset.py:62-65``, ``main.py:112-114``, ``trainer.py:140-142``).
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path
from typing import Optional, Union

import numpy as np
import torch
from torch.utils.data import Dataset

from . import _lib as L
from .reference import Running, parse_running

LABEL_MODES = ("stress_binary", "ternary", "amusement_binary")


def map_labels(y_raw: np.ndarray, mode: str) -> np.ndarray:
    """WESAD protocol labels 1=baseline 2=TSST 3=amusement 4=meditation -> class ids
    (dataset.py:29-34)."""
    if mode == "stress_binary":
        return (y_raw == 2).astype(np.int64)
    if mode == "ternary":
        out = np.zeros_like(y_raw, dtype=np.int64)
        out[y_raw == 3] = 1
        out[y_raw == 2] = 2
        return out
    if mode == "amusement_binary":
        # The second model of the hierarchical experiment (main.py:183-186) asks for this mode, which the reference's dataset.py
        # does not define (it raises).  Defined here as the obvious map: amusement (raw 3) -> 1, baseline
        # (raw 1) -> 0, every other window is dropped (label -1; WesadDataset removes those rows after the per-subject
        # normalisation, which like every other mode uses ALL of the subject's windows).
        out = np.full_like(y_raw, -1, dtype=np.int64)
        out[y_raw == 1] = 0
        out[y_raw == 3] = 1
        return out
    raise ValueError(f"Unknown classification_mode: {mode}")


def parse_reference(reference) -> Union[None, int, Running]:
    """The normalisation reference of a run: "subject" (every window of the subject supplies the statistics; the default),
    "baseline" (the windows whose raw protocol label is 1) or "baseline:K" (the first K >= 1 of those in file order; window k
    covers seconds 10 k .. 10 k + 60, so K windows are 60 + 10 (K - 1) seconds of rest).  Returns None for "subject", 0 for
    "baseline" and K for "baseline:K"; anything else raises ValueError.

    The causal running references "expanding", "trailing:K" and "decayed:H" (reference.parse_running: the monitors' grammar, here
    without a warm-up count ':W', which is a flag of the monitors) return a reference.Running: window n of a subject's file is
    normalised with the windows up to n, the file taken as consecutive windows of one recording."""
    if reference == "subject":
        return None
    if reference == "baseline":
        return 0
    if isinstance(reference, str) and reference.startswith("baseline:"):
        k = reference[len("baseline:"):]
        if k.isascii() and k.isdigit() and int(k) >= 1:
            return int(k)
    try:
        run = parse_running(reference, warmup=False)
    except ValueError as e:
        raise ValueError(f"normalisation reference: {e}") from None
    if run is not None:
        return run
    raise ValueError("normalisation reference must be 'subject', 'baseline', 'baseline:K' with K >= 1, 'expanding', 'trailing:K' with K in "
                     f"1..{L.RN_MAX_K} or 'decayed:H' with H in 1..{L.RD_MAX_H}, got {reference!r}")


def running_norm_reference(reference) -> Optional[Running]:
    """The reference.Running of a running normalisation reference, None for "subject", "baseline" and "baseline:K"."""
    run = parse_reference(reference)
    return run if isinstance(run, Running) else None


def reference_mask(y_raw: np.ndarray, reference) -> np.ndarray:
    """Which of a subject's windows supply the normalisation statistics (bool, one per window).  `y_raw` are the RAW protocol
    labels, before any class mapping: the mask is the same in every classification mode.  Under a running reference every window
    supplies statistics — to itself and to the windows after it."""
    k = parse_reference(reference)
    y_raw = np.asarray(y_raw)
    if k is None or isinstance(k, Running):
        return np.ones(y_raw.shape, dtype=bool)
    mask = y_raw == 1
    if k:
        mask[np.flatnonzero(mask)[k:]] = False
    return mask


def subject_reference(y_raw: np.ndarray, reference, sid) -> Optional[np.ndarray]:
    """The `ref` of normalise_subject / normalise_subject_device for subject `sid`: None for the "subject" rule, else the mask.
    A subject without a reference window gets the "subject" rule (None) and one warning line — the reference's code announces
    that fallback and then leaves such a subject un-normalised."""
    k = parse_reference(reference)
    if k is None or isinstance(k, Running):          # a running reference has no mask: normalise_subject_running / running=
        return None
    mask = reference_mask(y_raw, reference)
    if not mask.any():
        print(f"Warning: subject {sid} has no baseline window (raw label 1); normalising with the statistics of all its windows.")
        return None
    return mask


def normalise_subject(x: np.ndarray, names, ref: Optional[np.ndarray] = None) -> np.ndarray:
    """Per-subject, per-channel z-score over all of the subject's windows, std + 1e-8;
    the channel literally named 'chest_EDA' is log1p-transformed first (dataset.py:36-48).
    `x` is (N,T,C) float64 and is modified in place.

    `ref` (a bool mask over the N windows): mean and std come from the selected windows only and are applied to all of them
    (void/dataset.py:39-55 — the same np.mean / np.std calls on the same slices, so the result is that file's bit for bit).
    None, or a mask that selects nothing: the rule above."""
    if ref is not None and np.any(ref):
        base = x[np.asarray(ref, dtype=bool)]
        for ch, name in enumerate(names):
            if name == "chest_EDA":
                lg = np.log1p(base[:, :, ch])
                m, sd = np.mean(lg), np.std(lg) + 1e-8
                x[:, :, ch] = (np.log1p(x[:, :, ch]) - m) / sd
            else:
                m, sd = np.mean(base[:, :, ch]), np.std(base[:, :, ch]) + 1e-8
                x[:, :, ch] = (x[:, :, ch] - m) / sd
        return x
    mu = x.mean(axis=(0, 1))
    sd = x.std(axis=(0, 1)) + 1e-8
    for ch, name in enumerate(names):
        if name == "chest_EDA":
            lg = np.log1p(x[:, :, ch])
            x[:, :, ch] = (lg - lg.mean()) / (lg.std() + 1e-8)
        else:
            x[:, :, ch] = (x[:, :, ch] - mu[ch]) / sd[ch]
    return x


def running_statistics(v: np.ndarray, run: Running):
    """include/msig_rn.h's and msig_rd.h's definition in float64 numpy for a subject's (N, T, C) window file `v` (after log1p),
    taken as the consecutive windows of one recording: the pivot p = v[0, 0], window sums W1[n] = sum_t (v - p), W2[n] = sum_t
    (v - p)^2, the reference's sums A[n] — expanding: the carry A[n - 1] + W[n]; trailing:K: W[a] + ... + W[n] left to right,
    a = max(0, n - K + 1); decayed:H: lambda A[n - 1] + W[n], c[n] = lambda c[n - 1] + 1, lambda = exp2(-1 / H) — and
    dm = A1 / (c T), var = max(0, A2 / (c T) - dm^2), mean = p + dm, inv = 1 / (sqrt(var) + 1e-8).
    Returns (mean (N, C), inv (N, C), c (N,) float64)."""
    v = np.ascontiguousarray(v)          # numpy's summation order depends on the strides: one layout, one result
    N, T, _C = v.shape
    p = v[0, 0].copy()
    d = v - p
    W = np.stack([d.sum(axis=1), (d * d).sum(axis=1)], axis=1)                  # (N, 2, C)
    A, c = np.empty_like(W), np.empty(N, dtype=np.float64)
    for n in range(N):
        if n == 0:
            A[0], c[0] = W[0], 1.0
        elif run.kind == "expanding":
            A[n], c[n] = A[n - 1] + W[n], n + 1.0
        elif run.kind == "decayed":
            A[n], c[n] = run.decay * A[n - 1] + W[n], run.decay * c[n - 1] + 1.0
        else:
            a = max(0, n - run.K + 1)
            acc = W[a].copy()
            for k in range(a + 1, n + 1):
                acc = acc + W[k]
            A[n], c[n] = acc, n - a + 1.0
    cnt = (c * float(T))[:, None]
    dm = A[:, 0] / cnt
    var = np.maximum(A[:, 1] / cnt - dm * dm, 0.0)
    return p + dm, 1.0 / (np.sqrt(var) + 1e-8), c


def normalise_subject_running(x: np.ndarray, names, run: Running) -> np.ndarray:
    """A subject's (N, T, C) float64 windows under a running reference, in place: window n becomes (v - mean[n]) * inv[n] with
    running_statistics' record of window n; the channel literally named 'chest_EDA' is log1p-transformed first."""
    for ch, name in enumerate(names):
        if name == "chest_EDA":
            x[:, :, ch] = np.log1p(x[:, :, ch])
    mean, inv, _c = running_statistics(x, run)
    x -= mean[:, None, :]
    x *= inv[:, None, :]
    return x


class WesadDataset(Dataset):
    def __init__(self, data_path: Path, subjects: list, channels_to_use: list, all_channel_names: list,
                 classification_mode="stress_binary", cache: Optional[dict] = None, reference="subject"):
        """`cache` (optional, not in the reference): a dict shared between datasets of one run; a
        subject's normalised windows depend only on that subject, so the 3 x 15 datasets of a LOSO run
        can load and normalise each subject once instead of 45 times.
        `reference` (optional, not in the reference's dataset.py): which windows supply each subject's mean and std
        (parse_reference); "subject" is the rule above.  A running reference (expanding, trailing:K, decayed:H) normalises window n
        with the windows up to n in file order (normalise_subject_running) — like the mask, before amusement_binary drops rows."""
        data_path = Path(data_path)
        run = running_norm_reference(reference)
        self.classification_mode = classification_mode
        self.data_list, self.labels_list = [], []
        cols = [all_channel_names.index(ch) for ch in channels_to_use]
        for sid in subjects:
            key = (str(data_path), sid, tuple(cols), classification_mode, reference)
            if cache is not None and key in cache:
                x, y = cache[key]
            else:
                fx, fy = data_path / f"{sid}_X.npy", data_path / f"{sid}_y.npy"
                if not (fx.exists() and fy.exists()):
                    print(f"Warning: Skipping subject {sid} for data, file not found.")
                    continue
                x = np.load(fx)[:, :, cols]                       # fancy index -> private float64 copy
                y_raw = np.load(fy)
                y = map_labels(y_raw, classification_mode)
                # the mask is taken from the raw labels, before amusement_binary drops rows
                if run is not None:
                    x = normalise_subject_running(x, [all_channel_names[i] for i in cols], run)
                else:
                    x = normalise_subject(x, [all_channel_names[i] for i in cols], subject_reference(y_raw, reference, sid))
                if (y < 0).any():                                  # amusement_binary: windows of the other protocol phases are dropped
                    x, y = x[y >= 0], y[y >= 0]
                if cache is not None:
                    cache[key] = (x, y)
            self.data_list.append(x)
            self.labels_list.append(y)
        if not self.data_list:
            raise ValueError(f"No data loaded for subjects: {subjects}. Check paths and data existence.")
        self.data = np.concatenate(self.data_list, axis=0)
        self.labels = np.concatenate(self.labels_list, axis=0)
        # per-window ordinal of the window's subject among the subjects loaded, in order (adversary.domain_table)
        self.subject_ordinals = np.repeat(np.arange(len(self.labels_list), dtype=np.int32), [len(y) for y in self.labels_list])
        self._dev_cache = None

    def __len__(self):
        return len(self.labels)

    def __getitem__(self, idx):
        x = torch.from_numpy(self.data[idx]).float().permute(1, 0)
        return x, torch.tensor(self.labels[idx], dtype=torch.long)

    def device_tensors(self, device):
        """(N,C,T) fp32 windows and (N,) int64 labels in HBM (uploaded once, then cached)."""
        device = torch.device(device)
        if self._dev_cache is None or self._dev_cache[0].device != device:
            x = torch.from_numpy(np.ascontiguousarray(self.data.transpose(0, 2, 1), dtype=np.float32))
            self._dev_cache = (x.to(device), torch.from_numpy(self.labels.astype(np.int64)).to(device))
        return self._dev_cache


class SubjectStore:
    """All subjects of a run, normalised once and resident in HBM as ONE (N_total, C, T) fp32 store.

    A subject's normalised windows depend only on that subject (dataset.py:36-48), so the 45 datasets of
    a LOSO run are just index subsets of this store: no per-fold host concatenation, no per-fold upload.
    `normalise="host"` reproduces the reference's float64 numpy arithmetic and casts to fp32 exactly like
    `__getitem__` (dataset.py:63); `normalise="device"` does the reduction, the optional log1p, the z-score
    and the (N,T,C)->(N,C,T) transposition on the GPU in float64 (torch ops on the raw upload)."""

    def __init__(self, data_path: Path, subjects: list, channels_to_use: list, all_channel_names: list,
                 classification_mode="stress_binary", device="cuda", normalise="host", reference="subject"):
        """`reference`: which windows supply each subject's mean and std (parse_reference); with anything but "subject" one line
        per subject names the windows used, and `reference_windows` holds {subject: (reference windows used, fallback applied)}.
        Under a running reference (expanding, trailing:K, decayed:H) window n is normalised with the windows up to n in file order
        — the entry is ("per window", False) — and with normalise="device" `reference_tables` holds {subject: the (N, 2 * MAX_C + 1)
        table of one statistics record per window on the device}: msig_rn_sums on the raw upload as a recording of N * T samples
        at stride T, msig_rn_stats or msig_rd_stats, msig_rn_windows — the rows a Monitor feeds the model for that recording."""
        self.device = torch.device(device)
        run = running_norm_reference(reference)
        self.reference, self.reference_windows, self.reference_tables = reference, {}, {}
        data_path = Path(data_path)
        cols = [all_channel_names.index(ch) for ch in channels_to_use]
        names = [all_channel_names[i] for i in cols]
        if normalise not in ("host", "device"):
            raise ValueError(f"normalise must be 'host' or 'device', got {normalise!r}")
        if classification_mode == "amusement_binary":
            raise NotImplementedError("amusement_binary drops windows per subject: use WesadDataset (the hierarchical driver does)")
        xs, ys, self.ranges, start = [], [], {}, 0
        present = []
        for sid in subjects:
            fx, fy = data_path / f"{sid}_X.npy", data_path / f"{sid}_y.npy"
            if not (fx.exists() and fy.exists()):
                print(f"Warning: Skipping subject {sid} for data, file not found.")
                continue
            present.append((sid, fx, fy))

        def host_windows(job):       # the reference's float64 arithmetic, then its fp32 cast (dataset.py:36-48, :63)
            fx, ref = job
            x = np.load(fx)[:, :, cols]
            x = normalise_subject_running(x, names, run) if run is not None else normalise_subject(x, names, ref)
            return np.ascontiguousarray(x.transpose(0, 2, 1), dtype=np.float32)

        # the raw labels are read first: they say which windows are a subject's reference (None: the "subject" rule)
        y_raws = [np.load(fy) for _, _, fy in present]
        refs = [subject_reference(y_raw, reference, sid) for y_raw, (sid, _, _) in zip(y_raws, present)]

        # A subject's windows depend on that subject alone: the host path reads and normalises a few subjects at a time on
        # threads (numpy's reductions and copies run outside the interpreter lock; 0.9 -> 0.35 s for 15 x 270 windows) and
        # uploads them in subject order — the store is the same bit for bit.
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1))) as pool:
            host = pool.map(host_windows, [(fx, ref) for (_, fx, _), ref in zip(present, refs)]) if normalise == "host" else iter(())
            for (sid, fx, fy), y_raw, ref in zip(present, y_raws, refs):
                y = map_labels(y_raw, classification_mode)
                if normalise == "host":
                    xd = torch.from_numpy(next(host)).to(self.device)
                    n_ref = 0 if ref is None else int(ref.sum())
                elif run is not None:
                    table = torch.zeros((len(y), 2 * L.MAX_C + 1), dtype=torch.float64, device=self.device)
                    xd = normalise_subject_device(torch.from_numpy(np.load(fx)).to(self.device), cols, names, stats=table, running=run)
                    self.reference_tables[sid], n_ref = table, 0
                elif ref is None:
                    xd, n_ref = normalise_subject_device(torch.from_numpy(np.load(fx)).to(self.device), cols, names), 0
                else:       # the kernel counts the windows its mask selects: the line below reports what it used
                    stats = torch.empty(2 * L.MAX_C + 1, dtype=torch.float64, device=self.device)
                    xd = normalise_subject_device(torch.from_numpy(np.load(fx)).to(self.device), cols, names, ref, stats=stats)
                    n_ref = int(stats[2 * L.MAX_C].item())
                if run is not None:
                    self.reference_windows[sid] = ("per window", False)
                    print(f"[normalise {normalise}] {sid}: reference {reference}: per window, {len(y)} windows in file order")
                elif parse_reference(reference) is not None:
                    self.reference_windows[sid] = (n_ref, ref is None)
                    print(f"[normalise {normalise}] {sid}: reference {reference}: "
                          + (f"{n_ref} of {len(y)} windows" if ref is not None else f"no baseline window, all {len(y)} windows"))
                xs.append(xd)
                ys.append(torch.from_numpy(y.astype(np.int64)))
                self.ranges[sid] = (start, start + len(y))
                start += len(y)
        if not xs:
            raise ValueError(f"No data loaded for subjects: {subjects}. Check paths and data existence.")
        self.x = torch.cat(xs, dim=0).contiguous()
        self.labels_host = torch.cat(ys).numpy()
        self.y = torch.from_numpy(self.labels_host).to(self.device)

    @classmethod
    def from_wesad(cls, data_path: Path, subjects: list, channels_to_use: list, all_channel_names: list,
                   classification_mode="stress_binary", device="cuda", cache: Optional[dict] = None, reference="subject") -> "SubjectStore":
        """A store of any classification mode, amusement_binary included, built from WesadDataset's per-subject arrays (its
        `cache` shared): every window is the float64 -> fp32 cast of WesadDataset.device_tensors, so a StoreView of it feeds the
        same bits as a WesadDataset of those subjects.  A subject with no window of the mode keeps an empty range."""
        self = cls.__new__(cls)
        self.device = torch.device(device)
        self.reference, self.reference_windows, self.reference_tables = reference, {}, {}
        xs, ys, self.ranges, start = [], [], {}, 0
        for sid in subjects:
            if not ((Path(data_path) / f"{sid}_X.npy").exists() and (Path(data_path) / f"{sid}_y.npy").exists()):
                print(f"Warning: Skipping subject {sid} for data, file not found.")
                continue
            ds = WesadDataset(data_path, [sid], channels_to_use, all_channel_names, classification_mode=classification_mode, cache=cache,
                              reference=reference)
            xs.append(torch.from_numpy(np.ascontiguousarray(ds.data.transpose(0, 2, 1), dtype=np.float32)))
            ys.append(torch.from_numpy(ds.labels.astype(np.int64)))
            self.ranges[sid] = (start, start + len(ds))
            start += len(ds)
        if not xs:
            raise ValueError(f"No data loaded for subjects: {subjects}. Check paths and data existence.")
        self.x = torch.cat(xs, dim=0).contiguous().to(self.device)
        self.labels_host = torch.cat(ys).numpy()
        self.y = torch.from_numpy(self.labels_host).to(self.device)
        return self

    def view(self, subjects: list) -> "StoreView":
        return StoreView(self, subjects)


RUNNING_PIECE = 1 << 20          # windows per msig_rn_windows call of the running store build (the call's B is an int32)


def normalise_subject_device(raw: torch.Tensor, cols, names, ref=None, stats: Optional[torch.Tensor] = None,
                             running: Optional[Running] = None) -> torch.Tensor:
    """(N,T,C_all) raw float64 device tensor -> normalised (N,C,T) fp32 through msig_normalise_subject
    (float64 reduction, optional log1p, z-score, cast and transposition in HIP).

    `ref` (a bool mask over the N windows, numpy or torch): through msig_nr_normalise_subject (include/msig_nr.h) — mean and std of
    the selected windows, applied to all.  `stats` (with `ref`; a float64 device tensor of 2 * MAX_C + 1): receives the mean, the
    1 / (std + 1e-8) and the number of selected windows.

    `running` (a reference.Running, without `ref`): the file is a recording of L = N * T samples whose windows lie at stride T —
    msig_rn_sums, then msig_rn_stats (expanding, trailing:K) or msig_rd_stats (decayed:H), then msig_rn_windows in pieces of
    RUNNING_PIECE windows: row n is normalised with its own record.  `stats` (optional; a contiguous float64 device tensor of
    (N, 2 * MAX_C + 1)): receives the table of one record per window."""
    if not raw.is_cuda or raw.dtype != torch.float64 or raw.dim() != 3:
        raise ValueError("normalise_subject_device needs a (N,T,C_all) float64 GPU tensor")
    raw = raw.contiguous()
    N, T, C_all = raw.shape
    mask = 0
    for c, name in enumerate(names):
        if name == "chest_EDA":
            mask |= 1 << c
    out = torch.empty((N, len(cols), T), dtype=torch.float32, device=raw.device)
    carr = (C.c_int32 * len(cols))(*[int(c) for c in cols])
    st = C.c_void_p(torch.cuda.current_stream(raw.device).cuda_stream)
    if running is not None:
        if ref is not None:
            raise ValueError("a running reference takes no mask of reference windows")
        if stats is None:
            stats = torch.zeros((N, 2 * L.MAX_C + 1), dtype=torch.float64, device=raw.device)
        elif (stats.dtype != torch.float64 or stats.device != raw.device or tuple(stats.shape) != (N, 2 * L.MAX_C + 1) or not stats.is_contiguous()):
            raise ValueError(f"stats must be a contiguous float64 tensor of ({N}, {2 * L.MAX_C + 1}) on {raw.device}")
        head = (raw.data_ptr(), N * T, C_all, carr, len(cols), mask, T, T)                      # L = N * T, S = T: window n is row n
        sums = torch.empty((N, 2 * L.MAX_C), dtype=torch.float64, device=raw.device)
        L.check(L.lib().msig_rn_sums(*head, 0, N, sums.data_ptr(), st), "msig_rn_sums")
        if running.kind == "decayed":
            L.check(L.lib().msig_rd_stats(*head, sums.data_ptr(), N, running.decay, stats.data_ptr(), st), "msig_rd_stats")
        else:
            L.check(L.lib().msig_rn_stats(*head, sums.data_ptr(), N, running.K, stats.data_ptr(), st), "msig_rn_stats")
        for n0 in range(0, N, RUNNING_PIECE):
            B = min(RUNNING_PIECE, N - n0)
            L.check(L.lib().msig_rn_windows(*head, n0, B, stats[n0].data_ptr(), out[n0].data_ptr(), st), "msig_rn_windows")
        return out
    if ref is not None:
        if not isinstance(ref, torch.Tensor):
            ref = torch.from_numpy(np.ascontiguousarray(np.asarray(ref) != 0))
        ref = ref.to(raw.device).contiguous()                             # a device mask stays on the device: no synchronisation
        ref = ref.view(torch.uint8) if ref.dtype in (torch.bool, torch.uint8) else (ref != 0).view(torch.uint8)      # any non-zero byte selects
        if ref.shape != (N,):
            raise ValueError(f"ref must have one entry per window ({N}), got shape {tuple(ref.shape)}")
        if stats is not None and (stats.dtype != torch.float64 or stats.device != raw.device or stats.numel() < 2 * L.MAX_C + 1
                                  or not stats.is_contiguous()):
            raise ValueError(f"stats must be a contiguous float64 tensor of {2 * L.MAX_C + 1} on {raw.device}")
        scratch = torch.empty(L.lib().msig_nr_scratch_bytes(), dtype=torch.uint8, device=raw.device)
        L.check(L.lib().msig_nr_normalise_subject(raw.data_ptr(), N, T, C_all, carr, len(cols), mask, ref.data_ptr(), out.data_ptr(),
                                                  None if stats is None else stats.data_ptr(), scratch.data_ptr(), st),
                "msig_nr_normalise_subject")
        return out
    scratch = torch.empty(L.lib().msig_normalise_scratch_bytes(), dtype=torch.uint8, device=raw.device)
    L.check(L.lib().msig_normalise_subject(raw.data_ptr(), N, T, C_all, carr, len(cols), mask, out.data_ptr(), scratch.data_ptr(), st),
            "msig_normalise_subject")
    return out


class StoreView:
    """The windows of some subjects inside a SubjectStore; quacks like a WesadDataset for DeviceLoader
    and Trainer (`len`, `.labels`, `device_tensors`)."""

    def __init__(self, store: SubjectStore, subjects: list):
        idx = []
        for sid in subjects:
            if sid not in store.ranges:
                print(f"Warning: Skipping subject {sid} for data, file not found.")
                continue
            a, b = store.ranges[sid]
            idx.append(np.arange(a, b, dtype=np.int64))
        # per-window ordinal of the window's subject among the subjects of this view, in order (adversary.domain_table)
        self.subject_ordinals = np.repeat(np.arange(len(idx), dtype=np.int32), [len(i) for i in idx])
        if not idx:
            raise ValueError(f"No data loaded for subjects: {subjects}. Check paths and data existence.")
        self.store = store
        self.index_host = np.concatenate(idx)
        self.index = torch.from_numpy(self.index_host).to(store.device)
        self.labels = store.labels_host[self.index_host]

    def __len__(self):
        return len(self.index_host)

    def __getitem__(self, i):
        j = int(self.index_host[i])
        return self.store.x[j].cpu(), torch.tensor(self.labels[i], dtype=torch.long)

    def device_tensors(self, device):
        return self.store.x, self.store.y


class DeviceLoader:
    """Iterates (x, y) device batches of a WesadDataset without touching the host per step.
    Same iteration contract as ``DataLoader(ds, batch_size, shuffle)`` (no drop_last).

    `augment` (an ``augment.Augment``; training loaders only): every batch is one augmenting gather launch instead, keyed
    by (`aug_seed` = the loader's seed, `aug_step` = the batches this loader has served so far, counted from 1) — the same windows
    are augmented differently in every epoch, and two loaders with one seed serve the same batches.  None: the plain gather.

    `mixup` (a ``mixup.Mixup``; training loaders only, composes with `augment`: the batch is augmented, then mixed): every batch is
    one ``msig_st_gather_windows`` launch that blends row b with row B-1-b, lam drawn from the same (`aug_seed`, `aug_step`) on a
    stream of its own.  `last_lam` is the lam of the batch just served — the criterion needs it (Engine.train_step(mix_lambda=)).

    `last_index` is the int64 device tensor of the store positions of the batch just served (the gather's `idx`): subject-adversarial
    training looks the rows' domains up by it (Engine.train_step(batch_index=))."""

    def __init__(self, dataset: WesadDataset, batch_size: int, shuffle: bool, device, seed: Optional[int] = None, augment=None,
                 mixup=None):
        self.dataset, self.batch_size, self.shuffle = dataset, int(batch_size), bool(shuffle)
        self.device = torch.device(device)
        self.store, self.store_y = dataset.device_tensors(self.device)
        self.index = getattr(dataset, "index", None)      # StoreView: positions inside a shared SubjectStore
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(torch.initial_seed() if seed is None else seed)
        self._bufs = {}
        self.augment = None if augment is None or augment.off else augment       # all transforms at 0 is the plain gather: take it
        self.aug_seed, self.aug_step = int(torch.initial_seed() if seed is None else seed), 0
        if self.augment is not None:
            self.augment.check_window(int(self.store.shape[2]))
        self.mixup, self.last_lam = mixup, None
        self.last_index = None
        if mixup is not None and (int(self.store.shape[2]) < 4 or int(self.store.shape[2]) % 4):
            raise ValueError(f"mixup: the window length must be a multiple of 4, got {int(self.store.shape[2])}")

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def epoch_order(self) -> torch.Tensor:
        """Store positions of this epoch's windows, in visiting order (advances the shuffler like one `iter()`)."""
        n = len(self.dataset)
        order = torch.randperm(n, device=self.device, generator=self.gen) if self.shuffle else torch.arange(n, device=self.device)
        if self.index is not None:
            order = self.index[order]
        return order

    def __iter__(self):
        n = len(self.dataset)
        order = self.epoch_order()
        wfl = self.store.shape[1] * self.store.shape[2]
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        for i in range(0, n, self.batch_size):
            idx = self.last_index = order[i:i + self.batch_size].contiguous()
            b = idx.numel()
            if b not in self._bufs:   # two alternating buffers per batch size: the previous batch may still be in flight
                self._bufs[b] = [(torch.empty((b,) + tuple(self.store.shape[1:]), device=self.device),
                                  torch.empty(b, dtype=torch.int64, device=self.device)) for _ in range(2)]
            ox, oy = self._bufs[b][(i // self.batch_size) & 1]
            if self.mixup is None and self.augment is None:      # the plain gather: any window length (C * T % 4 != 0: element by element)
                L.check(L.lib().msig_gather_windows(self.store.data_ptr(), self.store_y.data_ptr(), idx.data_ptr(), b, wfl,
                                                    ox.data_ptr(), oy.data_ptr(), st), "msig_gather_windows")
                yield ox, oy
                continue
            # augmented, mixed or both: one call (include/msig_st.h) — a NULL msig_aug is none, lam 1 the augmented gather itself
            self.aug_step += 1
            lam = 1.0
            if self.mixup is not None:
                lam = self.last_lam = self.mixup.lam(self.aug_seed, self.aug_step)
            a = (C.byref(self.augment.struct([L.dropout_key(self.aug_seed, self.aug_step, L.AUG_STREAM_ID)]))
                 if self.augment is not None else None)
            L.check(L.lib().msig_st_gather_windows(self.store.data_ptr(), self.store_y.data_ptr(), idx.data_ptr(), b, self.store.shape[1],
                                                   self.store.shape[2], ox.data_ptr(), oy.data_ptr(), a, (C.c_float * 1)(lam), st),
                    "msig_st_gather_windows")
            yield ox, oy
