#!/usr/bin/env python3
"""Regenerates ``norm_reference.npz`` FROM THE REFERENCE ITSELF: raw windows of three small subjects and what the reference's
baseline-normalising ``WesadDataset`` (``void/dataset.py``) makes of them.

Runs only where the reference tree is present (``/root/reference``, or the directory given as the first argument); the fixture
it writes is data (inputs + the reference's outputs).  Nothing here is imported by the product.

    python tests/golden/make_norm_reference_golden.py

The set: T = 64, C_all = 5, all five channels selected in a permuted order.  chest_EDA (the one channel under log1p) is positive
and heavy-tailed, chest_Temp is 33 +- 0.05 (mean >> spread), chest_EMG is exactly constant; the first subject's raw labels are
1,1,2,3,4,1,2 — baseline windows that are not contiguous in file order — and every subject has at least one baseline window, so
the reference's un-normalised fallback never enters the fixture.
"""
import importlib.util
import sys
import tempfile
from pathlib import Path

import numpy as np

REF = Path(sys.argv[1]) if len(sys.argv) > 1 else Path("/root/reference")
OUT = Path(__file__).resolve().parent

spec = importlib.util.spec_from_file_location("void_dataset", REF / "void" / "dataset.py")
void_dataset = importlib.util.module_from_spec(spec)
spec.loader.exec_module(void_dataset)

T = 64
ALL_NAMES = ["chest_ECG", "chest_EDA", "chest_Temp", "chest_EMG", "chest_Resp"]
SELECTED = ["chest_Temp", "chest_Resp", "chest_EDA", "chest_ECG", "chest_EMG"]      # columns 2, 4, 1, 0, 3: a permutation, not sorted
LABELS = {"S2": [1, 1, 2, 3, 4, 1, 2], "S3": [2, 1, 3, 1, 4, 2, 1, 1], "S4": [3, 3, 1, 2, 4, 1, 2, 2, 1]}


def raw_subject(y, seed):
    """Raw windows whose level and spread depend on the protocol phase, so that baseline and whole-recording statistics differ."""
    rs = np.random.RandomState(seed)
    n = len(y)
    phase = np.asarray(y, dtype=np.float64)[:, None]
    x = np.empty((n, T, len(ALL_NAMES)), dtype=np.float64)
    x[:, :, 0] = rs.randn(n, T) * (0.6 + 0.2 * phase) + 0.3 * phase + rs.randn()
    x[:, :, 1] = np.exp(0.8 * rs.randn(n, T) + 0.25 * phase) + 0.1
    x[:, :, 2] = 33.0 + 0.05 * rs.randn(n, T) + 0.02 * phase
    x[:, :, 3] = 0.75
    x[:, :, 4] = rs.randn(n, T) * 1.3 - 0.4 * phase + rs.randn()
    return x


def main():
    arrays = {"all_channel_names": np.array(ALL_NAMES), "channels_to_use": np.array(SELECTED), "subjects": np.array(list(LABELS))}
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        for i, (sid, y) in enumerate(LABELS.items()):
            x, y = raw_subject(y, seed=20 + i), np.asarray(y, dtype=np.int64)
            assert (y == 1).any()
            np.save(tmp / f"{sid}_X.npy", x)
            np.save(tmp / f"{sid}_y.npy", y)
            arrays[f"X_{sid}"], arrays[f"y_{sid}"] = x, y
        for mode in ("binary", "ternary"):
            ds = void_dataset.WesadDataset(tmp, list(LABELS), SELECTED, ALL_NAMES, classification_mode=mode)
            assert ds.data.dtype == np.float64 and ds.data.shape == (sum(map(len, LABELS.values())), T, len(SELECTED))
            arrays[f"data_{mode}"], arrays[f"labels_{mode}"] = ds.data, ds.labels
    np.savez_compressed(OUT / "norm_reference.npz", **arrays)
    print(f"wrote {OUT / 'norm_reference.npz'} ({(OUT / 'norm_reference.npz').stat().st_size} bytes)")


if __name__ == "__main__":
    main()
