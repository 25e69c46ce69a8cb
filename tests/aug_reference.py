"""The augmenting gather of include/msig_aug.h restated in float32 numpy, bit for bit (a helper, not a test).

Every draw is a pure function of (key, row in the batch, channel, sample): row keys, then (row, channel) keys, then one fmix32 per
sample — the header writes the mixing out, this file mirrors it line by line.  `draws` exposes the intermediate draws for the
statistics tests; `augment` is the whole gather.
"""
import numpy as np

from oracle.cnn_gru_oracle import _fmix32, dropout_key  # noqa: F401  (dropout_key: re-exported for the tests)

STREAM_ID = 3
NOISE_K = np.float32(1.0 / np.sqrt(4.0 * (256.0 ** 2 - 1.0) / 12.0))
TAG_SCALE, TAG_CDROP, TAG_MASK, TAG_MLEN, TAG_MT0, TAG_KEEP = (np.uint32(0x80000000 + i) for i in range(1, 7))


def _mul32(a, b):
    return ((np.asarray(a, np.uint64) * np.uint64(b)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def row_keys(key, B):
    return _fmix32(np.uint32(key) ^ _mul32(np.arange(B), 0x9E3779B9))


def chan_keys(rk, C):
    """(B, C) keys of every (row, channel)."""
    step = _mul32(np.arange(1, C + 1), 0x7F4A7C15)
    return _fmix32(((rk[:, None].astype(np.uint64) + step[None, :].astype(np.uint64)) & np.uint64(0xFFFFFFFF)).astype(np.uint32))


def noise(words):
    """g: the standardised sum of the four bytes of each word — exact integer arithmetic, one fp32 multiplication."""
    w = np.asarray(words, np.uint32)
    s = ((w & 0xFF) + ((w >> 8) & 0xFF) + ((w >> 16) & 0xFF) + (w >> 24)).astype(np.int32) - np.int32(510)
    return s.astype(np.float32) * NOISE_K


def mulhi(words, n):
    return ((np.asarray(words, np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def threshold(p):
    """ceil(p * 2^32) - 1 of the fp32 value of p, in double precision: the event is `word <= threshold`."""
    v = np.ceil(float(np.float32(p)) * 4294967296.0) - 1.0
    return np.uint32(min(max(v, 0.0), 4294967295.0))


def draws(key, B, C, T, mask_prob=0.0, mask_max=0, chan_drop=0.0):
    """The per-row and per-(row, channel) draws: dict(masked (B,) bool, length (B,), t0 (B,), dropped (B, C) bool after the
    keep-one rule, drawn (B, C) bool before it)."""
    rk = row_keys(key, B)
    ck = chan_keys(rk, C)
    out = dict(masked=np.zeros(B, bool), length=np.zeros(B, np.int64), t0=np.zeros(B, np.int64), dropped=np.zeros((B, C), bool),
               drawn=np.zeros((B, C), bool))
    if np.float32(mask_prob) > 0:
        out["masked"] = _fmix32(rk ^ TAG_MASK) <= threshold(mask_prob)
        out["length"] = 1 + mulhi(_fmix32(rk ^ TAG_MLEN), mask_max)
        out["t0"] = np.array([mulhi(w, T - n + 1) for w, n in zip(_fmix32(rk ^ TAG_MT0), out["length"])], np.int64).reshape(B)
    if np.float32(chan_drop) > 0:
        drawn = _fmix32(ck ^ TAG_CDROP) <= threshold(chan_drop)
        dropped = drawn.copy()
        keep = mulhi(_fmix32(rk ^ TAG_KEEP), C)
        rows = np.nonzero(drawn.all(axis=1))[0]
        dropped[rows, keep[rows]] = False
        out["drawn"], out["dropped"] = drawn, dropped
    return out


def augment(store, idx, key, scale=0.0, jitter=0.0, mask_prob=0.0, mask_max=0, chan_drop=0.0):
    """store (N, C, T) float32, idx (B,) store positions -> the augmented (B, C, T) float32 batch of msig_aug_gather_windows with
    `key`.  A transform at 0 is skipped (not computed with a neutral value)."""
    store = np.asarray(store, np.float32)
    idx = np.asarray(idx, np.int64)
    B, (C, T) = len(idx), store.shape[1:]
    y = store[idx].copy()
    ck = chan_keys(row_keys(key, B), C)
    if np.float32(scale) > 0:
        gain = np.float32(1.0) + np.float32(scale) * noise(_fmix32(ck ^ TAG_SCALE))          # two fp32 roundings
        y = y * gain[:, :, None]
    if np.float32(jitter) > 0:
        t = np.arange(T, dtype=np.uint32)
        y = y + np.float32(jitter) * noise(_fmix32(ck[:, :, None] ^ t[None, None, :]))
    d = draws(key, B, C, T, mask_prob, mask_max, chan_drop)
    for r in np.nonzero(d["masked"])[0]:
        y[r, :, d["t0"][r]:d["t0"][r] + d["length"][r]] = 0.0
    y[d["dropped"]] = 0.0
    assert y.dtype == np.float32
    return y
