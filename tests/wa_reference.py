"""numpy fp32 restatement of include/msig_wa.h: the shadow's update and the two coefficient schedules, bit for bit.

update(s, p, a): a == 0 leaves s, a == 1 copies p, else s + a * (p - s) in three fp32 roundings (numpy rounds every float32
operation once and never fuses).  The schedules are computed in double and rounded once to fp32, as the host does.
"""
import numpy as np


def update(s, p, a):
    s, p, a = np.asarray(s, dtype=np.float32), np.asarray(p, dtype=np.float32), np.float32(a)
    if a == np.float32(0):
        return s.copy()
    if a == np.float32(1):
        return p.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        d = (p - s).astype(np.float32)
        t = (a * d).astype(np.float32)
        return (s + t).astype(np.float32)


def ema_coef(t, decay=0.99, warmup=10):
    d = float(decay) if warmup == 0 else min(float(decay), (1.0 + t) / (float(warmup) + t))
    return np.float32(1.0 - d)


def swa_coef(k):
    return np.float32(1.0 / (k + 1.0))


def replay_ema(initial, snapshots, decay=0.99, warmup=10, t0=0):
    """The shadow after one EMA update per snapshot (the model after each train step), from a copy of `initial`."""
    s = update(np.zeros_like(np.asarray(initial, dtype=np.float32)), initial, 1.0)
    for t, p in enumerate(snapshots):
        s = update(s, p, ema_coef(t0 + t, decay, warmup))
    return s


def replay_swa(iterates):
    """The running mean of the iterates as the SWA updates form it (the first is a copy)."""
    s = None
    for k, p in enumerate(iterates):
        s = update(np.zeros_like(np.asarray(p, dtype=np.float32)) if s is None else s, p, swa_coef(k))
    return s
