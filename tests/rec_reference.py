"""A numpy restatement of include/msig_rec.h and of monitor.py's host logic, written from the definitions and sharing no code with
either: the windows are MATERIALISED here, the statistics are taken in np.longdouble, and the smoothing / state machine / events
are plain loops over the definition."""
import numpy as np

MAX_C = 16


def count(L, T, S):
    return 0 if L < T else (L - T) // S + 1


def materialise(sig, T, S):
    """(N, T, C_all): window n = samples [n S, n S + T)."""
    N = count(sig.shape[0], T, S)
    return np.stack([sig[n * S:n * S + T] for n in range(N)]) if N else np.empty((0, T, sig.shape[1]), dtype=sig.dtype)


def multiplicity(L, T, S, w0, w1):
    """m_i = the number of windows n in [w0, w1) that cover sample i, by counting."""
    m = np.zeros(L, dtype=np.int64)
    for n in range(w0, w1):
        m[n * S:n * S + T] += 1
    return m


def transformed(sig, cols, log1p_mask):
    v = sig[:, cols].astype(np.float64)
    for c in range(len(cols)):
        if (log1p_mask >> c) & 1:
            v[:, c] = np.log1p(v[:, c])
    return v


def stats_longdouble(sig, cols, log1p_mask, T, S, w0, w1):
    """(mean, std) per selected channel of the materialised reference windows, in np.longdouble, two passes."""
    v = transformed(sig, cols, log1p_mask)
    win = materialise(v, T, S)[w0:w1].astype(np.longdouble).reshape(-1, len(cols))
    mean = win.sum(axis=0) / win.shape[0]
    var = ((win - mean) ** 2).sum(axis=0) / win.shape[0]
    return mean, np.sqrt(var)


def stats_weighted_longdouble(sig, cols, log1p_mask, T, S, w0, w1):
    """The same from the recording itself with the integer weights (the header's formula), in np.longdouble."""
    v = transformed(sig, cols, log1p_mask).astype(np.longdouble)
    m = multiplicity(sig.shape[0], T, S, w0, w1).astype(np.longdouble)[:, None]
    W = np.longdouble((w1 - w0) * T)
    p = v[w0 * S]
    mean = p + (m * (v - p)).sum(axis=0) / W
    var = (m * (v - p) ** 2).sum(axis=0) / W - (mean - p) ** 2
    return mean, np.sqrt(np.maximum(var, 0))


def batch(sig, cols, log1p_mask, T, S, n0, B, mean, inv):
    """(B, C, T) float32: (float)((v - mean) * inv) in float64, transposed."""
    v = transformed(sig, cols, log1p_mask)
    win = materialise(v, T, S)[n0:n0 + B]
    return np.ascontiguousarray((((win - np.asarray(mean, dtype=np.float64)) * np.asarray(inv, dtype=np.float64)).astype(np.float32)).transpose(0, 2, 1))


def ema(score, halflife):
    a = 1.0 - 2.0 ** (-1.0 / halflife)
    out = []
    for n, x in enumerate(score):
        out.append(float(x) if n == 0 else out[-1] + a * (float(x) - out[-1]))
    return np.array(out, dtype=np.float64)


def state_and_events(smoothed, t_end, on, off, min_on):
    """The hysteresis state with short episodes dropped, and (start_s, end_s, peak, mean) per kept episode."""
    raw, cur = [], False
    for v in smoothed:
        if cur:
            if v <= off:
                cur = False
        elif v >= on:
            cur = True
        raw.append(cur)
    state, events, n = [False] * len(raw), [], 0
    while n < len(raw):
        if not raw[n]:
            n += 1
            continue
        e = n
        while e < len(raw) and raw[e]:
            e += 1
        if e - n >= min_on:
            for k in range(n, e):
                state[k] = True
            seg = [float(smoothed[k]) for k in range(n, e)]
            events.append((float(t_end[n]), float(t_end[e - 1]), max(seg), sum(seg) / len(seg)))
        n = e
    return np.array(state, dtype=bool), events
