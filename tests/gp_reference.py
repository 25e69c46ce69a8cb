"""A numpy restatement of include/msig_gp.h — running references over recordings with MISSING samples — and of the host logic built
on it (ema_gaps, hysteresis_gaps, the live alarms), written from the header's definitions and sharing no code with the library or
with monitor.py / live.py.  The windows are materialised, a sample is missing when its float64 bit pattern has an all-ones exponent
field, a window's record is taken in the header's order (tests/rn_reference.py's `_ordered`, a missing sample adding zeros), a
reference is an ordered combination of records, and the statistics exist twice — in float64 and in np.longdouble (which samples are
missing is decided in float64 for both, as the header says).  Also the planted inputs of the gap tests."""
import numpy as np

import rd_reference as RD
import rn_reference as R

MAX_C, REC = R.MAX_C, R.REC
SUM, PIVOT, COV = 3 * MAX_C, 2 * MAX_C, MAX_C
STATE_HEAD, STATE_NEXT = 6 * MAX_C, 5 * MAX_C
EXPANDING, TRAILING, DECAYED = 0, 1, 2
QNAN = np.array([0x7ff8000000000000], dtype=np.uint64).view(np.float64)[0]


def missing(v64):
    """bool, elementwise: the float64's exponent field is all ones (NaN, +Inf, -Inf)."""
    bits = np.ascontiguousarray(v64, dtype=np.float64).view(np.uint64)
    return (bits & np.uint64(0x7ff0000000000000)) == np.uint64(0x7ff0000000000000)


def transformed(sig, cols, log1p_mask, dtype=np.float64):
    """(v (L, C) in `dtype`, ok (L, C) bool): the selected columns, log1p where the mask says so; ok from the float64 value's bits.
    A missing sample's v is 0 in the returned array (it is never used)."""
    with np.errstate(all="ignore"):
        v64 = sig[:, cols].astype(np.float64)
        v = sig[:, cols].astype(dtype)
        for c in range(len(cols)):
            if (log1p_mask >> c) & 1:
                v64[:, c] = np.log1p(v64[:, c])
                v[:, c] = np.log1p(v[:, c])
    ok = ~missing(v64)
    return np.where(ok, v, dtype(0)), ok


def pivot(v, ok, T, S, N):
    """(p (C,), found (C,) bool): the first valid sample of each channel in window order."""
    Cn = v.shape[1]
    p, found = np.zeros(Cn, dtype=v.dtype), np.zeros(Cn, dtype=bool)
    for c in range(Cn):
        for n in range(N):
            hit = np.flatnonzero(ok[n * S:n * S + T, c])
            if hit.size:
                p[c], found[c] = v[n * S + hit[0], c], True
                break
    return p, found


def window_records(v, ok, T, S, N, p):
    """(N, 3, C) in v's dtype: W1, W2 over the valid samples about p, and N, in the header's order."""
    out = np.zeros((N, 3, v.shape[1]), dtype=v.dtype)
    for n in range(N):
        m = ok[n * S:n * S + T]
        d = np.where(m, v[n * S:n * S + T] - p, v.dtype.type(0))
        out[n, 0], out[n, 1], out[n, 2] = R._ordered(d), R._ordered(d * d), R._ordered(m.astype(v.dtype))
    return out


def terms(W, T):
    """(N, 3, C): the records as terms of a reference — W1, W2 and the quotient N / T."""
    X = W.copy()
    X[:, 2] = W[:, 2] / W.dtype.type(T)
    return X


def first_window(n, mode):
    return max(0, n - mode[1] + 1) if mode[0] == TRAILING else 0


def reference(X, mode):
    """(A (N, 3, C), n_ref (N,)): the combined terms and the number of windows as msig_rn.h / msig_rd.h count them.
    mode = (kind, K, decay)."""
    kind, _K, lam = mode
    N = X.shape[0]
    A, n_ref = np.zeros_like(X), np.zeros(N, dtype=X.dtype)
    for n in range(N):
        if kind == TRAILING:
            a = first_window(n, mode)
            acc = X[a].copy()
            for k in range(a + 1, n + 1):
                acc = acc + X[k]
            A[n], n_ref[n] = acc, n - a + 1
        elif n == 0:
            A[0], n_ref[0] = X[0], 1
        elif kind == EXPANDING:
            A[n], n_ref[n] = A[n - 1] + X[n], n + 1
        else:
            A[n] = RD._fma(lam, A[n - 1].reshape(-1), X[n].reshape(-1)).reshape(X[n].shape)
            n_ref[n] = RD._fma(lam, n_ref[n - 1:n], np.ones(1, dtype=X.dtype))[0]
    return A, n_ref


def finish(A, p, T):
    """One window: (mean, inv) per channel; a channel whose count is 0 has (0, 0)."""
    dt = A.dtype.type
    cnt = A[2] * dt(T)
    has = cnt != 0
    safe = np.where(has, cnt, dt(1))
    dm = A[0] / safe
    var = np.maximum(A[1] / safe - dm * dm, dt(0))
    return np.where(has, p + dm, dt(0)), np.where(has, dt(1) / (np.sqrt(var) + dt(1e-8)), dt(0))


def stats_table(v, ok, T, S, N, mode):
    """(mean (N, C), inv (N, C), n_ref (N,), coverage (N, C), W (N, 3, C), has (N, C)) in v's dtype."""
    p, _found = pivot(v, ok, T, S, N)
    W = window_records(v, ok, T, S, N, p)
    X = terms(W, T)
    A, n_ref = reference(X, mode)
    mean, inv = np.zeros((N, v.shape[1]), dtype=v.dtype), np.zeros((N, v.shape[1]), dtype=v.dtype)
    for n in range(N):
        mean[n], inv[n] = finish(A[n], p, T)
    return mean, inv, n_ref, X[:, 2], W, A[:, 2] != 0


def std_longdouble(v, ok, T, S, N, mode):
    """(N, C): the weighted population std of the VALID materialised samples of window n's reference windows about their weighted
    mean, two passes in np.longdouble (weight 1, or lambda^(n - k) under decayed); 0 where there is no valid sample."""
    v = v.astype(np.longdouble)
    kind, _K, lam = mode
    out = np.zeros((N, v.shape[1]), dtype=np.longdouble)
    for n in range(N):
        a = first_window(n, mode)
        ks = list(range(a, n + 1))
        wt = np.array([np.longdouble(lam) ** (n - k) if kind == DECAYED and (lam > 0 or k == n) else
                       np.longdouble(0 if kind == DECAYED else 1) for k in ks], dtype=np.longdouble)
        wins = np.stack([v[k * S:k * S + T] for k in ks])
        m = np.stack([ok[k * S:k * S + T] for k in ks]) * wt[:, None, None]
        tot = m.sum(axis=(0, 1))
        safe = np.where(tot > 0, tot, 1)
        mean = (m * wins).sum(axis=(0, 1)) / safe
        out[n] = np.where(tot > 0, np.sqrt((m * (wins - mean) ** 2).sum(axis=(0, 1)) / safe), 0)
    return out


def rows(v64, ok, T, S, n0, mean, inv):
    """(B, C, T) float32 for windows n0 .. : (float)((v - mean_b) * inv_b) in float64 for a valid sample, +0.0 for a missing one."""
    out = []
    for b in range(len(mean)):
        sl = slice((n0 + b) * S, (n0 + b) * S + T)
        z = ((v64[sl] - mean[b]) * inv[b]).astype(np.float32)
        out.append(np.where(ok[sl], z, np.float32(0)).T)
    return np.ascontiguousarray(np.stack(out))


# ---- the host logic --------------------------------------------------------------------------------------------------------------
def lost(valid, lost_after):
    out, run = [], 0
    for ok in valid:
        run = 0 if ok else run + 1
        out.append(run >= lost_after)
    return np.array(out, dtype=bool)


def ema_gaps(score, valid, halflife, lost_after):
    a = 1.0 if halflife == 0 else 1.0 - 2.0 ** (-1.0 / float(halflife))
    out, s, fresh, run = [], 0.0, True, 0
    for v, ok in zip(score, valid):
        if ok:
            run = 0
            s = float(v) if fresh else s + a * (float(v) - s)
            fresh = False
        else:
            run += 1
            if run >= lost_after:
                fresh = True
        out.append(s)
    return np.array(out, dtype=np.float64)


def raw_state(smoothed, valid, on, off, lost_after):
    """The state before min_on: holds through invalid windows, off from the window where the invalid run reaches lost_after."""
    raw, cur, run = [], False, 0
    for v, ok in zip(smoothed, valid):
        if ok:
            run = 0
            if cur and v <= off:
                cur = False
            elif not cur and v >= on:
                cur = True
        else:
            run += 1
            if run >= lost_after:
                cur = False
        raw.append(cur)
    return raw


def hysteresis_gaps(smoothed, valid, on, off, min_on, lost_after):
    raw = raw_state(smoothed, valid, on, off, lost_after)
    out, n, N = np.zeros(len(raw), dtype=bool), 0, len(raw)
    while n < N:
        if raw[n]:
            a = n
            while n < N and raw[n]:
                n += 1
            if n - a >= min_on:
                out[a:n] = True
        else:
            n += 1
    return out


def alarms(smoothed, valid, on, off, min_on, lost_after):
    """[(kind, window, start_window)] of a live session, read off the whole vectors: a maximal run [a, b) of the raw state of at
    least min_on windows raises an onset at a + min_on - 1 and, if it ends before the stream does, an offset at b; a run [a, b) of
    invalid windows of at least lost_after raises `lost` at a + lost_after - 1 and, if the stream goes on, `back` at b.  At one
    window: back, offset, lost, onset."""
    raw = raw_state(smoothed, valid, on, off, lost_after)
    out, N = [], len(raw)

    def runs(flags):
        n = 0
        while n < N:
            if flags[n]:
                a = n
                while n < N and flags[n]:
                    n += 1
                yield a, n
            else:
                n += 1

    for a, b in runs(raw):
        if b - a >= min_on:
            out.append(("onset", a + min_on - 1, a))
            if b < N:
                out.append(("offset", b, a))
    for a, b in runs([not ok for ok in valid]):
        if b - a >= lost_after:
            out.append(("lost", a + lost_after - 1, a))
            if b < N:
                out.append(("back", b, a))
    rank = {"back": 0, "offset": 1, "lost": 2, "onset": 3}
    return sorted(out, key=lambda e: (e[1], rank[e[0]]))


# ---- the planted inputs of the gap tests -------------------------------------------------------------------------------------------
INPUTS = ("none", "sample0", "inf", "log1p_m1", "log1p_m2", "one_window", "late_pivot", "all_off", "drop5")
LOG_COL = 1          # lv_reference.NAMES8's chest_EDA


def plant(sig, kind, T, S, cols, lost_after):
    """A copy of the (L, 8) recording with the input `kind` planted.  `cols`: the selected columns (the single-channel inputs take
    cols[0]).  Needs at least lost_after + 6 windows."""
    x = sig.copy()
    rs = np.random.RandomState(len(kind) * 1000 + T + S)
    if kind == "sample0":
        x[0, :] = np.nan
    elif kind == "inf":
        at = rs.choice(x.shape[0], size=max(4, x.shape[0] // 40), replace=False)
        x[at[0::2], cols[0]] = np.inf
        x[at[1::2], cols[-1]] = -np.inf
        x[at[0], :] = np.inf
    elif kind in ("log1p_m1", "log1p_m2"):
        at = rs.choice(x.shape[0], size=max(3, x.shape[0] // 50), replace=False)
        x[at, LOG_COL] = -1.0 if kind == "log1p_m1" else -2.0
    elif kind == "one_window":
        x[3 * S:3 * S + T, cols[0]] = np.nan                      # exactly window 3
    elif kind == "late_pivot":
        x[:S + T, cols[0]] = np.nan                               # windows 0 and 1 whole: the pivot comes late, the count starts at 0
    elif kind == "all_off":
        x[2 * S:(2 + lost_after) * S + T, :] = np.nan             # windows 2 .. 2 + lost_after: lost_after + 1 of them
    elif kind == "drop5":
        x[rs.rand(*x.shape) < 0.05] = np.nan
    else:
        assert kind == "none"
    return x


# ---- the cases the host and the GPU tests share ------------------------------------------------------------------------------------
N_WINDOWS, LOST_AFTER = 12, 3
COLS = {"8of8": [7, 2, 0, 3, 1, 6, 5, 4], "3of8": [5, 1, 4], "1of8": [LOG_COL]}          # the log1p column is in each
SHAPES = [(256, 64, "8of8"), (200, 37, "3of8"), (200, 300, "8of8"), (256, 1, "1of8")]      # S divides T, does not, S > T, S = 1
MODES = {"expanding": (EXPANDING, 0, 0.0), "trailing1": (TRAILING, 1, 0.0), "trailing2": (TRAILING, 2, 0.0), "trailing7": (TRAILING, 7, 0.0),
         "trailing13": (TRAILING, N_WINDOWS + 1, 0.0), "decayed0": (DECAYED, 0, 0.0), "decayed1": (DECAYED, 0, 1.0),
         "decayed3": (DECAYED, 0, float(np.exp2(-1.0 / 3)))}
EPS = float(np.finfo(np.float64).eps)


def mask_of(cols):
    return sum(1 << c for c, col in enumerate(cols) if col == LOG_COL)


def case_recording(T, S, key, kind):
    """The (L, 8) float64 recording of a case: lv_reference's generator with the input planted; N_WINDOWS windows and a tail no window covers."""
    import lv_reference as LV
    sig = LV.recording((N_WINDOWS - 1) * S + T + min(2, S - 1), 9000 + 7 * T + S)
    return plant(sig, kind, T, S, COLS[key], LOST_AFTER)


def yardstick(got_mean, got_inv, T, S, key, kind, mode):
    """tests/test_running_gpu.py's criterion for one case and mode.  Returns a dict: r_mean, bound_mean, r_inv, bound_inv (N, C) — the
    error of a mean in units of the std of its reference's valid samples and of 1 / (std + 1e-8) in units of itself, against the
    np.longdouble restatement, and their bounds: 8 x the float64 restatement's own error on the same case (per channel, its
    largest over the case's windows) or, where that is smaller, a floor of 4 ulps — `flat_ok` (the entries whose reference samples
    are all equal meet the absolute condition) and `none_ok` (the entries without a reference are exactly 0), n_ref and coverage of
    the float64 restatement."""
    sig, cols = case_recording(T, S, key, kind), COLS[key]
    v64, ok = transformed(sig, cols, mask_of(cols), np.float64)
    vld, _ok = transformed(sig, cols, mask_of(cols), np.longdouble)
    N = N_WINDOWS
    m_ld, i_ld, _n, _c, _W, has = stats_table(vld, ok, T, S, N, mode)
    m_64, i_64, n_ref, cov, W, has64 = stats_table(v64, ok, T, S, N, mode)
    assert np.array_equal(has, has64)
    std = std_longdouble(vld, ok, T, S, N, mode)
    pos, flat = has & (std > 0), has & (std == 0)
    safe, isafe = np.where(pos, std, 1), np.where(has, i_ld, 1)
    r_mean, q_mean = np.where(pos, np.abs(got_mean - m_ld) / safe, 0), np.where(pos, np.abs(m_64 - m_ld) / safe, 0)
    r_inv, q_inv = np.where(pos, np.abs(got_inv - i_ld) / isafe, 0), np.where(pos, np.abs(i_64 - i_ld) / isafe, 0)
    bound_mean = np.maximum(8 * q_mean.max(axis=0)[None, :], 4 * EPS * (np.abs(m_ld) + std) / safe)
    bound_inv = np.maximum(8 * q_inv.max(axis=0)[None, :], 4 * EPS)
    p = pivot(vld, ok, T, S, N)[0][None, :].repeat(N, axis=0)
    dm = np.abs(m_ld - p)
    g_mean, g_inv = got_mean[flat], got_inv[flat]
    flat_ok = bool(np.all(np.abs(g_mean - m_ld[flat]) <= 4 * EPS * (np.abs(m_ld[flat]) + np.abs(p[flat]))) and np.all(g_inv <= 1e8)
                   and np.all(g_inv >= (1 / (np.sqrt(2 * EPS) * dm[flat] + 1e-8)).astype(np.float64) * (1 - 4 * EPS)))
    none_ok = bool(np.all(got_mean[~has] == 0) and np.all(got_inv[~has] == 0))
    return dict(r_mean=r_mean, bound_mean=bound_mean, r_inv=r_inv, bound_inv=bound_inv, flat_ok=flat_ok, none_ok=none_ok, n_ref=n_ref,
                coverage=cov, mean64=m_64, inv64=i_64, records=W, q_mean=q_mean, q_inv=q_inv, has=has, flat=int(flat.sum()))
