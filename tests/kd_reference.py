"""Test-only restatement of the distillation term and the teacher table (include/msig_kd.h) in numpy: fp64, and fp32 with the
header's operation order (one rounding per operation).  Its arithmetic is its own; nothing here is imported by the product."""
import math

import numpy as np

from mc_reference import ulp32, within_store_rounding  # noqa: F401  (the comparison rule, re-exported)


def teacher(logits, T):
    """logits (M, N, K) member-major -> (N, K) float64: the mean over the members, in increasing m, of softmax(logits / T),
    max-subtracted, python floats throughout (the header's order)."""
    lg = np.asarray(logits, dtype=np.float64)
    M, N, K = lg.shape
    T = float(np.float32(T))
    out = np.zeros((N, K))
    for n in range(N):
        rows = []
        for m in range(M):
            u = [float(v) / T for v in lg[m, n]]
            best = max(u)
            ex = [math.exp(v - best) for v in u]
            tot = 0.0
            for v in ex:
                tot += v
            rows.append([v / tot for v in ex])
        for k in range(K):
            acc = 0.0
            for m in range(M):
                acc += rows[m][k]
            out[n, k] = acc / M
    return out


def crafted_logits(M, N, K, seed):
    """(M, N, K) fp32: window 0 has a saturated member (logits +80 / -80), window 1 an exact two-way tie for the maximum in every
    member, window 2 all members equal; the others generic."""
    rs = np.random.RandomState(seed)
    lg = (3.0 * rs.randn(N, M, K)).astype(np.float32)
    lg[0, 0, :] = -80.0
    lg[0, 0, K - 1] = 80.0
    lg[1, :, 0] = lg[1].max(axis=1) + 1.0
    lg[1, :, 1] = lg[1, :, 0]
    lg[2, :, :] = lg[2, 0, :]
    return np.ascontiguousarray(lg.transpose(1, 0, 2))


def lookup(q, B, idx=None):
    """The batch's teacher rows (B, K) float32: q[idx[b]], or q[b]."""
    q = np.asarray(q, dtype=np.float32)
    return q[np.asarray(idx, dtype=np.int64)[:B]] if idx is not None else q[:B]


def blend(rows, lam):
    """qm_b = fadd(fmul(lam, q_b), fmul(1.f - lam, q_{B-1-b})) in fp32; lam == 1: q_b itself."""
    rows = np.asarray(rows, dtype=np.float32)
    lam = np.float32(lam)
    if lam == np.float32(1.0):
        return rows.copy()
    mu = np.float32(1.0) - lam
    return (lam * rows).astype(np.float32) + (mu * rows[::-1]).astype(np.float32)


def apply(z, dlogits, qm, alpha, T, dtype=np.float64):
    """The launch on one fold: z, dlogits (B, K) fp32 values, qm the blended fp32 teacher rows, alpha and T as the fp32 values the
    call carries.  Returns dict(dlogits, s, L_kd, stats) — in `dtype` arithmetic for dlogits and s (fp32: the header's operation
    order, kappa and 1.f - alpha formed as the library forms them); L_kd and stats always in fp64 from that dtype's u."""
    z, dl, qm = (np.asarray(v, dtype=np.float32) for v in (z, dlogits, qm))
    B, K = z.shape
    a32, T32 = np.float32(alpha), np.float32(T)
    if dtype == np.float32:
        om = np.float32(1.0) - a32
        kappa = np.float32(float(a32) * float(T32) / B)
        u = (z / T32).astype(np.float32)
        u = (u - u.max(axis=1, keepdims=True)).astype(np.float32)
        e = np.exp(u).astype(np.float32)
        S = np.zeros(B, dtype=np.float32)
        for c in range(K):
            S = (S + e[:, c]).astype(np.float32)
        s = (e / S[:, None]).astype(np.float32)
        out = ((om * dl).astype(np.float32) + (kappa * (s - qm).astype(np.float32)).astype(np.float32)).astype(np.float32)
    else:
        om, kappa = 1.0 - float(a32), float(a32) * float(T32) / B
        u = z.astype(np.float64) / float(T32)
        u = u - u.max(axis=1, keepdims=True)
        e = np.exp(u)
        S = e.sum(axis=1)
        s = e / S[:, None]
        out = om * dl.astype(np.float64) + kappa * (s - qm.astype(np.float64))
    qd = qm.astype(np.float64)
    ln_s = u.astype(np.float64) - np.log(S.astype(np.float64))[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = np.where(qd > 0, qd * (np.log(np.where(qd > 0, qd, 1.0)) - ln_s), 0.0)
    L_kd = float(T32) ** 2 * float(terms.sum()) / B
    agree = int((z.argmax(axis=1) == qm.argmax(axis=1)).sum())
    return dict(dlogits=out, s=s, L_kd=L_kd, stats=np.array([B * L_kd, float(agree), float(B)]))


def argmax_margins(z, qm):
    """The smallest gap between the two largest entries of any row of z and of qm: the counts are the same decision in fp32 and
    fp64 only where these are well above fp32 resolution (or exactly zero by construction)."""
    tz, tq = np.sort(np.asarray(z, dtype=np.float64), axis=1), np.sort(np.asarray(qm, dtype=np.float64), axis=1)
    return float((tz[:, -1] - tz[:, -2]).min()), float((tq[:, -1] - tq[:, -2]).min())
