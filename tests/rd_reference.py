"""A numpy restatement of include/msig_rd.h — the exponentially decayed running reference — and of the live state built on it,
written from the header's definitions on top of tests/rn_reference.py (the window sums, the pivot and the finishing lines are
msig_rn.h's and are taken from there unchanged): A_0 = W_0, c_0 = 1, A_n = fma(lambda, A_{n-1}, W_n), c_n = fma(lambda, c_{n-1}, 1),
statistics = rn_reference.finish with n_ref = c_n.  Everything exists twice — in float64, where the fused multiply-add is exact
(the rational a x + y rounded once), and in np.longdouble."""
from fractions import Fraction

import numpy as np

import rn_reference as R

MAX_C, REC = R.MAX_C, R.REC
STATE_C = 3 * MAX_C + 2          # MSIG_RD_STATE_C
MAX_H = 1 << 20


def decay_of(H):
    """The host's lambda for a half-life of H windows."""
    return float(np.exp2(-1.0 / H))


def _fma1(a, x, y):
    return float(Fraction(a) * Fraction(x) + Fraction(y))        # exact in rationals, then ONE rounding to float64 (half to even)


def fma64(a, x, y):
    """fma(a, x, y) in float64, elementwise and correctly rounded: the exact rational a x + y, rounded once."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    out = np.array([_fma1(float(a), float(u), float(w)) for u, w in zip(x.reshape(-1), np.broadcast_to(y, x.shape).reshape(-1))], dtype=np.float64)
    return out.reshape(x.shape)


def _fma(lam, prev, w):
    if w.dtype == np.float64:
        return fma64(lam, prev, w)
    return w.dtype.type(lam) * prev + w           # np.longdouble: the product and the sum in the wider type


def reference_sums(W, lam):
    """(A (N, 2, C), c (N,)) in W's dtype: the decayed sums and the effective window counts."""
    A, c = np.zeros_like(W), np.zeros(W.shape[0], dtype=W.dtype)
    for n in range(W.shape[0]):
        if n == 0:
            A[0], c[0] = W[0], 1
        else:
            A[n] = _fma(lam, A[n - 1], W[n])
            c[n] = _fma(lam, c[n - 1:n], np.ones(1, dtype=W.dtype))[0]
    return A, c


def stats_table(v, T, S, lam):
    """(mean (N, C), inv (N, C), c (N,)) of every window under decay lam, in v's dtype."""
    W = R.window_sums(v, T, S)
    A, c = reference_sums(W, lam)
    N = W.shape[0]
    mean, inv = np.zeros((N, v.shape[1]), dtype=v.dtype), np.zeros((N, v.shape[1]), dtype=v.dtype)
    for n in range(N):
        mean[n], inv[n] = R.finish(A[n], v[0], c[n], T)
    return mean, inv, c


def std_longdouble(v, T, S, lam):
    """(N, C): the weighted population std of the materialised samples of windows 0..n, window k weighted lam^(n - k), about their
    weighted mean — two passes in np.longdouble.  The yardstick's unit for a mean's error."""
    v = v.astype(np.longdouble)
    N = R.count(v.shape[0], T, S)
    lam = np.longdouble(lam)
    out = np.zeros((N, v.shape[1]), dtype=np.longdouble)
    for n in range(N):
        wts = np.array([lam ** (n - k) if (lam > 0 or k == n) else np.longdouble(0) for k in range(n + 1)], dtype=np.longdouble)
        wins = np.stack([v[k * S:k * S + T] for k in range(n + 1)])                   # (n + 1, T, C)
        tot = wts.sum() * T
        mean = (wts[:, None, None] * wins).sum(axis=(0, 1)) / tot
        out[n] = np.sqrt((wts[:, None, None] * (wins - mean) ** 2).sum(axis=(0, 1)) / tot)
    return out


class LiveState:
    """A host model of one session's state under msig_rd_lv_step: the pivot of sample 0, the carry A, c and the next expected
    window.  step(n, window) takes window n's own (T, C) transformed samples and returns (mean, inv, c_n)."""

    def __init__(self, lam):
        assert 0.0 <= lam <= 1.0
        self.lam, self.pivot, self.carry, self.c, self.next = lam, None, None, None, 0

    def step(self, n, win):
        assert n == self.next, "not the session's next window"
        if n == 0:
            self.pivot = win[0].copy()
        d = win - self.pivot
        w = np.stack([R._ordered(d), R._ordered(d * d)])
        if n == 0:
            self.carry, self.c = w, win.dtype.type(1)
        else:
            self.carry = _fma(self.lam, self.carry, w)
            self.c = _fma(self.lam, np.array([self.c], dtype=win.dtype), np.ones(1, dtype=win.dtype))[0]
        self.next += 1
        mean, inv = R.finish(self.carry, self.pivot, self.c, win.shape[0])
        return mean, inv, self.c
