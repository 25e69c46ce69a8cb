"""A numpy restatement of include/msig_rn.h and of the live state machine built on it, written from the header's definitions and
sharing no code with the library or with monitor.py / live.py: the windows are MATERIALISED here, a window's sums are taken in the
header's order (thread j of 256 takes samples j, j + 256, ...; the 64 lanes of a wave by xor-butterfly; the four waves in index
order), a reference is a left-to-right sum of window records, and everything exists twice — in float64 and in np.longdouble."""
import numpy as np

MAX_C = 16
REC = 2 * MAX_C + 1
MAX_K = 4096
WG, WAVE = 256, 64


def count(L, T, S):
    return 0 if L < T else (L - T) // S + 1


def transformed(sig, cols, log1p_mask, dtype=np.float64):
    """(L, C): the selected columns, log1p where the mask says so, computed in `dtype`."""
    v = sig[:, cols].astype(dtype)
    for c in range(len(cols)):
        if (log1p_mask >> c) & 1:
            v[:, c] = np.log1p(v[:, c])
    return v


def _ordered(d):
    """d: (T, C) in any dtype -> (C,) the sum over T in the header's order."""
    T, Cn = d.shape
    steps = -(-T // WG)
    pad = np.zeros((steps * WG, Cn), dtype=d.dtype)
    pad[:T] = d
    acc = np.zeros((WG, Cn), dtype=d.dtype)
    for s in range(steps):                       # thread j: samples j, j + 256, ...
        acc = acc + pad[s * WG:(s + 1) * WG]
    lanes = acc.reshape(WG // WAVE, WAVE, Cn)
    idx = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):               # v += shfl_xor(v, o)
        lanes = lanes + lanes[:, idx ^ o]
    r = lanes[:, 0]
    return ((r[0] + r[1]) + r[2]) + r[3]


def window_sums(v, T, S, pivot=None):
    """(N, 2, C) in v's dtype: W1 and W2 of every window about the pivot (default: v[0]), each over the window's own T samples."""
    p = v[0] if pivot is None else pivot
    N = count(v.shape[0], T, S)
    out = np.zeros((N, 2, v.shape[1]), dtype=v.dtype)
    for n in range(N):
        d = v[n * S:n * S + T] - p
        out[n, 0], out[n, 1] = _ordered(d), _ordered(d * d)
    return out


def first_window(n, K):
    return 0 if K == 0 else max(0, n - K + 1)


def reference_sums(W, K):
    """(N, 2, C): A[n] = W[a_n] + ... + W[n], left to right.  K = 0 carries the sum from window to window."""
    out = np.zeros_like(W)
    carry = None
    for n in range(W.shape[0]):
        if K == 0:
            carry = W[0].copy() if n == 0 else carry + W[n]
            out[n] = carry
        else:
            a = first_window(n, K)
            acc = W[a].copy()
            for k in range(a + 1, n + 1):
                acc = acc + W[k]
            out[n] = acc
    return out


def finish(A, p, n_ref, T):
    """One window: (mean, inv) per channel from its reference's sums, in A's dtype."""
    dt = A.dtype.type
    cnt = dt(n_ref) * dt(T)
    dm = A[0] / cnt
    var = np.maximum(A[1] / cnt - dm * dm, dt(0))
    return p + dm, dt(1) / (np.sqrt(var) + dt(1e-8))


def stats_table(v, T, S, K):
    """(mean (N, C), inv (N, C), counts (N,)) of every window under mode K, in v's dtype."""
    W = window_sums(v, T, S)
    A = reference_sums(W, K)
    N = W.shape[0]
    mean, inv, cnt = np.zeros((N, v.shape[1]), dtype=v.dtype), np.zeros((N, v.shape[1]), dtype=v.dtype), np.zeros(N, dtype=np.int64)
    for n in range(N):
        cnt[n] = n - first_window(n, K) + 1
        mean[n], inv[n] = finish(A[n], v[0], cnt[n], T)
    return mean, inv, cnt


def std_longdouble(v, T, S, K):
    """(N, C): the population std of the reference windows' materialised samples, two passes in np.longdouble."""
    v = v.astype(np.longdouble)
    N = count(v.shape[0], T, S)
    out = np.zeros((N, v.shape[1]), dtype=np.longdouble)
    for n in range(N):
        win = np.concatenate([v[k * S:k * S + T] for k in range(first_window(n, K), n + 1)])
        out[n] = np.sqrt(((win - win.mean(axis=0)) ** 2).mean(axis=0))
    return out


def rows(v, T, S, n0, mean, inv):
    """(B, C, T) float32 for windows n0 .. n0 + B - 1, row b with its own (mean[b], inv[b]): (float)((v - mean) * inv) in float64."""
    out = [(((v[(n0 + b) * S:(n0 + b) * S + T] - mean[b]) * inv[b]).astype(np.float32)).T for b in range(len(mean))]
    return np.ascontiguousarray(np.stack(out))


def record(mean, inv, n_ref, Cn):
    r = np.zeros(REC, dtype=np.float64)
    r[:Cn], r[MAX_C:MAX_C + Cn], r[2 * MAX_C] = mean, inv, n_ref
    return r


class LiveState:
    """A host model of one session's state: the pivot of sample 0, the expanding carry, the ring of the last K window records
    (slot k % K) and the next expected window.  step(n, window) takes window n's own (T, C) transformed samples."""

    def __init__(self, K):
        assert 0 <= K <= MAX_K
        self.K, self.pivot, self.carry, self.ring, self.next = K, None, None, [None] * K, 0

    def step(self, n, win):
        assert n == self.next, "not the session's next window"
        if n == 0:
            self.pivot = win[0].copy()
        d = win - self.pivot
        w = np.stack([_ordered(d), _ordered(d * d)])
        if self.K == 0:
            self.carry = w if n == 0 else self.carry + w
            acc, n_ref = self.carry, n + 1
        else:
            self.ring[n % self.K] = w
            a = first_window(n, self.K)
            acc = self.ring[a % self.K].copy()
            for k in range(a + 1, n + 1):
                acc = acc + self.ring[k % self.K]
            n_ref = n - a + 1
        self.next += 1
        mean, inv = finish(acc, self.pivot, n_ref, win.shape[0])
        return mean, inv, n_ref
