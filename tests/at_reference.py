"""Numpy restatement of include/msig_at.h: the path kernel, the reduction of the path batch's gradients,
and the quadrature, target and occlusion tables of multimodalsignal_amd/attribute.py.  Test-only; what tests/ab_reference.py is to
msig_ab.h.  fp64 throughout, rounded to fp32 where the kernels round."""
import numpy as np

BASE_ZERO, BASE_CHANNEL, BASE_SHARED, BASE_OWN = range(4)
MAX_POINTS = 256


def midpoint(P):
    """(alpha, w) of the midpoint rule: alpha_p = (p + 1/2) / P, w_p = 1 / P."""
    assert 1 <= P <= MAX_POINTS
    return (np.arange(P, dtype=np.float64) + 0.5) / P, np.full(P, 1.0 / P)


def ig_coef(P, C):
    return np.repeat(midpoint(P)[0][:, None], C, axis=1)


def occlusion_coef(C):
    coef = np.ones((C + 1, C))
    for c in range(C):
        coef[c, c] = 0.0
    return coef


def class_target(k, K):
    v = np.full(K, -1.0 / (K - 1))
    v[k] = 1.0
    return v


def broadcast_base(base, kind, N, C, T, dtype=np.float64):
    """The baseline as an (N, C, T) array."""
    if kind == BASE_ZERO:
        return np.zeros((N, C, T), dtype=dtype)
    b = np.asarray(base, dtype=dtype)
    if kind == BASE_CHANNEL:
        return np.broadcast_to(b.reshape(1, C, 1), (N, C, T)).copy()
    if kind == BASE_SHARED:
        return np.broadcast_to(b.reshape(1, C, T), (N, C, T)).copy()
    return b.reshape(N, C, T).copy()


def path(x, base, kind, coef):
    """xp (N * P, C, T) float32 = fmaf(coef[p][c], x - x0, x0): the difference is the fp32 one, the multiply-add is done in fp64
    (an exact product of two fp32 values, one addition) and rounded to fp32 — the fused operation up to a double rounding.  Where
    coef is exactly 1 the row holds x's own bits."""
    x = np.asarray(x, dtype=np.float32)
    N, C, T = x.shape
    P = coef.shape[0]
    b = broadcast_base(base, kind, N, C, T, np.float32)
    d = (x - b).astype(np.float32)                                   # IEEE fp32 subtraction
    c32 = np.asarray(coef, dtype=np.float32).astype(np.float64)
    xp = (c32[None, :, :, None] * d.astype(np.float64)[:, None] + b.astype(np.float64)[:, None]).astype(np.float32)
    xp = np.where(c32[None, :, :, None] == 1.0, x[:, None], xp)
    return xp.reshape(N * P, C, T)


def path_dlogits(v, P):
    return np.repeat(np.asarray(v, dtype=np.float32), P, axis=0)


def reduce_map(dx, x, base, kind, w):
    """The exact map in fp64, (N, C, T), and the rounding bound of the kernel's chain per element: P fused multiply-adds, the
    subtraction and the product round once each, every one by at most 2^-24 of a value no larger than |x - x0| * sum_p |w_p dx_p|."""
    x = np.asarray(x, dtype=np.float64)
    N, C, T = x.shape
    P = len(w)
    w64 = np.asarray(w, dtype=np.float32).astype(np.float64)
    d = x - broadcast_base(base, kind, N, C, T)
    g = np.asarray(dx, dtype=np.float64).reshape(N, P, C, T)
    G = (w64[None, :, None, None] * g).sum(axis=1)
    mag = (np.abs(w64)[None, :, None, None] * np.abs(g)).sum(axis=1)
    return d * G, (P + 2) * 2.0 ** -24 * np.abs(d) * mag


def sums_of_map(amap, bin):
    """(bins, chan, total) float32: the fp64 sums of the fp32 map values in index order, rounded once."""
    m = np.asarray(amap, dtype=np.float32).astype(np.float64)
    N, C, T = m.shape
    NB = -(-T // bin)
    bins = np.stack([m[:, :, j * bin:min(T, (j + 1) * bin)].sum(axis=2) for j in range(NB)], axis=2)
    chan = m.sum(axis=2)
    total = chan.sum(axis=1)
    return bins.astype(np.float32), chan.astype(np.float32), total.astype(np.float32)


def within_ulps(got, want, n=1):
    """Every element of the fp32 array `got` within n fp32 ulps of `want`."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return bool(np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= n * np.spacing(np.abs(want)).astype(np.float64)))


def integrated_gradients(grad_f, x, base, P):
    """IG of one window by the midpoint rule in fp64: grad_f(xp) -> df/dx at xp.  Returns (map, G)."""
    alpha, w = midpoint(P)
    G = np.zeros_like(x, dtype=np.float64)
    for a, wp in zip(alpha, w):
        G += wp * grad_f(base + a * (x - base))
    return (x - base) * G, G


def path_plan(N, P, path_batch):
    per = path_batch // P
    assert per >= 1
    return [(i, min(per, N - i)) for i in range(0, N, per)]
