"""Soft targets of include/msig_st.h restated (a helper, not a test): the mixed gather in float32 numpy, bit for bit, on top of
aug_reference, and the loss and its logit gradient of DESIGN.md section 17 in float64 numpy.

The partner of batch row b is row B-1-b.  `mix` is out[b] = fadd(fmul(lam, A_b), fmul(mu, A_{B-1-b})) with mu = 1.f - lam and A the
batch after every row's own augmentation; lam = 1 returns A itself (no arithmetic).  `loss_and_dlogits` is
lam * CE(z, y, w, eps) + (1 - lam) * CE(z, flip(y), w, eps) with mean reduction, written out term by term.
"""
import numpy as np

import aug_reference as R


def mix(store, idx, lam, key=0, **aug):
    """store (N, C, T) float32, idx (B,) store positions -> the (B, C, T) float32 batch of msig_st_gather_windows: augmented with
    `key` and the aug_reference.augment parameters in `aug` (none: the plain windows), then mixed with weight `lam`."""
    a = R.augment(store, idx, key, **aug) if aug else np.asarray(store, np.float32)[np.asarray(idx, np.int64)].copy()
    lam = np.float32(lam)
    if lam == np.float32(1.0):
        return a
    mu = np.float32(1.0) - lam
    own = lam * a                      # three separate fp32 roundings: numpy never contracts
    par = mu * a[::-1]
    out = own + par
    assert out.dtype == np.float32
    return out


def loss_and_dlogits(z, y, eps=0.0, lam=1.0, w=None):
    """z (B, K) logits, y (B,) labels -> (L, dL/dz (B, K)) in float64 by the formulas of include/msig_st.h."""
    z = np.asarray(z, np.float64)
    y = np.asarray(y, np.int64)
    B, K = z.shape
    w = np.ones(K) if w is None else np.asarray(w, np.float64)
    y2 = y[::-1]
    m = z.max(axis=1, keepdims=True)
    lse = m + np.log(np.exp(z - m).sum(axis=1, keepdims=True))
    ell = lse - z                                                  # l_b(c) = -log softmax(z_b)_c
    p = np.exp(-ell)
    rows = np.arange(B)
    W = w[y].sum()
    hard = lam * w[y] * ell[rows, y] + (1.0 - lam) * w[y2] * ell[rows, y2]
    L = ((1.0 - eps) * hard.sum() + (eps / K) * (ell * w[None, :]).sum()) / W
    oh, oh2 = np.zeros((B, K)), np.zeros((B, K))
    oh[rows, y] = 1.0
    oh2[rows, y2] = 1.0
    d = (1.0 - eps) * (lam * w[y][:, None] * (p - oh) + (1.0 - lam) * w[y2][:, None] * (p - oh2)) + (eps / K) * (p * w.sum() - w[None, :])
    return float(L), d / W
