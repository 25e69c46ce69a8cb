"""fp64 numpy restatement of include/msig_tt.h's objective: the entropy of the model's own predictions with the optional diversity
term, its exact gradient with respect to the logits, and the statistics the kernel accumulates.  Formula by formula the header's
text; the CPU tier holds the gradient to torch autograd of `loss_torch`, the GPU tier holds the kernel to `objective`."""
import numpy as np

TT_STATS, S_ENT, S_ROWS, S_HQ, S_STEPS, S_P, S_PRED = 36, 0, 1, 2, 3, 4, 20
BATCHES = (1, 2, 3, 63, 64, 65, 257, 2048)
CLASSES = (2, 3, 16)
DIVERSITIES = (0.0, 0.5, 1.0)
REGIMES = ("near_uniform", "equal", "saturated")


def logits_case(B: int, K: int, regime: str, seed: int = 0) -> np.ndarray:
    """(B, K) float32 logits of one regime: near-uniform rows (|z - mean| ~ 1e-3: lp + H cancels almost completely), exactly equal
    rows (it cancels to rounding) and saturated rows (|z| up to 80: p spans 70 decades)."""
    rs = np.random.RandomState(1000 * B + 10 * K + seed)
    if regime == "near_uniform":
        z = 0.3 + 1e-3 * rs.randn(B, K)
    elif regime == "equal":
        z = np.repeat(rs.randn(B, 1), K, axis=1)
    elif regime == "saturated":
        # Ordinary rows (b % 3 == 2) among saturated ones, whose peak class b % K leads by 52 or more: exp(-52) is below half an ulp of
        # 1, so the row's sum of exponentials is exactly 1 in fp64 and H_b, a sum of terms p lp of size exp(-margin), keeps its
        # RELATIVE accuracy.  (With a lead of 10 .. 36 the logarithm of 1 + exp(-margin) loses exp(margin) ulps, in this restatement
        # as in any fp64 evaluation of the header's formulas: a statistic of one or two such rows has no 1e-12 to be held to.)  The
        # peaks rotate over the classes, so q is never close to one-hot.  Every other saturated row has its peak TWICE (H_b = ln 2 at
        # logits of 60 .. 80: the row maximum must be subtracted, and the entropy term of the gradient is of order 1 there, which a
        # row with one peak cannot show), row 0 among them, so that every case down to B = 1 holds such a row.
        z = rs.randn(B, K)
        for b in range(B):
            if b % 3 != 2:
                v = 80.0 if b == 0 else rs.uniform(60.0, 79.0)
                z[b, b % K] = v
                if b % 2 == 0:
                    z[b, (b + 1) % K] = v
                    if K >= 3:
                        z[b, (b + 2) % K] = -80.0
    else:
        raise ValueError(regime)
    return z.astype(np.float32)


def objective(z, div: float):
    """dict of L, dlogits (fp64, before the one rounding to fp32), H (B,), q (K,), Hq, pred (B,) and `stats`, the TT_STATS values
    one launch adds to a zeroed accumulator."""
    z = np.asarray(z, dtype=np.float64)
    B, K = z.shape
    m = z.max(axis=1, keepdims=True)
    lp = z - m - np.log(np.exp(z - m).sum(axis=1, keepdims=True))
    p = np.exp(lp)
    H = -(p * lp).sum(axis=1)
    q = p.sum(axis=0) / B
    lq = np.where(q == 0.0, 0.0, np.log(np.where(q == 0.0, 1.0, q)))
    Hq = -(q * lq).sum()
    L = H.sum() / B - div * Hq
    c = (p * lq[None, :]).sum(axis=1)
    d = (-p * (lp + H[:, None]) + div * p * (lq[None, :] - c[:, None])) / B
    pred = z.argmax(axis=1)                              # numpy's argmax is the first maximum, as the kernel's
    stats = np.zeros(TT_STATS, dtype=np.float64)
    stats[S_ENT], stats[S_ROWS], stats[S_HQ], stats[S_STEPS] = H.sum(), B, Hq, 1.0
    stats[S_P:S_P + K] = p.sum(axis=0)
    stats[S_PRED:S_PRED + K] = np.bincount(pred, minlength=K)
    return {"L": float(L), "dlogits": d, "H": H, "q": q, "Hq": float(Hq), "pred": pred, "stats": stats}


def loss_torch(z, div: float):
    """L of a (B, K) float64 torch tensor, differentiable: what autograd differentiates in the CPU tier and what the fp64 oracle is
    given as loss_fn in the GPU tier.  Written with torch's own log_softmax, not with the formulas above."""
    import torch
    lp = torch.log_softmax(z, dim=1)
    p = lp.exp()
    H = -(p * lp).sum(dim=1)
    q = p.mean(dim=0)
    Hq = -(q * torch.where(q > 0, q, torch.ones_like(q)).log()).sum()
    return H.mean() - div * Hq


def ulp32(x):
    """The spacing of float32 at |x| (of the smallest normal below it)."""
    a = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), float(np.finfo(np.float32).tiny))
    return np.spacing(a.astype(np.float32)).astype(np.float64)


def mean_objective(stats, div: float) -> float:
    """The mean objective of a pass from its accumulated statistics (msig_tt.h)."""
    return float(stats[S_ENT] / stats[S_ROWS] - div * stats[S_HQ] / stats[S_STEPS])
