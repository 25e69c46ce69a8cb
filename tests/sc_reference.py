"""The supervised contrastive term of include/msig_sc.h restated in torch, runnable in fp32 and fp64: the closed form the kernels
compute (`restatement`), the loss written directly from its definition for autograd (`loss_direct`), and the case generator the
host and GPU tests share."""
import numpy as np
import torch


def sets(labels, groups, K, positives):
    """valid (B,), A (B, B), P (B, B) as boolean tensors: the definitions of msig_sc.h."""
    y = torch.as_tensor(labels, dtype=torch.int64)
    B = y.numel()
    valid = (y >= 0) & (y < K)
    if positives == "cross-subject":
        g = torch.as_tensor(groups, dtype=torch.int64)
        valid = valid & (g >= 0)
    else:
        g = torch.zeros(B, dtype=torch.int64)
    both = valid[:, None] & valid[None, :] & ~torch.eye(B, dtype=torch.bool)
    samey = y[:, None] == y[None, :]
    if positives == "cross-subject":
        sameg = g[:, None] == g[None, :]
        A = both & ~(samey & sameg)
        P = both & samey & ~sameg
    else:
        A = both
        P = both & samey
    return valid, A, P


def restatement(feat, labels, groups, K, tau, positives="class", dtype=torch.float64):
    """L, df (B, 128), stats [sum of the anchors' L_i, N_a, top-1 count], N_a and the smallest top-1 margin — the arithmetic of
    msig_sc.h spelled out, in `dtype`.  With no anchor: L = None and df = 0."""
    f = torch.as_tensor(feat).to(dtype)
    B = f.shape[0]
    _, A, P = sets(labels, groups, K, positives)
    nrm = torch.clamp_min(torch.linalg.vector_norm(f, dim=1), 1e-12)
    z = f / nrm[:, None]
    s = (z @ z.T) / tau
    neg_inf = torch.full_like(s, -float("inf"))
    sa = torch.where(A, s, neg_inf)
    has_a = A.any(dim=1)
    mx = torch.where(has_a, sa.max(dim=1).values, torch.zeros(B, dtype=dtype))
    e = torch.where(A, torch.exp(s - mx[:, None]), torch.zeros_like(s))
    se = e.sum(dim=1)
    lse = mx + torch.log(torch.where(has_a, se, torch.ones_like(se)))
    npos = P.sum(dim=1)
    anchor = npos > 0
    n_a = int(anchor.sum())
    if n_a == 0:
        return None, torch.zeros_like(f), [0.0, 0, 0], 0, float("inf")
    npf = torch.clamp_min(npos, 1).to(dtype)
    Li = lse - torch.where(P, s, torch.zeros_like(s)).sum(dim=1) / npf
    total = float(Li[anchor].to(torch.float64).sum())
    prob = torch.where(A, torch.exp(s - lse[:, None]), torch.zeros_like(s))
    Cm = torch.where(anchor[:, None], prob - P.to(dtype) / npf[:, None], torch.zeros_like(s)) / n_a
    dz = ((Cm + Cm.T) @ z) / tau
    df = (dz - z * (z * dz).sum(dim=1, keepdim=True)) / nrm[:, None]
    # top-1: the first maximum over A(i) is a positive; margin: how far the best of the other kind is
    arg = sa.argmax(dim=1)
    top = anchor & P[torch.arange(B), arg]
    best_p = torch.where(P, s, neg_inf).max(dim=1).values
    best_n = torch.where(A & ~P, s, neg_inf).max(dim=1).values
    margin = float((best_p - best_n).abs()[anchor].min())
    return total / n_a, df, [total, n_a, int(top.sum())], n_a, margin


def loss_direct(feat, labels, groups, K, tau, positives="class"):
    """The loss from its definition, for autograd: mean over anchors of -(1/|P(i)|) sum_p log( exp(s_ip) / sum_{a in A(i)} exp(s_ia) )."""
    f = feat
    _, A, P = sets(labels, groups, K, positives)
    z = f / torch.clamp_min(torch.linalg.vector_norm(f, dim=1, keepdim=True), 1e-12)
    s = (z @ z.T) / tau
    terms = []
    for i in range(f.shape[0]):
        if not bool(P[i].any()):
            continue
        log_den = torch.logsumexp(s[i][A[i]], dim=0)
        terms.append(-(s[i][P[i]] - log_den).mean())
    if not terms:
        return None
    return torch.stack(terms).mean()


def make_case(B, K, seed, n_groups=5, invalid=0.1, positions=None):
    """Features with class structure (so that the similarities spread), labels with ~`invalid` of them outside [0, K), a subject table
    over `positions` store positions with a few -1 entries, and the int64 store positions of the rows."""
    rs = np.random.RandomState(seed)
    positions = positions or max(2 * B, 8)
    y = rs.randint(0, K, size=B).astype(np.int64)
    centres = rs.randn(K, 128).astype(np.float32)
    f = (0.25 * centres[y] + rs.randn(B, 128)).astype(np.float32) * np.float32(rs.uniform(0.5, 3.0))
    bad = rs.rand(B) < invalid
    y[bad] = rs.choice(np.array([-1, K, K + 3], dtype=np.int64), size=int(bad.sum()))
    table = rs.randint(0, n_groups, size=positions).astype(np.int32)
    table[rs.rand(positions) < invalid / 2] = -1
    idx = rs.permutation(positions)[:B].astype(np.int64)
    return f, y, table, idx
