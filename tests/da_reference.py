"""numpy restatement of the subject discriminator's step (include/msig_da.h), in float64 or float32: the two-label mixup form of the
domain CrossEntropy, rows without a label (-1), n == 0, Adam with L2-in-gradient weight decay, the reversed feature gradient and the
statistics.  tests/test_adversary_host.py pins it to torch's autograd through a gradient-reversal Function and torch.optim.Adam."""
import numpy as np

KEYS = ("W0", "b0", "W3", "b3")


def layout(S):
    """Offsets (floats) of W0, b0, W3, b3 in the flat buffer; last entry = msig_da_param_floats(S)."""
    o, out = 0, []
    for n in (64 * 128, 64, S * 64, S):
        out.append(o)
        o += (n + 3) // 4 * 4
    return out + [o]


def split(flat, S, dtype=np.float64):
    lay = layout(S)
    flat = np.asarray(flat)
    return {"W0": flat[lay[0]:lay[0] + 8192].reshape(64, 128).astype(dtype), "b0": flat[lay[1]:lay[1] + 64].astype(dtype),
            "W3": flat[lay[2]:lay[2] + S * 64].reshape(S, 64).astype(dtype), "b3": flat[lay[3]:lay[3] + S].astype(dtype)}


def join(tensors, S, dtype=np.float32):
    lay = layout(S)
    flat = np.zeros(lay[-1], dtype=dtype)
    for o, k in zip(lay, KEYS):
        flat[o:o + tensors[k].size] = tensors[k].reshape(-1)
    return flat


def labels(dom, idx, S):
    """d_b = dom[idx[b]] (idx given) or dom[b]; a value outside [-1, S) reads as -1."""
    d = np.asarray(dom)[np.asarray(idx)] if idx is not None else np.asarray(dom)
    d = d.astype(np.int64).copy()
    d[(d < 0) | (d >= S)] = -1
    return d


def step(params, exp_avg, exp_avg_sq, feat, dfeat, d, lam=1.0, lam_rev=0.0, lr=1e-3, t=1, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
         dtype=np.float64):
    """One step.  params / exp_avg / exp_avg_sq: dicts of W0 (64,128), b0, W3 (S,64), b3; feat, dfeat (B,128); d (B,) labels in [-1, S).
    Returns dict(n, loss, grads, g, dfeat, params, exp_avg, exp_avg_sq, stats); with n == 0 everything comes back unchanged and
    stats is zero.  dtype float32: every array and scalar of the arithmetic in fp32 (the sums of n and the loss in fp64, as the kernel)."""
    ft = dtype
    P = {k: np.asarray(params[k], dtype=ft) for k in KEYS}
    M = {k: np.asarray(exp_avg[k], dtype=ft) for k in KEYS}
    V = {k: np.asarray(exp_avg_sq[k], dtype=ft) for k in KEYS}
    f, df = np.asarray(feat, dtype=ft), np.asarray(dfeat, dtype=ft)
    d = np.asarray(d, dtype=np.int64)
    B, S = f.shape[0], P["W3"].shape[0]
    d2 = d[::-1]
    lam_ = ft(lam)
    mu = ft(1.0) - lam_
    a1 = np.where(d >= 0, lam_, ft(0.0)).astype(ft)
    a2 = np.where(d2 >= 0, mu, ft(0.0)).astype(ft)
    n = float(np.sum(a1.astype(np.float64) + a2.astype(np.float64)))
    stats = np.zeros(3)
    if n == 0.0:
        return dict(n=0.0, loss=0.0, grads={k: np.zeros_like(P[k]) for k in KEYS}, g=np.zeros_like(f), dfeat=df.copy(), params=P, exp_avg=M,
                    exp_avg_sq=V, stats=stats)
    pre = f @ P["W0"].T + P["b0"]
    h = np.maximum(pre, ft(0.0))
    z = h @ P["W3"].T + P["b3"]
    mx = z.max(axis=1, keepdims=True)
    lse = (mx + np.log(np.exp(z - mx).sum(axis=1, keepdims=True))).astype(ft)
    p = np.exp(z - lse).astype(ft)
    rows = np.arange(B)
    l1 = (lse[:, 0] - z[rows, np.maximum(d, 0)]).astype(np.float64)
    l2 = (lse[:, 0] - z[rows, np.maximum(d2, 0)]).astype(np.float64)
    loss_sum = float(np.sum(np.where(d >= 0, a1.astype(np.float64) * l1, 0.0) + np.where(d2 >= 0, a2.astype(np.float64) * l2, 0.0)))
    e1 = np.zeros((B, S), dtype=ft)
    e1[rows[d >= 0], d[d >= 0]] = 1
    e2 = np.zeros((B, S), dtype=ft)
    e2[rows[d2 >= 0], d2[d2 >= 0]] = 1
    inv = ft(1.0) / ft(n)
    dz = ((a1[:, None] * (p - e1) + a2[:, None] * (p - e2)) * inv).astype(ft)
    dpre = np.where(h > 0, dz @ P["W3"], ft(0.0)).astype(ft)
    grads = {"W3": dz.T @ h, "b3": dz.sum(axis=0), "W0": dpre.T @ f, "b0": dpre.sum(axis=0)}
    g = (dpre @ P["W0"]).astype(ft)
    new_df = df.copy() if lam_rev == 0 else (df + (ft(-lam_rev) * g).astype(ft)).astype(ft)
    b1, b2 = ft(betas[0]), ft(betas[1])
    bc1, bc2 = 1.0 - float(b1) ** t, 1.0 - float(b2) ** t
    lr_over_bc1, inv_sqrt_bc2 = ft(lr / bc1), ft(1.0 / np.sqrt(bc2))
    NP, NM, NV = {}, {}, {}
    for k in KEYS:
        gr = (grads[k] + ft(weight_decay) * P[k]).astype(ft)
        NM[k] = (b1 * M[k] + (ft(1.0) - b1) * gr).astype(ft)
        NV[k] = (b2 * V[k] + (ft(1.0) - b2) * gr * gr).astype(ft)
        NP[k] = (P[k] - lr_over_bc1 * (NM[k] / (np.sqrt(NV[k]) * inv_sqrt_bc2 + ft(eps)))).astype(ft)
    stats[:] = [loss_sum, float(np.sum((d >= 0) & (z.argmax(axis=1) == d))), float(np.sum(d >= 0))]
    return dict(n=n, loss=loss_sum / n, grads=grads, g=g, dfeat=new_df, params=NP, exp_avg=NM, exp_avg_sq=NV, stats=stats)


def zeros_like(params):
    return {k: np.zeros_like(np.asarray(params[k], dtype=np.float64)) for k in KEYS}
