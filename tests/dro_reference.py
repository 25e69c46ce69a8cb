"""include/msig_dro.h restated in numpy: fp64 throughout, python-float loops in the header's order (rows in increasing b, groups in
increasing g, classes in increasing c).  The only fp32 roundings are the header's: q is rounded to fp32 when it is stored, and the
factor r reads that stored q.  r and the returned dlogits are NOT rounded (the device rounds r to fp32 and the product once more:
the GPU tests allow those roundings, nothing else)."""
import math

import numpy as np

MAX_GROUPS = 64
STATS = 3 * MAX_GROUPS + 2


def row_terms(z, y, w=None, eps=0.0):
    """(t_b, m_b) of every row: lists of python floats."""
    z = np.asarray(z, dtype=np.float32)
    B, K = z.shape
    e = float(np.float32(eps))
    keep, spread = 1.0 - e, e / K
    t, m = [], []
    for b in range(B):
        yb = int(y[b])
        if yb < 0 or yb >= K:
            t.append(0.0); m.append(0.0)
            continue
        mx = float(max(z[b]))
        d = [float(z[b, c]) - mx for c in range(K)]
        S = 0.0
        for c in range(K):
            S = S + math.exp(d[c])
        lnS = math.log(S)
        allc, own = 0.0, 0.0
        for c in range(K):
            wl = (float(w[c]) if w is not None else 1.0) * -(d[c] - lnS)
            allc = allc + wl
            if c == yb:
                own = wl
        t.append(keep * own + spread * allc)
        m.append(float(w[yb]) if w is not None else 1.0)
    return t, m


def criterion_dlogits(z, y, w=None, eps=0.0):
    """include/msig_st.h's dL/dz with lam = 1 in fp64: what the criterion leaves in MSIG_WS_DLOGITS (there rounded to fp32)."""
    z = np.asarray(z, dtype=np.float64)
    B, K = z.shape
    wv = np.ones(K) if w is None else np.asarray(w, dtype=np.float64)
    e = float(np.float32(eps))
    p = np.exp(z - z.max(axis=1, keepdims=True))
    p = p / p.sum(axis=1, keepdims=True)
    W = float(sum(float(wv[int(v)]) for v in y))
    out = np.zeros((B, K))
    for b in range(B):
        yb = int(y[b])
        for c in range(K):
            out[b, c] = ((1.0 - e) * wv[yb] * (p[b, c] - (1.0 if c == yb else 0.0)) + (e / K) * (p[b, c] * wv.sum() - wv[c])) / W
    return out


def row_groups(grp, B, G, idx=None, y=None, K=None):
    """g_b of every row, -1 for a row in no group (a group outside [0, G), or a label outside [0, K))."""
    out = []
    for b in range(B):
        g = int(grp[int(idx[b])] if idx is not None else grp[b])
        if g < 0 or g >= G or (y is not None and not 0 <= int(y[b]) < K):
            g = -1
        out.append(g)
    return out


def apply(z, y, grp, q, eta, G, w=None, eps=0.0, dlogits=None, idx=None, frozen=False, stats=None):
    """One msig_dro_apply.  q: the G stored weights.  Returns a dict: q (G, fp32 values in float64: what is stored afterwards), r (B,
    fp64, unrounded), dlogits ((B, K) fp64 product r_b * dlogits, or None), stats (float64[STATS] after the call, or None), T, W_g,
    n, Wall, present, wrote (False: no group is present and nothing at all is written)."""
    z = np.asarray(z, dtype=np.float32)
    B, K = z.shape
    t, m = row_terms(z, y, w, eps)
    gb = row_groups(grp, B, G, idx, y, K)
    Wall = 0.0
    for b in range(B):
        Wall = Wall + m[b]
    T, Wg, n = [0.0] * G, [0.0] * G, [0] * G
    for b in range(B):
        if gb[b] >= 0:
            T[gb[b]] = T[gb[b]] + t[b]; Wg[gb[b]] = Wg[gb[b]] + m[b]; n[gb[b]] += 1
    present = [n[g] > 0 and Wg[g] > 0.0 for g in range(G)]
    q_in = [float(np.float32(v)) for v in np.asarray(q).reshape(-1)[:G]]
    st = None if stats is None else np.array(stats, dtype=np.float64)
    dl = None if dlogits is None else np.asarray(dlogits, dtype=np.float64)
    if not any(present):
        return dict(q=np.array(q_in), r=np.zeros(B), dlogits=dl, stats=st, T=T, W_g=Wg, n=n, Wall=Wall, present=present, wrote=False,
                    groups=gb)
    if frozen:
        q_out = list(q_in)
    else:
        qn, Z = [], 0.0
        for g in range(G):
            v = q_in[g] * math.exp(float(np.float32(eta)) * (T[g] / Wg[g])) if present[g] else q_in[g]
            qn.append(v); Z = Z + v
        q_out = [float(np.float32(qn[g] / Z)) for g in range(G)]
    fac = [q_out[g] * Wall / Wg[g] if present[g] else 0.0 for g in range(G)]
    r = np.array([fac[g] if g >= 0 else 0.0 for g in gb])
    robust = 0.0
    for g in range(G):
        if present[g]:
            robust = robust + q_out[g] * (T[g] / Wg[g])
    if st is not None and not frozen:
        for g in range(G):
            if n[g] > 0:
                st[g] += T[g]; st[MAX_GROUPS + g] += Wg[g]; st[2 * MAX_GROUPS + g] += n[g]
        st[3 * MAX_GROUPS] += robust; st[3 * MAX_GROUPS + 1] += 1.0
    return dict(q=np.array(q_out), r=r, dlogits=None if dl is None else r[:, None] * dl, stats=st, T=T, W_g=Wg, n=n, Wall=Wall,
                present=present, wrote=True, robust=robust, groups=gb)
