"""Test-only restatement of the ensemble reduction (include/msig_en.h) in fp64 python floats, every sum in the header's order.  Its
arithmetic is its own (nothing of mc_reference.reduce is called); the comparison rule is the project's, mc_reference.within_store_rounding.
Nothing here is imported by the product."""
import math

import numpy as np

from mc_reference import ulp32, within_store_rounding  # noqa: F401  (the comparison rule, re-exported)

FLOAT_OUTS = ("mean_p", "std_p", "entropy", "expected_entropy", "mutual_info", "disagreement")
INT_OUTS = ("pred", "votes", "member_pred")
OUTS = ("mean_p", "std_p", "pred", "entropy", "expected_entropy", "mutual_info", "votes", "member_pred", "disagreement")
COMMON = OUTS[:7]          # what msig_mc_reduce also has


def _softmax(row):
    """(p, H(p), first argmax) of one row of logits."""
    best, arg = row[0], 0
    for k in range(1, len(row)):
        if row[k] > best:
            best, arg = row[k], k
    ex = [math.exp(v - best) for v in row]
    z = 0.0
    for v in ex:
        z += v
    p = [v / z for v in ex]
    h = 0.0
    for v in p:
        h -= v * math.log(v) if v > 0.0 else 0.0
    return p, h, arg


def disagreement_from_votes(votes, M):
    """1 - sum_k v_k (v_k - 1) / (M (M - 1)): the share of unordered member pairs that differ; 0 for M = 1."""
    if M < 2:
        return 0.0
    same = 0
    for v in votes:
        same += int(v) * (int(v) - 1)
    return 1.0 - same / (M * (M - 1))


def reduce(logits):
    """logits: (M, N, K), member-major.  Returns float64 / int64 arrays under the names of OUTS."""
    lg = np.asarray(logits, dtype=np.float64)
    M, N, K = lg.shape
    out = dict(mean_p=np.zeros((N, K)), std_p=np.zeros((N, K)), pred=np.zeros(N, dtype=np.int64), entropy=np.zeros(N),
               expected_entropy=np.zeros(N), mutual_info=np.zeros(N), votes=np.zeros((N, K), dtype=np.int64),
               member_pred=np.zeros((N, M), dtype=np.int64), disagreement=np.zeros(N))
    for n in range(N):
        rows = [_softmax([float(v) for v in lg[m, n]]) for m in range(M)]
        for m, (_, _, arg) in enumerate(rows):
            out["member_pred"][n, m] = arg
            out["votes"][n, arg] += 1
        mu = []
        for k in range(K):
            tot = 0.0
            for m in range(M):
                tot += rows[m][0][k]
            mean = tot / M
            dev = 0.0
            for m in range(M):
                d = rows[m][0][k] - mean
                dev += d * d
            mu.append(mean)
            out["mean_p"][n, k], out["std_p"][n, k] = mean, math.sqrt(dev / M)
        arg, h = 0, 0.0
        for k in range(K):
            if mu[k] > mu[arg]:
                arg = k
            h -= mu[k] * math.log(mu[k]) if mu[k] > 0.0 else 0.0
        eh = 0.0
        for m in range(M):
            eh += rows[m][1]
        eh /= M
        out["pred"][n], out["entropy"][n], out["expected_entropy"][n], out["mutual_info"][n] = arg, h, eh, h - eh
        out["disagreement"][n] = disagreement_from_votes(out["votes"][n], M)
    return out


def crafted_logits(M, N, K, seed):
    """(M, N, K) fp32 with tests/test_mc_dropout_gpu.py's crafted windows: window 0 has one saturated member (a logit gap of 60),
    window 1 an exact two-way tie for the maximum in every member, window 2 all members equal; the others generic."""
    rs = np.random.RandomState(seed)
    lg = (3.0 * rs.randn(N, M, K)).astype(np.float32)
    lg[0, 0, :] = 0.0
    lg[0, 0, K - 1] = 60.0
    lg[1, :, 0] = lg[1].max(axis=1) + 1.0
    lg[1, :, 1] = lg[1, :, 0]
    lg[2, :, :] = lg[2, 0, :]
    return np.ascontiguousarray(lg.transpose(1, 0, 2))
