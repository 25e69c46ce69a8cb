"""Test-only restatement of Monte-Carlo dropout (include/msig_mc.h, multimodalsignal_amd/uncertainty.py) in numpy and the oracle's
pieces: the replication, the reduction in fp64 with explicit in-order loops, the stochastic tail from a given trunk output, and the
host metrics.  Nothing here is imported by the product."""
import math

import numpy as np
import torch

from oracle import cnn_gru_oracle as O


def expand(src, S):
    """(N, R) -> (N * S, R): row n * S + s is row n."""
    src = np.asarray(src)
    out = np.empty((src.shape[0] * S,) + src.shape[1:], dtype=src.dtype)
    for n in range(src.shape[0]):
        for s in range(S):
            out[n * S + s] = src[n]
    return out


def _plogp(p):
    return p * math.log(p) if p > 0.0 else 0.0


def reduce(logits, N, S, K):
    """msig_mc_reduce in fp64 (python floats), every sum in the header's order.  Returns a dict of float64 / int64 arrays: mean_p,
    std_p (N, K), pred, entropy, expected_entropy, mutual_info (N), votes (N, K)."""
    lg = np.asarray(logits, dtype=np.float64).reshape(N, S, K)
    out = dict(mean_p=np.zeros((N, K)), std_p=np.zeros((N, K)), pred=np.zeros(N, dtype=np.int64), entropy=np.zeros(N),
               expected_entropy=np.zeros(N), mutual_info=np.zeros(N), votes=np.zeros((N, K), dtype=np.int64))
    for n in range(N):
        ps, hs = [], []
        for s in range(S):
            row = [float(v) for v in lg[n, s]]
            mx, am = row[0], 0
            for k in range(1, K):
                if row[k] > mx:
                    mx, am = row[k], k
            e = [math.exp(v - mx) for v in row]
            tot = 0.0
            for k in range(K):
                tot += e[k]
            p = [e[k] / tot for k in range(K)]
            h = 0.0
            for k in range(K):
                h -= _plogp(p[k])
            ps.append(p)
            hs.append(h)
            out["votes"][n, am] += 1
        m = []
        for k in range(K):
            acc = 0.0
            for s in range(S):
                acc += ps[s][k]
            mk = acc / S
            sq = 0.0
            for s in range(S):
                d = ps[s][k] - mk
                sq += d * d
            m.append(mk)
            out["mean_p"][n, k] = mk
            out["std_p"][n, k] = math.sqrt(sq / S)
        am, h = 0, 0.0
        for k in range(K):
            if m[k] > m[am]:
                am = k
            h -= _plogp(m[k])
        eh = 0.0
        for s in range(S):
            eh += hs[s]
        eh /= S
        out["pred"][n], out["entropy"][n], out["expected_entropy"][n], out["mutual_info"][n] = am, h, eh, h - eh
    return out


def ulp32(ref):
    """The spacing of fp32 at |ref| (fp64 in, fp64 out)."""
    return np.spacing(np.abs(np.asarray(ref, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def within_store_rounding(got, ref):
    """|got - ref| <= 2 ulp_fp32(ref) + 1e-12: the device's fp64 exp / log are not correctly rounded, so a stored fp32 value can
    differ from the rounded reference only where the fp64 value sits at a rounding boundary."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return bool(np.all(np.abs(got - ref) <= 2.0 * ulp32(ref) + 1e-12))


def tail(named, src, S, seed, j, thr, dtype):
    """The stochastic tail of chunk j in `dtype`: `src` is the trunk's output for the chunk's windows — H0 (nb, TP, 128) for the
    two-layer model, the padded FEAT (nb, 128) for the one-layer model — every window repeated S times (window i, sample s = row
    i * S + s), the GRU mask on element (row * TP + t) * 128 + u, the head mask on row * 64 + v.  Returns logits (nb * S, K)."""
    p = {k: torch.as_tensor(v).to(dtype) for k, v in named.items() if "running" not in k and "num_batches" not in k}
    x = torch.as_tensor(np.asarray(src)).to(dtype).repeat_interleave(S, dim=0)
    rows = x.shape[0]
    scale = O.dropout_scale(thr)

    def W(layer, sfx):
        return (p[f"gru.weight_ih_l{layer}{sfx}"], p[f"gru.weight_hh_l{layer}{sfx}"],
                p[f"gru.bias_ih_l{layer}{sfx}"], p[f"gru.bias_hh_l{layer}{sfx}"])

    if "gru.weight_ih_l1" in p:
        TP = x.shape[1]
        if thr > 0:
            keep = O.dropout_keep(O.dropout_key(seed, j, O.STREAM_GRU), x.numel(), thr)
            x = x * (torch.from_numpy(keep.reshape(tuple(x.shape))).to(dtype) * scale)
        h1f = O.gru_direction(x, *W(1, ""), reverse=False)
        H = p["gru.weight_hh_l1"].shape[1]
        h1r = O.gru_cell(x[:, TP - 1, :], torch.zeros(rows, H, dtype=dtype), *W(1, "_reverse"))
        feat = torch.cat([h1f[:, -1, :], h1r], dim=1)
    else:
        H = p["gru.weight_hh_l0"].shape[1]
        feat = torch.cat([x[:, :H], x[:, 64:64 + H]], dim=1)          # the real columns of the padded row
    hid = torch.clamp_min(feat @ p["classifier.0.weight"].t() + p["classifier.0.bias"], 0)
    if thr > 0:
        keep = O.dropout_keep(O.dropout_key(seed, j, O.STREAM_HEAD), hid.numel(), thr)
        hid = hid * (torch.from_numpy(keep.reshape(tuple(hid.shape))).to(dtype) * scale)
    return (hid @ p["classifier.3.weight"].t() + p["classifier.3.bias"]).numpy()


# ---- the host metrics, restated the slow way ---------------------------------------------------------------------------------------
def auroc_pairs(score, positive):
    """P(score of a positive > score of a negative) + P(equal) / 2 over all pairs; None without a positive or a negative."""
    pos = [s for s, f in zip(score, positive) if f]
    neg = [s for s, f in zip(score, positive) if not f]
    if not pos or not neg:
        return None
    tot = 0.0
    for a in pos:
        for b in neg:
            tot += 1.0 if a > b else (0.5 if a == b else 0.0)
    return tot / (len(pos) * len(neg))


def selective(correct, uncertainty, coverage):
    """Accuracy on the ceil(coverage % of N) windows kept when the most uncertain are dropped first, among equals the higher index first."""
    idx = sorted(range(len(correct)), key=lambda i: (uncertainty[i], i))
    keep = -(-len(correct) * coverage // 100)
    return sum(1.0 for i in idx[:keep] if correct[i]) / keep


def ece(confidence, correct, bins=15):
    n, tot = len(confidence), 0.0
    for b in range(bins):
        sel = [i for i in range(n) if (b / bins < confidence[i] <= (b + 1) / bins) or (b == 0 and confidence[i] == 0.0)]
        if sel:
            acc = sum(1.0 for i in sel if correct[i]) / len(sel)
            conf = sum(confidence[i] for i in sel) / len(sel)
            tot += abs(acc - conf) * len(sel) / n
    return tot
