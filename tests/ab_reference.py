"""Label-free BatchNorm adaptation (include/msig_ab.h) restated in torch from the oracle's own pieces —
``channel_gate``, ``conv1d_strided``, ``batchnorm``, ``relu_maxpool`` of oracle.cnn_gru_oracle — in float64 (the reference) or
float32 (`own`: what plain fp32 arithmetic costs on the same case).

    stage 1   y1 = conv1(gate(x) * x) for all N windows; m1, v1 = mean and UNBIASED variance over all N * L1 positions;
              rm1' = (1 - alpha) * rm1 + alpha * m1, rv1' likewise
    stage 2   z1 = bn1(y1) in its EVAL form with rm1', rv1';  p1 = pool(relu(z1));  y2 = conv2(p1);  m2, v2 over N * L2 positions,
              blended the same way

The set is cut into batches (`batch`); a batch's statistics are what ``batchnorm(training=True, momentum=1)`` leaves as running
statistics from (0, 0) — its mean and unbiased variance — and batches are merged by the pairwise update of Chan et al. (count, mean,
sum of squared deviations), which is exact arithmetic's whole-set statistic and well conditioned in either precision.

`wrong` builds the two deliberately wrong versions the GPU gate must reject: "biased" (variance / n instead of / (n - 1)) and
"source_bn1" (stage 2 normalised with the SOURCE BatchNorm-1 statistics instead of the adapted ones).
"""
import torch

from oracle import cnn_gru_oracle as O

KEYS = ("cnn_encoder.1.running_mean", "cnn_encoder.1.running_var", "cnn_encoder.5.running_mean", "cnn_encoder.5.running_var")


def _cast(d, dtype):
    return {k: torch.as_tensor(v).to(dtype) for k, v in d.items() if "num_batches" not in k}


def conv1_out(p, x, kind="cnn_gru_attention"):
    if kind == "cnn_gru_attention":
        _, _, s = O.channel_gate(x, p["channel_attention.fc.0.weight"], p["channel_attention.fc.2.weight"])
        x = x * s[:, :, None]
    return O.conv1d_strided(x, p["cnn_encoder.0.weight"], 2, 3)


def conv2_out(p, y1, rm1, rv1):
    z1, _, _ = O.batchnorm(y1, p["cnn_encoder.1.weight"], p["cnn_encoder.1.bias"], rm1, rv1, training=False)
    return O.conv1d_strided(O.relu_maxpool(z1), p["cnn_encoder.4.weight"], 2, 2)


def batch_stats(y):
    """(count, mean, sum of squared deviations) per channel of one batch (B, CH, L), through the oracle's BatchNorm."""
    ch = y.shape[1]
    one, zero = torch.ones(ch, dtype=y.dtype), torch.zeros(ch, dtype=y.dtype)
    _, mean, unbiased = O.batchnorm(y, one, zero, zero, zero, training=True, momentum=1.0)
    n = y.shape[0] * y.shape[2]
    return n, mean, unbiased * (n - 1)


def merge(a, b):
    """Chan et al.: the statistics of the union of two disjoint sets."""
    if a is None:
        return b
    (na, ma, qa), (nb, mb, qb) = a, b
    n = na + nb
    d = mb - ma
    return n, ma + d * (nb / n), qa + qb + d * d * (na * nb / n)


def blend(src, target, alpha):
    return (1 - alpha) * src + alpha * target


def adapt(params, buffers, x, alpha=1.0, batch=None, dtype=torch.float64, kind="cnn_gru_attention", wrong=None):
    """The four adapted running statistics {key: tensor of `dtype`} for the windows `x` (N, C, T) cut into batches of `batch`
    (None: one batch)."""
    p, src = _cast(params, dtype), _cast(buffers, dtype)
    x = torch.as_tensor(x).to(dtype)
    cuts = [x[i:i + (batch or x.shape[0])] for i in range(0, x.shape[0], batch or x.shape[0])]
    fin = lambda n, q: q / n if wrong == "biased" else q / (n - 1)
    y1 = [conv1_out(p, xb, kind) for xb in cuts]
    acc = None
    for y in y1:
        acc = merge(acc, batch_stats(y))
    out = {KEYS[0]: blend(src[KEYS[0]], acc[1], alpha), KEYS[1]: blend(src[KEYS[1]], fin(acc[0], acc[2]), alpha)}
    rm1, rv1 = (src[KEYS[0]], src[KEYS[1]]) if wrong == "source_bn1" else (out[KEYS[0]], out[KEYS[1]])
    acc = None
    for y in y1:
        acc = merge(acc, batch_stats(conv2_out(p, y, rm1, rv1)))
    out[KEYS[2]] = blend(src[KEYS[2]], acc[1], alpha)
    out[KEYS[3]] = blend(src[KEYS[3]], fin(acc[0], acc[2]), alpha)
    return out
