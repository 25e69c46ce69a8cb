"""numpy restatement of the head epoch (include/msig_ft.h msig_ft_head_epoch) that the GPU tests compare against.

    hid = dropout(relu(feat[idx] @ W0^T + b0));  logits = hid @ W3^T + b3
    loss = CrossEntropy(logits, y[idx], weight = cw or none), mean reduction as torch
    Adam (L2-in-gradient weight decay, bias correction by the step count) on W0, b0, W3, b3

in the dtype it is given (float64: the reference; float32: what plain fp32 arithmetic costs on the same case, `own`).
tests/test_calibration_host.py pins it to torch (Linear / ReLU / Linear + CrossEntropyLoss(weight) + Adam(weight_decay)).
Dropout is the project's: keep mask oracle.cnn_gru_oracle.dropout_keep(dropout_key(seed, step, 2), rows * 64, thr), element index
= row inside the mini-batch * 64 + hidden unit, kept elements scaled by dropout_scale(thr).

`wrong`: negative controls — "no_bias_correction" drops Adam's bias correction, "no_dropout_scale" the 1 / (1 - p) of dropout.
"""
import numpy as np

from oracle import cnn_gru_oracle as O

HEAD_KEYS = ("classifier.0.weight", "classifier.0.bias", "classifier.3.weight", "classifier.3.bias")


def init_state(head, dtype):
    p = {k: np.array(head[k], dtype=dtype) for k in HEAD_KEYS}
    return {"p": p, "m": {k: np.zeros_like(v) for k, v in p.items()}, "v": {k: np.zeros_like(v) for k, v in p.items()}}


def step(state, feat, y, idx, t, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, cw=None, thr=0, seed=0, dtype=np.float64,
         wrong=None):
    """One mini-batch step with optimiser step count t (1-based) on the rows `idx`; updates `state` in place.
    Returns (summed loss of the step = mean * rows, correct rows, the four gradients before weight decay)."""
    p = state["p"]
    f = np.asarray(feat, dtype=dtype)[idx]
    yy = np.asarray(y, dtype=np.int64)[idx]
    nb, K = len(idx), p["classifier.3.bias"].shape[0]
    pre = f @ p["classifier.0.weight"].T + p["classifier.0.bias"]
    act = np.maximum(pre, 0)
    mask = np.ones((nb, 64), dtype=dtype)
    if thr > 0:
        keep = O.dropout_keep(O.dropout_key(seed, t, O.STREAM_HEAD), nb * 64, thr).reshape(nb, 64)
        scale = 1.0 if wrong == "no_dropout_scale" else O.dropout_scale(thr)
        mask = np.where(keep, dtype(scale), dtype(0))
    hid = act * mask
    logits = hid @ p["classifier.3.weight"].T + p["classifier.3.bias"]
    mx = logits.max(axis=1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(logits - mx).sum(axis=1))
    prob = np.exp(logits - lse[:, None])
    w = np.ones(nb, dtype=dtype) if cw is None else np.asarray(cw, dtype=dtype)[yy]
    W = w.sum()
    nll = lse - logits[np.arange(nb), yy]
    loss = (w * nll).sum() / W
    onehot = np.zeros((nb, K), dtype=dtype)
    onehot[np.arange(nb), yy] = 1
    dlog = (w[:, None] * (prob - onehot)) / W
    g = {"classifier.3.weight": dlog.T @ hid, "classifier.3.bias": dlog.sum(axis=0)}
    dpre = (dlog @ p["classifier.3.weight"]) * mask * (pre > 0)
    g["classifier.0.weight"] = dpre.T @ f
    g["classifier.0.bias"] = dpre.sum(axis=0)
    b1, b2 = dtype(betas[0]), dtype(betas[1])
    bc1 = 1.0 - float(betas[0]) ** t
    bc2 = 1.0 - float(betas[1]) ** t
    if wrong == "no_bias_correction":
        bc1 = bc2 = 1.0
    for k in HEAD_KEYS:
        gr = (g[k] + dtype(weight_decay) * p[k]).astype(dtype)
        state["m"][k] = (b1 * state["m"][k] + (dtype(1) - b1) * gr).astype(dtype)
        state["v"][k] = (b2 * state["v"][k] + (dtype(1) - b2) * gr * gr).astype(dtype)
        denom = (np.sqrt(state["v"][k]) / dtype(np.sqrt(bc2)) + dtype(eps)).astype(dtype)
        p[k] = (p[k] - dtype(lr / bc1) * (state["m"][k] / denom)).astype(dtype)
    correct = int((logits.argmax(axis=1) == yy).sum())
    return float(loss) * nb, correct, g


def epochs(head, feat, y, orders, batch, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, cw=None, thr=0, seed=0,
           dtype=np.float64, wrong=None, step0=1):
    """Runs every row of `orders` ((epochs, n) row indices) as one epoch of mini-batches of `batch` rows (short last step kept).
    Returns (state, [summed loss per epoch])."""
    state, t, losses = init_state(head, dtype), int(step0), []
    for order in np.asarray(orders):
        tot = 0.0
        for i in range(0, len(order), batch):
            ls, _, _ = step(state, feat, y, order[i:i + batch], t, lr, betas, eps, weight_decay, cw, thr, seed, dtype, wrong)
            tot += ls
            t += 1
        losses.append(tot)
    return state, losses


def implied_gradient(exp_avg, p_before, beta1=0.9, weight_decay=0.0):
    """The gradient that ONE step from zero moments implies: its update leaves exp_avg = (1 - beta1) * (g + wd * p)."""
    return np.asarray(exp_avg, np.float64) / (1.0 - beta1) - weight_decay * np.asarray(p_before, np.float64)
