"""Times classifier-only training steps (few-shot subject calibration) three ways, in one process on one GPU:

  (1) msig_ft_head_epoch / msig_ft_head_epoch_multi: an epoch of S = 3 and S = 16 steps of batch 16 on cached features in ONE launch,
      for one fold and for fifteen folds;
  (2) the same steps without the new call — the only correct route before it existed: an eval-mode model(x) kept for a backward,
      loss.backward() (full BPTT through a GRU whose gradients are thrown away), torch.optim.Adam over the classifier's parameters —
      on the same windows;
  (3) the fused full-model msig_train_step at the same batch, for scale (it trains every tensor: not a substitute).

Every shape is warmed up; a timed window is `--window-ms` of back-to-back calls between device events; the variants are visited in
turn, `--repeats` times, and the log gives median, minimum and maximum per step for each.

    python tools/calibration_timing.py [--out profiles/calibration_timing.log]
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from multimodalsignal_amd import _lib as L  # noqa: E402
from multimodalsignal_amd.calibrate import epoch_orders  # noqa: E402
from multimodalsignal_amd.models import CnnGruAttentionModel  # noqa: E402


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "calibration_timing.log")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=150.0)
    ap.add_argument("--folds", type=int, default=15)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("calibration_timing.py needs the GPU: a CPU run says nothing about these times")
    dev = torch.device("cuda:0")
    Cc, K, T, B, NF = 6, 2, 3840, 16, a.folds
    torch.manual_seed(0)
    model = CnnGruAttentionModel(Cc, K).to(dev)
    eng = model.engine()
    lib, st = L.lib(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    variants = {}

    for S in (3, 16):
        N = S * B
        g = torch.Generator().manual_seed(S)
        x = torch.randn(N, Cc, T, generator=g).to(dev)
        y = torch.randint(0, K, (N,), generator=g).to(dev)
        feat = model.embed(x)
        order = torch.as_tensor(epoch_orders(N, 1, seed=1)[0]).to(dev)
        sizes = [("params", eng.n_flat * 4), ("ea", eng.n_flat * 4), ("eas", eng.n_flat * 4), ("feat", N * 512), ("labels", N * 8), ("order", N * 4),
                 ("acc", 16)]
        off, at = {}, 0
        for name, nb in sizes:
            off[name] = at
            at += (nb + 255) // 256 * 256
        mem = torch.zeros((NF, at), dtype=torch.uint8, device=dev)
        for f in range(NF):
            mem[f, off["params"]:off["params"] + eng.n_flat * 4].view(torch.float32).copy_(eng.params)
            mem[f, off["feat"]:off["feat"] + N * 512].view(torch.float32).copy_(feat.reshape(-1))
            mem[f, off["labels"]:off["labels"] + N * 8].view(torch.int64).copy_(y)
            mem[f, off["order"]:off["order"] + N * 4].view(torch.int32).copy_(order)
        h = L.FtHead()
        h.K, h.N, h.n_order, h.batch, h.first_step, h.n_steps, h.dropout_thr = K, N, N, B, 0, S, 128
        h.cls_offset, h.step0, h.seed = eng.layout[L.P_CLS0_W], 1, 3
        h.lr, h.beta1, h.beta2, h.eps, h.weight_decay = 1e-3, 0.9, 0.999, 1e-8, 1e-4
        base = mem.data_ptr()
        h.feat, h.labels, h.order = base + off["feat"], base + off["labels"], base + off["order"]
        h.params, h.exp_avg, h.exp_avg_sq, h.loss_acc = base + off["params"], base + off["ea"], base + off["eas"], base + off["acc"]
        m = L.FtMulti()
        m.n, m.stride_bytes = NF, at
        for f in range(NF):
            m.slot[f], m.lr[f], m.step0[f], m.seed[f] = f, 1e-3, 1, f
        keep = (mem, x, y, feat, order)

        def one(h=h, keep=keep):
            L.check(lib.msig_ft_head_epoch(C.byref(h), st), "msig_ft_head_epoch")

        def many(h=h, m=m, keep=keep):
            L.check(lib.msig_ft_head_epoch_multi(C.byref(h), C.byref(m), st), "msig_ft_head_epoch_multi")

        variants[f"(1) head_epoch S={S} 1 fold"] = (one, S)
        variants[f"(1) head_epoch S={S} {NF} folds"] = (many, S)

        # (2) the un-fused route on the same windows
        for p in model.parameters():
            p.requires_grad_(False)
        cls = list(model.classifier.parameters())
        for p in cls:
            p.requires_grad_(True)
        opt = torch.optim.Adam(cls, lr=1e-3, weight_decay=1e-4)
        crit = torch.nn.CrossEntropyLoss()
        model.eval()

        def unfused(x=x, y=y, order=order, S=S, opt=opt):
            for s in range(S):
                idx = order[s * B:(s + 1) * B].long()
                opt.zero_grad()
                loss = crit(model(x[idx]), y[idx])
                loss.backward()
                opt.step()

        variants[f"(2) eval forward + backward + torch Adam on the classifier S={S}"] = (unfused, S)

    g = torch.Generator().manual_seed(9)
    xb = torch.randn(B, Cc, T, generator=g).to(dev)
    yb = torch.randint(0, K, (B,), generator=g).to(dev)
    eng2 = CnnGruAttentionModel(Cc, K).to(dev).engine()
    cnt = [0]

    def fused():
        cnt[0] += 1
        eng2.train_step(xb, yb, 1e-3, weight_decay=1e-4, step=cnt[0], dropout_p=0.5, seed=1)

    variants[f"(3) msig_train_step (every tensor) B={B}"] = (fused, 1)

    calls = {}
    for name, (fn, S) in variants.items():            # warm up every shape, then size the windows
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t = window(fn, 5)
        calls[name] = max(5, int(a.window_ms / max(t, 1e-3)))
    res = {name: [] for name in variants}
    for _ in range(a.repeats):                         # the variants in turn, so that drift hits all of them alike
        for name, (fn, S) in variants.items():
            res[name].append(window(fn, calls[name]) / S)
    lines = [f"calibration timing: C={Cc} T={T} K={K} batch={B}, dropout 0.5, {a.repeats} windows of ~{a.window_ms:.0f} ms per variant, visited in turn",
             f"device: {torch.cuda.get_device_name(0)}   date: {time.strftime('%Y-%m-%d')}",
             f"{'variant':<78} {'us/step median':>15} {'min':>9} {'max':>9} {'calls/window':>13}"]
    out = {}
    for name, v in res.items():
        v = np.array(v) * 1e3
        lines.append(f"{name:<78} {np.median(v):>15.2f} {v.min():>9.2f} {v.max():>9.2f} {calls[name]:>13d}")
        out[name] = {"us_per_step_median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}
    text = "\n".join(lines) + "\n"
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(text)
    print(text)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
