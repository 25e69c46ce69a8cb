"""The cases of tests/golden/head_mlp.npz: inputs regenerated from fixed numpy seeds, and the library calls that turn them into the
recorded outputs — shared by tests/golden/make_head_mlp_golden.py (which records them once, from the library in which the
128 -> 64 -> K classifier was written out five times: head_fwd_kernel + head_bwd_kernel, head_step_kernel, head_epoch_kernel,
da_step_kernel) and tests/test_head_mlp_golden_gpu.py (which compares bits).  Nothing here is imported by the product.

Recorded per output tensor: the SHA-256 of its bytes and its first 64 elements as integers of the element's width.

C = 3 and T = 64 everywhere; a train case is STEPS fused steps with dropout 0.5 unless it says otherwise.  The shapes are the
smallest at which each shared piece of csrc/head_mlp.h can still go wrong:
B = 37, K = 9     three groups of 16 rows, the last with 5; 9 * 64 = 576 dW3 elements = two full register slots of 256 and a
                  quarter of the third (the slots the RANGE=3 negative control drops)
B = 16, K = 16    one exactly full group, all four dW3 slots, `tid < K` at MSIG_MAX_K
B = 2064, K = 16  129 groups on head_bwd_kernel's 128 workgroups (one takes two groups, its accumulators carry over), too many for
                  the fused head: head_fwd_kernel, ce_kernel, head_bwd_kernel
B = 12, K = 3     distillation: the head runs unfused at one group
B = 40 / 256      the discriminator: three chunks the last half full, and MSIG_DA_MAX_BATCH (every thread owns a row)
head epoch        K = 16, steps of 37, 37 and 20 rows (three chunks each, the last of 5 and of 4 rows)"""
import ctypes as C
import hashlib

import numpy as np

LR, WD = 1e-3, 1e-2
CC, T = 3, 64
STEPS = 2
MID = dict(B=37, K=9)
FULL = dict(B=16, K=16)
LARGE = dict(B=2064, K=16)
TINY = dict(B=12, K=3)
CW9 = (0.5, 2.0, 1.25, 1.0, 0.75, 3.0, 0.25, 1.5, 1.0)
CW16 = CW9 + (0.6, 1.1, 2.5, 0.9, 1.0, 0.3, 1.7)
SOFT = dict(label_smoothing=0.1, mix_lambda=0.7)
TRAIN_CASES = (("plain", MID, {}),
               ("class_weight", MID, dict(class_weight=CW9)),
               ("soft", MID, dict(SOFT)),
               ("class_weight_soft", MID, dict(SOFT, class_weight=CW9)),
               ("no_dropout", MID, dict(dropout_p=0.0)),
               ("full_group", FULL, {}),
               ("unfused_large", LARGE, dict(SOFT, class_weight=CW16)),
               ("unfused_distill", TINY, dict(distill=0.5)),
               ("da_S2", dict(B=40, K=9), dict(dann=dict(S=2))),
               ("da_S16_masked", dict(B=40, K=9), dict(dann=dict(S=16, masked=True), mix_lambda=0.7)),
               ("da_lambda0", dict(B=40, K=9), dict(dann=dict(S=2, lam=0.0))),
               ("da_max_batch", dict(B=256, K=9), dict(dann=dict(S=16))))
DA_POSITIONS = 300                                    # entries of the masked case's domain table, read through batch_index
FOLD_LRS, FOLD_STEP0, FOLD_LAMS = (1e-3, 3e-3), (1, 6), (1.0, 0.7)
FOLD_CW = (CW9, tuple(reversed(CW9)))
FT = dict(K=16, N=100, n_order=94, batch=37, n_steps=3, thr=128)          # steps of 37, 37 and 20 rows
FT_MULTI = dict(lr=(1e-3, 3e-3), step0=(4, 9), seed=(11, 12))
REGIONS = (("LOGITS", "f", "BK"), ("PROBS", "f", "BK"), ("PRED", "i", "B"), ("HID", "f", "B64"), ("DLOGITS", "f", "BK"),
           ("DFEAT", "f", "B128"), ("LOSS", "f", "3"))


def record(t):
    """A device tensor -> (sha256 digest as 32 uint8, first 64 elements as same-width integers)."""
    a = t.detach().contiguous().cpu().numpy()
    flat = a.reshape(-1).view({1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize])
    return np.frombuffer(hashlib.sha256(flat.tobytes()).digest(), dtype=np.uint8).copy(), flat[:64].copy()


def _stream(torch, dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _batch(torch, dev, B, K, seed):
    rs = np.random.RandomState(seed)
    y = rs.randint(0, K, size=B).astype(np.int64)
    y[:min(K, B)] = np.arange(min(K, B))
    return torch.as_tensor(rs.randn(B, CC, T).astype(np.float32)).to(dev), torch.as_tensor(y).to(dev)


def _engine(torch, dev, K, seed, storage_engine=None):
    from oracle import cnn_gru_oracle as O
    from multimodalsignal_amd.runtime import Engine
    e = storage_engine if storage_engine is not None else Engine(CC, K, dev)
    e.load_named(O.init_params(CC, K, seed=seed))
    return e


def regions(L, torch, ws, B, K, training=True, names=None):
    """What the head kernels themselves wrote into the workspace `ws` (uint8) of a call of this shape."""
    off = L.workspace_layout(B, CC, T, K, training)
    shapes = {"BK": B * K, "B": B, "B64": B * 64, "B128": B * 128, "3": 3}
    return {f"ws.{n}": ws[off[L.WS[n]]:off[L.WS[n] + 1]].view(torch.float32 if d == "f" else torch.int32)[:shapes[s]]
            for n, d, s in REGIONS if names is None or n in names}


def _ws(e):
    return e._ws[e._last][0]


def train_case(L, torch, dev, name):
    """STEPS consecutive train steps of one model, each on its own batch: the head's workspace regions after the last step, the
    loss accumulator, parameters and both moments — and the discriminator's state where the step trains one."""
    shape, opt = next((s, o) for n, s, o in TRAIN_CASES if n == name)
    opt = dict(opt)
    B, K = shape["B"], shape["K"]
    e = _engine(torch, dev, K, seed=5)
    if "class_weight" in opt:
        opt["class_weight"] = torch.tensor(opt["class_weight"], dtype=torch.float32, device=dev)
    opt.setdefault("dropout_p", 0.5)
    adv, da = None, opt.pop("dann", None)
    if da is not None:
        from multimodalsignal_amd.adversary import SubjectAdversary
        S = da["S"]
        adv = SubjectAdversary(S, lam=da.get("lam", 0.5), schedule="constant", seed=9)
        rs = np.random.RandomState(1000 + S + B)
        if da.get("masked"):
            table = rs.randint(0, S, size=DA_POSITIONS).astype(np.int32)
            table[rs.rand(DA_POSITIONS) < 0.3] = -1
            opt["batch_index"] = torch.as_tensor(rs.permutation(DA_POSITIONS)[:B].astype(np.int64)).to(dev)
        else:
            table = (np.arange(B, dtype=np.int32) * 7) % S
        adv.set_domains(table)
        adv.bind(dev)
        opt["adversary"] = adv
    alpha = opt.pop("distill", None)
    if alpha is not None:
        from multimodalsignal_amd.distill import Distillation
        kd = Distillation(alpha, 2.0)
        q = np.random.RandomState(31).rand(B, K).astype(np.float32) + 0.05
        kd.set_teacher(q / q.sum(1, keepdims=True, dtype=np.float32))
        opt["distill"] = kd.bind(dev)
    for s in range(1, STEPS + 1):
        x, y = _batch(torch, dev, B, K, 100 * s + B)
        e.train_step(x, y, LR, weight_decay=WD, step=s, seed=7, **opt)
    torch.cuda.synchronize()
    out = {"params": e.params, "exp_avg": e.exp_avg, "exp_avg_sq": e.exp_avg_sq, "loss_acc": e.loss_acc}
    out.update(regions(L, torch, _ws(e), B, K))
    if adv is not None:
        out.update({"da_params": adv.params, "da_exp_avg": adv.exp_avg, "da_exp_avg_sq": adv.exp_avg_sq, "da_stats": adv.stats})
    return {k: record(v) for k, v in out.items()}


def eval_case(L, torch, dev, with_labels):
    """msig_st_forward, not training, B = 37, K = 9: head_fwd_kernel, then ce_kernel (labels) or softmax_kernel (none)."""
    B, K = MID["B"], MID["K"]
    e = _engine(torch, dev, K, seed=5)
    x, y = _batch(torch, dev, B, K, 300 + B)
    e.forward(x, y if with_labels else None)
    torch.cuda.synchronize()
    out = regions(L, torch, _ws(e), B, K, False, ("LOGITS", "PROBS", "PRED", "HID") + (("LOSS",) if with_labels else ()))
    if with_labels:
        out["loss_acc"] = e.loss_acc
    return {k: record(v) for k, v in out.items()}


def backward_case(L, torch, dev):
    """An eval forward kept for a backward, then Engine.backward with a given dlogits: head_bwd_kernel alone, dscale = 1."""
    B, K = MID["B"], MID["K"]
    e = _engine(torch, dev, K, seed=5)
    x, y = _batch(torch, dev, B, K, 400 + B)
    b = e.forward(x, y, keep_for_backward=True)
    dl = torch.as_tensor((0.1 * np.random.RandomState(41).randn(B, K)).astype(np.float32)).to(dev)
    e.backward(b, dlogits=dl)
    torch.cuda.synchronize()
    out = regions(L, torch, _ws(e), B, K, True, ("LOGITS", "HID", "DFEAT"))
    out["grads"] = e.grads
    return {k: record(v) for k, v in out.items()}


def fold_case(L, torch, dev):
    """STEPS msig_st_train_step_multi launches of two folds, B = 37, K = 9, class weights of their own, smoothing 0.1, fold 0 at
    lam = 1 and fold 1 at lam = 0.7, different learning rates and step counts."""
    from multimodalsignal_amd.runtime import FoldArena
    B, K = MID["B"], MID["K"]
    n = len(FOLD_LRS)
    arena = FoldArena(CC, K, dev, n, B, T)
    for f in range(n):
        _engine(torch, dev, K, seed=20 + f, storage_engine=arena.engine(f))
        arena.set_class_weight(f, FOLD_CW[f])
    ea, eas, slots = arena.ptr("exp_avg"), arena.ptr("exp_avg_sq"), list(range(n))
    for s in range(STEPS):
        for f in range(n):
            x, y = _batch(torch, dev, B, K, 1000 * f + s)
            arena.view(f, "x", torch.float32)[:x.numel()].copy_(x.reshape(-1))
            arena.view(f, "y", torch.int64)[:B].copy_(y)
        steps = [FOLD_STEP0[f] + s for f in range(n)]
        m = arena.multi(slots, key_gru=[L.dropout_key(100 + f, steps[f], 1) for f in range(n)],
                        key_head=[L.dropout_key(100 + f, steps[f], 2) for f in range(n)], lr=list(FOLD_LRS), steps=steps)
        desc, sd = arena.batch(B, True, 0.5), arena.soft(slots, 0.1, list(FOLD_LAMS), arena.ptr("cw"))
        L.check(L.lib().msig_st_train_step_multi(C.byref(desc), C.byref(m), C.byref(sd), ea, eas, 0.9, 0.999, 1e-8, WD, steps[0],
                                                 _stream(torch, dev)), "msig_st_train_step_multi")
    torch.cuda.synchronize()
    out = {}
    for f in range(n):
        out.update({f"fold{f}.{k}": arena.view(f, k) for k in ("params", "exp_avg", "exp_avg_sq", "acc")})
        out.update({f"fold{f}.{k}": v for k, v in regions(L, torch, arena.view(f, "ws"), B, K).items()})
    return {k: record(v) for k, v in out.items()}


def head_epoch_case(L, torch, dev, multi):
    """msig_ft_head_epoch (one fold) or msig_ft_head_epoch_multi (two folds of different lr, step0 and seed): three steps on the bare
    128 -> 64 -> 16 head, dropout threshold 128, class weights on, non-zero moments, weight decay on."""
    K, N = FT["K"], FT["N"]
    n = 2 if multi else 1
    n_flat = (64 * 128 + 64 + (K * 64 + 3) // 4 * 4 + K + 3) // 4 * 4
    sizes = [("params", n_flat * 4), ("ea", n_flat * 4), ("eas", n_flat * 4), ("feat", N * 512), ("labels", N * 8), ("order", FT["n_order"] * 4),
             ("cw", K * 4), ("acc", 16)]
    off, at = {}, 0
    for name, nb in sizes:
        off[name] = (at, nb)
        at += (nb + 255) // 256 * 256
    mem = torch.zeros((n, at), dtype=torch.uint8, device=dev)
    view = lambda s, name, dt: mem[s, off[name][0]:off[name][0] + off[name][1]].view(dt)
    for s in range(n):
        rs = np.random.RandomState(77 + s)
        put = lambda name, a, dt: view(s, name, getattr(torch, np.dtype(dt).name)).copy_(torch.as_tensor(np.ascontiguousarray(a).astype(dt)).reshape(-1))
        put("params", 0.1 * rs.randn(n_flat), np.float32)
        put("ea", 0.01 * rs.randn(n_flat), np.float32)
        put("eas", 1e-3 * rs.rand(n_flat), np.float32)
        put("feat", rs.randn(N, 128), np.float32)
        put("labels", rs.permutation(N) % K, np.int64)
        put("order", rs.permutation(N)[:FT["n_order"]], np.int32)
        put("cw", np.asarray(CW16) if s == 0 else np.asarray(CW16)[::-1], np.float32)
    ptr = lambda name: mem.data_ptr() + off[name][0]
    h = L.FtHead()
    h.K, h.N, h.n_order, h.batch, h.first_step, h.n_steps, h.dropout_thr = K, N, FT["n_order"], FT["batch"], 0, FT["n_steps"], FT["thr"]
    h.cls_offset, h.step0, h.seed = 0, FT_MULTI["step0"][0], FT_MULTI["seed"][0]
    h.lr, h.beta1, h.beta2, h.eps, h.weight_decay = FT_MULTI["lr"][0], 0.9, 0.999, 1e-8, WD
    h.feat, h.labels, h.order = ptr("feat"), ptr("labels"), ptr("order")
    h.params, h.exp_avg, h.exp_avg_sq, h.class_weight, h.loss_acc = ptr("params"), ptr("ea"), ptr("eas"), ptr("cw"), ptr("acc")
    if multi:
        m = L.FtMulti()
        m.n, m.stride_bytes = n, at
        for i in range(n):
            m.slot[i], m.lr[i], m.step0[i], m.seed[i] = i, FT_MULTI["lr"][i], FT_MULTI["step0"][i], FT_MULTI["seed"][i]
        L.check(L.lib().msig_ft_head_epoch_multi(C.byref(h), C.byref(m), _stream(torch, dev)), "msig_ft_head_epoch_multi")
    else:
        L.check(L.lib().msig_ft_head_epoch(C.byref(h), _stream(torch, dev)), "msig_ft_head_epoch")
    torch.cuda.synchronize()
    dts = {"params": torch.float32, "ea": torch.float32, "eas": torch.float32, "acc": torch.float64}
    return {f"fold{s}.{k}": record(view(s, k, dt)) for s in range(n) for k, dt in dts.items()}


def all_cases():
    """(key, callable(L, torch, dev) -> {output: (sha, head)}) for every case."""
    cases = [(f"train/{n}", lambda L, t, d, n=n: train_case(L, t, d, n)) for n, _, _ in TRAIN_CASES]
    cases.append(("train/two_folds", fold_case))
    cases += [(f"eval/{'labels' if w else 'no_labels'}", lambda L, t, d, w=w: eval_case(L, t, d, w)) for w in (True, False)]
    cases.append(("backward/given_dlogits", backward_case))
    cases += [(f"head_epoch/{'two_folds' if m else 'one_fold'}", lambda L, t, d, m=m: head_epoch_case(L, t, d, m)) for m in (False, True)]
    return cases
