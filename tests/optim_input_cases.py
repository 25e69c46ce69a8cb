"""The cases of tests/golden/optim_input.npz: inputs regenerated from fixed numpy seeds, and the library calls that turn them into the
recorded outputs — shared by tests/golden/make_optim_input_golden.py (which records them once, from the library as it was before the
Adam update, the column reduction and the per-subject normalisation each became one piece of source) and
tests/test_optim_input_golden_gpu.py (which compares bits).  Nothing here is imported by the product.

Recorded per output tensor: the SHA-256 of its bytes and its first 64 elements as integers of the element's width.

The train-step shapes, and which reduction job of the step's last launch is which (csrc: launch_head_step, launch_frontend_bwd; a
job's partial rows are summed by colsum_lane, 8 row-lanes, a main loop that takes 64 rows at a time and a tail loop that takes 8):
SMALL  B = 12, C = 3, K = 3, T = 5136 — the fused head (one launch, its loss workgroup riding in the reduction launch):
       the four head jobs have ceil(B / 16) = 1 partial row (fewer than 8: only the tail loop, seven row-lanes idle), cls3's bias
       among them with K = 3 columns; conv1's weight job has B = 12 rows (tail loop, twice for four row-lanes); conv2's weight job
       has B * ceil(L2 / 128) = 12 * 6 = 72 rows (main loop once, then the tail loop) — job_rows() computes the three.
LARGE  B = 2064 > 16 * 128, T = 64: the head runs unfused, the reduction launch has no loss workgroup; 128 and 1024 partial rows."""
import ctypes as C
import hashlib

import numpy as np

LR, WD = 1e-3, 1e-2
SMALL = dict(B=12, C=3, K=3, T=5136)
LARGE = dict(B=2064, C=3, K=3, T=64)
STEPS = 3
CLIP_SMALL = 1e-3                                    # far below any gradient norm of these steps: coef < 1 on every step
TRAIN_CASES = (("plain", SMALL, {}), ("large", LARGE, {}),
               ("class_weight", SMALL, dict(class_weight=(0.5, 2.0, 1.25))),
               ("soft", SMALL, dict(label_smoothing=0.1, mix_lambda=0.7)),
               ("clip", SMALL, dict(max_grad_norm=CLIP_SMALL)),
               ("clip_inf", SMALL, dict(max_grad_norm=float("inf"))),
               ("cnn_gru", SMALL, dict(kind="cnn_gru")),
               ("dann", SMALL, dict(dann=True)))
FOLD_LRS, FOLD_STEP0 = (1e-3, 3e-3), (1, 6)          # the fold batch of two: fold 1 is five optimiser steps ahead
ADAM_N = (4, 4 * (2048 * 256 + 300))                 # one float4; a thread of the 2048 x 256 grid takes a second iteration
FT = dict(K=3, N=13, n_order=13, batch=5, n_steps=3, step0=4)     # steps of 5, 5 and 3 rows
NORM_SHAPES = ((1, 100), (3, 300), (20, 256), (129, 1024))
NORM_C_ALL, NORM_COLS, NORM_LOG1P = 5, (3, 0, 4), 1 << 1          # log1p on the second selected channel (raw column 0)
GUARD = 4096                                          # poisoned bytes behind the plain call's scratch


def job_rows(B, T, **_):
    """(head, conv1 weight, conv2 weight) partial rows of a fused-head step of this shape."""
    L1 = (T + 6 - 7) // 2 + 1
    P1 = (L1 + 2 - 3) // 2 + 1
    L2 = (P1 + 4 - 5) // 2 + 1
    return (B + 15) // 16, min(B, 1024), min(B * ((L2 + 127) // 128), 1024)


def record(t):
    """A device tensor -> (sha256 digest as 32 uint8, first 64 elements as same-width integers)."""
    a = t.detach().contiguous().cpu().numpy()
    flat = a.reshape(-1).view({1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize])
    return np.frombuffer(hashlib.sha256(flat.tobytes()).digest(), dtype=np.uint8).copy(), flat[:64].copy()


def _stream(torch, dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _batch(torch, dev, B, C, K, T, seed):
    rs = np.random.RandomState(seed)
    y = rs.randint(0, K, size=B).astype(np.int64)
    y[:K] = np.arange(K)
    return torch.as_tensor(rs.randn(B, C, T).astype(np.float32)).to(dev), torch.as_tensor(y).to(dev)


def _params(L, C, K, kind, seed):
    from oracle import cnn_gru_oracle as O
    p = O.init_params(C, K, seed=seed)
    return {k: v for k, v in p.items() if kind != "cnn_gru" or k not in L.GATE_KEYS}


def train_case(L, torch, dev, name):
    """STEPS consecutive fused steps of one model, each on its own batch: parameters, both moments, the loss accumulator — and the
    gradient buffer with the clip statistics where the step clips, the discriminator's state where it trains one."""
    from multimodalsignal_amd.runtime import Engine
    shape, opt = next((s, o) for n, s, o in TRAIN_CASES if n == name)
    opt = dict(opt)
    B, Cc, K, T = shape["B"], shape["C"], shape["K"], shape["T"]
    kind = opt.pop("kind", "cnn_gru_attention")
    e = Engine(Cc, K, dev, kind=kind)
    e.load_named(_params(L, Cc, K, kind, seed=5))
    if "class_weight" in opt:
        opt["class_weight"] = torch.tensor(opt["class_weight"], dtype=torch.float32, device=dev)
    adv = None
    if opt.pop("dann", False):
        from multimodalsignal_amd.adversary import SubjectAdversary
        adv = SubjectAdversary(3, lam=0.5, schedule="constant", seed=9)
        adv.set_domains(np.arange(B, dtype=np.int32) % 3)
        adv.bind(dev)
        opt["adversary"] = adv
    for s in range(1, STEPS + 1):
        x, y = _batch(torch, dev, B, Cc, K, T, 100 * s + B)
        e.train_step(x, y, LR, weight_decay=WD, step=s, dropout_p=0.5, seed=7, **opt)
    torch.cuda.synchronize()
    out = {"params": e.params, "exp_avg": e.exp_avg, "exp_avg_sq": e.exp_avg_sq, "loss_acc": e.loss_acc}
    if "max_grad_norm" in opt:
        out["grads"], out["gc_stats"] = e.grads, e.gc_state[:L.GC_NSTAT]
    if adv is not None:
        out.update({"da_params": adv.params, "da_exp_avg": adv.exp_avg, "da_exp_avg_sq": adv.exp_avg_sq, "da_stats": adv.stats})
    info = e.grad_stats() if "max_grad_norm" in opt else None
    return {k: record(v) for k, v in out.items()}, info


def fold_case(L, torch, dev):
    """STEPS msig_train_step_multi launches of two folds whose step counts and learning rates differ."""
    from multimodalsignal_amd.runtime import FoldArena
    B, Cc, K, T = SMALL["B"], SMALL["C"], SMALL["K"], SMALL["T"]
    n = len(FOLD_LRS)
    arena = FoldArena(Cc, K, dev, n, B, T)
    for f in range(n):
        arena.engine(f).load_named(_params(L, Cc, K, "cnn_gru_attention", seed=20 + f))
    ea, eas = arena.ptr("exp_avg"), arena.ptr("exp_avg_sq")
    for s in range(STEPS):
        for f in range(n):
            x, y = _batch(torch, dev, B, Cc, K, T, 1000 * f + s)
            arena.view(f, "x", torch.float32)[:x.numel()].copy_(x.reshape(-1))
            arena.view(f, "y", torch.int64)[:B].copy_(y)
        steps = [FOLD_STEP0[f] + s for f in range(n)]
        m = arena.multi(list(range(n)), key_gru=[L.dropout_key(100 + f, steps[f], 1) for f in range(n)],
                        key_head=[L.dropout_key(100 + f, steps[f], 2) for f in range(n)], lr=list(FOLD_LRS), steps=steps)
        desc = arena.batch(B, True, 0.5)
        L.check(L.lib().msig_train_step_multi(C.byref(desc), C.byref(m), ea, eas, 0.9, 0.999, 1e-8, WD, steps[0], _stream(torch, dev)),
                "msig_train_step_multi")
    torch.cuda.synchronize()
    return {f"fold{f}.{k}": record(arena.view(f, k)) for f in range(n) for k in ("params", "exp_avg", "exp_avg_sq", "acc")}


def adam_case(L, torch, dev, n):
    """Two msig_adam_step calls (steps 3 and 4) on n elements from non-zero moments, weight decay on."""
    rs = np.random.RandomState(n % 9973)
    p, g, m = (torch.as_tensor((s * rs.randn(n)).astype(np.float32)).to(dev) for s in (0.5, 0.1, 0.05))
    v = torch.as_tensor((0.01 * rs.rand(n)).astype(np.float32)).to(dev)
    for step in (3, 4):
        L.check(L.lib().msig_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, LR, 0.9, 0.999, 1e-8, WD, step,
                                       _stream(torch, dev)), "msig_adam_step")
    torch.cuda.synchronize()
    return {"params": record(p), "exp_avg": record(m), "exp_avg_sq": record(v)}


def head_epoch_case(L, torch, dev):
    """One msig_ft_head_epoch call: three steps on the bare 128 -> 64 -> K head from non-zero moments, weight decay on."""
    K, N = FT["K"], FT["N"]
    n_flat = 64 * 128 + 64 + (K * 64 + 3) // 4 * 4 + K
    n_flat = (n_flat + 3) // 4 * 4
    rs = np.random.RandomState(77)
    dv = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a).astype(dt)).to(dev)
    params, ea = dv(0.1 * rs.randn(n_flat), np.float32), dv(0.01 * rs.randn(n_flat), np.float32)
    eas = dv(1e-3 * rs.rand(n_flat), np.float32)
    feat, labels = dv(rs.randn(N, 128), np.float32), dv(np.arange(N) % K, np.int64)
    order = dv(rs.permutation(N)[:FT["n_order"]], np.int32)
    acc = torch.zeros(2, dtype=torch.float64, device=dev)
    h = L.FtHead()
    h.K, h.N, h.n_order, h.batch, h.first_step, h.n_steps, h.dropout_thr = K, N, FT["n_order"], FT["batch"], 0, FT["n_steps"], 0
    h.cls_offset, h.step0, h.seed = 0, FT["step0"], 11
    h.lr, h.beta1, h.beta2, h.eps, h.weight_decay = LR, 0.9, 0.999, 1e-8, WD
    h.feat, h.labels, h.order = feat.data_ptr(), labels.data_ptr(), order.data_ptr()
    h.params, h.exp_avg, h.exp_avg_sq, h.class_weight, h.loss_acc = params.data_ptr(), ea.data_ptr(), eas.data_ptr(), None, acc.data_ptr()
    L.check(L.lib().msig_ft_head_epoch(C.byref(h), _stream(torch, dev)), "msig_ft_head_epoch")
    torch.cuda.synchronize()
    return {"params": record(params), "exp_avg": record(ea), "exp_avg_sq": record(eas), "loss_acc": record(acc)}


def norm_raw(N, T):
    """(N, T, 5) float64: column 0 positive and heavy-tailed (it goes through log1p), column 3 a temperature of 33 +- 0.05 (the
    channel the shifted sums exist for), column 4 plain; 1 and 2 are not selected."""
    rs = np.random.RandomState(1000 * N + T)
    raw = rs.randn(N, T, NORM_C_ALL)
    raw[:, :, 0] = np.exp(rs.randn(N, T))
    raw[:, :, 3] = 33.0 + 0.05 * rs.randn(N, T)
    raw[:, :, 4] = 2.0 * rs.randn(N, T) - 1.0
    return raw


def norm_mask(N):
    """Some of the windows: every third one, window 0 first (N = 1: its only window)."""
    return (np.arange(N) % 3 == 0).astype(np.uint8)


def norm_case(L, torch, dev, N, T):
    """The plain call — on a scratch of exactly msig_normalise_scratch_bytes() with poison behind it, which must survive — and the
    masked call with its stats output."""
    lib, st = L.lib(), _stream(torch, dev)
    raw = torch.as_tensor(norm_raw(N, T)).to(dev)
    cols = (C.c_int32 * len(NORM_COLS))(*NORM_COLS)
    nb = lib.msig_normalise_scratch_bytes()
    scratch = torch.full((nb + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    out = torch.full((N, len(NORM_COLS), T), -77.0, dtype=torch.float32, device=dev)
    L.check(lib.msig_normalise_subject(raw.data_ptr(), N, T, NORM_C_ALL, cols, len(NORM_COLS), NORM_LOG1P, out.data_ptr(),
                                       scratch.data_ptr(), st), "msig_normalise_subject")
    torch.cuda.synchronize()
    guard_ok = bool((scratch[nb:] == 0xA5).all())
    ref = torch.as_tensor(norm_mask(N)).to(dev)
    scratch2 = torch.empty(lib.msig_nr_scratch_bytes(), dtype=torch.uint8, device=dev)
    stats = torch.full((2 * L.MAX_C + 1,), -77.0, dtype=torch.float64, device=dev)
    out2 = torch.full_like(out, -77.0)
    L.check(lib.msig_nr_normalise_subject(raw.data_ptr(), N, T, NORM_C_ALL, cols, len(NORM_COLS), NORM_LOG1P, ref.data_ptr(),
                                          out2.data_ptr(), stats.data_ptr(), scratch2.data_ptr(), st), "msig_nr_normalise_subject")
    torch.cuda.synchronize()
    return {"plain": record(out), "masked": record(out2), "stats": record(stats)}, guard_ok


def all_cases():
    """(key, callable(L, torch, dev) -> {output: (sha, head)}) for every case."""
    cases = [(f"train/{n}", lambda L, t, d, n=n: train_case(L, t, d, n)[0]) for n, _, _ in TRAIN_CASES]
    cases.append(("train/two_folds", fold_case))
    cases += [(f"adam/n{n}", lambda L, t, d, n=n: adam_case(L, t, d, n)) for n in ADAM_N]
    cases.append(("head_epoch", head_epoch_case))
    cases += [(f"norm/N{N}_T{T}", lambda L, t, d, N=N, T=T: norm_case(L, t, d, N, T)[0]) for N, T in NORM_SHAPES]
    return cases
