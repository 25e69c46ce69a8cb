"""Shared helpers for the -m gpu parity tests: run the HIP path through the C ABI and
collect, stage by stage, its deviation from the CPU oracle."""
import numpy as np
import torch

from oracle import cnn_gru_oracle as O


# Tolerances (round 4) ADAPT to the case: every compared tensor is also produced by the oracle in fp32, and the disagreement of
# that fp32 run with the fp64 run — `own`, relative to the tensor's largest magnitude like every error here — is what plain fp32
# arithmetic costs on THIS input (shape, sequence length, cancellation).  The HIP path is fp32 arithmetic too (fp32 MFMA, or
# split-bf16 products that are no less accurate, profiles/r01_bf16x3_microbench.log), so its error has to stay within a small
# multiple of `own`:   tol = max(floor, K x own).
# Calibration (gpurun_out/r04_parity_dump1.jsonl, 81 run_case reports of the whole -m gpu matrix; tools/parity_table.py):
#   stage      worst err  worst err/own     stage      worst err  worst err/own     weight gradients (err > 3e-7)      worst err  err/own
#   gate_s      1.3e-07      1.5            d_logits    3.7e-07     (own ~ 0)       gru.weight_ih / weight_hh            1.9e-06    3.0
#   conv1       2.8e-07      1.3            d_feat      3.5e-07      2.0            gru.bias_ih / bias_hh                1.4e-06    4.2
#   pool1       3.4e-07      1.3            d_gru_l0    4.4e-07      1.6            cnn_encoder.{0,4}.weight             4.0e-06    1.5
#   conv2       4.9e-07      1.9            d_pool2     7.4e-07      1.8            cnn_encoder.{1,5}.{weight,bias}      1.4e-06 *  2.3
#   pool2       1.4e-06      2.0            d_bn2       1.0e-06      2.6            channel_attention.fc.{0,2}.weight    2.1e-06    5.7
#   gru_l0      1.8e-06      1.5            d_pool1     1.2e-06      2.0            classifier.0.{weight,bias}           8.3e-07    1.7
#   gru_l1_fwd  1.6e-06      1.9            d_bn1       9.7e-07 *    2.3            classifier.3.weight                  1.6e-06    2.0
#   feat        9.6e-07      1.8            d_gate_s    9.7e-07 *    2.4            classifier.3.bias (sums to ~0)       3.5e-06   53
#   cls_hidden  8.0e-07      2.8            loss        2.3e-07      -
#   logits      1.7e-06      4.6            running_mean / var  3.2e-07 / 6.4e-08
#   * without the one case that has an adopted MaxPool near-tie (B = 3100, T = 960: ONE window of 1.9e7 routes its gradient to the
#     neighbouring position: d_bn1 1.4e-4, d_gate_s 2.3e-5, cnn_encoder.1.bias 8.2e-6): stages downstream of the pooling backward
#     get TIE_SLACK x their tolerance per adopted decision.
# K = 8 for the stages, 6 for the weight gradients (whose `own` is the larger and the better conditioned yardstick); the floors
# cover the cases where `own` is accidentally tiny (two-row batches, sums that cancel to ~0).  Round 3's fixed constants were
# 20-40 x the worst observed error: a regression confined to ONE contraction passed them.
# Negative controls (make negctl NEGCTL=1..5,9: the split-bf16 product without its a1 * b1 cross term — 2^-16 relative per
# product — in one class of contractions; tools/negative_controls.sh, profiles/r04_negative_control.log): each of them FAILS.
# The same table over TRAINED-LIKE parameters (saturated gates, signed / zero BatchNorm gamma, saturated logits: tests/regimes.py,
# tests/test_trained_regimes_gpu.py, held to these constants unchanged) is in DESIGN.md section 2, "Trained-like regimes"; its
# negative controls (make negctl REGIME=k) in profiles/regime_negative_control.log.
# The same table over INPUT regimes (offsets of 10 spreads, units, spikes, zero spans, flat windows: tests/input_regimes.py,
# tests/test_input_regimes_gpu.py, held to these constants unchanged) is in DESIGN.md section 2, "Input regimes"; its negative
# controls (make negctl INPUT=k) in profiles/input_negative_control.log.
# The same table over WINDOW LENGTHS (every residue T % 16, unaligned lengths and T % 8 == 4 across the conv chunk borders, T' = 2 .. 8:
# tests/window_lengths.py, tests/test_window_lengths_gpu.py, held to these constants unchanged) is in DESIGN.md section 2, "Window
# lengths"; its negative controls (make negctl LENGTH=k) in profiles/length_negative_control.log.
# The same table over STAGE-2 regimes (conv2 channels at mean^2 / var of 16 .. 200 and 500 .. 1300 at 1, 2, 4, 24, 37 and 300 work items,
# zeroed and 1e-3 / 1e3 convolution rows: tests/regimes.py, tests/test_stage2_regimes_host.py, tests/test_stage2_regimes_gpu.py, held to
# these constants unchanged) is in DESIGN.md section 2, "Stage-2 regimes"; its negative control (make negctl STAGE2=1) in
# profiles/stage2_negative_control.log.
# The same table over BATCH SIZES (every row count of a ragged last batch tile, neighbouring batches across every switch of the launchers:
# tests/batch_sizes.py, tests/test_batch_sizes_host.py, tests/test_batch_sizes_gpu.py, held to these constants unchanged) is in
# DESIGN.md section 2, "Batch sizes"; its negative controls (make negctl BATCH=k) in profiles/batch_negative_control.log.
K_STAGE, STAGE_FLOOR = 8.0, 2e-6
K_GRAD = 6.0
GRAD_FLOORS = (("gru.", 3e-6), ("classifier.3.bias", 1.2e-5), ("", 6e-6))      # first matching prefix
GRAD_FLOOR = 6e-6      # the general floor (kept under this name for the tests that check gradients on their own)
TIE_SLACK = 10.0
TIE_SLACK_DBN1 = 40.0      # d_bn1 itself: the adopted window's gradient element is compared at full size (observed 1.4e-4 = 31 x the plain tolerance)
FIXED_TOL = {"loss": 2e-6, "running_mean": 3e-6, "running_var": 1e-6}


def stage_tol(name, own, slack=1.0):
    """Tolerance of one stage comparison: max(floor, K x the fp32 oracle's own disagreement with the fp64 oracle)."""
    return max(STAGE_FLOOR, K_STAGE * (own or 0.0)) * slack


def grad_tol(key, own, slack=1.0):
    floor = next(f for pre, f in GRAD_FLOORS if key.startswith(pre))
    return max(floor, K_GRAD * own) * slack


def to_t(d, dtype=torch.float32):
    out = {}
    for k, v in d.items():
        t = torch.as_tensor(v)
        out[k] = t if "num_batches" in k else t.to(dtype)
    return out


def split_named(named):
    params = {k: v for k, v in named.items() if "running" not in k and "num_batches" not in k}
    buffers = {k: v for k, v in named.items() if k not in params}
    return params, buffers


def rel_err(a, ref):
    a = np.asarray(a, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    if ref.size == 0:
        return 0.0
    scale = max(np.abs(ref).max(), 1e-12)
    return float(np.abs(a - ref).max() / scale)


def routed_dz(dp, code, L):
    """dz = dL/d(bn output) (B, L, CH) from dP (B, P, CH) and the forward pass's pooling decisions (B, P, CH/4) bytes, 2 bits
    per channel: 0/1/2 = left/centre/right candidate won and is positive, 3 = no gradient (include/msig.h WS_POOLC*)."""
    B, P, CH = dp.shape
    win = (code[:, :, :, None] >> (2 * np.arange(4, dtype=np.uint8))[None, None, None, :]) & 3     # (B, P, CH/4, 4)
    win = win.reshape(B, P, CH)
    dz = np.zeros((B, L, CH), dtype=np.float64)
    ph = np.arange(P)
    for k in range(3):
        t = 2 * ph - 1 + k
        ok = (t >= 0) & (t < L)
        contrib = np.where(win == k, dp, 0.0)[:, ok, :]
        dz[:, t[ok], :] += contrib          # for a fixed candidate index the target positions are distinct
    return dz


def run_case(engine, named, x, y, dropout_p=0.0, seed=0, step=0, check_backward=True, launch=None, tag=None, adopt=True):
    """Returns {stage: (relative max error, tolerance)} for forward (+ backward) stages.
    launch: None = engine.forward / engine.backward; otherwise a callable(phase) for phase "fwd" / "bwd" that has the HIP path
    produce the same workspace regions and gradient buffer some other way (e.g. ONE msig_train_step_multi over several folds,
    after which every fold's engine is compared) — parameters / buffers / inputs are then the caller's to load beforehand."""
    import multimodalsignal_amd._lib as L
    C, K = engine.C, engine.K
    B, _, T = x.shape
    L1, P1, L2, TP = O.stage_lengths(T)
    params, buffers = split_named(to_t(named))
    for k, spec in O.buffer_specs().items():
        if k not in buffers:
            buffers[k] = O.init_buffers()[k]
    xt, yt = torch.as_tensor(x), torch.as_tensor(y)
    dev = engine.device
    if launch is None:
        engine.load_named({**params, **buffers})
        b = engine.forward(xt.to(dev), yt.to(dev), training=True, dropout_p=dropout_p, seed=seed, step=step)
    else:
        launch("fwd")
    torch.cuda.synchronize()
    # fp64 oracle: tells how far fp32 itself is from exact arithmetic
    fw = dict(dropout_p=dropout_p, seed=seed, step=step)
    p64, b64 = split_named(to_t(named, torch.float64))
    for k in buffers:
        b64.setdefault(k, buffers[k] if "num_batches" in k else buffers[k].double())
    loss64, grads64, st64, _ = O.loss_and_grads(p64, b64, xt.double(), yt, retain=True, **fw)
    # MaxPool's argmax is a discrete decision: where two candidates of a window agree to within fp32 resolution, which of
    # them is "the" maximum differs between any two fp32 implementations (one such window in ~2e7 at B=3100 x T=960), and
    # the gradient then lands one or two positions away.  Only for such near-ties the oracle adopts the decision of the
    # HIP path (recomputed here from ITS conv output and BN constants, as bn_relu_pool / pool_bn_bwd_pass1 do:
    # z = fma(y, scale, shift), first maximum wins); everywhere else the oracle's own argmax stands, so a wrong tie
    # rule or a wrong window still fails.  The number of adopted decisions is reported and bounded.
    choice, n_adopted = {}, 0
    for stage, yname, sname, CH, Lc in (("pool1", "Y1", "BN1_STAT", 16, L1), ("pool2", "Y2", "BN2_STAT", 32, L2)):
        yh = engine.region(yname, torch.float32, (B, Lc, CH)).cpu().double().permute(0, 2, 1)
        stt = engine.region(sname, torch.float32, (4, CH)).cpu().double()
        zh = (yh * stt[2][None, :, None] + stt[3][None, :, None]).float()            # fma in fp32: exact product, one rounding
        ch_hip = O.first_argmax(O.pool_windows(torch.clamp_min(zh, 0)))
        win = O.pool_windows(torch.clamp_min(st64["bn" + stage[-1]].detach(), 0))
        ch_ref = O.first_argmax(win)
        top = win.max(dim=3).values
        hip_val = win.gather(3, ch_hip.to(torch.int64)[..., None]).squeeze(3)
        near = (ch_hip != ch_ref) & ((top - hip_val) <= 4e-6 * torch.clamp_min(top.abs(), 1e-3))   # HIP's pick is within fp32 noise of the maximum
        if not adopt:           # constructed exact-tie cases: the oracle's own first-maximum rule stands everywhere
            near = torch.zeros_like(near)
        n_adopted += int(near.sum())
        choice[stage] = torch.where(near, ch_hip, ch_ref)
    if n_adopted:
        loss64, grads64, st64, _ = O.loss_and_grads(p64, b64, xt.double(), yt, retain=True, pool_choice=choice, **fw)
    # the fp32 oracle routes through the same windows, so that `own` below measures arithmetic, not its own near-tie flips
    loss, grads, st, nb = O.loss_and_grads(params, buffers, xt, yt, retain=True, pool_choice=choice, **fw)
    R = lambda name, shape, dtype=torch.float32: engine.region(name, dtype, shape).cpu().numpy()
    rep = {"pool_near_ties_adopted": (float(n_adopted), 8.0)}
    rep_own = {}

    def put(name, got, key, own32=None, slack=1.0):
        """key: the stage's name in the oracle's stage dict, or the fp64 reference itself (then own32 = the fp32 oracle's value
        of the same tensor).  The tolerance adapts to the fp32 oracle's own disagreement with the fp64 oracle (stage_tol)."""
        ref64 = st64[key].detach().numpy() if isinstance(key, str) else key
        if own32 is None:
            own32 = st[key].detach().numpy()
        own = rel_err(own32, ref64)
        rep_own[name] = own
        rep[name] = (rel_err(got, ref64), stage_tol(name, own, slack))

    put("gate_s", R("GATE_S", (B, C)), "gate_s")
    put("conv1", R("Y1", (B, L1, 16)).transpose(0, 2, 1), "conv1")
    put("pool1", R("P1", (B, P1, 16)).transpose(0, 2, 1), "pool1")
    put("conv2", R("Y2", (B, L2, 32)).transpose(0, 2, 1), "conv2")
    put("pool2", R("P2", (B, TP, 32)).transpose(0, 2, 1), "pool2")
    put("gru_l0", R("H0", (B, TP, 128)), "gru_l0")
    put("gru_l1_fwd", R("H1", (B, TP, 64)), "gru_l1_fwd")
    put("feat", R("FEAT", (B, 128)), "feat")
    put("cls_hidden", R("HID", (B, 64)), "cls_hidden")
    put("logits", R("LOGITS", (B, K)), "logits")
    rep["loss"] = (abs(float(R("LOSS", (4,))[0]) - float(loss64)) / max(abs(float(loss64)), 1e-6), FIXED_TOL["loss"])
    bn = engine.bn_state.cpu().numpy()
    for i, (k, sl) in enumerate((("cnn_encoder.1.running_mean", slice(0, 16)), ("cnn_encoder.1.running_var", slice(16, 32)),
                                 ("cnn_encoder.5.running_mean", slice(32, 64)), ("cnn_encoder.5.running_var", slice(64, 96)))):
        rep[k] = (rel_err(bn[sl], nb[k].numpy()), FIXED_TOL["running_var" if "var" in k else "running_mean"])
    if not check_backward:
        _dump(rep, tag, x.shape, dropout_p, rep_own)
        return rep, None
    if launch is None:
        engine.backward(b)
    else:
        launch("bwd")
    torch.cuda.synchronize()
    g64 = lambda k: grads64[k].numpy()
    g32 = lambda k: grads[k].numpy()
    tie = 1.0 + TIE_SLACK * n_adopted          # an adopted near-tie moves one window's gradient by one position in the fp32 run
    put("d_logits", R("DLOGITS", (B, K)), g64("stage/logits"), g32("stage/logits"))
    put("d_feat", R("DFEAT", (B, 128)), g64("stage/feat"), g32("stage/feat"))
    put("d_gru_l0", R("DH0", (B, TP, 128)), g64("stage/gru_l0_dropped"), g32("stage/gru_l0_dropped"))
    dx0 = R("DX0", (2, B, TP, 32))
    put("d_pool2", (dx0[0] + dx0[1]).transpose(0, 2, 1), g64("stage/pool2"), g32("stage/pool2"))
    # WS_DY2 holds dL/d(bn2 output) (dP2 routed through the forward pass's pooling decisions WS_POOLC2; the BatchNorm-backward
    # second pass of stage 2 is fused into the conv2 backward kernels).  Stage 1's dz is never stored: conv1_bwd routes WS_DP1
    # through WS_POOLC1 on the fly — rebuilt here the same way, and the stage-2 tensor is cross-checked against its own codes.
    dz2 = R("DY2", (B, L2, 32))
    put("d_bn2", dz2.transpose(0, 2, 1), g64("stage/bn2"), g32("stage/bn2"))
    np.testing.assert_array_equal(dz2, routed_dz((dx0[0] + dx0[1]).astype(np.float64), R("POOLC2", (B, TP, 8), torch.uint8), L2).astype(np.float32))
    dp1 = R("DP1", (B, P1, 16))
    put("d_pool1", dp1.transpose(0, 2, 1), g64("stage/pool1"), g32("stage/pool1"))
    put("d_bn1", routed_dz(dp1.astype(np.float64), R("POOLC1", (B, P1, 4), torch.uint8), L1).transpose(0, 2, 1), g64("stage/bn1"), g32("stage/bn1"), slack=1.0 + TIE_SLACK_DBN1 * n_adopted)
    if "stage/gate_s" in grads64:
        put("d_gate_s", R("DS", (B, C)), g64("stage/gate_s"), g32("stage/gate_s"), slack=tie)
    gviews = engine.named_param_views(engine.grads)
    for k in L.PARAM_KEYS:
        own = rel_err(grads[k].numpy(), g64(k))
        front = k.startswith("cnn_encoder.0") or k.startswith("cnn_encoder.1") or k.startswith("channel_attention")
        rep["grad/" + k] = (rel_err(gviews[k].cpu().numpy(), g64(k)), grad_tol(k, own, tie if front else 1.0))
        rep_own["grad/" + k] = own
    _dump(rep, tag, x.shape, dropout_p, rep_own)
    return rep, (loss64, grads64)


def _dump(rep, tag, shape, p, own=None):
    """MSIG_PARITY_DUMP=<file>: appends every report as one JSON line (the table of worst observed errors that the tolerances in
    this file are derived from is made from one such run: tools/parity_table.py)."""
    import json, os
    path = os.environ.get("MSIG_PARITY_DUMP")
    if not path:
        return
    test = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
    with open(path, "a") as f:
        f.write(json.dumps({"test": test, "tag": tag, "shape": list(shape), "p": p, "err": {k: v[0] for k, v in rep.items()},
                            "tol": {k: v[1] for k, v in rep.items()}, "own": own or {}}) + "\n")


def format_report(rep):
    lines = []
    for k, (e, tol) in rep.items():
        lines.append(f"{'FAIL' if not (e <= tol) else 'ok  '} {k:45s} err={e:.3e} tol={tol:.1e}")
    return "\n".join(lines)


def failures(rep):
    return [k for k, (e, tol) in rep.items() if not (e <= tol)]


# ---- the narrow entry points, called directly ---------------------------------------------------------------------------------------
# Engine.train_step / Engine.forward always issue the widest library call; the "is the counterpart" tests and
# tests/test_step_dispatch_gpu.py put the entry point a header names on the other side of their comparison with these.
def legacy_train_step(e, x, y, lr, weight_decay=0.0, step=1, dropout_p=0.0, seed=0, class_weight=None, betas=(0.9, 0.999), eps=1e-8):
    """One fused step of engine `e` through msig_cg_train_step (the cnn_gru kind), msig_cw_train_step (a class-weight tensor) or
    msig_train_step, with EmbeddedEngine's scatter / gather around it.  Returns the name of the entry point it called."""
    import ctypes as C
    from multimodalsignal_amd import _lib as L
    cw = e._class_weight(class_weight)
    if hasattr(e, "scatter"):
        e.scatter()
    e.ensure_adam_state()
    b = e._batch(x, y, True, dropout_p, seed, step)
    tail = (e.exp_avg.data_ptr(), e.exp_avg_sq.data_ptr(), lr, betas[0], betas[1], eps, weight_decay, step, e._stream())
    if e.kind == "cnn_gru":
        name, rc = "msig_cg_train_step", L.lib().msig_cg_train_step(C.byref(b), cw, *tail)
    elif cw is not None:
        name, rc = "msig_cw_train_step", L.lib().msig_cw_train_step(C.byref(b), cw, *tail)
    else:
        name, rc = "msig_train_step", L.lib().msig_train_step(C.byref(b), *tail)
    L.check(rc, name)
    if hasattr(e, "gather"):
        e.gather()
    return name


def narrow_train_step(e, x, y, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=1, dropout_p=0.0, seed=0, class_weight=None,
                      max_grad_norm=None, label_smoothing=0.0, mix_lambda=None, adversary=None, batch_index=None, distill=None, sam=None,
                      dro=None, supcon=None, entry=None):
    """One fused step of engine `e` through the NARROWEST entry point whose signature has every term given — msig_sc_train_step with
    `supcon`, else msig_dro_train_step with `dro`, else msig_sam_train_step with `sam`, else msig_kd_train_step with `distill`, else
    msig_da_train_step — or through `entry`, called directly on the library with the descriptors Engine.train_step builds and with its
    bookkeeping (the adversary's lambda and step count, EmbeddedEngine's scatter / gather).  Engine.train_step always issues the
    widest call; this is the other side of the comparisons that hold it to the narrower ones.  Returns the entry point's name."""
    import ctypes as C
    from multimodalsignal_amd import _lib as L
    ref = lambda d: None if d is None else C.byref(d)      # noqa: E731
    name = entry or ("msig_sc_train_step" if supcon is not None else "msig_dro_train_step" if dro is not None else
                     "msig_sam_train_step" if sam is not None else "msig_kd_train_step" if distill is not None else "msig_da_train_step")
    cw, max_norm, smooth, lam = e._checked(class_weight, max_grad_norm, label_smoothing, mix_lambda)
    if adversary is not None and hasattr(e, "hidden"):
        adversary.restrict_features(e.hidden)
    if hasattr(e, "scatter"):
        e.scatter()
    e.ensure_adam_state()
    b = e._batch(x, y, True, dropout_p, seed, step)
    idx = None if batch_index is None else batch_index.data_ptr()
    a = k = sd = dd = cd = None
    if adversary is not None:
        adversary.last_lambda = adversary.next_lambda()
        a = adversary.descriptor([adversary.last_lambda], [lr * adversary.lr_mult], [adversary.step + 1], idx=idx, betas=betas, eps=eps,
                                 weight_decay=weight_decay)
    if distill is not None:
        k = distill.descriptor(idx=idx)
    if sam is not None:
        state = e.ensure_sam_state()
        sd = sam.descriptor(e.kind, state.data_ptr(), state.numel() * 8)
    if dro is not None:
        dd = dro.descriptor(idx=idx)
    if supcon is not None:
        cd = supcon.descriptor(idx=idx)
    terms = {"msig_da_train_step": (a,), "msig_kd_train_step": (a, k), "msig_sam_train_step": (k, sd), "msig_dro_train_step": (a, k, sd, dd),
             "msig_sc_train_step": (a, k, sd, dd, cd)}[name]
    given = [d for d in (a, k, sd, dd, cd) if d is not None]
    assert all(any(d is t for t in terms) for d in given), f"{name} has no parameter for a term that was given"
    rc = getattr(L.lib(), name)(C.byref(b), C.byref(e._st(cw, max_norm, smooth, lam)), *[ref(t) for t in terms], e.exp_avg.data_ptr(),
                                e.exp_avg_sq.data_ptr(), lr, betas[0], betas[1], eps, weight_decay, step, e._stream())
    L.check(rc, name)
    if adversary is not None:
        adversary.step += 1
    e._keep = e._keep + (batch_index,)
    if hasattr(e, "gather"):
        e.gather()
    return name


def legacy_forward(e, x, y=None, training=False, keep_for_backward=False, class_weight=None, dropout_p=0.0, seed=0, step=0):
    """A forward of engine `e` through msig_cg_forward, msig_cw_forward or msig_forward, chosen as legacy_train_step chooses."""
    import ctypes as C
    from multimodalsignal_amd import _lib as L
    cw = e._class_weight(class_weight)
    if hasattr(e, "scatter"):
        e.scatter()
    b = e._batch(x, y, training, dropout_p, seed, step, keep_for_backward)
    if e.kind == "cnn_gru":
        name, rc = "msig_cg_forward", L.lib().msig_cg_forward(C.byref(b), cw, e._stream())
    elif cw is not None:
        name, rc = "msig_cw_forward", L.lib().msig_cw_forward(C.byref(b), cw, e._stream())
    else:
        name, rc = "msig_forward", L.lib().msig_forward(C.byref(b), e._stream())
    L.check(rc, name)
    return name
