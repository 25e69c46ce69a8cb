"""GPU tier: the HIP path (through the C ABI) against the CPU oracle and the golden
vectors.  Tolerances are relative to the largest magnitude of the compared tensor;
fp32 vs the fp64 oracle, so they bound fp32 rounding through up to 240 recurrent steps."""
import numpy as np
import pytest
import torch

from conftest import load_golden_model
from oracle import cnn_gru_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tier needs an MI355X"
    return torch.device("cuda:0")


@pytest.fixture
def kernel_forms():
    """Pins the GRU kernel forms (msig_batch.fwd_form / bwd_form of every descriptor the binding builds) for one test, back to auto afterwards."""
    from multimodalsignal_amd import _lib as L
    yield L.set_kernel_form
    L.set_kernel_form("auto", "auto")


def _engine(C, K, dev):
    from multimodalsignal_amd.runtime import Engine
    return Engine(C, K, dev)


@pytest.mark.parametrize("name", ["model_c6_k2_t512", "model_c2_k3_t256", "model_c4_k2_t200", "model_c6_k2_t3840"])
def test_golden_case_stages(name, dev):
    from gpu_common import run_case, format_report, failures
    meta, params_np, g = load_golden_model(name)
    eng = _engine(meta["C"], meta["K"], dev)
    rep, _ = run_case(eng, params_np, g["x"], g["y"])
    print("\n" + format_report(rep))
    assert not failures(rep), format_report(rep)
    # and directly against the reference's own numbers (fp32 torch CPU)
    logits = eng.region("LOGITS", torch.float32, (meta["B"], meta["K"])).cpu().numpy()
    np.testing.assert_allclose(logits, g["train_logits"], rtol=2e-4, atol=5e-5)
    assert abs(float(eng.region("LOSS")[0]) - float(g["train_loss"])) < 2e-5
    gv = eng.named_param_views(eng.grads)
    for k, v in gv.items():
        ref_norm = float(g["gradnorm/" + k])
        got = float(v.double().norm())
        assert abs(got - ref_norm) <= 3e-3 * ref_norm + 1e-7, (k, got, ref_norm)


# kernel-form sets of the parity matrix: name -> (forward form, backward form)
#   "ws6"   = THE SHIPPED throughput selection (>= 192 batch tiles): wave-specialised forward gru_fwd_ws + gru_bwd_b6 for layer 0
#             (bulk waves recompute W_hn h + b_hn and stage x / h_prev) + gru_bwd_b3<128> for layer 1
#   "split" = THE SHIPPED latency selection (< 192 tiles): bulk projection + lean recurrence, split backward (seq4 + dx + dw)
#   "ws"    = gru_fwd_ws + the one-wave-per-SIMD software-pipelined backward gru_bwd_b4
#   "ws5"   = gru_fwd_ws + the two-waves-per-SIMD backward gru_bwd_b5 for layer 0 (chain waves + bulk waves)
#   "b3"    = throughput kernels of round 2, every contraction on split-bf16 MFMA (gru_fwd_b3; fused backward gru_bwd_b3 for both layers)
#   "fp32"  = throughput forward on fp32 MFMA (gru_fwd_seq) + gru_bwd_b3
FORMS = {"ws6": ("ws", "b6"), "split": ("split", "split"), "ws": ("ws", "b4"), "ws5": ("ws", "b5"), "b3": ("b3", "b3"), "fp32": ("fp32", "b3")}
SHIPPED, OTHER = ["ws6", "split"], ["ws", "ws5", "b3", "fp32"]
SHAPES = [(1, 6, 2, 256, 0.0), (17, 6, 2, 320, 0.0), (33, 3, 3, 256, 0.5),
          (16, 8, 2, 208, 0.5), (5, 1, 2, 136, 0.3), (40, 6, 2, 512, 0.5),
          (3, 5, 2, 250, 0.5), (2, 2, 2, 137, 0.0), (4, 16, 4, 264, 0.25),
          (2, 6, 2, 16, 0.5), (3, 4, 3, 40, 0.0),       # T' = 1 and T' = 3: one-step recurrences
          (3, 3, 2, 7680, 0.5), (2, 8, 2, 7680, 0.5),  # preprocess.py's RAW_FS = 128: 60 s = 7680 samples, 3 / all 8 chest channels
          (2, 6, 2, 3840, 0.5),                        # the default window: conv1_bwd cuts it into 8 one-chunk segments (7680: 8 x 2)
          (3100, 6, 2, 64, 0.5)]                        # 194 batch tiles, the last one ragged (12 rows)
# the non-default forms (selectable for diagnostics, not shipped as defaults) keep three representative shapes: ragged tiles with
# C < 4 and K = 3, the 3-tile case the negative controls use, and the many-tile case with a ragged last tile
REPRESENTATIVE = [(33, 3, 3, 256, 0.5), (40, 6, 2, 512, 0.5), (3100, 6, 2, 64, 0.5)]


# (the second 7680-sample shape differs from the first in the channel count only, i.e. in the front end: once, under the form the
#  real B = 64 training runs, is enough — each of these cases is ~18 s of fp64 oracle on the box's CPU)
# BASELINE configs[3], the channel-ablation sweep's shapes at the REAL window length: ECG-only / EDA-only (C = 1), wrist-only (2),
# chest-only (4) x 3840 samples, where conv1_fwd<C> / conv1_bwd<C> run their 8-segment path (round 4 met C = 1, 2, 4 at T <= 264 only)
ABLATION_SHAPES = [(2, 1, 2, 3840, 0.5), (2, 2, 2, 3840, 0.5), (2, 4, 2, 3840, 0.5)]
CASES = ([(*sh, f) for f in SHIPPED for sh in SHAPES if not (sh == (2, 8, 2, 7680, 0.5) and f == "ws6")] + [(*sh, f) for f in OTHER for sh in REPRESENTATIVE]
         + [(*sh, "split") for sh in ABLATION_SHAPES])


@pytest.mark.parametrize("B,C,K,T,p,form", CASES)
def test_random_shapes_with_dropout(B, C, K, T, p, dev, form, kernel_forms):
    """Every shape under both shipped form sets, three representative shapes under each of the others (round 3 ran the full
    15 x 7 cross product: 105 cases and most of the tier's 10 minutes; now 15 x 2 - 1 + 3 x 4 = 41), and the ablation sweep's
    channel counts at the full window length under the form they train in (3 cases)."""
    from gpu_common import run_case, format_report, failures
    kernel_forms(*FORMS[form])
    params = {k: v.numpy() for k, v in O.init_params(C, K, seed=100 + B).items()}
    rs = np.random.RandomState(B * 7 + T)
    x = (rs.randn(B, C, T) * (0.5 + rs.rand(1, C, 1)) + rs.randn(1, C, 1)).astype(np.float32)
    y = rs.randint(0, K, size=(B,)).astype(np.int64)
    eng = _engine(C, K, dev)
    rep, _ = run_case(eng, params, x, y, dropout_p=p, seed=1234, step=3, tag=form)
    print("\n" + format_report(rep))
    assert not failures(rep), format_report(rep)


@pytest.mark.parametrize("scale,form", [(2.0, "split"), (2.0, "ws6"), (1e-4, "split"), (0.0, "ws6")])
def test_two_piece_fp16_scales_follow_the_weights(scale, form, dev, kernel_forms):
    """The forward recurrences and the layer-1 projection run on two-piece fp16 (msig_dev.h f16x2): fp16's range holds because h is
    bounded and every weight fragment is scaled by a power of two taken from its own maximum.  GRU weights 2 x the initialisation
    (|w| up to 0.25: the fragments' scales drop an octave; from 6 x on the recurrence is chaotic — the fp32 oracle itself is 4e-3 away from
    the fp64 one in layer 0 — and the comparison says nothing), 1e-4 x (fragments that would be subnormal) and all-zero
    recurrent weights (the scale's fallback) against the fp64 oracle under both shipped form sets, at the usual tolerances."""
    from gpu_common import run_case, format_report, failures
    kernel_forms(*FORMS[form])
    B, C, K, T, p = 24, 6, 2, 400, 0.5
    params = {k: v.numpy().copy() for k, v in O.init_params(C, K, seed=77).items()}
    for k in params:
        if k.startswith("gru.weight_hh") or k.startswith("gru.weight_ih_l1"):
            params[k] = (params[k] * scale).astype(np.float32)
    rs = np.random.RandomState(5)
    x = (rs.randn(B, C, T) * (0.5 + rs.rand(1, C, 1)) + rs.randn(1, C, 1)).astype(np.float32)
    y = rs.randint(0, K, size=(B,)).astype(np.int64)
    eng = _engine(C, K, dev)
    rep, _ = run_case(eng, params, x, y, dropout_p=p, seed=99, step=2, tag=f"f16scale{scale}_{form}")
    print("\n" + format_report(rep))
    assert not failures(rep), format_report(rep)
    assert np.isfinite(eng.named_param_views(eng.grads)["gru.weight_hh_l0"].cpu().numpy()).all()


@pytest.mark.parametrize("B,C,K,T,p", [(3100, 6, 2, 960, 0.5),      # 194 tiles x T' = 60: the prefetch rings and the two-step dW pairing in steady state
                                      (4100, 3, 2, 160, 0.5)])     # 257 tiles (> the 256 / 128 persistent workgroups: accumulators carried
                                                                   # across a workgroup's tiles), ragged last tile (4 rows), T' = 10
def test_throughput_forms_many_tiles_against_oracle(B, C, K, T, p, dev):
    """Default kernel selection (>= 192 batch tiles: gru_fwd_ws for both layers, gru_bwd_b6 for layer 0, gru_bwd_b3<128> for layer 1)
    against the fp64 oracle at many tiles AND long sequences — the small-shape cases above reach these kernels only through the
    form override with one or two tiles."""
    from gpu_common import run_case, format_report, failures
    params = {k: v.numpy() for k, v in O.init_params(C, K, seed=100 + B).items()}
    rs = np.random.RandomState(B * 7 + T)
    x = (rs.randn(B, C, T) * (0.5 + rs.rand(1, C, 1)) + rs.randn(1, C, 1)).astype(np.float32)
    y = rs.randint(0, K, size=(B,)).astype(np.int64)
    eng = _engine(C, K, dev)
    rep, _ = run_case(eng, params, x, y, dropout_p=p, seed=1234, step=3)
    print("\n" + format_report(rep))
    assert not failures(rep), format_report(rep)


@pytest.mark.parametrize("form", ["ws", "ws5", "ws6", "b3", "split", "fp32"])
def test_step0_reads_this_launch_lds_images(form, dev, kernel_forms):
    """Regression for the LDS-initialisation race class (failure 2: gru_fwd_seq read bias_s / the weight images /
    the zeroed state tile in step 0 without a barrier after the prologue that writes them).  Such a read is masked whenever
    the CU's LDS still holds the identical image from the previous launch — which is what repeated launches with the same
    weights leave behind.  So: launch once with weights A, then check a launch with DIFFERENT weights B (large GRU biases,
    so a stale bias / weight / state image moves h_0 far beyond tolerance) against the oracle, for every recurrence kernel:
    gru_fwd_ws / gru_fwd_b3 / gru_fwd_seq / gru_fwd_rec forward, gru_bwd_b3 / gru_bwd_seq backward."""
    from gpu_common import run_case, format_report, failures
    kernel_forms(*FORMS[form])
    B, C, K, T = 37, 4, 2, 72          # 3 batch tiles (the last one ragged), T' = 5 (odd: also the unpaired last step of gru_bwd_b3)
    rs = np.random.RandomState(11)
    x = rs.randn(B, C, T).astype(np.float32)
    y = rs.randint(0, K, size=(B,)).astype(np.int64)
    eng = _engine(C, K, dev)
    for seed in (5, 6):                # A, then B
        params = {k: v.numpy().copy() for k, v in O.init_params(C, K, seed=seed).items()}
        r2 = np.random.RandomState(100 + seed)
        for k in params:
            if k.startswith("gru.bias"):
                params[k] = r2.uniform(-1.0, 1.0, size=params[k].shape).astype(np.float32)
        rep, _ = run_case(eng, params, x, y, dropout_p=0.25, seed=77, step=seed)
        assert not failures(rep), f"weights set {seed}:\n" + format_report(rep)


def test_eval_mode_matches_golden(dev):
    meta, params_np, g = load_golden_model("model_c6_k2_t512")
    eng = _engine(meta["C"], meta["K"], dev)
    eng.load_named({k: torch.as_tensor(v) for k, v in params_np.items()})
    before = eng.bn_state.clone()
    eng.forward(torch.as_tensor(g["x"]).to(dev), None, training=False)
    torch.cuda.synchronize()
    logits = eng.region("LOGITS", torch.float32, (meta["B"], meta["K"])).cpu().numpy()
    np.testing.assert_allclose(logits, g["eval_logits"], rtol=2e-4, atol=5e-5)
    assert torch.equal(before, eng.bn_state) and int(eng.bn_count.sum()) == int(g["param/cnn_encoder.1.num_batches_tracked"]) * 2
    probs = eng.region("PROBS", torch.float32, (meta["B"], meta["K"])).cpu().numpy()
    np.testing.assert_allclose(probs.sum(1), 1.0, rtol=1e-5)
    pred = eng.region("PRED", torch.int32, (meta["B"],)).cpu().numpy()
    assert (pred == g["eval_logits"].argmax(1)).all()


@pytest.mark.parametrize("name", ["model_c6_k2_t512", "model_c2_k3_t256"])
def test_three_fused_train_steps_match_reference(name, dev):
    meta, params_np, g = load_golden_model(name)
    eng = _engine(meta["C"], meta["K"], dev)
    eng.load_named({k: torch.as_tensor(v) for k, v in params_np.items()})
    x, y = torch.as_tensor(g["x"]).to(dev), torch.as_tensor(g["y"]).to(dev)
    for step in (1, 2, 3):
        eng.train_step(x, y, lr=1e-3, weight_decay=1e-4, step=step)
        torch.cuda.synchronize()
        assert abs(float(eng.region("LOSS")[0]) - float(g[f"loss_step{step}"])) < 1e-4, step
    pv = eng.named_param_views()
    for k, v in pv.items():
        ref = g["after3/" + k]
        if ref.size == 0:
            continue
        got = v.cpu().numpy()
        bad = np.abs(got - ref) > 3e-5 + 2e-3 * np.abs(ref)
        assert bad.mean() <= 5e-3 and np.abs(got - ref).max() <= 6e-3 + 3e-5, (k, bad.mean(), np.abs(got - ref).max())
    bv = eng.bn_views()
    for k in ("cnn_encoder.1.running_mean", "cnn_encoder.1.running_var", "cnn_encoder.5.running_mean", "cnn_encoder.5.running_var"):
        np.testing.assert_allclose(bv[k].cpu().numpy(), g["after3/" + k], rtol=1e-4, atol=1e-5)
    assert int(eng.bn_count[0]) == 3 + int(g["param/cnn_encoder.1.num_batches_tracked"])


def test_full_size_batch_properties(dev):
    """BASELINE.json's full size (B=8192, 6 ch, T=3840), checked through size-independent properties:
    a batch made of 64 distinct windows repeated 128x has the same BatchNorm statistics, the same mean
    loss and the same (mean-reduced) gradients as the 64-window batch, and every replica gets the same
    logits; and the fused train step is bitwise reproducible."""
    from multimodalsignal_amd.runtime import Engine
    C, K, T, B0, REP = 6, 2, 3840, 64, 128
    params = O.init_params(C, K, seed=77)
    rs = np.random.RandomState(5)
    x0 = torch.as_tensor((rs.randn(B0, C, T) * (0.5 + rs.rand(1, C, 1)) + rs.randn(1, C, 1)).astype(np.float32)).to(dev)
    y0 = torch.as_tensor(rs.randint(0, K, size=(B0,)).astype(np.int64)).to(dev)
    small, big = Engine(C, K, dev), Engine(C, K, dev)
    big.load_named(params)
    # the yardstick itself first: the 64-window run (latency-form kernels) against the fp64 oracle, stage by stage
    from gpu_common import run_case, format_report, failures
    rep, _ = run_case(small, {k: v.numpy() for k, v in params.items()}, x0.cpu().numpy(), y0.cpu().numpy())
    assert not failures(rep), format_report(rep)
    xb, yb = x0.repeat(REP, 1, 1).contiguous(), y0.repeat(REP).contiguous()
    bb = big.forward(xb, yb, training=True); big.backward(bb)
    torch.cuda.synchronize()
    l_s, l_b = float(small.region("LOSS")[0]), float(big.region("LOSS")[0])
    assert abs(l_s - l_b) <= 2e-6 * max(abs(l_s), 1.0)
    lg_s = small.region("LOGITS", torch.float32, (B0, K)).cpu().numpy()
    lg_b = big.region("LOGITS", torch.float32, (B0 * REP, K)).cpu().numpy().reshape(REP, B0, K)
    np.testing.assert_allclose(lg_b[0], lg_s, rtol=2e-4, atol=2e-5)
    assert (lg_b == lg_b[0:1]).all()                     # replicas are bit-identical (rows are independent)
    np.testing.assert_allclose(big.bn_state.cpu().numpy(), small.bn_state.cpu().numpy(), rtol=2e-5, atol=1e-6)
    gs, gb = small.named_param_views(small.grads), big.named_param_views(big.grads)
    for k in gs:
        a, b = gs[k].cpu().numpy(), gb[k].cpu().numpy()
        scale = max(np.abs(a).max(), 1e-12)
        assert np.abs(a - b).max() <= 2e-3 * scale, (k, np.abs(a - b).max() / scale)
    # determinism: the same fused step twice from the same state gives bit-identical weights
    e1, e2 = Engine(C, K, dev), Engine(C, K, dev)
    e1.load_named(params); e2.load_named(params)
    for e in (e1, e2):
        for step in (1, 2):
            e.train_step(xb, yb, lr=1e-3, weight_decay=1e-4, step=step, dropout_p=0.5, seed=3)
    torch.cuda.synchronize()
    assert torch.equal(e1.params, e2.params) and torch.equal(e1.bn_state, e2.bn_state)
    assert torch.isfinite(e1.params).all()


@pytest.mark.parametrize("B", [8, 272])
def test_train_step_captured_in_a_hip_graph_replays_identically(B, dev):
    """The library never synchronises or allocates: a whole train step can be captured into a
    hipGraph; replaying it from the same state gives bit-identical parameters to launching it directly."""
    from multimodalsignal_amd.runtime import Engine
    C, K, T = 6, 2, 256
    params = {k: v.numpy() for k, v in O.init_params(C, K, seed=5).items()}
    rs = np.random.RandomState(B)
    x = torch.from_numpy(rs.randn(B, C, T).astype(np.float32)).to(dev)
    y = torch.from_numpy(rs.randint(0, K, size=(B,)).astype(np.int64)).to(dev)

    def fresh():
        eng = Engine(C, K, dev)
        eng.load_named({k: torch.from_numpy(v) for k, v in params.items()})
        eng.ensure_adam_state()
        return eng

    kw = dict(lr=1e-3, weight_decay=1e-4, step=1, dropout_p=0.5, seed=11)
    direct = fresh()
    direct.train_step(x, y, **kw)
    torch.cuda.synchronize()
    graphed = fresh()
    graphed.workspace(B, T, True)                       # allocate outside the capture
    side = torch.cuda.Stream(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        graphed.train_step(x, y, **kw)
    torch.cuda.synchronize()
    before = graphed.params.clone()
    np.testing.assert_array_equal(before.cpu().numpy(), fresh().params.cpu().numpy())    # capture launched nothing
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(graphed.params.cpu().numpy(), direct.params.cpu().numpy())
    np.testing.assert_array_equal(graphed.exp_avg_sq.cpu().numpy(), direct.exp_avg_sq.cpu().numpy())
    assert float(graphed.region("LOSS")[0]) == float(direct.region("LOSS")[0])


@pytest.mark.parametrize("forms", [("ws", "b4"), ("ws", "b5"), ("ws", "b6"), ("ws", "b3"), ("split", "split"), ("auto", "auto")])
def test_fold_batch_train_step_against_oracle(forms, dev, kernel_forms):
    """msig_train_step_multi directly against the fp64 oracle: three folds x B = 64 with different weights, inputs and dropout
    streams in ONE set of launches (blockIdx.z = fold).  ("ws", "b3") are the FOLDS = true instantiations of the throughput-form
    GRU kernels, otherwise only compared with their own sequential runs; ("split", "split") the fold-aware latency forms; ("auto", "auto") what
    the LOSO driver's launches get (FoldArena pins form_folds = 1: gru_fwd_ws for layer 0, projection + recurrence for layer 1,
    latency backward)."""
    import ctypes as C
    from gpu_common import run_case, format_report, failures
    from multimodalsignal_amd import _lib as L
    from multimodalsignal_amd.runtime import FoldArena
    kernel_forms(*forms)
    NF, B, Cc, K, T, p, step = 3, 64, 6, 2, 512, 0.5, 2
    arena = FoldArena(Cc, K, dev, NF, B, T)
    engines, cases = [arena.engine(s) for s in range(NF)], []
    for f in range(NF):
        params = {k: v.numpy() for k, v in O.init_params(Cc, K, seed=300 + f).items()}
        rs = np.random.RandomState(40 + f)
        x = (rs.randn(B, Cc, T) * (0.5 + rs.rand(1, Cc, 1)) + rs.randn(1, Cc, 1)).astype(np.float32)
        y = rs.randint(0, K, size=(B,)).astype(np.int64)
        engines[f].load_named({k: torch.as_tensor(v) for k, v in params.items()})
        arena.view(f, "x", torch.float32)[:x.size].copy_(torch.as_tensor(x).reshape(-1))
        arena.view(f, "y", torch.int64)[:B].copy_(torch.as_tensor(y))
        engines[f].workspace(B, T, True)
        engines[f]._last = (B, T, True)
        cases.append((params, x, y, 1000 + f))
    m = arena.multi(list(range(NF)), key_gru=[L.dropout_key(c[3], step, 1) for c in cases],
                    key_head=[L.dropout_key(c[3], step, 2) for c in cases], lr=[1e-3] * NF, steps=[step, step + 5, step + 9])
    desc = arena.batch(B, True, p)
    done = []

    def launch(phase):
        if phase == "fwd" and not done:
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            L.check(L.lib().msig_train_step_multi(C.byref(desc), C.byref(m), arena.ptr("exp_avg"), arena.ptr("exp_avg_sq"),
                                                  0.9, 0.999, 1e-8, 1e-4, step, st), "msig_train_step_multi")
            done.append(1)

    before = [e.params.clone() for e in engines]
    for f in range(NF):
        params, x, y, seed = cases[f]
        rep, _ = run_case(engines[f], params, x, y, dropout_p=p, seed=seed, step=step, launch=launch, tag=f"multi{forms[1]}_{f}")
        assert not failures(rep), f"fold {f}:\n" + format_report(rep)
    # the Adam update of the same launch, per fold with ITS step count (msig_multi.step), from zero moments: m = 0.1 g', v = 0.001 g'^2
    # with g' = g + wd * p, p -= lr / bc1(step) * m / (sqrt(v) / sqrt(bc2(step)) + eps)
    for f in range(NF):
        g = engines[f].grads + 1e-4 * before[f]
        s = int(m.step[f])
        bc1, bc2 = 1 - 0.9 ** s, 1 - 0.999 ** s
        mm, vv = 0.1 * g, 0.001 * g * g
        want = before[f] - (1e-3 / bc1) * mm / (vv.sqrt() / bc2 ** 0.5 + 1e-8)
        np.testing.assert_allclose(engines[f].params.cpu().numpy(), want.cpu().numpy(), rtol=2e-5, atol=2e-7, err_msg=f"fold {f}")


@pytest.mark.parametrize("NF,B", [(0, 64), (0, 24), (3, 64), (9, 64)])
def test_forward_forms_are_bit_identical(NF, B, dev, kernel_forms):
    """The library chooses the forward GRU form per layer and per LAUNCH (layer 0 gru_fwd_ws, layer 1 projection + recurrence
    below 32 tiles per launch and gru_fwd_ws from there on): a fold's numbers may depend on neither its companions nor the
    grouping, so the forms must agree in every bit — logits of an evaluation pass, and parameters, gradients, BatchNorm state
    and loss accumulator after two training steps with dropout, under `split`, `ws` and the automatic mix.  NF = 0: a
    stand-alone model (the FOLDS = false kernels), a full and a ragged batch; NF = 3 / 9: fold batches of 12 tiles (the mix
    runs layer 1 in the latency form) and of 36 (gru_fwd_ws for both layers).  The backward form is the latency form throughout."""
    import ctypes as C
    from multimodalsignal_amd import _lib as L
    from multimodalsignal_amd.runtime import FoldArena
    Cc, K, T, p = 6, 2, 512, 0.5
    n = max(NF, 1)
    rs = np.random.RandomState(5 + NF)
    xs = [(rs.randn(B, Cc, T) * (0.5 + rs.rand(1, Cc, 1))).astype(np.float32) for _ in range(n)]
    ys = [rs.randint(0, K, size=(B,)).astype(np.int64) for _ in range(n)]

    def run(fwd):
        kernel_forms(fwd, "split")
        out = {}
        if NF == 0:
            eng = _engine(Cc, K, dev)
            eng.load_named({k: v for k, v in O.init_params(Cc, K, seed=77).items()})
            x, y = torch.as_tensor(xs[0]).to(dev), torch.as_tensor(ys[0]).to(dev)
            eng.forward(x, y, training=False)
            out["logits"] = eng.region("LOGITS", shape=(B, K)).clone()
            for step in (1, 2):
                eng.train_step(x, y, 1e-3, weight_decay=1e-4, step=step, dropout_p=p, seed=9)
            out.update(params=eng.params.clone(), grads=eng.grads.clone(), bn=eng.bn_state.clone())
        else:
            arena = FoldArena(Cc, K, dev, NF, B, T)
            for f in range(NF):
                e = arena.engine(f)
                e.load_named({k: v for k, v in O.init_params(Cc, K, seed=77 + f).items()})
                arena.view(f, "x", torch.float32)[:xs[f].size].copy_(torch.as_tensor(xs[f]).reshape(-1))
                arena.view(f, "y", torch.int64)[:B].copy_(torch.as_tensor(ys[f]))
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            m = arena.multi(list(range(NF)), key_gru=[11 + f for f in range(NF)], key_head=[31 + f for f in range(NF)], lr=[1e-3] * NF)
            L.check(L.lib().msig_forward_multi(C.byref(arena.batch(B, False, 0.0)), C.byref(m), st), "msig_forward_multi")
            logits = []
            for f in range(NF):
                e = arena.engine(f)
                e.workspace(B, T, False)
                e._last = (B, T, False)
                logits.append(e.region("LOGITS", shape=(B, K)).clone())
            out["logits"] = torch.stack(logits)
            desc = arena.batch(B, True, p)
            for step in (1, 2):
                L.check(L.lib().msig_train_step_multi(C.byref(desc), C.byref(m), arena.ptr("exp_avg"), arena.ptr("exp_avg_sq"),
                                                      0.9, 0.999, 1e-8, 1e-4, step, st), "msig_train_step_multi")
            for k in ("params", "grads", "bn_state", "acc"):
                out[k] = torch.stack([arena.view(f, k, torch.int32).clone() for f in range(NF)])
        torch.cuda.synchronize()
        return out

    ref = run("split")
    assert float(ref["grads"].view(torch.float32).abs().max()) > 0 and float(ref["logits"].abs().max()) > 0
    for other in ("ws", "auto"):
        got = run(other)
        for k in ref:
            a, b = ref[k].contiguous().view(torch.int32), got[k].contiguous().view(torch.int32)
            assert torch.equal(a, b), f"{other} vs split: {k}: {int((a != b).sum())} of {a.numel()} words differ"


def test_eval_logits_do_not_depend_on_the_batching(dev):
    """EVAL_BATCH_SIZE rests on this: an evaluation pass gives every window the same logits, bit for bit,
    whatever batch it arrives in — 3100 windows at once (194 batch tiles: gru_fwd_ws for both layers), in batches of 1024 (64 tiles:
    gru_fwd_ws), 640 (40 tiles), 64 (4 tiles: layer 1 as projection + recurrence) or 50 (ragged tiles)."""
    Cc, K, T, N = 6, 2, 128, 3100
    eng = _engine(Cc, K, dev)
    eng.load_named({k: v for k, v in O.init_params(Cc, K, seed=5).items()})
    eng.bn_state.copy_(torch.rand_like(eng.bn_state) + 0.5)            # running statistics that are not the initial 0 / 1
    rs = np.random.RandomState(3)
    x = torch.as_tensor((rs.randn(N, Cc, T) * (0.5 + rs.rand(1, Cc, 1))).astype(np.float32)).to(dev)
    eng.forward(x, None, training=False)
    whole = eng.region("LOGITS", shape=(N, K)).clone()
    assert float(whole.abs().max()) > 0
    for bs in (1024, 640, 64, 50):
        parts = []
        for i in range(0, N, bs):
            eng.forward(x[i:i + bs].contiguous(), None, training=False)
            parts.append(eng.region("LOGITS", shape=(min(bs, N - i), K)).clone())
        got = torch.cat(parts)
        assert torch.equal(whole.view(torch.int32), got.view(torch.int32)), \
            f"batches of {bs}: {int((whole.view(torch.int32) != got.view(torch.int32)).sum())} of {whole.numel()} logits differ"


def test_train_steps_do_not_depend_on_what_else_runs_on_the_gpu(dev):
    """Launches of a step carry riders — layer 1's dW beside layer 0's chains, the loss sums beside the weight-gradient reduction —
    and a rider that read what another workgroup of its launch writes would make the step's bits a matter of timing (round 5 built one
    such: HISTORY.md section 10).  Eight fused train steps of a fold batch (two folds, C = 6: the gate MLP is live) from the same state,
    alone and beside two other streams that run their own fold batches to shift every launch's timing: every parameter, moment,
    gradient, BatchNorm statistic and loss sum agrees in every bit."""
    import ctypes as C
    import threading
    from multimodalsignal_amd import _lib as L
    from multimodalsignal_amd.runtime import FoldArena
    NF, B, Cc, K, T = 2, 64, 6, 2, 768

    def make(seed):
        torch.manual_seed(seed)
        ar = FoldArena(Cc, K, dev, NF, B, T)
        for f in range(NF):
            ar.engine(f).load_named({k: v for k, v in O.init_params(Cc, K, seed=seed + f).items()})
            ar.view(f, "x", torch.float32).normal_()
            ar.view(f, "y", torch.int64).random_(0, K)
        return ar

    def run(ar, n, stream):
        m = ar.multi(list(range(NF)), key_gru=[5, 6], key_head=[7, 8], lr=[1e-3] * NF)
        desc = ar.batch(B, True, 0.5)
        st = C.c_void_p(stream.cuda_stream)
        for k in range(n):
            L.check(L.lib().msig_train_step_multi(C.byref(desc), C.byref(m), ar.ptr("exp_avg"), ar.ptr("exp_avg_sq"), 0.9, 0.999, 1e-8, 1e-4, k + 1, st),
                    "msig_train_step_multi")
        stream.synchronize()

    def state(ar):
        return {k: torch.stack([ar.view(f, k, torch.int32).clone() for f in range(NF)]) for k in ("params", "grads", "exp_avg", "exp_avg_sq", "bn_state", "acc")}

    alone = make(40)
    run(alone, 8, torch.cuda.Stream(dev))
    want = state(alone)
    for trial in range(3):
        busy = make(40)
        others = [make(90 + 10 * i) for i in range(2)]
        ths = [threading.Thread(target=run, args=(o, 24, torch.cuda.Stream(dev))) for o in others]
        for t in ths:
            t.start()
        run(busy, 8, torch.cuda.Stream(dev))
        for t in ths:
            t.join()
        got = state(busy)
        for k in want:
            assert torch.equal(want[k], got[k]), f"trial {trial}: {k}: {int((want[k] != got[k]).sum())} of {want[k].numel()} words differ"


def test_fold_batch_rejects_an_unsupported_form_before_any_launch(dev, kernel_forms):
    """A fold batch runs the latency form and gru_fwd_ws only.  A descriptor that names another forward form (here gru_fwd_b3) is
    refused with MSIG_E_FORM by the argument checks of msig_train_step_multi / msig_forward_multi — BEFORE the first launch: the
    BatchNorm running statistics, the step counters and the weights are untouched (round 4 returned the code from the GRU launcher,
    after the front end had already run)."""
    import ctypes as C
    from multimodalsignal_amd import _lib as L
    from multimodalsignal_amd.runtime import FoldArena
    kernel_forms("auto", "auto")
    arena = FoldArena(6, 2, dev, 2, 64, 256)
    for s_ in range(2):
        e = arena.engine(s_)
        e.params.normal_(0, 0.05)
        arena.view(s_, "x", torch.float32).normal_()
        arena.view(s_, "y", torch.int64).random_(0, 2)
    m = arena.multi([0, 1], [1, 2], [3, 4], [1e-3, 1e-3], steps=[1, 1])
    desc = arena.batch(64, True, 0.5)
    L.apply_forms(desc, fwd="b3", bwd="b3")
    torch.cuda.synchronize()
    before = arena.mem.clone()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = L.lib().msig_train_step_multi(C.byref(desc), C.byref(m), arena.ptr("exp_avg"), arena.ptr("exp_avg_sq"), 0.9, 0.999, 1e-8, 1e-4, 1, st)
    rc2 = L.lib().msig_forward_multi(C.byref(desc), C.byref(m), st)
    torch.cuda.synchronize()
    assert rc == -5 and rc2 == -5                                      # MSIG_E_FORM
    assert torch.equal(arena.mem, before)                              # not one byte of any arena has changed: nothing was launched
    L.apply_forms(desc, fwd="ws", bwd="b6")                            # a form fold batches do run: accepted
    L.check(L.lib().msig_train_step_multi(C.byref(desc), C.byref(m), arena.ptr("exp_avg"), arena.ptr("exp_avg_sq"), 0.9, 0.999, 1e-8, 1e-4, 1, st), "ws/b6")
    torch.cuda.synchronize()
    assert not torch.equal(arena.view(0, "bn_state", torch.float32), before[0].view(torch.uint8)[arena.off["bn_state"][0]:arena.off["bn_state"][0] + arena.off["bn_state"][1]].view(torch.float32))


@pytest.mark.parametrize("Cc", [6, 3, 16, 7, 13])      # 7: an instantiation of its own (Cr = 1); 13: the generic form, Cr = 3
def test_channel_attention_forward_standalone(Cc, dev):
    """ChannelAttention.forward on its own (models.py:24-31; msig_channel_attention) against the oracle's gate, C < 4 included
    (empty hidden layer: the gate is 0.5 everywhere)."""
    from multimodalsignal_amd.models import ChannelAttention
    torch.manual_seed(3)
    ca = ChannelAttention(Cc).to(dev)
    rs = np.random.RandomState(Cc)
    x = torch.as_tensor((rs.randn(5, Cc, 250) * 2 + 0.3).astype(np.float32))
    with torch.no_grad():
        got = ca(x.to(dev)).cpu()
    w1, w2 = ca.fc[0].weight.detach().cpu().double(), ca.fc[2].weight.detach().cpu().double()
    mean = x.double().mean(dim=2)
    s = torch.sigmoid(torch.relu(mean @ w1.T) @ w2.T) if Cc >= 4 else torch.full((5, Cc), 0.5, dtype=torch.float64)
    want = x.double() * s[:, :, None]
    assert float((got.double() - want).abs().max() / want.abs().max()) <= 2e-6
    with pytest.raises(RuntimeError, match="inference-only"):
        ca(x.to(dev).requires_grad_(True))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ca(x)


def test_one_layer_32_unit_model(dev):
    """The hierarchical experiment's second model (main.py:35-40: gru_hidden_size=32, gru_num_layers=1) — run EMBEDDED in the
    64-unit kernels (runtime.EmbeddedEngine, msig_batch.gru_layers = 1) — against the imported reference's recorded numbers
    (tests/golden/model_m2_c3_k2_t512.npz) and the fp64 oracle: eval logits, train logits / loss / every gradient through autograd,
    three fused train steps, and the padding of the embedding staying exactly zero."""
    from multimodalsignal_amd.models import CnnGruAttentionModel
    meta, params_np, g = load_golden_model("model_m2_c3_k2_t512")
    sd = {k: torch.as_tensor(v) for k, v in params_np.items()}
    x, y = torch.as_tensor(g["x"]).to(dev), torch.as_tensor(g["y"]).to(dev)

    def fresh():
        m = CnnGruAttentionModel(meta["C"], meta["K"], gru_hidden_size=32, gru_num_layers=1, dropout=0.0)
        assert list(m.state_dict().keys()) == list(sd.keys()) and all(tuple(v.shape) == tuple(sd[k].shape) for k, v in m.state_dict().items())
        m.load_state_dict(sd)
        return m.to(dev)

    m = fresh().eval()
    with torch.no_grad():
        np.testing.assert_allclose(m(x).cpu().numpy(), g["eval_logits"], rtol=2e-4, atol=5e-5)
    m.train()
    logits = m(x)
    loss = torch.nn.CrossEntropyLoss()(logits, y)
    loss.backward()
    np.testing.assert_allclose(logits.detach().cpu().numpy(), g["train_logits"], rtol=2e-4, atol=5e-5)
    assert abs(float(loss) - float(g["train_loss"])) < 2e-5
    # gradients: against the fp64 oracle (tolerance as for the reference configuration: gpu_common.grad_tol)
    from gpu_common import grad_tol, rel_err, split_named, to_t
    p64, b64 = split_named(to_t(params_np, torch.float64))
    p32, b32 = split_named(to_t(params_np))
    _, g64, _, _ = O.loss_and_grads(p64, b64, x.cpu().double(), y.cpu())
    _, g32, _, _ = O.loss_and_grads(p32, b32, x.cpu(), y.cpu())
    for k, p in m.named_parameters():
        if p.numel():
            own = rel_err(g32[k].numpy(), g64[k].numpy())
            assert rel_err(p.grad.cpu().numpy(), g64[k].numpy()) <= grad_tol(k, own), (k, own)
            ref = g["grad/" + k]
            np.testing.assert_allclose(p.grad.cpu().numpy(), ref, rtol=3e-3, atol=3e-4 * max(np.abs(ref).max(), 1e-6), err_msg=k)
    # three fused steps (zero_grad + forward + CE + backward + Adam), as the reference's loop recorded them
    m2 = fresh().train()
    eng = m2.engine()
    for step in (1, 2, 3):
        eng.train_step(x, y, lr=1e-3, weight_decay=1e-4, step=step)
        torch.cuda.synchronize()
        assert abs(float(eng.region("LOSS")[0]) - float(g[f"loss_step{step}"])) < 1e-4, step
    for k, v in m2.state_dict().items():
        ref = g["after3/" + k]
        if ref.size == 0 or "num_batches" in k:
            continue
        got = v.cpu().numpy()
        bad = np.abs(got - ref) > 3e-5 + 2e-3 * np.abs(ref)
        assert bad.mean() <= 5e-3 and np.abs(got - ref).max() <= 6e-3 + 3e-5, (k, bad.mean(), np.abs(got - ref).max())
    # the embedding's padding (units 32..63 of every gate, layer 1, the unused feature columns) is exactly zero, still
    pad = torch.ones_like(eng.params, dtype=torch.bool)
    pad[eng.index] = False
    assert pad.any() and not eng.params[pad].any()


def _case(B, C, K, T, seed):
    params = {k: v.numpy() for k, v in O.init_params(C, K, seed=seed).items()}
    rs = np.random.RandomState(seed)
    x = (rs.randn(B, C, T) * (0.5 + rs.rand(1, C, 1)) + rs.randn(1, C, 1)).astype(np.float32)
    y = rs.randint(0, K, size=(B,)).astype(np.int64)
    return params, x, y


@pytest.mark.parametrize("fwd_bwd,then", [(("ws", "b6"), "b3"), (("ws", "b6"), "split"), (("ws", "b3"), "b6"), (("split", "split"), "b6")])
def test_any_backward_form_may_follow_any_forward_call(fwd_bwd, then, dev):
    """The stash contract of ABI 4 (include/msig.h): msig_forward and msig_backward are two calls with two descriptors, so the
    forward pass writes the THREE-vector stash whatever backward form its descriptor names — a caller that changes the form in
    between (round 3: a process-global switch; silently wrong gradients under b6 -> b3) gets correct gradients.  Checked against
    the fp64 oracle stage by stage, the backward pass running under `then`."""
    from gpu_common import run_case, format_report, failures
    from multimodalsignal_amd import _lib as L
    B, C, K, T = 40, 6, 2, 512
    params, x, y = _case(B, C, K, T, 41)
    eng = _engine(C, K, dev)
    eng.load_named({k: torch.as_tensor(v) for k, v in params.items()})
    box = {}

    def launch(phase):
        if phase == "fwd":
            L.set_kernel_form(*fwd_bwd)
            try:
                box["b"] = eng.forward(torch.as_tensor(x).to(dev), torch.as_tensor(y).to(dev), training=True, dropout_p=0.5, seed=9, step=2)
            finally:
                L.set_kernel_form("auto", "auto")
        else:
            b = box["b"]
            assert b.bwd_form == L.BWD_FORMS[fwd_bwd[1]] + 1
            L.apply_forms(b, fwd_bwd[0], then)                    # the SAME workspace, another backward form
            eng.backward(b)

    rep, _ = run_case(eng, params, x, y, dropout_p=0.5, seed=9, step=2, launch=launch, tag=f"{fwd_bwd[1]}->{then}")
    assert not failures(rep), format_report(rep)


def test_gru_layers_zero_means_two(dev):
    """msig_batch.gru_layers: 0 and 2 both mean the reference's two-layer GRU (a zero-initialised descriptor carries 0) — same
    kernel forms, same stash, bit-identical step (round 3 took the two-vector stash only for == 2)."""
    import ctypes as Ct
    from multimodalsignal_amd import _lib as L
    B, C, K, T = 24, 6, 2, 256
    params, x, y = _case(B, C, K, T, 17)
    xd, yd = torch.as_tensor(x).to(dev), torch.as_tensor(y).to(dev)
    out = []
    for layers in (2, 0):
        eng = _engine(C, K, dev)
        eng.load_named({k: torch.as_tensor(v) for k, v in params.items()})
        eng.ensure_adam_state()
        eng.gru_layers = layers
        L.set_kernel_form("ws", "b6")
        try:
            eng.train_step(xd, yd, lr=1e-3, weight_decay=1e-4, step=1, dropout_p=0.5, seed=5)
        finally:
            L.set_kernel_form("auto", "auto")
        torch.cuda.synchronize()
        out.append((eng.params.clone(), eng.grads.clone(), float(eng.region("LOSS")[0])))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]


def test_maxpool_exact_ties_take_the_first_candidate(dev):
    """MaxPool's tie rule (nn.MaxPool1d: the FIRST maximum of a window receives the gradient, models.py:49,53) on constructed
    EXACT ties, checked without the near-tie adoption of run_case.  Windows 0-2 hold signals of period 2 in time: conv1 has stride
    2, so every interior output position of a window sees the same samples and computes bit-identical values — in the oracle and
    in the kernels alike (the same products in the same order) — and all three candidates of every interior pooling window tie,
    in stage 1 and (p1 being constant in time) in stage 2.  Windows 3-5 are ordinary noise, so that the BatchNorm statistics are
    not degenerate."""
    from gpu_common import run_case, format_report, failures
    B, C, K, T = 6, 6, 2, 256
    params, x, y = _case(B, C, K, T, 23)
    rs = np.random.RandomState(1)
    even, odd = rs.randn(3, C, 1).astype(np.float32), rs.randn(3, C, 1).astype(np.float32)
    x[:3, :, 0::2] = even
    x[:3, :, 1::2] = odd
    eng = _engine(C, K, dev)
    rep, _ = run_case(eng, params, x, y, dropout_p=0.0, adopt=False, tag="exact_ties")
    assert rep["pool_near_ties_adopted"][0] == 0
    assert not failures(rep), format_report(rep)
    # the decisions themselves: in the tied windows every interior pooling window with a positive value recorded candidate 0 (left);
    # 3 = nothing positive (the first / last positions see the convolutions' zero padding and do not tie)
    L1, P1, L2, TP = O.stage_lengths(T)
    for name, P, CH in (("POOLC1", P1, 16), ("POOLC2", TP, 32)):
        code = eng.region(name, torch.uint8, (B, P, CH // 4)).cpu().numpy()
        win = ((code[:, :, :, None] >> (2 * np.arange(4, dtype=np.uint8))[None, None, None, :]) & 3).reshape(B, P, CH)
        interior = win[:3, 2:P - 2, :]
        assert set(np.unique(interior)) <= {0, 3}, (name, np.unique(interior, return_counts=True))
        assert (interior == 0).any()
        assert not (win[:, 0, :] == 0).any()                         # position 0: the left candidate is the -inf padding, it never wins
        assert {1, 2} & set(np.unique(win[3:, 2:P - 2, :]))          # the noise windows do use the other candidates


@pytest.mark.parametrize("form", ["split", "ws6"])
def test_one_layer_model_with_dropout_against_oracle(form, dev, kernel_forms):
    """The hierarchical experiment's second model as its driver runs it: dropout 0.5 (main.py:39) — classifier dropout on the
    64-wide hidden layer, no inter-layer GRU dropout (one layer: layer 0's upstream gradient must NOT be masked) — against the
    fp64 oracle with the same counter-based masks, under the latency forms and the shipped throughput forms."""
    from gpu_common import grad_tol, rel_err, split_named, to_t
    from multimodalsignal_amd.models import CnnGruAttentionModel
    kernel_forms(*FORMS[form])
    B, C, K, T, seed = 21, 3, 2, 320, 77
    torch.manual_seed(5)
    m = CnnGruAttentionModel(C, K, gru_hidden_size=32, gru_num_layers=1, dropout=0.5).to(dev).train()
    m.set_dropout_seed(seed)
    rs = np.random.RandomState(3)
    x = torch.as_tensor((rs.randn(B, C, T) * 1.5 + 0.2).astype(np.float32))
    y = torch.as_tensor(rs.randint(0, K, size=(B,)).astype(np.int64))
    named = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    logits = m(x.to(dev))
    loss = torch.nn.CrossEntropyLoss()(logits, y.to(dev))
    loss.backward()
    p64, b64 = split_named(to_t(named, torch.float64))
    p32, b32 = split_named(to_t(named))
    fw = dict(dropout_p=0.5, seed=seed, step=1)                       # the first training forward of the model is step 1
    l64, g64, st64, _ = O.loss_and_grads(p64, b64, x.double(), y, **fw)
    _, g32, _, _ = O.loss_and_grads(p32, b32, x, y, **fw)
    assert float((st64["cls_hidden"] == 0).double().mean()) > 0.3       # the mask is active in the oracle
    assert rel_err(logits.detach().cpu().numpy(), st64["logits"].detach().numpy()) <= 3.5e-5
    assert abs(float(loss) - float(l64)) <= 6e-6 * max(abs(float(l64)), 1e-6)
    for k, p in m.named_parameters():
        if p.numel():
            own = rel_err(g32[k].numpy(), g64[k].numpy())
            assert rel_err(p.grad.cpu().numpy(), g64[k].numpy()) <= grad_tol(k, own), (k, own)


@pytest.mark.parametrize("B,form", [(24, "split"), (64, "split"), (40, "ws6"), (300, "split"), (2048, "split"), (2060, "split")])
def test_fused_step_equals_separate_calls_bit_for_bit(B, form, dev, kernel_forms):
    """msig_train_step takes shortcuts that the separate calls (msig_forward with labels, msig_backward, msig_adam_step) do not —
    under gru_bwd_b6 the two-vector stash with W_hn h recomputed, every weight-gradient reduction and Adam in one launch, and up to
    2048 windows (128 groups of 16 rows; 2060 is the first size past it) the classifier's forward, CrossEntropy and backward as
    ONE launch with the loss summed in the step's last one — built from the same arithmetic: losses, the head's outputs and
    gradients are bit-identical (and so is the first update)."""
    kernel_forms(*FORMS[form])
    fused_equals_separate_calls(B, 6, 2, 384, (1, 2), dev)


def fused_equals_separate_calls(B, C, K, T, steps, dev, resync=False):
    """The comparison of test_fused_step_equals_separate_calls_bit_for_bit at one shape over `steps` (the kernel forms are the caller's).
    resync: after a step's comparisons the separate engine takes over the fused one's parameters and moments, so that the NEXT step
    starts from one state again and can be compared bit for bit too — without it the last-bit differences of the second update make
    every later forward differ."""
    from multimodalsignal_amd.runtime import Engine
    params, x, y = _case(B, C, K, T, 300 + B)
    xd, yd = torch.as_tensor(x).to(dev), torch.as_tensor(y).to(dev)
    fused, apart = Engine(C, K, dev), Engine(C, K, dev)
    for e in (fused, apart):
        e.load_named({k: torch.as_tensor(v) for k, v in params.items()})
        e.ensure_adam_state()
    for step in steps:
        fused.train_step(xd, yd, lr=1e-3, weight_decay=1e-4, step=step, dropout_p=0.5, seed=21)
        b = apart.forward(xd, yd, training=True, dropout_p=0.5, seed=21, step=step)
        apart.backward(b)
        apart.adam_step(1e-3, weight_decay=1e-4, step=step)
        torch.cuda.synchronize()
        assert float(fused.region("LOSS")[0]) == float(apart.region("LOSS")[0]), step
        assert torch.equal(fused.region("LOSS")[:3], apart.region("LOSS")[:3]), step                 # mean loss, summed loss, #correct
        for name, n, dt in (("HID", B * 64, torch.float32), ("LOGITS", B * K, torch.float32), ("PROBS", B * K, torch.float32),
                            ("DLOGITS", B * K, torch.float32), ("PRED", B, torch.int32), ("DFEAT", B * 128, torch.float32)):
            assert torch.equal(fused.region(name, dt)[:n], apart.region(name, dt)[:n]), (step, name)
        gf, ga = fused.named_param_views(fused.grads), apart.named_param_views(apart.grads)
        bad = {k: float((gf[k] - ga[k]).abs().max()) for k in gf if not torch.equal(gf[k], ga[k])}
        assert not bad, (step, "gradients differ", bad)
        # the update itself: the fused reduction + Adam launch and the stand-alone adam kernel are two compilations of the same
        # expression, which contract their multiply-adds differently from the second step on (m, v != 0): last-bit differences
        np.testing.assert_allclose(fused.params.cpu().numpy(), apart.params.cpu().numpy(), rtol=3e-7, atol=2e-9)
        if step == 1:
            assert torch.equal(fused.params, apart.params)
        assert torch.equal(fused.bn_state, apart.bn_state), step
        if resync:
            for name in ("params", "exp_avg", "exp_avg_sq"):
                getattr(apart, name).copy_(getattr(fused, name))
    assert torch.equal(fused.loss_acc, apart.loss_acc) and float(fused.loss_acc[0]) > 0          # msig_batch.loss_acc: both steps' summed losses
