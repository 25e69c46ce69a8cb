"""GPU tier: the HIP path against the fp64 oracle over BATCH SIZES (tests/batch_sizes.py; DESIGN.md "Batch sizes").

Every other parity test meets the batch size at a handful of hand-picked values: ragged last tiles of 1, 2, 3, 4, 5, 8, 12 and 16
rows, 194 and 257 batch tiles but never 191 or 192, and no pair of neighbouring batches across any of the launchers' switches.  Here a
two-tile batch runs with every row count 1 .. 15 in its last tile under both shipped form sets, one ragged tile with the row counts
the suite never had, and the fused train step on both sides of every predicate batch_sizes.paths() restates — with the side a
case took ASSERTED from the kernels the call launched (msig_profile_report) wherever the side changes a kernel name; grid caps
and strides that change no name rest on paths(), which tests/test_batch_sizes_host.py holds.  The tolerances are the project's own,
unchanged (gpu_common.stage_tol / grad_tol, OWN_CAP, run_case's cap of 8 adopted near-ties); the cases and seeds are batch_sizes'
tables, which the host file holds, with the oracle alone, to: `own` <= OWN_CAP, a live gate MLP, at most 8 fp32 / fp64 pooling
disagreements, each side of every predicate reached.  Negative controls: make negctl BATCH=k, tools/negative_controls.sh batch,
profiles/batch_negative_control.log."""
import ctypes as Ct

import numpy as np
import pytest
import torch

import batch_sizes as BS
from oracle import cnn_gru_oracle as O
from test_trained_regimes_gpu import OWN_CAP, oracle_stages64, run_case_own
from test_window_lengths_gpu import FORM_PAIRS, check_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tier needs an MI355X"
    return torch.device("cuda:0")


@pytest.fixture
def kernel_forms():
    from multimodalsignal_amd import _lib as L
    yield L.set_kernel_form
    L.set_kernel_form("auto", "auto")


@pytest.fixture
def launched():
    """Records the kernels launched while the test runs: launched() -> {kernel name: launches}."""
    from multimodalsignal_amd import _lib as L
    torch.cuda.synchronize()
    L.profile_enable(True)
    try:
        yield lambda: {k: v[0] for k, v in L.profile_report().items()}
    finally:
        L.profile_enable(False)


def assert_side(names, p, call, n_folds=1):
    want, never = BS.expected_kernels(p, call, n_folds)
    assert want <= set(names) and not (never & set(names)), (sorted(want - set(names)), sorted(never & set(names)), sorted(names))


def stage_case(case, table, call, dev, kernel_forms, launched, monkeypatch, tmp_path):
    """One case through msig_forward + msig_backward (call "fb") or through the fused train step (call "step")."""
    from multimodalsignal_amd.runtime import Engine
    kernel_forms(*FORM_PAIRS[case.form])
    params, x, y = BS.build_case(case)
    eng = Engine(case.C, case.K, dev)
    launch = None
    if call == "step":
        eng.load_named({k: torch.as_tensor(v) for k, v in params.items()})
        xd, yd = torch.as_tensor(x).to(dev), torch.as_tensor(y).to(dev)

        def launch(phase):
            if phase == "fwd":
                eng.train_step(xd, yd, 1e-3, step=BS.FW["step"], dropout_p=case.p, seed=BS.FW["seed"])

    rep, ref, own = run_case_own(monkeypatch, tmp_path, eng, params, x, y, launch=launch, tag=f"batch_{table}_{case.form}", dropout_p=case.p, **BS.FW)
    names = launched()
    check_case(eng, rep, ref, own)
    assert_side(names, BS.paths(case.B, case.T, form=case.form), call)


@pytest.mark.parametrize("case", BS.RESIDUES, ids=BS.case_id)
def test_every_row_count_of_a_ragged_last_tile_against_oracle(case, dev, kernel_forms, launched, monkeypatch, tmp_path):
    """B = 17 .. 31: a full tile and a tile of 1 .. 15 rows, T' = 5, under both shipped form sets.  The padding rows of the last tile are
    clamped copies of row B - 1 in every GRU kernel and must add nothing to dW, db or dX."""
    assert BS.paths(case.B, case.T).nt == 2
    stage_case(case, "residue", "fb", dev, kernel_forms, launched, monkeypatch, tmp_path)


@pytest.mark.parametrize("case", BS.SINGLES, ids=BS.case_id)
def test_one_ragged_tile_against_oracle(case, dev, kernel_forms, launched, monkeypatch, tmp_path):
    """B = 6, 7, 9, 10, 11, 13, 14, 15 under the default selection, six channels: the row counts of ONE tile that no other parity
    test has."""
    assert BS.paths(case.B, case.T).nt == 1
    stage_case(case, "single", "fb", dev, kernel_forms, launched, monkeypatch, tmp_path)


@pytest.mark.parametrize("case", BS.STRADDLES, ids=BS.case_id)
def test_train_step_on_both_sides_of_every_switch_against_oracle(case, dev, kernel_forms, launched, monkeypatch, tmp_path):
    """Neighbouring batch sizes across every predicate of batch_sizes.paths() through Engine.train_step: stages, loss, running
    statistics and every gradient of the step against the oracle, and the side taken from the kernels it launched.  The cases of a
    group are prefixes of one another, so a failure on one side and a pass on the other names the branch."""
    stage_case(case, "straddle", "step", dev, kernel_forms, launched, monkeypatch, tmp_path)


@pytest.mark.parametrize("B", BS.FOLD_BATCHES)
def test_fold_batch_across_the_fused_backward_threshold_against_oracle(B, dev, kernel_forms, launched, monkeypatch, tmp_path):
    """ONE msig_train_step_multi over three folds with msig_multi.form_folds = 3 (built as
    test_window_lengths_gpu.test_fold_batch_at_an_unaligned_length_against_oracle builds its launch): 9 tiles per launch at B = 48
    (the latency form), 12 at B = 49 (gru_bwd_b6 / gru_bwd_b3 in their fold instantiation, the last row alone in its tile).  The
    folds differ in parameters, inputs and dropout seeds, and every fold is held to the oracle."""
    from multimodalsignal_amd import _lib as L
    from multimodalsignal_amd.runtime import FoldArena
    kernel_forms("auto", "auto")
    Cc, K, T, p, step, NF = BS.FOLD_C, BS.FOLD_K, BS.FOLD_T, BS.FOLD_P, BS.FOLD_STEP, len(BS.FOLD_CASES)
    arena = FoldArena(Cc, K, dev, NF, B, T)
    engines, cases = [arena.engine(s) for s in range(NF)], []
    for f in range(NF):
        params, x, y, seed = BS.fold_case(B, f)
        engines[f].load_named({k: torch.as_tensor(v) for k, v in params.items()})
        arena.view(f, "x", torch.float32)[:x.size].copy_(torch.as_tensor(x).reshape(-1))
        arena.view(f, "y", torch.int64)[:B].copy_(torch.as_tensor(y))
        engines[f].workspace(B, T, True)
        engines[f]._last = (B, T, True)
        cases.append((params, x, y, seed))
    m = arena.multi(list(range(NF)), key_gru=[L.dropout_key(c[3], step, 1) for c in cases],
                    key_head=[L.dropout_key(c[3], step, 2) for c in cases], lr=[1e-3] * NF, steps=[step] * NF)
    m.form_folds = NF                        # the backward form of the LAUNCH: nt x 3 crosses MSIG_FOLD_TILES between 48 and 49
    desc = arena.batch(B, True, p)
    done = []

    def launch(phase):
        if phase == "fwd" and not done:
            st = Ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            L.check(L.lib().msig_train_step_multi(Ct.byref(desc), Ct.byref(m), arena.ptr("exp_avg"), arena.ptr("exp_avg_sq"),
                                                  0.9, 0.999, 1e-8, 1e-4, step, st), "msig_train_step_multi")
            done.append(1)

    for f, (params, x, y, seed) in enumerate(cases):
        rep, ref, own = run_case_own(monkeypatch, tmp_path, engines[f], params, x, y, launch=launch, tag=f"batch_multi_{B}",
                                     dropout_p=p, seed=seed, step=step)
        if f == 0:
            names = launched()
        check_case(engines[f], rep, ref, own)
    assert_side(names, BS.paths(B, T, n_folds=NF, form_folds=NF), "step", NF)


@pytest.mark.parametrize("i", range(len(BS.EVAL_CASES)), ids=[str(c[0]) for c in BS.EVAL_CASES])
def test_eval_mode_logits_against_oracle(i, dev, launched):
    """Engine.forward(training=False) at B = 2049 (129 tiles), 3057 (192 tiles, the last row alone: the throughput forward) and 31 with
    running statistics that are no golden file's own against the fp64 oracle's eval-mode logits; bn_state and bn_count are untouched."""
    from gpu_common import rel_err, split_named, stage_tol, to_t
    from multimodalsignal_amd.runtime import Engine
    params, x = BS.eval_case(i)
    B, C, T = x.shape
    K = params["classifier.3.weight"].shape[0]
    ref = oracle_stages64(params, x, training=False)["logits"]
    p32, b32 = split_named(to_t(params))
    with torch.no_grad():
        st32, _ = O.forward(p32, {**O.init_buffers(), **b32}, torch.as_tensor(x), training=False)
    own = rel_err(st32["logits"].numpy(), ref)
    assert own <= OWN_CAP, own
    eng = Engine(C, K, dev)
    eng.load_named({k: torch.as_tensor(v) for k, v in params.items()})
    before, count = eng.bn_state.clone(), eng.bn_count.clone()
    assert float(before[:16].abs().min()) == 3.0 and float(before[16:32].min()) == pytest.approx(min(BS.EVAL_VARS))      # the statistics did load
    eng.forward(torch.as_tensor(x).to(dev), None, training=False)
    torch.cuda.synchronize()
    names = launched()
    got = eng.region("LOGITS", torch.float32, (B, K)).cpu().numpy()
    err, tol = rel_err(got, ref), stage_tol("logits", own)
    print(f"eval logits err={err:.3e} tol={tol:.1e} own={own:.2e}")
    assert np.isfinite(got).all() and err <= tol, (err, tol, own)
    assert torch.equal(before, eng.bn_state) and torch.equal(count, eng.bn_count)
    p = BS.paths(B, T)
    assert ("gru_fwd_ws_l1" in names) == p.l1_ws and ("gru_fwd_rec_l1" in names) == (not p.l1_ws) and "softmax" in names and "ce" not in names
