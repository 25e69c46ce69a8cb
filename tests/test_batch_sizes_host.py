"""CPU tier: what keeps tests/test_batch_sizes_gpu.py honest, from the oracle alone (tests/batch_sizes.py; DESIGN.md "Batch sizes").

  1. For every case of every table: every `own` — the fp32 oracle's disagreement with the fp64 oracle, which the GPU tolerances scale —
     is at most OWN_CAP; the fp32 and the fp64 oracle disagree on at most MAX_ADOPTED pooling decisions (gpu_common.run_case's cap on
     adopted near-ties); at C >= 4 both channel_attention gradients are non-zero in fp64 and the gate MLP's pre-activations are far
     enough from ReLU's kink (window_lengths.gate_kink); no pooling window's maximum lies within the fp32 oracle's own error of zero
     (batch_sizes.pool_kink; one group is exempt, batch_sizes.KINK_EXEMPT says why).  These are conditions on the cases, not measurements of the HIP path.
  2. Coverage, from batch_sizes.paths() over the tables: a case on each side of every predicate paths() knows, a ragged last tile of
     every row count 1 .. 15, every straddle group on both sides of the predicates it exists for and a prefix chain in x, y and
     parameters.  A later edit cannot quietly drop a side.
  3. paths() itself at a few hand-computed shapes."""
import numpy as np
import pytest

import batch_sizes as BS
from input_regimes import oracle_report
from oracle import cnn_gru_oracle as O
from test_trained_regimes_gpu import OWN_CAP
from test_window_lengths_host import MAX_ADOPTED, _assert_case, _unique

STAGE = BS.RESIDUES + BS.SINGLES + BS.STRADDLES


def _assert_off_the_kink(params, x, **fw):
    for stage, (n, top, err0) in BS.pool_kink(params, x, **fw).items():
        assert n == 0, f"{stage}: {n} pooling windows whose maximum is within the fp32 oracle's error near zero ({err0:.1e}); the smallest is {top:.1e}"


# ---- 1. conditioning ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", _unique(STAGE), ids=BS.case_id)
def test_stage_cases_are_well_conditioned_and_live(case):
    params, x, y = BS.build_case(case)
    own, st64, g64, flips = oracle_report(params, x, y, dropout_p=case.p, **BS.FW)
    _assert_case(own, g64, flips, case.C, named=params, st64=st64)
    if case._replace(form="auto") not in [c._replace(form="auto") for g in BS.KINK_EXEMPT for c in BS.STRADDLE_GROUPS[g]]:
        _assert_off_the_kink(params, x, dropout_p=case.p, **BS.FW)


@pytest.mark.parametrize("B", BS.FOLD_BATCHES)
@pytest.mark.parametrize("f", range(len(BS.FOLD_CASES)))
def test_fold_cases_are_well_conditioned(f, B):
    params, x, y, seed = BS.fold_case(B, f)
    own, st64, g64, flips = oracle_report(params, x, y, dropout_p=BS.FOLD_P, seed=seed, step=BS.FOLD_STEP)
    _assert_case(own, g64, flips, BS.FOLD_C, named=params, st64=st64)
    _assert_off_the_kink(params, x, dropout_p=BS.FOLD_P, seed=seed, step=BS.FOLD_STEP)


@pytest.mark.parametrize("i", range(len(BS.EVAL_CASES)), ids=[str(c[0]) for c in BS.EVAL_CASES])
def test_eval_cases_are_well_conditioned(i):
    params, x = BS.eval_case(i)
    own, _, _, flips = oracle_report(params, x, np.zeros(len(x), dtype=np.int64), training=False)
    assert own["logits"] <= OWN_CAP, own
    assert flips <= MAX_ADOPTED


# ---- 2. coverage -------------------------------------------------------------------------------------------------------------------------
def _all_paths():
    ps = [BS.paths(c.B, c.T, form=c.form) for c in STAGE]
    NF = len(BS.FOLD_CASES)
    ps += [BS.paths(B, BS.FOLD_T, n_folds=NF, form_folds=NF) for B in BS.FOLD_BATCHES]
    return ps


def test_tables_reach_each_side_of_every_predicate():
    ps = _all_paths()
    sides = {"ws_only": (False, True), "l1_ws": (False, True), "fused_bwd": (False, True), "dw_capped": (False, True), "dw_units_max": (8, 9),
             "rec_exclusive": (True, False), "proj_capped": (False, True), "dx_capped": (False, True), "dxdw_l0_capped": (False, True),
             "gru_rows_capped": (False, True), "fused_l0_rounds": (1, 2), "fused_l1_rounds": (1, 2), "whole_window": (False, True),
             "conv1_bwd_capped": (False, True), "fin_capped": (False, True), "conv1_fwd_capped": (False, True),
             "conv2_fwd_capped": (False, True), "bn2_pass1_capped": (False, True), "conv2_bwd_capped": (False, True),
             "head_fused": (True, False), "head_bwd_rounds": (1, 2), "ce_passes": (1, 2)}
    assert set(sides) == set(BS.Paths._fields) - {"nt", "last_rows", "units", "seg"}, "a predicate of paths() without a coverage claim"
    for field, (lo, hi) in sides.items():
        seen = {getattr(p, field) for p in ps}
        assert lo in seen and hi in seen, (field, seen)
    assert {p.seg for p in ps} >= {1, 2, 5}
    assert {p.ce_passes for p in ps} >= {1, 2, 3, 4, 5}
    # conv1_bwd's cap both with whole-window items (B >= 256) and with segments (B < 256)
    assert {(p.whole_window, p.conv1_bwd_capped) for p in ps} >= {(True, False), (True, True), (False, False), (False, True)}


def test_every_row_count_of_a_ragged_last_tile():
    for form in ("ws6", "split"):
        rows = {BS.paths(c.B, c.T, form=c.form).last_rows for c in BS.RESIDUES if c.form == form}
        assert rows == set(range(1, 16)), (form, rows)
    assert all(BS.paths(c.B, c.T).nt == 2 for c in BS.RESIDUES)
    single = {BS.paths(c.B, c.T).last_rows for c in BS.SINGLES}
    assert single == {6, 7, 9, 10, 11, 13, 14, 15} and all(BS.paths(c.B, c.T).nt == 1 for c in BS.SINGLES)
    assert O.stage_lengths(BS.RESIDUE_T)[-1] == 5 and O.stage_lengths(BS.SINGLE_T)[-1] == 5
    # the fused backward, the throughput forward and the fold batch each meet a tile whose last row is alone
    assert any(p.fused_bwd and p.ws_only and p.last_rows == 1 and p.nt == 192 for p in _all_paths())
    NF = len(BS.FOLD_CASES)
    lo, hi = (BS.paths(B, BS.FOLD_T, n_folds=NF, form_folds=NF) for B in BS.FOLD_BATCHES)
    assert (lo.nt * NF, lo.fused_bwd, hi.nt * NF, hi.fused_bwd, hi.last_rows) == (9, False, 12, True, 1)
    assert not BS.paths(BS.FOLD_BATCHES[1], BS.FOLD_T, n_folds=NF, form_folds=1).fused_bwd       # only form_folds crosses MSIG_FOLD_TILES


def test_straddle_groups_cross_their_predicates_as_prefix_chains():
    assert set(BS.STRADDLE_GROUPS) == set(BS.STRADDLE_PREDICATES)
    for name, group in BS.STRADDLE_GROUPS.items():
        assert [c.B for c in group] == sorted(c.B for c in group) and len({(c.C, c.K, c.T, c.form, c.pseed, c.xseed) for c in group}) == 1, name
        ps = [BS.paths(c.B, c.T, form=c.form) for c in group]
        for field, lo, hi in BS.STRADDLE_PREDICATES[name]:
            vals = [getattr(p, field) for p in ps]
            k = vals.index(hi)
            assert k > 0 and all(v == lo for v in vals[:k]) and all(v != lo for v in vals[k:]), (name, field, vals)
        if any(p.last_rows == 1 for p in ps) and len(group) > 2:
            assert any(p.last_rows == 16 for p in ps), name
        big = BS.build_case(group[-1])
        for c in group[:-1]:
            params, x, y = BS.build_case(c)
            assert x.shape[0] == c.B and np.array_equal(x, big[1][:c.B]) and np.array_equal(y, big[2][:c.B]), (name, c.B)
            assert all(np.array_equal(v, big[0][k]) for k, v in params.items()), (name, c.B)
    for B in BS.FOLD_BATCHES[:-1]:
        for f in range(len(BS.FOLD_CASES)):
            a, b = BS.fold_case(B, f), BS.fold_case(BS.FOLD_BATCHES[-1], f)
            assert np.array_equal(a[1], b[1][:B]) and np.array_equal(a[2], b[2][:B]) and a[3] == b[3]
            assert all(np.array_equal(v, b[0][k]) for k, v in a[0].items())


def test_expected_kernels_follow_the_paths():
    want, never = BS.expected_kernels(BS.paths(3057, 64), "step")
    assert {"gru_fwd_ws_l1", "gru_bwd_b6_l0", "gru_bwd_b3_l1", "head_fwd", "ce", "head_bwd"} <= want and "head_step" in never
    want, never = BS.expected_kernels(BS.paths(496, 64), "step")
    assert {"gru_fwd_proj_l1", "gru_fwd_rec_l1", "gru_bwd_seq4_l0+dw_l1", "gru_bwd_dxdw_l0", "head_step"} <= want
    assert {"gru_fwd_ws_l1", "gru_bwd_b6_l0", "ce"} <= never
    want, never = BS.expected_kernels(BS.paths(496, 64), "fb")
    assert "head_step" in never and {"head_fwd", "ce", "head_bwd"} <= want


# ---- 3. paths() --------------------------------------------------------------------------------------------------------------------------
def test_paths_restate_the_launchers_predicates():
    p = BS.paths(64, 3840)                                   # the reference's batch: 4 tiles x 240 steps
    assert (p.nt, p.last_rows, p.units, p.ws_only, p.l1_ws, p.fused_bwd) == (4, 16, 960, False, False, False)
    assert (p.dw_capped, p.dw_units_max, p.proj_capped, p.dx_capped, p.rec_exclusive, p.seg) == (False, 8, True, True, True, 8)
    p = BS.paths(3100, 64)                                   # 194 tiles, the last with 12 rows
    assert (p.nt, p.last_rows, p.ws_only, p.fused_bwd, p.fused_l0_rounds, p.fused_l1_rounds, p.dw_capped) == (194, 12, True, True, 2, 1, None)
    assert (p.head_fused, p.head_bwd_rounds, p.ce_passes, p.fin_capped) == (False, 2, 4, True)
    assert BS.paths(3057, 64).nt == 192 and BS.paths(3056, 64).nt == 191 and BS.paths(3057, 64).last_rows == 1
    assert BS.paths(2048, 64).head_fused and not BS.paths(2049, 64).head_fused
    assert BS.paths(3100, 64, form="split").fused_bwd is False and BS.paths(3100, 64, form="split").rec_exclusive is None
    assert BS.paths(24, 256, form="ws6").fused_bwd and BS.paths(24, 256, form="ws6").l1_ws
    assert BS.paths(64, 256, n_folds=15).l1_ws and not BS.paths(64, 256, n_folds=15).fused_bwd and BS.paths(64, 256, n_folds=15, form_folds=15).fused_bwd
