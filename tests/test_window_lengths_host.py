"""CPU tier: what keeps tests/test_window_lengths_gpu.py honest, from the oracle alone (tests/window_lengths.py; DESIGN.md "Window lengths").

  1. The oracle is right at unaligned lengths: in fp64 it equals oracle/cpu_model.CpuCnnGru — the stock torch.nn layers — on the logits
     and every parameter gradient to 1e-12, at every T of the tables and every T in 16..47 (the golden vectors are all at multiples of 8).
  2. For every case of every table: every `own` — the fp32 oracle's disagreement with the fp64 oracle, which the GPU tolerances scale —
     is at most OWN_CAP; the fp32 and the fp64 oracle disagree on at most MAX_ADOPTED pooling decisions (gpu_common.run_case's cap on
     adopted near-ties); at C >= 4 both channel_attention gradients are non-zero in fp64 and the gate MLP's pre-activations are far
     enough from ReLU's kink that their fp32 rounding alone cannot move dW2 by half its tolerance (window_lengths.gate_kink).
  3. Coverage, from window_lengths.paths() over the tables: a later edit cannot quietly drop a path."""
import numpy as np
import pytest
import torch

import window_lengths as WL
from gpu_common import rel_err
from input_regimes import oracle_report
from oracle import cnn_gru_oracle as O
from test_trained_regimes_gpu import OWN_CAP

MAX_ADOPTED = 8
TABLE_T = sorted({c.T for c in WL.RESIDUES + WL.CROSSINGS + WL.SHORT} | {WL.FOLD_SHAPE[3], WL.EVAL_CASE[3], WL.CNN_GRU_CASE[3]}
                 | {c[2] for c in WL.XGRAD_CASES})
STOCK_T = sorted(set(TABLE_T) | set(range(16, 48)))


def _unique(cases):
    """The cases without their kernel form: the oracle has none."""
    return sorted({c._replace(form="-") for c in cases})


def _assert_case(own, g64, flips, C, gated=True, named=None, st64=None):
    over = {k: v for k, v in own.items() if not (v <= OWN_CAP)}
    assert not over, f"the fp32 oracle's own error exceeds {OWN_CAP}: {over}"
    if gated and C >= 4 and g64:
        for k in ("channel_attention.fc.0.weight", "channel_attention.fc.2.weight"):
            assert float(np.abs(g64[k]).max()) > 0, f"the gate MLP is dead: the oracle's gradient of {k} is exactly zero"
        kink, margin = WL.gate_kink(named, st64, g64.get("stage/gate_s"))
        assert kink <= WL.KINK_MAX, f"rounding the gate MLP's pre-activations alone moves dW2 by {kink:.1e} of its largest element"
        assert margin > 1.0, f"a pre-activation of the gate MLP is within fp32 rounding of zero (|a| / bound = {margin:.2f})"
    assert flips <= MAX_ADOPTED, f"the fp32 and the fp64 oracle disagree on {flips} pooling decisions"


# ---- 1. the oracle against stock torch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", STOCK_T)
def test_oracle_equals_stock_torch_layers_in_fp64(T):
    from oracle.cpu_model import CpuCnnGru
    B, C, K = 2, 6, 2
    named = O.init_params(C, K, seed=WL.pseed(C), dtype=torch.float64)
    x, y = WL.base_input(B, C, K, T, 7 * B + T)
    xt, yt = torch.as_tensor(x).double(), torch.as_tensor(y)
    m = CpuCnnGru(C, K, dropout=0.0).double().train()
    missing, unexpected = m.load_state_dict(named, strict=False)
    assert not unexpected and all("running" in k or "num_batches" in k for k in missing)
    with torch.no_grad():
        assert m.cnn_encoder(xt).shape[2] == O.stage_lengths(T)[-1]
    logits = m(xt)
    torch.nn.CrossEntropyLoss()(logits, yt).backward()
    _, g, st, _ = O.loss_and_grads(dict(named), O.init_buffers(torch.float64), xt, yt)
    assert rel_err(st["logits"].detach().numpy(), logits.detach().numpy()) <= 1e-12
    stock = dict(m.named_parameters())
    assert set(stock) == set(g)
    for k, v in g.items():
        if v.numel():
            assert rel_err(v.numpy(), stock[k].grad.numpy()) <= 1e-12, k


# ---- 2. conditioning ---------------------------------------------------------------------------------------------------------------------
def test_tables_state_the_stage_lengths():
    for T, lengths in WL.CROSSING_LENGTHS.items():
        assert O.stage_lengths(T) == lengths, T
    assert sorted({c.T for c in WL.CROSSINGS}) == sorted(WL.CROSSING_LENGTHS)
    for T, tp in WL.SHORT_T.items():
        assert O.stage_lengths(T)[-1] == tp, T
    for c in WL.RESIDUES:
        assert WL.paths(c.B, c.C, c.T).n1 == 1


@pytest.mark.parametrize("case", _unique(WL.RESIDUES + WL.CROSSINGS + WL.SHORT), ids=WL.case_id)
def test_stage_cases_are_well_conditioned_and_live(case):
    params, x, y = WL.build_case(case)
    own, st64, g64, flips = oracle_report(params, x, y, dropout_p=case.p, **WL.FW)
    _assert_case(own, g64, flips, case.C, named=params, st64=st64)


@pytest.mark.parametrize("f", range(len(WL.FOLD_CASES)))
def test_fold_cases_are_well_conditioned_and_live(f):
    params, x, y, seed = WL.fold_case(f)
    own, st64, g64, flips = oracle_report(params, x, y, dropout_p=WL.FOLD_SHAPE[4], seed=seed, step=WL.FOLD_STEP)
    _assert_case(own, g64, flips, WL.FOLD_SHAPE[1], named=params, st64=st64)


def test_eval_case_is_well_conditioned():
    params, x = WL.eval_case()
    own, _, _, flips = oracle_report(params, x, np.zeros(len(x), dtype=np.int64), training=False)
    assert own["logits"] <= OWN_CAP, own
    assert flips <= MAX_ADOPTED


def _module_report(named, x, y, training, fw):
    import test_input_grad_gpu as IG
    dx64, g64, st64 = IG._oracle(named, x, y, torch.float64, training, fw)
    choice = {"pool" + k[-1]: O.first_argmax(O.pool_windows(torch.clamp_min(st64[k].detach(), 0))) for k in ("bn1", "bn2")}
    dx32, g32, st32 = IG._oracle(named, x, y, torch.float32, training, fw, pool_choice=choice)
    own = {k: rel_err(st32[k].detach().numpy(), st64[k].detach().numpy()) for k in ("conv1", "pool1", "pool2", "feat", "logits")}
    own.update({"grad/" + k: rel_err(g32[k].numpy(), g64[k].numpy()) for k in g64 if g64[k].numel()})
    own["grad/x"] = rel_err(dx32.numpy(), dx64.numpy())
    _, _, free32 = IG._oracle(named, x, y, torch.float32, training, fw)
    flips = sum(int((O.first_argmax(O.pool_windows(torch.clamp_min(free32[k].detach(), 0))) != choice["pool" + k[-1]]).sum()) for k in ("bn1", "bn2"))
    return own, {k: v.numpy() for k, v in g64.items()}, flips, {k: v.detach().numpy() for k, v in st64.items()}


@pytest.mark.parametrize("B,C,T,training,mseed", WL.XGRAD_CASES, ids=[f"{c[2]}-{'train' if c[3] else 'eval'}" for c in WL.XGRAD_CASES])
def test_input_gradient_cases_are_well_conditioned_and_live(B, C, T, training, mseed):
    named, x, y = WL.module_case("cnn_gru_attention", B, C, WL.xgrad_classes(C, B), T, mseed, 10 * C + B)
    fw = dict(dropout_p=0.5, seed=1000 + C, step=1) if training else dict(dropout_p=0.0, seed=0, step=0)
    own, g64, flips, st64 = _module_report(named, x, y, training, fw)
    _assert_case(own, g64, flips, C, named={k: v.numpy() for k, v in named.items()}, st64=st64)


def test_cnn_gru_case_is_well_conditioned(monkeypatch):
    B, C, K, T = WL.CNN_GRU_CASE
    monkeypatch.setattr(O, "channel_gate", lambda x_, W1, W2: (x_.mean(dim=2), torch.zeros(x_.shape[0], 0, dtype=x_.dtype),
                                                                torch.ones(x_.shape[0], x_.shape[1], dtype=x_.dtype)))
    named, x, y = WL.module_case("cnn_gru", B, C, K, T, C + T, 7 * B + T)
    own, g64, flips, _ = _module_report(named, x, y, True, dict(dropout_p=0.5, seed=31, step=1))
    _assert_case(own, g64, flips, C, gated=False)


# ---- 3. coverage -------------------------------------------------------------------------------------------------------------------------
def test_tables_reach_every_path():
    stage = WL.RESIDUES + WL.CROSSINGS + WL.SHORT
    assert {c.T % 16 for c in stage} == set(range(16))
    assert {c.T % 16 for c in WL.RESIDUES if c.C == 6} == set(range(16))
    ps = [(c, WL.paths(c.B, c.C, c.T)) for c in stage]
    wanted = {"an unaligned second conv1 chunk": lambda c, p: not p.x_vec and p.n1 >= 2,
              "T % 8 == 4 at a compile-time channel count, two chunks": lambda c, p: p.x_vec and not p.bwd_pipe and c.C <= 8 and p.n1 >= 2,
              "an unaligned second conv2 chunk": lambda c, p: not p.x_vec and p.n2 >= 2,
              "segments of more than one chunk off the prefetch path": lambda c, p: p.seg > 1 and p.cps > 1 and not p.bwd_pipe,
              "whole-window items off the prefetch path": lambda c, p: c.B >= 256 and not p.bwd_pipe and p.n1 >= 2,
              "the generic instantiation at an unaligned multi-chunk length": lambda c, p: c.C > 8 and not p.x_vec and p.n1 >= 2,
              "the generic instantiation at T % 8 == 4": lambda c, p: c.C > 8 and c.T % 8 == 4}
    for what, pred in wanted.items():
        assert any(pred(c, p) for c, p in ps), what
    dx = {(p.dx_quads, p.dx_pair_store) for B, C, T, training, _ in WL.XGRAD_CASES if training
          for p in [WL.paths(B, C, T)] if -(-O.stage_lengths(T)[0] // 256) >= 2}
    assert {(False, False), (False, True), (True, False)} <= dx, dx
    assert any(not training for *_, training, _ in WL.XGRAD_CASES)
    assert sorted({O.stage_lengths(c.T)[-1] for c in WL.SHORT}) == [2, 5, 6, 7, 8]
    assert {c.form for c in WL.SHORT} == {"ws6", "split"} and all(c.B == 33 and c.C == 3 and c.K == 3 for c in WL.SHORT)
    for shape in (WL.FOLD_SHAPE[:4], WL.EVAL_CASE[:4], WL.CNN_GRU_CASE):
        p = WL.paths(shape[0], shape[1], shape[3])
        assert not p.x_vec and p.n1 >= 2 and p.n2 >= 2, shape


def test_paths_restate_the_kernels_predicates():
    p = WL.paths(2, 6, 3840)
    assert p == WL.Paths(True, True, True, True, True, 8, 4, 1, 8)              # the default window: 8 one-chunk segments
    assert WL.paths(2, 6, 7680)[-2:] == (2, 8) and WL.paths(256, 6, 7680)[-2:] == (15, 1)
    assert WL.paths(2, 9, 512).fwd_pipe is False and WL.paths(2, 9, 512).bwd_pipe is False
    assert WL.paths(2, 2, 4100)[5:] == (9, 5, 2, 5) and WL.paths(2, 3, 2100)[5:] == (5, 3, 1, 5)
    p = WL.paths(2, 6, 516)
    assert p.x_vec and p.fwd_pipe and not p.bwd_pipe and not p.dx_quads and p.dx_pair_store and p.n1 == 2
    assert WL.paths(2, 6, 8).bwd_pipe is False                                   # L1 = 4 < 8
