"""CPU tier: the hierarchical experiment's fold batches — one-layer models in lockstep, the embedding of the one-layer model in
the padded arena layout, and the wave / budget bookkeeping of the fold-batch drivers."""
from types import SimpleNamespace

import pytest
import torch

from multimodalsignal_amd import _lib as L
from multimodalsignal_amd.main import MAX_TRAIN_STREAMS, cap_waves, chunk_schedule, rank_units
from multimodalsignal_amd.models import CnnGruAttentionModel
from multimodalsignal_amd.multifold import lockstep_compatible
from multimodalsignal_amd.runtime import embedding_index
from multimodalsignal_amd.waves import deal


def _prep(model, store, bs=64, epochs=10, patience=5):
    ld = lambda b: SimpleNamespace(batch_size=b, store=store)
    return {"model": model, "loaders": (ld(bs), ld(bs), ld(bs)),
            "config": {"trainer": {"epochs": epochs, "early_stopping": {"patience": patience}}}}


def test_lockstep_compatible_accepts_one_layer_folds_and_rejects_mixed_depths():
    store = torch.zeros(4, 3, 8)
    m2 = [CnnGruAttentionModel(3, 2, gru_hidden_size=32, gru_num_layers=1) for _ in range(3)]
    m1 = CnnGruAttentionModel(3, 2)
    assert lockstep_compatible([_prep(m, store) for m in m2])
    assert lockstep_compatible([_prep(m1, store)])
    assert not lockstep_compatible([_prep(m2[0], store), _prep(m1, store)])
    assert not lockstep_compatible([_prep(m1, store), _prep(m2[0], store)])
    assert not lockstep_compatible([_prep(m2[0], store), _prep(m2[1], torch.zeros(4, 3, 8))])     # another store


def test_embedding_index_round_trips_a_reference_m2_state_dict():
    Cin, K = 3, 2
    torch.manual_seed(0)
    m2 = CnnGruAttentionModel(Cin, K, gru_hidden_size=32, gru_num_layers=1)
    sd = m2.state_dict()
    shapes, index = embedding_index(Cin, K)
    assert [k for k, _ in shapes] == [k for k in L.PARAM_KEYS if "_l1" not in k]
    assert all(tuple(sd[k].shape) == tuple(s) for k, s in shapes)
    layout, pshapes = L.param_layout(Cin, K), L.param_shapes(Cin, K)
    assert index.numel() == len(set(index.tolist())) and int(index.max()) < layout[-1]
    small = torch.cat([sd[k].reshape(-1) for k, _ in shapes])
    flat = torch.zeros(layout[-1])
    flat[index] = small                                                    # scatter
    assert torch.equal(flat[index], small)                                 # gather: bit for bit
    back, at = {}, 0
    for k, s in shapes:
        n = int(torch.tensor(s).prod())
        back[k] = flat[index][at:at + n].view(s)
        at += n
    for k in back:
        assert torch.equal(back[k], sd[k]), k
    # the padding: unit u of gate g at row g * 64 + u of a 64-unit tensor, nothing else; layer 1 holds nothing
    i = L.PARAM_KEYS.index("gru.weight_hh_l0_reverse")
    whh = flat[layout[i]:layout[i + 1]].view(pshapes[i])
    assert torch.equal(whh[64:96, :32], sd["gru.weight_hh_l0_reverse"][32:64]) and not whh[32:64].any() and not whh[:, 32:].any()
    j = L.PARAM_KEYS.index("gru.weight_ih_l1")
    assert not flat[layout[j]:layout[L.PARAM_KEYS.index("classifier.0.weight")]].any()
    c0 = L.PARAM_KEYS.index("classifier.0.weight")
    w = flat[layout[c0]:layout[c0 + 1]].view(pshapes[c0])
    assert torch.equal(w[:, 64:96], sd["classifier.0.weight"][:, 32:]) and not w[:, 32:64].any() and not w[:, 96:].any()


def test_cap_waves_spills_into_the_next_wave():
    assert cap_waves([[1, 2, 3]]) == [[1, 2, 3]]
    assert cap_waves([list(range(9)), [9]], cap=4) == [[0, 1, 2, 3], [4, 5, 6, 7], [8], [9]]
    waves = cap_waves([list(range(2 * MAX_TRAIN_STREAMS + 1))])
    assert all(len(w) <= MAX_TRAIN_STREAMS for w in waves) and sum(waves, []) == list(range(2 * MAX_TRAIN_STREAMS + 1))


def test_chunk_schedule_comes_from_the_chunks_own_trainers():
    m = CnnGruAttentionModel(3, 2)
    store = torch.zeros(1)
    assert chunk_schedule([_prep(m, store, epochs=30, patience=7), _prep(m, store, epochs=30, patience=3)]) == (30, 3)
    assert chunk_schedule([_prep(m, store, epochs=0, patience=4)]) == (0, 4)


# ---- the deal: which units share a fold batch, which batches run side by side (waves.deal: data -> data) ----
def _simple_deal(n_cfgs, n_folds, world=1, rank=0, concurrent_folds=15, lockstep_groups=4):
    """The deal of run_experiments: units numbered fold-major, configuration-minor, dealt to the ranks by folds_for_rank."""
    cfgs = {f"c{i}": {"subjects": [f"S{k}" for k in range(n_folds)]} for i in range(n_cfgs)}
    _, mine, groups = rank_units(cfgs, world, rank)
    return deal(groups, mine, concurrent_folds, lockstep_groups, sweep=len(groups) > 1)


def _hier_deal(n_folds, world=1, rank=0, concurrent_folds=15, lockstep_groups=4):
    """The deal of run_hierarchical_experiment: units (fold, model), the two models the groups that train side by side."""
    mine = list(range(rank, n_folds, world))
    return deal([[(k, tag) for k in mine] for tag in ("m1", "m2")], mine, concurrent_folds, lockstep_groups, fold_of=lambda u: u[0])


def _m(tag, folds):
    return [(k, tag) for k in folds]


def test_deal_of_one_configuration():
    assert _simple_deal(1, 15) == [[[0, 4, 8, 12], [1, 5, 9, 13], [2, 6, 10, 14], [3, 7, 11]]]
    assert _simple_deal(1, 15, world=2, rank=1) == [[[1, 7, 13], [3, 9], [5, 11]]]
    assert _simple_deal(1, 15, concurrent_folds=4) == [[[0, 2], [1, 3]], [[4, 6], [5, 7]], [[8, 10], [9, 11]], [[12, 13, 14]]]
    assert _simple_deal(1, 6, lockstep_groups=3) == [[[0, 3], [1, 4], [2, 5]]]
    assert _simple_deal(1, 6, lockstep_groups=1) == [[[0, 1, 2, 3, 4, 5]]]
    assert _simple_deal(1, 3) == [[[0, 1, 2]]]
    assert _simple_deal(1, 1) == [[[0]]]


def test_deal_of_a_sweep_is_one_batch_per_configuration():
    assert _simple_deal(4, 15) == [[list(range(c, 60, 4)) for c in range(4)]]
    assert _simple_deal(8, 5) == [[list(range(c, 40, 8)) for c in range(4)], [list(range(c, 40, 8)) for c in range(4, 8)]]
    assert _simple_deal(2, 20) == [[list(range(0, 32, 2)), [32, 34, 36, 38], list(range(1, 33, 2)), [33, 35, 37, 39]]]
    assert _simple_deal(4, 15, concurrent_folds=2) == _simple_deal(4, 15)          # a sweep ignores concurrent_folds


def test_deal_of_the_hierarchical_models():
    even, odd = list(range(0, 15, 2)), list(range(1, 15, 2))
    assert _hier_deal(15) == [[_m("m1", even), _m("m1", odd), _m("m2", even), _m("m2", odd)]]
    assert _hier_deal(5, world=2, rank=0) == [[_m("m1", [0, 2, 4]), _m("m2", [0, 2, 4])]]
    assert _hier_deal(5, concurrent_folds=2) == [[_m("m1", [0, 1]), _m("m2", [0, 1])], [_m("m1", [2, 3]), _m("m2", [2, 3])],
                                                 [_m("m1", [4]), _m("m2", [4])]]
    assert _hier_deal(15, lockstep_groups=1) == [[_m("m1", range(15)), _m("m2", range(15))]]


def test_deal_never_exceeds_the_stream_and_fold_limits():
    for waves in (_simple_deal(1, 40, concurrent_folds=40, lockstep_groups=6), _simple_deal(8, 20), _hier_deal(40, concurrent_folds=40)):
        assert all(len(wv) <= MAX_TRAIN_STREAMS and all(1 <= len(b) <= L.MAX_FOLDS for b in wv) for wv in waves)
        units = [u for wv in waves for b in wv for u in b]
        assert len(units) == len(set(units))
