"""CPU tier: the hierarchical experiment's fold batches — one-layer models in lockstep, the embedding of the one-layer model in
the padded arena layout, and the wave / budget bookkeeping of the fold-batch drivers."""
from types import SimpleNamespace

import pytest
import torch

from multimodalsignal_amd import _lib as L
from multimodalsignal_amd.main import MAX_TRAIN_STREAMS, cap_waves, chunk_schedule
from multimodalsignal_amd.models import CnnGruAttentionModel
from multimodalsignal_amd.multifold import lockstep_compatible
from multimodalsignal_amd.runtime import embedding_index


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
