"""Records tests/golden/gru_forms.npz: a SHA-256 and the first 64 elements of every output of the cases of tests/gru_form_cases.py —
every GRU kernel form as separate forward / backward calls, the fused step under ("ws", "b6"), fold batches, forwards that keep
nothing, the one-layer model and a batch of 194 tiles.  Run ONCE on the MI355X against the library built from the commit BEFORE
csrc/gru_frag.h, launch_fwd_layer and stamps_report existed:

    MSIG_LIB=/path/to/that/libmsig_hip.so python tests/golden/make_gru_forms_golden.py

Only digests and heads are stored; the test regenerates the inputs.  Before anything is written the premises of the cases are
checked: the step counts of the window lengths, the tile counts of the batch sizes, that every form set meets every step count and
both batch sizes, and that every case gives the same bits twice."""
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parent), str(HERE.parent.parent)]

import gru_form_cases as GC  # noqa: E402
from multimodalsignal_amd import _lib as L  # noqa: E402
from oracle import cnn_gru_oracle as O  # noqa: E402


def check_premises():
    assert {tp: O.stage_lengths(T)[3] for tp, T in GC.T_OF_TP.items()} == {tp: tp for tp in (1, 5, 6, 7)}
    assert sorted(tp % 3 for tp in GC.T_OF_TP) == [0, 1, 1, 2] and {tp % 2 for tp in GC.T_OF_TP} == {0, 1}
    assert [(B + 15) // 16 for B in GC.BATCHES] == [2, 3] and [B % 16 for B in GC.BATCHES] == [1, 8]
    for form in GC.FORMS:
        assert {GC.batch_of(form, tp) for tp in GC.T_OF_TP} == set(GC.BATCHES), form
    assert (GC.MANY["B"] + 15) // 16 >= 192 and GC.FOLD_B == 16 and GC.NF == 3
    keys = [k for k, _ in GC.all_cases()]
    assert len(keys) == len(set(keys))


def main():
    dev = torch.device("cuda")
    print("library:", L.LIB_PATH)
    check_premises()
    out = {}
    for key, run in GC.all_cases():
        a, b = run(L, torch, dev), run(L, torch, dev)
        for name, (sha, head) in a.items():
            assert np.array_equal(sha, b[name][0]), (key, name, "not deterministic")
            out[f"{key}/{name}/sha"], out[f"{key}/{name}/head"] = sha, head
        if key.startswith("folds/"):                          # a fold's parameters, gradients and accumulator are the step's, not zeros
            assert all(a[f"fold{f}.{k}"][1].any() for f in range(GC.NF) for k in ("params", "grads", "acc")), key
        print(key, sorted(a), flush=True)
    path = Path(sys.argv[1]) if len(sys.argv) > 1 else HERE / "gru_forms.npz"      # optional argument: another place to write to
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {path.stat().st_size} bytes")


if __name__ == "__main__":
    main()
