"""Records tests/golden/head_mlp.npz: a SHA-256 and the first 64 elements of every output of the cases of tests/head_mlp_cases.py —
fused, unfused, fold-batched and adversarial train steps, eval forwards, a separate backward and head epochs.  Run ONCE on the
MI355X against the library built from the commit BEFORE csrc/head_mlp.h existed:

    MSIG_LIB=/path/to/that/libmsig_hip.so python tests/golden/make_head_mlp_golden.py [OUT.npz]

Only digests and heads are stored; the test regenerates the inputs.  An existing file is never overwritten: remove it first.  Before
anything is written the premises of the cases are checked (group and slot counts, the short last step of the head epoch, -1 entries
among the masked discriminator rows), and that every case gives the same bits twice."""
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parent), str(HERE.parent.parent)]

import head_mlp_cases as HC  # noqa: E402
from multimodalsignal_amd import _lib as L  # noqa: E402


def check_premises():
    B, K = HC.MID["B"], HC.MID["K"]
    assert (B + 15) // 16 == 3 and B % 16 == 5 and 512 < K * 64 < 768 and len(HC.CW9) == K
    assert HC.FULL == dict(B=16, K=L.MAX_K) and len(HC.CW16) == L.MAX_K
    assert (HC.LARGE["B"] + 15) // 16 == 129 and HC.TINY["B"] <= 16
    assert [s["B"] for n, s, _ in HC.TRAIN_CASES if n.startswith("da_")] == [40, 40, 40, L.DA_MAX_BATCH]
    ft = HC.FT
    assert ft["K"] == L.MAX_K and 32 < ft["batch"] <= 48 and ft["n_steps"] == 3 and 0 < ft["n_order"] - 2 * ft["batch"] < ft["batch"]
    rs = np.random.RandomState(1000 + 16 + 40)
    table = rs.randint(0, 16, size=HC.DA_POSITIONS)
    table[rs.rand(HC.DA_POSITIONS) < 0.3] = -1
    rows = table[rs.permutation(HC.DA_POSITIONS)[:40]]
    assert 0 < (rows < 0).sum() < 40, rows


def main():
    path = Path(sys.argv[1]) if len(sys.argv) > 1 else HERE / "head_mlp.npz"
    if path.exists():
        sys.exit(f"{path} exists: a recorded file is not overwritten (remove it first)")
    dev = torch.device("cuda")
    print("library:", L.LIB_PATH)
    check_premises()
    out = {}
    for key, run in HC.all_cases():
        a, b = run(L, torch, dev), run(L, torch, dev)
        for name, (sha, head) in a.items():
            assert np.array_equal(sha, b[name][0]), (key, name, "not deterministic")
            assert head.any() or name.endswith("PRED"), (key, name, "all zero: nothing was recorded")
            out[f"{key}/{name}/sha"], out[f"{key}/{name}/head"] = sha, head
        print(key, sorted(a))
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {path.stat().st_size} bytes")


if __name__ == "__main__":
    main()
