"""Records tests/golden/optim_input.npz: a SHA-256 and the first 64 elements of every output of the cases of
tests/optim_input_cases.py — fused train steps, msig_adam_step, msig_ft_head_epoch and both per-subject normalisations.  Run ONCE on
the MI355X against the library built from the commit BEFORE adam_update, colsum_column and the one normalisation family existed:

    MSIG_LIB=/path/to/that/libmsig_hip.so python tests/golden/make_optim_input_golden.py

Only digests and heads are stored; the test regenerates the inputs.  Before anything is written the premises of the cases are
checked: the reduction jobs' row counts, the clip coefficients, the second grid-stride iteration of msig_adam_step, the partial
counts of the normalisation shapes, and that every case gives the same bits twice."""
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parent), str(HERE.parent.parent)]

import optim_input_cases as OC  # noqa: E402
from multimodalsignal_amd import _lib as L  # noqa: E402


def check_premises(dev):
    head, conv1, conv2 = OC.job_rows(**OC.SMALL)
    assert head < 8 and 8 <= conv1 < 64 and conv2 >= 64 and OC.SMALL["K"] % 32 != 0, (head, conv1, conv2)
    assert OC.SMALL["B"] <= 16 and (OC.LARGE["B"] + 15) // 16 > 128
    assert min(OC.ADAM_N) == 4 and max(OC.ADAM_N) // 4 > 2048 * 256
    parts = [(N * T + 255) // 256 for N, T in OC.NORM_SHAPES]
    assert parts == [1, 4, 20, 516], parts
    assert all(0 < OC.norm_mask(N).sum() < N for N, _ in OC.NORM_SHAPES[1:])
    for name, want in (("clip", OC.STEPS), ("clip_inf", 0)):
        st = OC.train_case(L, torch, dev, name)[1]
        assert st["clipped"] == want and st["last"] > 10 * OC.CLIP_SMALL, (name, st)
        print(f"{name}: gradient norms up to {st['max']:.4g}, clipped steps {st['clipped']}")
    for N, T in OC.NORM_SHAPES:
        assert OC.norm_case(L, torch, dev, N, T)[1], ("plain normalisation wrote past its scratch", N, T)


def main():
    dev = torch.device("cuda")
    print("library:", L.LIB_PATH)
    check_premises(dev)
    out = {}
    for key, run in OC.all_cases():
        a, b = run(L, torch, dev), run(L, torch, dev)
        for name, (sha, head) in a.items():
            assert np.array_equal(sha, b[name][0]), (key, name, "not deterministic")
            out[f"{key}/{name}/sha"], out[f"{key}/{name}/head"] = sha, head
        print(key, sorted(a))
    path = HERE / "optim_input.npz"
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {path.stat().st_size} bytes")


if __name__ == "__main__":
    main()
