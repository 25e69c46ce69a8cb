"""Records tests/golden/member_stats.npz: the bits msig_mc_reduce, msig_en_reduce[_multi] and msig_kd_teacher[_multi] write for the
cases of tests/member_stats_cases.py.  Run ONCE on the MI355X against the library built from the commit BEFORE the three reduction
kernels became instantiations of csrc/member_stats.h:

    MSIG_LIB=/path/to/that/libmsig_hip.so python tests/golden/make_member_stats_golden.py

Only outputs are stored (int32 views); the test regenerates the inputs.  Before anything is recorded the inputs are checked on the CPU
against the independent restatements, and every call with one optional output NULL must leave the other outputs' bits unchanged."""
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parent), str(HERE.parent.parent)]

import en_reference  # noqa: E402
import kd_reference  # noqa: E402
import member_stats_cases as MS  # noqa: E402
from multimodalsignal_amd import _lib as L  # noqa: E402


def check_inputs():
    """en_reference.reduce and kd_reference.teacher are finite on every case; among them at least one probability is exactly 0 and
    at least one argmax is decided by the first-of-equals rule (in a row and in a mean)."""
    zeros = row_ties = mean_ties = 0
    for M, K, _ in MS.all_cases():
        lg = MS.logits(M, K)
        ref = en_reference.reduce(lg)
        assert all(np.isfinite(np.asarray(v, dtype=np.float64)).all() for v in ref.values()), (M, K)
        top = np.sort(lg, axis=2)
        row_ties += int((top[:, :, -1] == top[:, :, -2]).sum())
        mu = np.sort(ref["mean_p"], axis=1)
        mean_ties += int((mu[:, -1] == mu[:, -2]).sum())
        zeros += int((ref["mean_p"] == 0.0).sum())
        for T in MS.TEMPERATURES:
            q = kd_reference.teacher(lg, T)
            assert np.isfinite(q).all(), (M, K, T)
            zeros += int((q == 0.0).sum())
    assert zeros >= 1 and row_ties >= 1 and mean_ties >= 1, (zeros, row_ties, mean_ties)
    print(f"inputs: {zeros} exact-zero probabilities, {row_ties} row ties, {mean_ties} mean ties")


def main():
    check_inputs()
    dev = torch.device("cuda")
    print("library:", L.LIB_PATH)
    out = {}
    for M, K, multi in MS.all_cases():
        full = MS.run(L, torch, dev, M, K, multi=multi)
        for skip in MS.OPTIONAL_OUTS:
            part = MS.run(L, torch, dev, M, K, multi=multi, skip=skip)
            for k, v in part.items():
                assert np.array_equal(v, full[k]), (M, K, multi, skip, k)
        out.update({f"{MS.case_key(M, K, multi)}/{k}": v for k, v in full.items()})
    path = HERE / "member_stats.npz"
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {path.stat().st_size} bytes")


if __name__ == "__main__":
    main()
