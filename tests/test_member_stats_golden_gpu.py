"""The member reduction (csrc/member_stats.h) against the bits its three predecessors wrote: tests/golden/member_stats.npz was
recorded from the library before mc_reduce_kernel, en_reduce_kernel and kd_teacher_kernel became instantiations of one body
(tests/golden/make_member_stats_golden.py).  The cross-tests between the three calls compare the shared code with itself; this does not."""
from pathlib import Path

import numpy as np
import pytest
import torch

import member_stats_cases as MS

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).parent / "golden" / "member_stats.npz"


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_the_golden_file_holds_exactly_the_cases(golden):
    want = set()
    for M, K, multi in MS.all_cases():
        names = ([f"en_multi/{o}" for o in MS.EN_OUTS] + ["kd_multi"]) if multi else (
            [f"mc/{o}" for o in MS.MC_OUTS] + [f"en/{o}" for o in MS.EN_OUTS] + [f"kd/{T!r}" for T in MS.TEMPERATURES])
        want |= {f"{MS.case_key(M, K, multi)}/{n}" for n in names}
    assert set(golden) == want
    assert all(v.dtype == np.int32 for v in golden.values())


@pytest.mark.parametrize("M,K,multi", MS.all_cases())
def test_every_output_carries_the_recorded_bits(golden, M, K, multi):
    """All outputs given, then each optional output NULL in turn: every output written is the recorded int32 pattern."""
    from multimodalsignal_amd import _lib as L
    dev = torch.device("cuda")
    for skip in (None,) + MS.OPTIONAL_OUTS:
        got = MS.run(L, torch, dev, M, K, multi=multi, skip=skip)
        assert got, (M, K, multi, skip)
        for name, bits in got.items():
            want = golden[f"{MS.case_key(M, K, multi)}/{name}"]
            assert bits.dtype == np.int32 and bits.shape == want.shape and np.array_equal(bits, want), (name, skip)
