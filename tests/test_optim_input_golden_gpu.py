"""The Adam update (msig_dev.h adam_update), the column reduction (head.hip colsum_column) and the per-subject normalisation
(normalise.hip) against the bits their predecessors wrote: tests/golden/optim_input.npz was recorded from the library in which Adam
was written four times, the reduction three times and the normalisation twice (tests/golden/make_optim_input_golden.py).  The
cross-tests — clip at inf against the unclipped step, an all-or-none mask against msig_normalise_subject, the fused step against the
separate calls — compare the shared code with itself; this does not."""
from pathlib import Path

import numpy as np
import pytest
import torch

import optim_input_cases as OC

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).parent / "golden" / "optim_input.npz"
CASES = OC.all_cases()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_the_golden_file_holds_exactly_the_cases(golden):
    keys = {k.rsplit("/", 2)[0] for k in golden}
    assert keys == {k for k, _ in CASES}
    assert {k.rsplit("/", 1)[1] for k in golden} == {"sha", "head"}
    assert all(v.shape == (32,) and v.dtype == np.uint8 for k, v in golden.items() if k.endswith("/sha"))


@pytest.mark.parametrize("key", [k for k, _ in CASES])
def test_every_output_carries_the_recorded_bits(golden, key):
    from multimodalsignal_amd import _lib as L
    got = dict(CASES)[key](L, torch, torch.device("cuda"))
    want = {k[len(key) + 1:-len("/sha")] for k in golden if k.startswith(key + "/") and k.endswith("/sha")}
    assert set(got) == want and got
    for name, (sha, head) in got.items():
        ghead = golden[f"{key}/{name}/head"]
        assert head.dtype == ghead.dtype and np.array_equal(head, ghead), (name, "first elements", head[:8], ghead[:8])
        assert np.array_equal(sha, golden[f"{key}/{name}/sha"]), (name, "SHA-256 of the whole tensor; its first 64 elements agree")


@pytest.mark.parametrize("N,T", OC.NORM_SHAPES)
def test_the_plain_normalisation_stays_inside_its_scratch(N, T):
    """msig_normalise_scratch_bytes() is smaller than the masked call's layout: bytes behind it keep their poison."""
    from multimodalsignal_amd import _lib as L
    assert OC.norm_case(L, torch, torch.device("cuda"), N, T)[1]
