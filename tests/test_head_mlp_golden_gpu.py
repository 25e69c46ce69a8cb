"""The 128 -> 64 -> K classifier's pieces (csrc/head_mlp.h) — in head_fwd_kernel / ce_kernel / head_bwd_kernel, head_step_kernel,
head_epoch_kernel and da_step_kernel — against the bits their predecessors wrote: tests/golden/head_mlp.npz was recorded from the
library in which each of those kernels spelled the classifier out in full (tests/golden/make_head_mlp_golden.py).  The cross-tests
— the fused step against the separate calls, the head epoch against train steps — compare the shared code with itself; this does not."""
from pathlib import Path

import numpy as np
import pytest
import torch

import head_mlp_cases as HC

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).parent / "golden" / "head_mlp.npz"
CASES = HC.all_cases()


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
