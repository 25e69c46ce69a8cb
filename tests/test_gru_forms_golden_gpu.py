"""Pins the bits of every GRU kernel form — forward and backward, one model and fold batches, kept and unkept forwards, one and
two layers, 1 to 7 recurrent steps, ragged batch tiles — to tests/golden/gru_forms.npz, recorded from the library as it was before
the kernels' prologues and the forward launch ladder were each written once (tests/golden/make_gru_forms_golden.py).  The
cross-tests — the forward forms against each other, the fused step against the separate calls, any backward form after any
forward call — compare the shared code with itself; this does not."""
from pathlib import Path

import numpy as np
import pytest
import torch

import gru_form_cases as GC

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).parent / "golden" / "gru_forms.npz"
CASES = GC.all_cases()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_the_golden_file_holds_exactly_the_cases(golden):
    keys = {k.rsplit("/", 2)[0] for k in golden}
    assert keys == {k for k, _ in CASES} and len(keys) == len(CASES)
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
