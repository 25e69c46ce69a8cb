"""Reference-masked normalisation (include/msig_nr.h), the C ABI checked without a GPU: the header's calls are exported beside
the unchanged headers, the versions agree, and each rejection happens before a launch (fake, aligned, never dereferenced device
pointers, as in test_averaging_cabi.py — so only calls that must be refused are made here)."""
import ctypes as C
import re
from pathlib import Path

import pytest

from multimodalsignal_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
NR_HEADER = (ROOT / "include" / "msig_nr.h").read_text()
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3


def test_msig_nr_header_calls_are_exported_and_the_other_headers_are_unchanged():
    names = sorted(set(re.findall(r"\b(msig_nr_\w+)\(", re.sub(r"/\*.*?\*/", "", NR_HEADER, flags=re.S))))
    assert names == ["msig_nr_abi_version", "msig_nr_normalise_subject", "msig_nr_scratch_bytes"]
    lib = L.lib()
    for n in names:
        assert getattr(lib, n) is not None
    assert lib.msig_nr_abi_version() == int(re.search(r"#define MSIG_NR_ABI_VERSION (\d+)", NR_HEADER).group(1)) == L.NR_ABI_VERSION == 1
    assert len(set(re.findall(r"\b(msig_\w+)\(", (ROOT / "include" / "msig.h").read_text()))) == 26
    assert (lib.msig_abi_version(), lib.msig_cw_abi_version(), lib.msig_cg_abi_version(), lib.msig_ft_abi_version(), lib.msig_gc_abi_version(),
            lib.msig_aug_abi_version(), lib.msig_st_abi_version(), lib.msig_ab_abi_version(), lib.msig_at_abi_version(),
            lib.msig_mc_abi_version(), lib.msig_da_abi_version(), lib.msig_wa_abi_version(), lib.msig_en_abi_version()) \
        == (5, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1)
    assert (L.ABI_VERSION, L.CW_ABI_VERSION, L.CG_ABI_VERSION, L.FT_ABI_VERSION, L.GC_ABI_VERSION, L.AUG_ABI_VERSION, L.ST_ABI_VERSION,
            L.AB_ABI_VERSION, L.AT_ABI_VERSION, L.MC_ABI_VERSION, L.DA_ABI_VERSION, L.WA_ABI_VERSION, L.EN_ABI_VERSION) \
        == (5, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1)
    # msig_normalise_subject is still there, with its own scratch size
    assert lib.msig_normalise_scratch_bytes() == (512 * 2 * L.MAX_C + 2 * L.MAX_C) * 8


def test_scratch_holds_two_sets_of_partials_the_pivots_and_the_statistics():
    assert L.lib().msig_nr_scratch_bytes() == (2 * 512 * 2 * L.MAX_C + L.MAX_C + 2 * L.MAX_C + 1) * 8


def _addr():
    keep_alive = (C.c_char * 8192)()
    return keep_alive, (C.addressof(keep_alive) + 255) // 256 * 256


def _call(addr, **kw):
    """msig_nr_normalise_subject over fake pointers: raw at addr, ref + 1024, out + 2048, stats + 3072, scratch + 4096."""
    cols = kw.get("cols", [2, 0, 1])
    carr = None if cols is None else (C.c_int32 * max(1, len(cols)))(*cols)
    a = dict(raw=addr, N=7, T=64, C_all=5, cols=carr, C=3 if cols is None else len(cols), mask=0b10, ref=addr + 1024, out=addr + 2048,
             stats=addr + 3072, scratch=addr + 4096)
    a.update({k: v for k, v in kw.items() if k != "cols"})
    return L.lib().msig_nr_normalise_subject(a["raw"], a["N"], a["T"], a["C_all"], a["cols"], a["C"], a["mask"], a["ref"], a["out"], a["stats"],
                                             a["scratch"], None)


@pytest.mark.parametrize("name", ["raw", "cols", "ref", "out", "scratch"])
def test_null_pointers(name):
    _k, addr = _addr()
    assert _call(addr, **{name: None}) == E_NULL


@pytest.mark.parametrize("kw", [dict(N=0), dict(N=-3), dict(T=0), dict(T=-1), dict(C_all=0), dict(C=0), dict(C=-1), dict(C=L.MAX_C + 1),
                                dict(cols=[0, 5, 1]), dict(cols=[-1]), dict(cols=[0, 1, 2], C_all=2)], ids=str)
def test_bad_shapes(kw):
    _k, addr = _addr()
    if kw.get("C", 0) > 3:
        kw = dict(kw, cols=[0] * kw["C"])
    assert _call(addr, **kw) == E_SHAPE


@pytest.mark.parametrize("name", ["raw", "scratch", "stats"])
def test_misalignment(name):
    _k, addr = _addr()
    base = {"raw": addr, "scratch": addr + 4096, "stats": addr + 3072}[name]
    for off in (1, 4):
        assert _call(addr, **{name: base + off}) == E_ALIGN


def test_the_order_of_the_checks():
    """NULL before shape before alignment, as the header lists them; ref and out need no alignment and stats may be absent."""
    _k, addr = _addr()
    assert _call(addr, out=None, N=0, raw=addr + 4) == E_NULL
    assert _call(addr, N=0, raw=addr + 4) == E_SHAPE
    assert _call(addr, cols=[9], scratch=addr + 4097) == E_SHAPE
    assert _call(addr, stats=None, ref=addr + 1025, out=addr + 2052, scratch=addr + 4100) == E_ALIGN        # the scratch alone
