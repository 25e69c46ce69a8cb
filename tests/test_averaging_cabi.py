"""Weight averaging (include/msig_wa.h), the C ABI checked without a GPU: the header's calls are exported beside the unchanged
headers, the binding's mirror matches the build, and each rejection happens before a launch (descriptors with fake, aligned, never
dereferenced pointers, as in test_adversary_cabi.py).  A call whose every coefficient is 0 launches nothing, so a valid descriptor
over fake pointers returns 0: that is how "the checks pass" is observed here."""
import ctypes as C
import re
from pathlib import Path

import pytest

from multimodalsignal_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
WA_HEADER = (ROOT / "include" / "msig_wa.h").read_text()
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
BN = ("bn_state", "bn_count", "avg_bn_state", "avg_bn_count")


def test_msig_wa_header_calls_are_exported_and_the_other_headers_are_unchanged():
    names = sorted(set(re.findall(r"\b(msig_wa_\w+)\(", WA_HEADER)))
    assert names == ["msig_wa_abi_version", "msig_wa_struct_bytes", "msig_wa_update", "msig_wa_update_multi"]
    lib = L.lib()
    for n in names:
        assert getattr(lib, n) is not None
    assert lib.msig_wa_abi_version() == int(re.search(r"#define MSIG_WA_ABI_VERSION (\d+)", WA_HEADER).group(1)) == L.WA_ABI_VERSION == 1
    assert len(set(re.findall(r"\b(msig_\w+)\(", (ROOT / "include" / "msig.h").read_text()))) == 26
    assert (lib.msig_abi_version(), lib.msig_cw_abi_version(), lib.msig_cg_abi_version(), lib.msig_ft_abi_version(), lib.msig_gc_abi_version(),
            lib.msig_aug_abi_version(), lib.msig_st_abi_version(), lib.msig_ab_abi_version(), lib.msig_at_abi_version(),
            lib.msig_mc_abi_version(), lib.msig_da_abi_version()) == (5, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1)
    assert (L.ABI_VERSION, L.CW_ABI_VERSION, L.CG_ABI_VERSION, L.FT_ABI_VERSION, L.GC_ABI_VERSION, L.AUG_ABI_VERSION, L.ST_ABI_VERSION,
            L.AB_ABI_VERSION, L.AT_ABI_VERSION, L.MC_ABI_VERSION, L.DA_ABI_VERSION) == (5, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1)


def test_mirror_matches_the_header():
    body = re.search(r"typedef struct msig_wa \{(.*?)\} msig_wa;", WA_HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n for decl in body.split(";") for n in re.findall(r"[\s*,](\w+)(?:\[\w+\])?\s*(?=,|$)", decl.strip())]
    assert fields == [n for n, _ in L.Wa._fields_]
    assert L.lib().msig_wa_struct_bytes() == C.sizeof(L.Wa) == 8 + 6 * 8 + 4 * L.MAX_FOLDS


def _addr():
    keep_alive = (C.c_char * 8192)()
    return keep_alive, (C.addressof(keep_alive) + 255) // 256 * 256


def _wa(addr, coef=(0.0, 0.0), **kw):
    """A descriptor over fake pointers: model buffers at addr + 0 / 1024 / 2048, the shadow's 4096 further on."""
    w = L.Wa()
    w.n_flat = kw.get("n_flat", 1028)
    base = {"params": addr, "bn_state": addr + 1024, "bn_count": addr + 2048, "avg_params": addr + 4096, "avg_bn_state": addr + 5120,
            "avg_bn_count": addr + 6144}
    for name, v in base.items():
        setattr(w, name, kw.get(name, v))
    for i, a in enumerate(coef):
        w.coef[i] = a
    return w


def _multi(n=2, **kw):
    m = L.Multi()
    m.n, m.stride_bytes = n, kw.get("stride_bytes", 1 << 20)
    for i in range(n):
        m.slot[i] = kw.get("slots", list(range(n)))[i]
    return m


def _calls(w, m=None):
    lib = L.lib()
    wp = C.byref(w) if w is not None else None
    return [lib.msig_wa_update(wp, None), lib.msig_wa_update_multi(wp, C.byref(m if m is not None else _multi()), None)]


def test_valid_descriptors_pass_every_check_and_all_zero_coefficients_launch_nothing():
    _k, addr = _addr()
    assert _calls(_wa(addr)) == [0, 0]
    assert _calls(_wa(addr, n_flat=4)) == [0, 0]
    assert _calls(_wa(addr, **{k: None for k in BN})) == [0, 0]                      # parameters only
    assert _calls(_wa(addr, bn_count=addr + 2056, avg_bn_count=addr + 6152)) == [0, 0]      # counts need 8-byte alignment only
    # coefficients beyond the folds of the launch are not read
    w = _wa(addr)
    w.coef[2] = float("nan")
    assert _calls(w) == [0, 0]
    w = _wa(addr)
    w.coef[1] = 7.0
    assert L.lib().msig_wa_update(C.byref(w), None) == 0


def test_null_pointers():
    _k, addr = _addr()
    lib = L.lib()
    assert _calls(None) == [E_NULL, E_NULL]
    assert lib.msig_wa_update_multi(C.byref(_wa(addr)), None, None) == E_NULL
    for name in ("params", "avg_params"):
        assert _calls(_wa(addr, coef=(0.5, 0.5), **{name: None})) == [E_NULL, E_NULL], name
    # the four BatchNorm pointers: all or none
    for r in (1, 2, 3):
        for missing in ([BN[i] for i in range(4) if (mask >> i) & 1] for mask in range(1, 15) if bin(mask).count("1") == r):
            assert _calls(_wa(addr, coef=(0.5, 0.5), **{k: None for k in missing})) == [E_NULL, E_NULL], missing


@pytest.mark.parametrize("n_flat", [0, 3, -4, 1027, 6, 2])
def test_bad_length_is_a_shape_error(n_flat):
    _k, addr = _addr()
    assert _calls(_wa(addr, coef=(0.5, 0.5), n_flat=n_flat)) == [E_SHAPE, E_SHAPE]


@pytest.mark.parametrize("bad", [float("nan"), -0.25, 1.5, float("inf"), -float("inf")])
def test_bad_coefficient_of_a_participating_fold_is_a_shape_error(bad):
    _k, addr = _addr()
    assert _calls(_wa(addr, coef=(bad, 0.5))) == [E_SHAPE, E_SHAPE]
    assert _calls(_wa(addr, coef=(0.0, bad))) == [0, E_SHAPE]            # the second fold's counts in the fold batch only


def test_aliasing_is_a_shape_error():
    _k, addr = _addr()
    assert _calls(_wa(addr, coef=(0.5, 0.5), avg_params=addr)) == [E_SHAPE, E_SHAPE]
    assert _calls(_wa(addr, coef=(0.5, 0.5), avg_bn_state=addr + 1024)) == [E_SHAPE, E_SHAPE]


def test_misalignment():
    _k, addr = _addr()
    for name, off in (("params", 8), ("avg_params", 4), ("bn_state", 8), ("avg_bn_state", 12)):
        w = _wa(addr, coef=(0.5, 0.5))
        setattr(w, name, getattr(w, name) + off)
        assert _calls(w) == [E_ALIGN, E_ALIGN], name
    for name in ("bn_count", "avg_bn_count"):
        w = _wa(addr, coef=(0.5, 0.5))
        setattr(w, name, getattr(w, name) + 4)
        assert _calls(w) == [E_ALIGN, E_ALIGN], name


def test_msig_multis_own_checks_come_first():
    _k, addr = _addr()
    bad = _wa(addr, coef=(0.5, 0.5), n_flat=3)
    assert _calls(bad, _multi(stride_bytes=100)) == [E_SHAPE, E_ALIGN]
    assert _calls(bad, _multi(slots=[1, 1])) == [E_SHAPE, E_SHAPE]          # msig_multi: two folds in one arena
    m = _multi()
    m.n = 0
    assert _calls(_wa(addr), m) == [0, E_SHAPE]
    m.n = L.MAX_FOLDS + 1
    assert _calls(_wa(addr), m) == [0, E_SHAPE]


def test_the_order_of_the_checks():
    """NULL before shape before alignment, as the header lists them."""
    _k, addr = _addr()
    assert _calls(_wa(addr, coef=(0.5, 0.5), params=None, n_flat=3)) == [E_NULL, E_NULL]
    assert _calls(_wa(addr, coef=(0.5, 0.5), n_flat=3, avg_params=addr + 4100)) == [E_SHAPE, E_SHAPE]
    assert _calls(_wa(addr, coef=(2.0, 0.5), avg_params=addr + 4100)) == [E_SHAPE, E_SHAPE]


def test_host_side_coefficient_check():
    assert L.check_average_coef(0) == 0.0 and L.check_average_coef(1) == 1.0 and L.check_average_coef(0.1) == C.c_float(0.1).value
    for bad in (float("nan"), -0.1, 1.0001, "0.5", None, True):
        with pytest.raises(ValueError):
            L.check_average_coef(bad)
