"""Deep ensembles (include/msig_en.h), the C ABI checked without a GPU: the header's calls are exported, the binding's constants match
it, the other headers' ABI versions are what they were, and each rejection happens before the first launch (fake, aligned, never
dereferenced pointers, as in test_mc_dropout_cabi.py — a call that passed every check would launch, so only rejected calls are made
here)."""
import ctypes as C
import re
from pathlib import Path

from multimodalsignal_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "msig_en.h").read_text()
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
K = 3
OUTPUTS = ("mean_p", "std_p", "pred", "entropy", "expected_entropy", "mutual_info", "votes", "member_pred", "disagreement")

_keep_alive = (C.c_char * 8192)()
A = (C.addressof(_keep_alive) + 255) // 256 * 256          # an aligned address nothing ever reads


def test_header_calls_are_exported_and_constants_match():
    names = sorted(set(re.findall(r"\b(msig_en_[a-z0-9_]+)\s*\(", HEADER)))
    assert names == ["msig_en_abi_version", "msig_en_reduce", "msig_en_reduce_multi"]
    lib = L.lib()
    for n in names:
        assert getattr(lib, n) is not None
    assert lib.msig_en_abi_version() == int(re.search(r"#define MSIG_EN_ABI_VERSION (\d+)", HEADER).group(1)) == L.EN_ABI_VERSION == 1
    assert int(re.search(r"#define MSIG_EN_MAX_MEMBERS (\d+)", HEADER).group(1)) == L.EN_MAX_MEMBERS == 256
    # the other headers' calls are still there, at the versions they had
    assert (lib.msig_abi_version(), lib.msig_cw_abi_version(), lib.msig_cg_abi_version(), lib.msig_ft_abi_version(), lib.msig_gc_abi_version(),
            lib.msig_aug_abi_version(), lib.msig_st_abi_version(), lib.msig_ab_abi_version(), lib.msig_at_abi_version(), lib.msig_mc_abi_version(),
            lib.msig_da_abi_version(), lib.msig_wa_abi_version()) == (5, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1)
    assert (L.ABI_VERSION, L.MC_ABI_VERSION, L.MC_MAX_SAMPLES, L.MAX_FOLDS) == (5, 1, 256, 16)


def _reduce(**kw):
    a = dict(logits=A, stride=5 * K, M=7, N=5, K=K, **{o: A for o in OUTPUTS})
    a.update(kw)
    return L.lib().msig_en_reduce(a["logits"], a["stride"], a["M"], a["N"], a["K"], *(a[o] for o in OUTPUTS), None)


def _multi(n=3, stride=256, slots=None, form_folds=1):
    m = L.Multi()
    m.n, m.stride_bytes, m.form_folds = n, stride, form_folds
    for i, s in enumerate(slots if slots is not None else range(min(max(n, 0), L.MAX_FOLDS))):
        m.slot[i] = s
    return m


def _reduce_multi(multi=None, **kw):
    a = dict(logits=A, N=5, K=K, **{o: A for o in OUTPUTS})
    a.update(kw)
    m = _multi() if multi is None else multi
    return L.lib().msig_en_reduce_multi(a["logits"], None if m is False else C.byref(m), a["N"], a["K"], *(a[o] for o in OUTPUTS), None)


def test_reduce_rejections():
    assert _reduce(logits=None) == E_NULL and _reduce(mean_p=None) == E_NULL
    for bad in (dict(M=0), dict(M=-1), dict(M=L.EN_MAX_MEMBERS + 1), dict(N=0), dict(N=-3), dict(K=1), dict(K=L.MAX_K + 1),
                dict(N=1 << 30, M=2, stride=1 << 40), dict(stride=5 * K - 1), dict(stride=0), dict(stride=-1)):
        assert _reduce(**bad) == E_SHAPE, bad
    for f in ("logits",) + OUTPUTS:
        for off in (1, 2):
            assert _reduce(**{f: A + off}) == E_ALIGN, (f, off)
    # NULL is checked before the shape, the shape before the alignment
    assert _reduce(logits=None, M=0) == E_NULL and _reduce(M=0, mean_p=A + 2) == E_SHAPE


def test_reduce_multi_rejections():
    assert _reduce_multi(multi=False) == E_NULL                                   # msig_multi's own checks first
    assert _reduce_multi(logits=None) == E_NULL and _reduce_multi(mean_p=None) == E_NULL
    for bad in (_multi(n=0), _multi(n=L.MAX_FOLDS + 1), _multi(n=-1), _multi(slots=[0, 1, 1]), _multi(slots=[0, -1, 2]), _multi(form_folds=17)):
        assert _reduce_multi(multi=bad) == E_SHAPE
    for bad in (_multi(stride=0), _multi(stride=-256), _multi(stride=128), _multi(stride=260)):
        assert _reduce_multi(multi=bad) == E_ALIGN                                # msig_multi's stride rule
    for bad in (dict(N=0), dict(K=1), dict(K=L.MAX_K + 1), dict(N=22)):          # 22 * 3 floats = 264 bytes > the 256-byte stride
        assert _reduce_multi(**bad) == E_SHAPE, bad
    assert _reduce_multi(N=1 << 30, multi=_multi(n=2, stride=1 << 40)) == E_SHAPE
    for f in ("logits",) + OUTPUTS:
        assert _reduce_multi(**{f: A + 2}) == E_ALIGN, f
    # a multi that fails its own checks is refused before the NULL logits are looked at
    assert _reduce_multi(multi=_multi(n=0), logits=None) == E_SHAPE
