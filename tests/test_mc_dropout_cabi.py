"""Monte-Carlo dropout (include/msig_mc.h), the C ABI checked without a GPU: the header's calls are exported, the binding's constants
match it, the other headers' ABI versions are what they were, and each rejection happens before the first launch (fake, aligned,
never dereferenced pointers, as in test_attribute_cabi.py — a call that passed every check would launch, so only rejected calls
are made here)."""
import ctypes as C
import re
from pathlib import Path

from multimodalsignal_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "msig_mc.h").read_text()
E_NULL, E_SHAPE, E_ALIGN, E_WORKSPACE = -1, -2, -3, -4
CH, T, K = 6, 256, 3

_keep_alive = (C.c_char * 8192)()
A = (C.addressof(_keep_alive) + 255) // 256 * 256          # an aligned address nothing ever reads


def test_header_calls_are_exported_and_constants_match():
    names = sorted(set(re.findall(r"\b(msig_mc_[a-z0-9_]+)\s*\(", HEADER)))
    assert names == ["msig_mc_abi_version", "msig_mc_expand", "msig_mc_reduce", "msig_mc_tail", "msig_mc_trunk"]
    lib = L.lib()
    for n in names:
        assert getattr(lib, n) is not None
    assert lib.msig_mc_abi_version() == int(re.search(r"#define MSIG_MC_ABI_VERSION (\d+)", HEADER).group(1)) == L.MC_ABI_VERSION
    assert int(re.search(r"#define MSIG_MC_MAX_SAMPLES (\d+)", HEADER).group(1)) == L.MC_MAX_SAMPLES == 256
    kinds = {k: int(v) for k, v in re.findall(r"#define MSIG_MC_KIND_(ATTENTION|CNN_GRU)\s+(\d+)", HEADER)}
    assert kinds == {"ATTENTION": L.MC_KINDS["cnn_gru_attention"], "CNN_GRU": L.MC_KINDS["cnn_gru"]} and sorted(kinds.values()) == [0, 1]
    # the other headers' calls are still there, at the versions they had
    assert (lib.msig_abi_version(), lib.msig_cw_abi_version(), lib.msig_cg_abi_version(), lib.msig_ft_abi_version(), lib.msig_gc_abi_version(),
            lib.msig_aug_abi_version(), lib.msig_st_abi_version(), lib.msig_ab_abi_version(), lib.msig_at_abi_version()) == (5, 1, 1, 1, 1, 1, 1, 1, 1)


def _batch(B=4, **kw):
    b = L.Batch()
    b.shape = L.Shape(B, CH, T, K)
    b.training, b.keep_for_backward = 0, 0
    b.bn_momentum, b.bn_eps = 0.1, 1e-5
    b.dropout_thr = 128
    b.x = b.params = b.grads = b.bn_state = b.bn_count = b.ws = A
    b.labels, b.dx, b.loss_acc = None, None, None
    b.ws_bytes = 1 << 62
    b.gru_layers = 2
    for k, v in kw.items():
        if k == "shape":
            b.shape = L.Shape(*v)
        else:
            setattr(b, k, v)
    return b


def _trunk(kind=0, **kw):
    return L.lib().msig_mc_trunk(C.byref(_batch(**kw)), kind, None)


def _tail(kind=0, **kw):
    return L.lib().msig_mc_tail(C.byref(_batch(**kw)), kind, None)


def test_trunk_and_tail_reject_before_launching():
    lib = L.lib()
    for call, fn in ((_trunk, lib.msig_mc_trunk), (_tail, lib.msig_mc_tail)):
        assert fn(None, 0, None) == E_NULL
        for f in ("params", "bn_state", "bn_count", "ws"):
            assert call(**{f: None}) == E_NULL, (call.__name__, f)
        assert call(training=1) == E_SHAPE
        assert call(keep_for_backward=1) == E_SHAPE
        assert call(dx=A) == E_SHAPE
        for kind in (-1, 2):
            assert call(kind=kind) == E_SHAPE
        assert call(dropout_thr=257) == E_SHAPE and call(dropout_thr=-1) == E_SHAPE
        assert call(gru_layers=3) == E_SHAPE
        for bad in ((0, CH, T, K), (4, 0, T, K), (4, 17, T, K), (4, CH, 15, K), (4, CH, T, 1), (4, CH, T, 17)):
            assert call(shape=bad) == E_SHAPE, bad
        for f in ("params", "ws"):
            assert call(**{f: A + 4}) == E_ALIGN, (call.__name__, f)
        for kind in (0, 1):
            need = L.workspace_layout(4, CH, T, K, False)[-1]
            assert call(kind=kind, ws_bytes=need - 1) == E_WORKSPACE
        assert call(fwd_form=9) == -5
    assert _trunk(x=None) == E_NULL and _trunk(x=A + 8) == E_ALIGN       # the trunk reads the windows; the tail reads no input


def test_tail_mask_index_bound():
    """T = 256: TP = 16, so rows * TP * 128 > 2^31 from rows = 2^20 + 1 on — rejected before the workspace is even sized."""
    assert L.stage_lengths(T)[3] == 16
    assert _tail(shape=((1 << 20) + 1, CH, T, K)) == E_SHAPE
    assert _tail(shape=((1 << 20) + 1, CH, T, K), gru_layers=1) == E_SHAPE
    # exactly 2^31 elements is inside the bound: the next check that fails is the workspace's
    assert _tail(shape=(1 << 20, CH, T, K), ws_bytes=1024) == E_WORKSPACE


def _expand(**kw):
    a = dict(src=A, dst=A + 4096, N=3, S=5, R=128)
    a.update(kw)
    return L.lib().msig_mc_expand(a["src"], a["dst"], a["N"], a["S"], a["R"], None)


def _reduce(**kw):
    a = dict(logits=A, N=5, S=7, K=K, mean_p=A, std_p=A, pred=A, entropy=A, expected_entropy=A, mutual_info=A, votes=A)
    a.update(kw)
    return L.lib().msig_mc_reduce(a["logits"], a["N"], a["S"], a["K"], a["mean_p"], a["std_p"], a["pred"], a["entropy"], a["expected_entropy"],
                                  a["mutual_info"], a["votes"], None)


def test_expand_rejections():
    assert _expand(src=None) == E_NULL and _expand(dst=None) == E_NULL
    for bad in (dict(S=0), dict(S=L.MC_MAX_SAMPLES + 1), dict(S=-1), dict(N=0), dict(N=-2), dict(R=0), dict(R=-4), dict(N=1 << 30, S=2),
                dict(N=1 << 22, S=1, R=1 << 20), dict(R=1 << 40)):
        assert _expand(**bad) == E_SHAPE, bad
    # 16-byte alignment is NOT required (such buffers take the element-wise form): only a pointer that is no float's address is refused
    for f in ("src", "dst"):
        for off in (1, 2, 3):
            assert _expand(**{f: A + off}) == E_ALIGN, (f, off)


def test_reduce_rejections():
    assert _reduce(logits=None) == E_NULL and _reduce(mean_p=None) == E_NULL
    for bad in (dict(S=0), dict(S=L.MC_MAX_SAMPLES + 1), dict(N=0), dict(K=1), dict(K=L.MAX_K + 1), dict(N=1 << 30, S=2)):
        assert _reduce(**bad) == E_SHAPE, bad
    for f in ("logits", "mean_p", "std_p", "pred", "entropy", "expected_entropy", "mutual_info", "votes"):
        assert _reduce(**{f: A + 2}) == E_ALIGN, f
