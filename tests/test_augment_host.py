"""Window augmentation inside the training gather (include/msig_aug.h), checked without a GPU: the header's calls are exported beside
the unchanged headers, the binding's mirror matches the build, every rejection happens before a launch (fake, aligned, never
dereferenced pointers, as in test_grad_clip_cabi.py), `Augment` / `Augment.parse` / the command line follow the same rules, and the
draws of the numpy restatement (tests/aug_reference.py) have the statistics the header promises — bounds derived, seeds fixed."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest

import aug_reference as R
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd.augment import Augment

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "msig_aug.h").read_text()
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
B, CH, T = 8, 6, 512
NAN = float("nan")


# ---- header, exports, mirror ------------------------------------------------------------------------------------------------
def test_header_calls_are_exported_and_the_other_headers_are_unchanged():
    names = sorted(set(re.findall(r"\b(msig_aug_\w+)\(", HEADER)))
    assert names == ["msig_aug_abi_version", "msig_aug_gather_windows", "msig_aug_gather_windows_multi", "msig_aug_struct_bytes"]
    lib = L.lib()
    for n in names:
        assert getattr(lib, n) is not None
    assert lib.msig_aug_abi_version() == int(re.search(r"#define MSIG_AUG_ABI_VERSION (\d+)", HEADER).group(1)) == L.AUG_ABI_VERSION
    assert lib.msig_aug_struct_bytes() == C.sizeof(L.Aug)
    assert len(set(re.findall(r"\b(msig_\w+)\(", (ROOT / "include" / "msig.h").read_text()))) == 26
    assert (lib.msig_abi_version(), lib.msig_cw_abi_version(), lib.msig_cg_abi_version(), lib.msig_ft_abi_version(),
            lib.msig_gc_abi_version()) == (5, 1, 1, 1, 1)


def test_mirror_matches_the_header():
    body = re.search(r"typedef struct msig_aug \{(.*?)\} msig_aug;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\w+\])?\s*(?:,|$)", decl.strip())]
    assert fields == [n for n, _ in L.Aug._fields_]
    assert int(re.search(r"#define MSIG_AUG_STREAM_ID (\d+)", HEADER).group(1)) == L.AUG_STREAM_ID == R.STREAM_ID == 3
    k = np.float32(float(re.search(r"#define MSIG_AUG_NOISE_K ([0-9.e-]+)f", HEADER).group(1)))
    assert k == R.NOISE_K == np.float32(1.0 / math.sqrt(4 * (256 ** 2 - 1) / 12))


def test_stream_id_3_is_free():
    """Stream ids 1 and 2 are the GRU and head dropout; no source but augment's names 3."""
    src = "".join(p.read_text() for p in (ROOT / "multimodalsignal_amd").rglob("*") if p.suffix in (".py", ".hip", ".h") and "augment" not in p.name)
    used = {int(v) for v in re.findall(r"dropout_keys?\([^()]*,\s*(\d+)\)", src)}
    assert used == {1, 2}


# ---- rejections, all before a launch ----------------------------------------------------------------------------------------
def _addr():
    keep_alive = (C.c_char * 8192)()
    return keep_alive, (C.addressof(keep_alive) + 255) // 256 * 256


def _aug(**kw):
    a = L.Aug()
    a.scale_sigma, a.jitter_sigma = kw.get("scale", 0.1), kw.get("jitter", 0.05)
    a.mask_prob, a.mask_max, a.chan_drop_prob = kw.get("mask_prob", 0.5), kw.get("mask_max", 64), kw.get("chan_drop", 0.1)
    return a


def _multi(n=2):
    m = L.Multi()
    m.n, m.stride_bytes = n, 1 << 20
    for i in range(n):
        m.slot[i] = i
    return m


def _calls(a, addr, B_=B, C_=CH, T_=T, store="addr", idx="addr", out="addr", m="default", stride=None):
    lib = L.lib()
    ap = C.byref(a) if a is not None else None
    pick = lambda v: addr if v == "addr" else v
    mm = _multi() if m == "default" else m
    return [lib.msig_aug_gather_windows(pick(store), addr, pick(idx), B_, C_, T_, pick(out), addr, ap, None),
            lib.msig_aug_gather_windows_multi(pick(store), addr, pick(idx), B_ if stride is None else stride, B_, C_, T_, pick(out), addr,
                                              C.byref(mm) if mm is not None else None, ap, None)]


def test_null_arguments():
    _k, addr = _addr()
    assert _calls(None, addr) == [E_NULL] * 2
    for which in ("store", "idx", "out"):
        assert _calls(_aug(), addr, **{which: None}) == [E_NULL] * 2, which
    assert _calls(_aug(), addr, m=None, T_=510)[1] == E_NULL


@pytest.mark.parametrize("kw", [dict(scale=-0.1), dict(scale=NAN), dict(jitter=-1e-6), dict(jitter=NAN), dict(mask_prob=-0.1),
                                dict(mask_prob=1.5), dict(mask_prob=NAN), dict(chan_drop=1.0), dict(chan_drop=-0.1), dict(chan_drop=NAN),
                                dict(mask_max=0), dict(mask_max=-3), dict(mask_max=T + 1)])
def test_bad_parameters_are_shape_errors(kw):
    _k, addr = _addr()
    assert _calls(_aug(**kw), addr + 4) == [E_SHAPE] * 2           # misaligned too: the parameters are checked first


def test_bad_shapes_are_shape_errors():
    _k, addr = _addr()
    for kw in (dict(T_=510), dict(T_=0), dict(T_=2), dict(C_=0), dict(C_=L.MAX_C + 1), dict(B_=0), dict(B_=-1)):
        assert _calls(_aug(), addr + 4, **kw) == [E_SHAPE] * 2, kw
    assert _calls(_aug(), addr, stride=B - 1)[1] == E_SHAPE
    assert _calls(_aug(mask_prob=0.0, mask_max=0), addr + 4) == [E_ALIGN] * 2       # mask_max is read only when the mask is on
    assert _calls(_aug(mask_max=T, mask_prob=1.0, chan_drop=0.999), addr + 4) == [E_ALIGN] * 2      # the ends of the ranges are valid


def test_alignment_follows_the_plain_gather():
    _k, addr = _addr()
    assert _calls(_aug(), addr, store=addr + 8) == [E_ALIGN] * 2
    assert _calls(_aug(), addr, out=addr + 4) == [E_ALIGN] * 2
    lib = L.lib()
    assert lib.msig_gather_windows(addr + 8, addr, addr, B, CH * T, addr, addr, None) == E_ALIGN
    # all four at 0 takes the plain gather's launch, after the same checks
    assert _calls(_aug(scale=0.0, jitter=0.0, mask_prob=0.0, chan_drop=0.0), addr, out=addr + 4) == [E_ALIGN] * 2


def test_msig_multis_own_checks_come_first():
    _k, addr = _addr()
    bad = _multi(2)
    bad.slot[1] = 0
    assert _calls(_aug(), addr, m=bad)[1] == E_SHAPE
    bad = _multi(2)
    bad.stride_bytes = 100
    assert _calls(_aug(scale=-1.0), addr, m=bad, T_=510)[1] == E_ALIGN          # before the shape errors of the augmentation
    bad = _multi(0)
    assert _calls(_aug(), addr + 4, m=bad)[1] == E_SHAPE


def test_plain_gather_takes_any_window_length():
    """msig_gather_windows[_multi] (include/msig.h): window_floats is any count >= 1; only a multiple of 4 — the 16-byte copy —
    asks for 16-byte aligned rows.  The augmenting gathers keep their multiple-of-4 rule (test_bad_shapes_are_shape_errors)."""
    _k, addr = _addr()
    lib = L.lib()
    mm = C.byref(_multi())

    def plain(wf, store=addr, idx=addr, out=addr, B_=B, stride=B, m=mm):
        return [lib.msig_gather_windows(store, addr, idx, B_, wf, out, addr, None),
                lib.msig_gather_windows_multi(store, addr, idx, stride, B_, wf, out, addr, m, None)]

    for wf in (0, -1, -4, -CH * 251):
        assert plain(wf, store=addr + 4) == [E_SHAPE] * 2, wf
    for wf in (CH * 251, CH * T):
        for which in ("store", "idx", "out"):
            assert plain(wf, **{which: None}) == [E_NULL] * 2, (wf, which)
        assert plain(wf, m=None)[1] == E_NULL
        assert plain(wf, B_=0) == [E_SHAPE] * 2 and plain(wf, stride=B - 1)[1] == E_SHAPE
    assert plain(CH * T, store=addr + 8) == [E_ALIGN] * 2 and plain(CH * T, out=addr + 4) == [E_ALIGN] * 2
    # 6 x 251 floats: rows are 4-byte aligned at best, and no alignment is asked for — the call gets as far as msig_multi's own checks
    bad = _multi(2)
    bad.slot[1] = 0
    assert plain(CH * 251, store=addr + 4, out=addr + 4, m=C.byref(bad))[1] == E_SHAPE
    assert plain(CH * T, store=addr + 4, out=addr + 4, m=C.byref(bad))[1] == E_ALIGN


# ---- Augment / parse / command line -----------------------------------------------------------------------------------------
def test_augment_round_trips():
    a = Augment(scale=0.1, jitter=0.05, mask_prob=0.5, mask_max=320, chan_drop=0.1)
    assert (a.scale, a.jitter, a.mask_prob, a.mask_max, a.chan_drop) == (0.1, 0.05, 0.5, 320, 0.1) and not a.off
    assert Augment.parse("scale=0.1,jitter=0.05,mask=0.5:320,chandrop=0.1") == a == Augment.parse(a.spec())
    assert a.spec() == "scale=0.1,jitter=0.05,mask=0.5:320,chandrop=0.1"
    assert Augment.parse("chandrop=0.25, scale=2") == Augment(scale=2.0, chan_drop=0.25)
    assert Augment().off and Augment.parse("none").off and Augment().spec() == "none" and Augment.parse(Augment().spec()) == Augment()
    assert Augment(mask_prob=1.0, mask_max=1).spec() == "mask=1.0:1"
    s = a.struct([7, 9])
    assert (s.mask_max, s.reserved, s.key[0], s.key[1], s.key[2]) == (320, 0, 7, 9, 0)
    assert (s.scale_sigma, s.chan_drop_prob) == (np.float32(0.1), np.float32(0.1))
    with pytest.raises(AttributeError):
        a.scale = 1.0
    assert Augment.coerce(None) is None and Augment.coerce(a) is a and Augment.coerce("jitter=0.5") == Augment(jitter=0.5)


@pytest.mark.parametrize("kw", [dict(scale=-0.1), dict(scale=NAN), dict(jitter=-1.0), dict(jitter=NAN), dict(mask_prob=1.1, mask_max=4),
                                dict(mask_prob=-0.5, mask_max=4), dict(mask_prob=NAN, mask_max=4), dict(mask_prob=0.5), dict(mask_prob=0.5, mask_max=0),
                                dict(mask_prob=0.5, mask_max=2.5), dict(chan_drop=1.0), dict(chan_drop=1.0 - 1e-12), dict(chan_drop=-0.1),
                                dict(chan_drop=NAN), dict(scale="0.1"), dict(jitter=None)])
def test_augment_value_errors(kw):
    with pytest.raises(ValueError):
        Augment(**kw)


@pytest.mark.parametrize("spec", ["scale", "scale=", "scale=x", "gain=0.1", "scale=0.1,scale=0.2", "mask=0.5", "mask=0.5:x", "mask=0.5:0",
                                  "chandrop=1", "jitter=-1", "scale=0.1;jitter=0.1"])
def test_parse_value_errors(spec):
    with pytest.raises(ValueError):
        Augment.parse(spec)


def test_window_checks():
    Augment(mask_prob=0.5, mask_max=512).check_window(512)
    with pytest.raises(ValueError):
        Augment(mask_prob=0.5, mask_max=513).check_window(512)
    with pytest.raises(ValueError):
        Augment(scale=0.1).check_window(510)


def test_cli_builds_the_key_only_when_the_flag_is_given():
    from multimodalsignal_amd import main as M
    spec = "scale=0.1,jitter=0.05,mask=0.5:64,chandrop=0.1"
    for mode in ([], ["--ablation"], ["--hierarchical"], ["--model", "cnn_gru_attention", "cnn_gru"], ["--concurrent-folds", "1"]):
        args = M.parse_args(M.build_parser(), ["--synthetic", "x", "--augment", spec, *mode])
        assert M.build_cfg(args, ["cnn_gru_attention"])["augment"] == Augment.parse(spec)
        args = M.parse_args(M.build_parser(), ["--synthetic", "x", *mode])
        assert "augment" not in M.build_cfg(args, ["cnn_gru_attention"])
    for bad in ("scale=-1", "mask=0.5:99999", "nonsense"):
        with pytest.raises(SystemExit):
            M.parse_args(M.build_parser(), ["--synthetic", "x", "--augment", bad])


# ---- statistics of the restatement: derived bounds, fixed seeds ---------------------------------------------------------------
def test_noise_statistics():
    """g over N = 64 * 6 * 512 draws: a standardised 4-term sum of uniform bytes (mean 0, variance 1, kurtosis 2.7).  The sample
    mean has standard deviation 1 / sqrt(N); the sample variance sqrt((kurtosis - 1) / N) = sqrt(1.7 / N); six of each."""
    Bn, Cn, Tn = 64, 6, 512
    ck = R.chan_keys(R.row_keys(R.dropout_key(1234, 1, R.STREAM_ID), Bn), Cn)
    g = R.noise(R._fmix32(ck[:, :, None] ^ np.arange(Tn, dtype=np.uint32)[None, None, :])).astype(np.float64).ravel()
    N = g.size
    assert N == 64 * 6 * 512
    print(f"noise: mean {g.mean():+.3e} (bound {6 / math.sqrt(N):.3e}), var - 1 {g.var() - 1:+.3e} (bound {6 * math.sqrt(1.7 / N):.3e}), "
          f"range [{g.min():.4f}, {g.max():.4f}] within +-{510 * float(R.NOISE_K):.4f}")
    assert abs(g.mean()) <= 6 / math.sqrt(N)
    assert abs(g.var() - 1.0) <= 6 * math.sqrt(1.7 / N)
    assert np.abs(g).max() <= np.float32(510) * R.NOISE_K


def test_mask_and_channel_dropout_statistics():
    """20 000 windows: event fractions within six binomial standard deviations of their probabilities, spans inside the window and
    reaching both of its ends, lengths covering 1..mask_max, never a window with every channel zeroed."""
    N, Cn, Tn, p_mask, mmax, p_drop = 20000, 6, 64, 0.5, 16, 0.3
    d = R.draws(R.dropout_key(99, 7, R.STREAM_ID), N, Cn, Tn, mask_prob=p_mask, mask_max=mmax, chan_drop=p_drop)
    f_mask, f_drop = d["masked"].mean(), d["drawn"].mean()
    sd_mask, sd_drop = math.sqrt(p_mask * (1 - p_mask) / N), math.sqrt(p_drop * (1 - p_drop) / (N * Cn))
    print(f"masked {f_mask:.4f} (p {p_mask}, 6 sd {6 * sd_mask:.4f}); channels drawn {f_drop:.4f} (p {p_drop}, 6 sd {6 * sd_drop:.4f})")
    assert abs(f_mask - p_mask) <= 6 * sd_mask
    assert abs(f_drop - p_drop) <= 6 * sd_drop
    ln, t0 = d["length"], d["t0"]
    assert ln.min() == 1 and ln.max() == mmax and set(ln.tolist()) == set(range(1, mmax + 1))
    assert t0.min() == 0 and (t0 + ln).max() == Tn and (t0 >= 0).all() and (t0 + ln <= Tn).all()
    assert not d["dropped"].all(axis=1).any()
    # the keep-one rule changes only the rows whose every channel was drawn, and exactly one channel of each
    allrows = d["drawn"].all(axis=1)
    assert (d["dropped"][~allrows] == d["drawn"][~allrows]).all() and (d["dropped"][allrows].sum(axis=1) == Cn - 1).all()
    # with few channels and a high probability the rule has rows to act on
    d2 = R.draws(R.dropout_key(5, 1, R.STREAM_ID), N, 2, Tn, chan_drop=0.9)
    assert d2["drawn"].all(axis=1).sum() > N // 2 and not d2["dropped"].all(axis=1).any()
    assert set(np.nonzero(~d2["dropped"][d2["drawn"].all(axis=1)])[1].tolist()) == {0, 1}          # the hash keeps either channel


def test_restatement_skips_transforms_at_zero_and_keys_rows_not_windows():
    rs = np.random.RandomState(0)
    store = rs.randn(5, 3, 16).astype(np.float32)
    store[0, 0, :4] = -0.0
    idx = np.array([0, 3, 0, 4])
    key = R.dropout_key(1, 1, R.STREAM_ID)
    assert R.augment(store, idx, key).tobytes() == store[idx].tobytes()
    y = R.augment(store, idx, key, scale=0.2, jitter=0.1)
    assert not np.array_equal(y[0], y[2])                 # window 0 twice in the batch: augmented twice, differently
    assert not np.array_equal(R.augment(store, idx, key + 1, scale=0.2, jitter=0.1), y)
    assert np.signbit(R.augment(store, idx, key, scale=0.2)[0, 0, :4]).all()       # -0.0 * gain stays -0.0: nothing was added
