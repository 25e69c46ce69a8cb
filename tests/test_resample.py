"""The causal polyphase FIR resampler on the CPU tier (include/msig_rs.h, multimodalsignal_amd/resample.py):
the tap table against scipy's firwin, the output count against a count taken one output at a time, the definition's restatement
(tests/rs_reference.py) against scipy.signal.resample_poly, a constant input, and the refusals.  Nothing here needs a GPU: the library
loads without one, and its host functions are called through the C ABI."""
import numpy as np
import pytest

import rs_reference as RS
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd import resample as res

RATIOS = [(16, 175), (2, 3), (3, 2), (1, 7), (7, 1)]
IDS = [f"{up}over{down}" for up, down in RATIOS]


def _half(up, down):
    return 10 * max(up, down)


def _walk(n, cols, seed):
    """A random walk at a scale of about 16: a slip of one sample or one phase errs at the scale of its steps."""
    rs = np.random.RandomState(seed)
    x = np.cumsum(rs.randn(n, cols), axis=0)
    return np.ascontiguousarray(x * (16.0 / np.abs(x).max()))


@pytest.mark.parametrize("up,down", RATIOS, ids=IDS)
def test_taps_are_scipys_firwin(up, down):
    from scipy import signal
    half = _half(up, down)
    want = signal.firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
    got = res.fir_taps(up, down)
    assert got.dtype == np.float64 and got.shape == want.shape
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"{up}/{down}: taps against firwin {err:.3g} of max|h|")
    assert err <= 1e-14
    assert np.array_equal(got, got[::-1])                        # zero phase: the table is symmetric to the bit


def test_ratio_of_wesads_chest_device():
    assert res.ratio(700, 64) == (16, 175) and res.ratio(700.0, 64.0) == (16, 175) and res.ratio(64, 700) == (175, 16)
    r = res.FirResampler(700, 64, "cpu")
    assert (r.L, r.M, r.half, r.taps.shape[0], r.tail_rows) == (16, 175, 1750, 3501, 219)
    assert r.out_count(5000) == 448 and r.max_rows(448) == 5009 and r.out_count(5010) == 449
    assert len(range(*RS.support(300, 16, 175, 1750))) + 1 == 219           # taps of one output
    assert abs(r.latency_s - 110 / 700) < 1e-15
    assert "700" in r.spelling and "64" in r.spelling and "16/175" in r.spelling


@pytest.mark.parametrize("up,down", RATIOS, ids=IDS)
def test_out_count_against_a_count_one_by_one(up, down):
    half = _half(up, down)
    lib = L.lib()
    for n in range(0, 3 * (2 * half // up) + 1):
        want = RS.out_count_brute(n, up, down, half)
        assert res.out_count(n, up, down, half) == want, n
        assert lib.msig_rs_out_count(n, up, down, half) == want, n
    r = res.FirResampler(down, up, "cpu")                        # fs_out / fs_in = up / down
    for k in range(0, 12):
        assert r.out_count(r.max_rows(k)) <= k < r.out_count(r.max_rows(k) + 1)


def test_out_count_refuses_through_the_c_abi():
    lib = L.lib()
    assert lib.msig_rs_abi_version() == L.RS_ABI_VERSION
    for args in [(-1, 16, 175, 1750), (10, 0, 175, 1750), (10, 16, 0, 1750), (10, 4097, 1, 40970), (10, 1, 4097, 40970), (10, 3, 3, 30),
                 (10, 4, 6, 60), (10, 16, 175, 174), (10, 16, 175, L.RS_MAX_HALF + 1)]:
        assert lib.msig_rs_out_count(*args) == -2, args


@pytest.mark.parametrize("up,down", RATIOS, ids=IDS)
def test_restatement_is_resample_polys_head(up, down):
    from scipy import signal
    half = _half(up, down)
    n_in = 5000 if (up, down) == (16, 175) else 40 * (2 * half // up) + 3
    x = _walk(n_in, 3, 100 * up + down)
    h = res.fir_taps(up, down)
    got = RS.resample(x, h, up, down, half)
    want = signal.resample_poly(x, up, down, axis=0)
    n = res.out_count(n_in, up, down, half)
    assert got.shape == (n, 3) and 0 < n <= want.shape[0]
    if (up, down) == (16, 175):
        assert (n, want.shape[0]) == (448, 458)
    err = np.abs(got - want[:n]).max()
    step = np.abs(np.diff(x, axis=0)).max()
    print(f"{up}/{down}: restatement against resample_poly {err:.3g} at a signal scale of {np.abs(x).max():.3g}; largest step {step:.3g}")
    assert err <= 1e-9 * np.abs(x).max()
    ld = RS.resample(x, h, up, down, half, np.longdouble)
    assert ld.dtype == np.longdouble and np.abs(got - ld).max() <= 1e-12 * np.abs(x).max()


@pytest.mark.parametrize("up,down", RATIOS, ids=IDS)
def test_constant_input_gives_the_constant_in_the_interior(up, down):
    """An interior output of the constant c is c times the sum of its phase's taps.  The table sums to `up`, and the sum of one phase
    differs from 1 by the filter's response at the up - 1 images of DC, each below the Kaiser window's stop-band ripple:
    A = beta / 0.1102 + 8.7 = 54.1 dB at beta = 5, delta = 10^(-A / 20) = 1.98e-3.  Bound: (up - 1) delta |c|, plus 1e-12 |c| for the
    float64 sums (where up = 1 there is no image and the one phase is the whole table)."""
    half = _half(up, down)
    n_in = 12 * (2 * half // up) + 5
    c = 3.75
    y = RS.resample(np.full((n_in, 2), c), res.fir_taps(up, down), up, down, half)
    inner = [m for m in range(y.shape[0]) if m * down - half >= 0]
    assert len(inner) > 10
    err = np.abs(y[inner] - c).max()
    bound = ((up - 1) * 10 ** (-(5.0 / 0.1102 + 8.7) / 20) + 1e-12) * c
    print(f"{up}/{down}: constant {c}: largest deviation {err:.3g}, bound {bound:.3g}")
    assert err <= bound


def test_refusals():
    for fs_in, fs_out in [(700, 64.1), (64, 64), (64.0, 64), (1, 4097), (4097, 1), (700, 0), (-700, 64), (float("nan"), 64), (np.pi, 64)]:
        with pytest.raises(ValueError):
            res.ratio(fs_in, fs_out)
        with pytest.raises(ValueError):
            res.FirResampler(fs_in, fs_out, "cpu")
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            res.FirResampler(700, 64, "cpu", half_width=bad)
    with pytest.raises(ValueError):
        res.FirResampler(700, 64, "cpu", beta=-1.0)
    with pytest.raises(ValueError):
        res.FirResampler(4096, 1, "cpu", half_width=2000)        # more taps than the library takes
    with pytest.raises(ValueError):
        res.FirResampler(700, 64, "cpu").apply(np.zeros((10, 2)))      # taps on the CPU: there is no CPU fallback
    from multimodalsignal_amd import preprocess
    with pytest.raises(ValueError):
        preprocess.resample_signal(np.zeros(100), 700, 64, method="linear")


def test_calls_refuse_over_fake_pointers_before_any_launch():
    """The checks of msig_rs_resample and msig_rs_lv_push come before any launch, so they answer without a GPU and never touch memory:
    the pointers here are made-up addresses."""
    import ctypes as C
    lib = L.lib()
    P, H = 0x10000, 0x20000
    i32, i64 = lambda *v: (C.c_int32 * len(v))(*v), lambda *v: (C.c_int64 * len(v))(*v)      # noqa: E731
    off = dict(x=P, n_in=5000, C_all=3, h=H, L=16, M=175, half=1750, y=0x30000, n_out=448)
    for name, value, code in [("h", None, -1), ("x", None, -1), ("y", None, -1), ("n_out", 449, -2), ("n_out", 458, -2), ("C_all", 0, -2),
                              ("L", 32, -2), ("M", 16, -2), ("half", 174, -2), ("x", P + 4, -3), ("y", 0x30004, -3), ("h", H + 2, -3)]:
        a = dict(off, **{name: value})
        assert lib.msig_rs_resample(*[a[k] for k in ("x", "n_in", "C_all", "h", "L", "M", "half", "y", "n_out")], None) == code, (name, value)
    live = dict(pool=P, sessions=4, R=100, ring_bytes=6400, C_all=8, tails=0x40000, tail_rows=219, tail_bytes=219 * 64, h=H, L=16, M=175, half=1750,
                sess=i32(0, 3), raw=i64(0, 500), len=i64(300, 700), n=2, staging=0x50000)
    order = ("pool", "sessions", "R", "ring_bytes", "C_all", "tails", "tail_rows", "tail_bytes", "h", "L", "M", "half", "sess", "raw", "len", "n", "staging")
    for name, value, code in [("pool", None, -1), ("tails", None, -1), ("h", None, -1), ("sess", None, -1), ("raw", None, -1), ("len", None, -1),
                              ("sessions", 4097, -2), ("R", 0, -2), ("ring_bytes", 6392, -2), ("L", 175, -2), ("L", 35, -2), ("M", 4097, -2),
                              ("half", 174, -2), ("tail_rows", 218, -2), ("tail_bytes", 219 * 64 - 8, -2), ("n", 0, -2), ("n", 5, -2),
                              ("sess", i32(0, 4), -2), ("sess", i32(3, 3), -2), ("raw", i64(0, -1), -2), ("len", i64(-1, 700), -2),
                              ("len", i64(300, 1097), -2), ("pool", P + 4, -3), ("tails", 0x40004, -3), ("staging", 0x50004, -3),
                              ("ring_bytes", 6404, -3), ("tail_bytes", 219 * 64 + 4, -3), ("h", H + 4, -3)]:
        a = dict(live, **{name: value})
        assert lib.msig_rs_lv_push(*[a[k] for k in order], None) == code, (name, value)
