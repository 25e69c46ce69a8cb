"""Causal running references on the GPU, kernel level through the C ABI (include/msig_rn.h): the statistics
tables against the np.longdouble restatement (tests/rn_reference.py) with the float64 restatement's own error as the yardstick, the
rows bit for bit from the device's own table, one record for all rows against msig_rec_windows, the arena slots, trailing:K with
K > N against expanding, and the independence of the window sums from the batch.

Cases: S divides T (16, 4), S does not (10, 3), S > T (4, 7), a single sample (T = 1), one past the workgroup (T = 257), above
workgroup x waves (T = 1030); C = 1 (with and without the log1p bit) and C = 16 (one log1p bit); N = 1 and N = 40; K = 0, 1, 2, 7 and
K > N; a constant channel (the variance clamps at 0) and an offset channel (every sample after the pivot lies 1e4 away from it).

The statistics test prints every figure it asserts on; what they were on an MI355X is in its docstring."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import rn_reference as R
from multimodalsignal_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = float(np.finfo(np.float64).eps)
MC = L.MAX_C

C_ALL = 18
LOG_COL, TEMP_COL, CONST_COL, OFFSET_COL = 1, 3, 6, 9
COLS = {"16of18": [17, 2, 0, 3, 1, 6, 5, 4, 9, 8, 7, 12, 16, 10, 15, 13], "1log": [LOG_COL], "1off": [OFFSET_COL]}
TS = [(16, 4), (10, 3), (4, 7), (1, 1), (257, 5), (1030, 64)]
NS = [1, 40]
KS = [0, 1, 2, 7, 41]                          # 41 > N for both N
CASES = [(T, S, N, key) for T, S in TS for N in NS for key in COLS]
IDS = [f"t{T}-s{S}-n{N}-{key}" for T, S, N, key in CASES]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "the gpu tier needs an MI355X"


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _mask_of(cols):
    return sum(1 << c for c, col in enumerate(cols) if col == LOG_COL)


@functools.lru_cache(maxsize=None)
def _recording(T, S, N):
    """(L, 18) float64 with a slow drift and a tail no window covers.  Column 1 is positive and heavy-tailed (the one under log1p), 3
    has mean >> spread, 6 is exactly constant, 9 is the offset channel: sample 0 — the pivot — near 0, every later sample near 1e4."""
    Ln = (N - 1) * S + T + min(3, S - 1)
    rs = np.random.RandomState(7000 * T + 10 * S + N)
    spread = 0.5 + rs.rand(C_ALL)
    sig = rs.randn(Ln, C_ALL) * spread + rs.randn(C_ALL) + 0.7 * spread * np.sin(2 * np.pi * np.arange(Ln) / Ln)[:, None]
    sig[:, LOG_COL] = np.exp(0.8 * rs.randn(Ln) + 0.5 * np.sin(2 * np.pi * np.arange(Ln) / Ln)) + 0.1
    sig[:, TEMP_COL] = 33.0 + 0.05 * rs.randn(Ln) + 0.03 * np.arange(Ln) / Ln
    sig[:, CONST_COL] = 0.75
    sig[:, OFFSET_COL] = rs.randn(Ln) + 1e4 * (np.arange(Ln) > 0)
    sig = np.ascontiguousarray(sig)
    assert R.count(Ln, T, S) == N
    return sig, torch.from_numpy(sig).to(DEV)


def _head(dev, cols, T, S):
    return dev.data_ptr(), dev.shape[0], dev.shape[1], (C.c_int32 * len(cols))(*cols), len(cols), _mask_of(cols), T, S


def _sums(T, S, N, key, n0=0, B=None):
    _sig, dev = _recording(T, S, N)
    B = N - n0 if B is None else B
    out = torch.full((B + 1, 2 * MC), float("nan"), dtype=torch.float64, device=DEV)
    L.check(L.lib().msig_rn_sums(*_head(dev, COLS[key], T, S), n0, B, out.data_ptr(), _stream()), "msig_rn_sums")
    torch.cuda.synchronize()
    assert torch.isnan(out[B]).all(), "wrote past the table"
    return out[:B]


def _device_now(T, S, N, key):
    """The window sums of all N windows (one call) and the statistics table per K."""
    _sig, dev = _recording(T, S, N)
    sums = _sums(T, S, N, key)
    tables = {}
    for K in KS:
        tab = torch.full((N + 1, 2 * MC + 1), float("nan"), dtype=torch.float64, device=DEV)
        L.check(L.lib().msig_rn_stats(*_head(dev, COLS[key], T, S), sums.data_ptr(), N, K, tab.data_ptr(), _stream()), "msig_rn_stats")
        torch.cuda.synchronize()
        assert torch.isnan(tab[N]).all(), "wrote past the table"
        tables[K] = tab[:N]
    return sums, tables


_device = functools.lru_cache(maxsize=None)(_device_now)          # computed once, shared by the tests


def _selected(rec, Cn):
    """The written entries of records (N, 2 MAX_C + 1): the selected channels' mean and inv, and the count."""
    return np.concatenate([rec[:, :Cn], rec[:, MC:MC + Cn], rec[:, 2 * MC:]], axis=1)


@functools.lru_cache(maxsize=None)
def _restated(T, S, N, key):
    sig, _dev = _recording(T, S, N)
    cols = COLS[key]
    return R.transformed(sig, cols, _mask_of(cols), np.float64), R.transformed(sig, cols, _mask_of(cols), np.longdouble)


# ---- 1. the statistics ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S,N,key", CASES, ids=IDS)
def test_statistics_against_the_longdouble_restatement(T, S, N, key):
    """msig_rn_sums + msig_rn_stats against rn_reference's np.longdouble restatement, for K = 0, 1, 2, 7 and K > N.  The error of a
    mean is measured in units of the std of the window's reference (two passes over its materialised samples in np.longdouble), the
    error of 1 / (std + 1e-8) in units of itself.  Bound, per channel and statistic: 8 x the float64 restatement's own error against
    np.longdouble ON THE SAME CASE — its largest over the case's windows, since the ratio of two roundings of one window is
    unbounded whenever the restatement's happens to land on the reference — or, where that is smaller, a floor of 4 float64 ulps of
    the value: of |mean| + std for the mean (the scale its error is measured on: the finalisation alone rounds two divisions, the
    fused variance, the square root, the sum with the pivot and the reciprocal, half an ulp each), of the value for the reciprocal.
    Where the reference's samples are all EQUAL (std = 0: the constant channel, window 0 of T = 1, every window of T = 1 under
    K = 1) neither unit exists, and the condition is absolute: the mean within 4 ulps of |mean| + |pivot|; the fused variance is the
    rounding error of an exactly vanishing difference, at most 2 eps dm^2 (half an ulp of A2 / count and of dm^2), so
    1 / (sqrt(2 eps) |dm| + 1e-8) <= inv <= 1e8, and exactly 1e8 where the samples equal the pivot (dm = 0: the clamp).
    The counts are exact.  Two calls give the same bits.
    Measured on an MI355X over all 36 cases (profiles/running_parity.log): error / bound at most 0.125 for the
    mean — the device's means have the float64 restatement's bits, which adds in the same order — and at most 0.586 for
    1 / (std + 1e-8) (T = 1, N = 40, 16 channels, K = 2); 33 of the 36 cases at or below 0.26."""
    sums, tables = _device(T, S, N, key)
    v64, vld = _restated(T, S, N, key)
    Cn = v64.shape[1]
    worst_mean, worst_inv, stds = 0.0, 0.0, {}
    for K in KS:
        got = tables[K].cpu().numpy()
        m_ld, i_ld, cnt = R.stats_table(vld, T, S, K)
        m_64, i_64, _c = R.stats_table(v64, T, S, K)
        span = 0 if K > N else K                                  # K > N has expanding's reference windows
        std = stds[span] = stds[span] if span in stds else R.std_longdouble(vld, T, S, span)
        assert np.array_equal(got[:, 2 * MC], cnt.astype(np.float64))
        assert np.all(np.isnan(got[:, Cn:MC])) and np.all(np.isnan(got[:, MC + Cn:2 * MC]))          # only the selected channels' slots
        flat = std == 0
        pos = ~flat
        safe = np.where(pos, std, 1)
        e_mean, o_mean = np.abs(got[:, :Cn] - m_ld), np.abs(m_64 - m_ld)
        e_inv, o_inv = np.abs(got[:, MC:MC + Cn] - i_ld) / i_ld, np.abs(i_64 - i_ld) / i_ld
        r_mean, q_mean = np.where(pos, e_mean / safe, 0), np.where(pos, o_mean / safe, 0)
        r_inv, q_inv = np.where(pos, e_inv, 0), np.where(pos, o_inv, 0)
        yard_mean, yard_inv = 8 * q_mean.max(axis=0), 8 * q_inv.max(axis=0)                       # per channel, over the case's windows
        floor_mean = 4 * EPS * (np.abs(m_ld) + std) / safe
        bound_mean, bound_inv = np.maximum(yard_mean[None, :], floor_mean), np.maximum(yard_inv[None, :], 4 * EPS)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio_mean = float(np.nan_to_num((r_mean / bound_mean).astype(np.float64)).max())
            ratio_inv = float(np.nan_to_num((r_inv / bound_inv).astype(np.float64)).max())
        worst_mean, worst_inv = max(worst_mean, ratio_mean), max(worst_inv, ratio_inv)
        print(f"msig_rn_stats T={T} S={S} N={N} {key} K={K}: mean error / std max {float(r_mean.max()):.3e} (float64 restatement's "
              f"{float(q_mean.max()):.3e}); inv relative error max {float(r_inv.max()):.3e} (restatement's {float(q_inv.max()):.3e}); "
              f"error / bound max: mean {ratio_mean:.3f}, inv {ratio_inv:.3f}; {int(flat.sum())} entries with std = 0")
        assert np.all(r_mean <= bound_mean), (K, r_mean.max(), yard_mean)
        assert np.all(r_inv <= bound_inv), (K, r_inv.max(), yard_inv)
        if flat.any():
            p = vld[0][None, :].repeat(N, axis=0)
            dm = np.abs(m_ld - p)
            g_mean, g_inv = got[:, :Cn][flat], got[:, MC:MC + Cn][flat]
            assert np.all(np.abs(g_mean - m_ld[flat]) <= 4 * EPS * (np.abs(m_ld[flat]) + np.abs(p[flat])))
            assert np.all(g_inv <= 1e8) and np.all(g_inv >= (1 / (np.sqrt(2 * EPS) * dm[flat] + 1e-8)).astype(np.float64) * (1 - 4 * EPS))
            assert np.all(g_inv[dm[flat] == 0] == 1e8) and np.all(g_mean[dm[flat] == 0] == p[flat][dm[flat] == 0].astype(np.float64))
    if CONST_COL in COLS[key]:
        c = COLS[key].index(CONST_COL)
        for K in KS:
            got = tables[K].cpu().numpy()
            assert np.all(got[:, c] == 0.75) and np.all(got[:, MC + c] == 1e8)                      # the variance clamps at 0
    print(f"msig_rn_stats T={T} S={S} N={N} {key}: error / bound at most {worst_mean:.3f} (mean), {worst_inv:.3f} (inv)")
    again = _device_now(T, S, N, key)
    for sl in (slice(0, Cn), slice(MC, MC + Cn)):
        assert np.array_equal(again[0].cpu().numpy()[:, sl].view(np.uint64), sums.cpu().numpy()[:, sl].view(np.uint64))
    for K in KS:
        assert np.array_equal(_selected(again[1][K].cpu().numpy(), Cn).view(np.uint64), _selected(tables[K].cpu().numpy(), Cn).view(np.uint64))


# ---- 2. the rows ---------------------------------------------------------------------------------------------------------------------
def _rn_windows(T, S, N, key, table, n0=0, B=None):
    _sig, dev = _recording(T, S, N)
    cols = COLS[key]
    B = N - n0 if B is None else B
    n = B * len(cols) * T
    out = torch.full((n + 64,), -77.0, dtype=torch.float32, device=DEV)
    L.check(L.lib().msig_rn_windows(*_head(dev, cols, T, S), n0, B, table.data_ptr(), out.data_ptr(), _stream()), "msig_rn_windows")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[n:] == -77.0), "wrote past the batch"
    return got[:n].reshape(B, len(cols), T)


def _rec_windows(T, S, N, key, stats, n0, B):
    _sig, dev = _recording(T, S, N)
    cols = COLS[key]
    out = torch.empty((B, len(cols), T), dtype=torch.float32, device=DEV)
    L.check(L.lib().msig_rec_windows(*_head(dev, cols, T, S), n0, B, stats.data_ptr(), out.data_ptr(), _stream()), "msig_rec_windows")
    return out


@pytest.mark.parametrize("T,S,N,key", CASES, ids=IDS)
def test_rows_from_the_devices_own_table_bit_for_bit(T, S, N, key):
    """msig_rn_windows with the device's own table (K = 0 and K = 2; for N = 40 also windows [3, 40) alone): every row equals the
    restatement's (float)((v - mean_b) * inv_b) with row b's record bit for bit.  The channel under log1p is compared the way
    tests/test_recording_gpu.py compares it — against the library's own log1p: msig_rec_windows of that single window with row b's
    record as its statistics, which every other channel equals too."""
    _sums_, tables = _device(T, S, N, key)
    v64, _vld = _restated(T, S, N, key)
    cols = COLS[key]
    plain = [c for c, col in enumerate(cols) if col != LOG_COL]
    for K in (0, 2):
        tab = tables[K].contiguous()
        host = tab.cpu().numpy()
        for n0 in ((0, 3) if N > 3 else (0,)):
            got = _rn_windows(T, S, N, key, tab[n0:].contiguous(), n0)
            want = R.rows(v64, T, S, n0, host[n0:, :len(cols)], host[n0:, MC:MC + len(cols)])
            assert got.shape == want.shape
            assert np.array_equal(got[:, plain].view(np.uint32), want[:, plain].view(np.uint32)), (K, n0)
            one = torch.stack([_rec_windows(T, S, N, key, tab[n], n, 1)[0] for n in range(n0, N)])
            torch.cuda.synchronize()
            assert np.array_equal(got.view(np.uint32), one.cpu().numpy().view(np.uint32)), (K, n0)
        if N > 1 and T > 1:
            assert np.any(got != 0) and np.all(np.isfinite(got))
    if N == 40 and key != "1log":               # the records differ from window to window
        assert host[5, plain[0]] != host[30, plain[0]]


# ---- 3. one record for all rows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S,N,key", [c for c in CASES if c[2] == 40], ids=[i for c, i in zip(CASES, IDS) if c[2] == 40])
def test_one_record_for_all_rows_is_msig_rec_windows(T, S, N, key):
    _sig, dev = _recording(T, S, N)
    lib = L.lib()
    stats = torch.zeros(2 * MC + 1, dtype=torch.float64, device=DEV)
    scratch = torch.empty(lib.msig_rec_scratch_bytes(), dtype=torch.uint8, device=DEV)
    L.check(lib.msig_rec_stats(*_head(dev, COLS[key], T, S), 2, 11, stats.data_ptr(), scratch.data_ptr(), _stream()), "msig_rec_stats")
    for n0, B in ((0, N), (5, 17)):
        want = _rec_windows(T, S, N, key, stats, n0, B)
        got = _rn_windows(T, S, N, key, stats[None, :].repeat(B, 1).contiguous(), n0, B)
        assert np.array_equal(got.view(np.uint32), want.cpu().numpy().view(np.uint32)), (n0, B)


# ---- 4. the arena slots --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S,key", [(16, 4, "16of18"), (10, 3, "1log"), (4, 7, "16of18"), (257, 5, "1off"), (1030, 64, "16of18")])
def test_multi_fills_every_slot_with_the_same_bits(T, S, key):
    """msig_rn_windows_multi into arena slots 2 and 0 of three: both hold msig_rn_windows' bits, slot 1 and the rest of every arena
    stay as they were."""
    from multimodalsignal_amd.runtime import Arenas
    N, Cn = 40, len(COLS[key])
    _sig, dev = _recording(T, S, N)
    tab = _device(T, S, N, key)[1][7].contiguous()
    ar = Arenas(3, DEV, (("other", 1000), ("x", 16 * Cn * T * 4), ("tail", 256)))
    for n0, B in ((0, 16), (16, 16), (32, 5)):
        want = _rn_windows(T, S, N, key, tab[n0:].contiguous(), n0, B)
        ar.mem.fill_(0x5A)
        L.check(L.lib().msig_rn_windows_multi(*_head(dev, COLS[key], T, S), n0, B, tab[n0].data_ptr(), ar.ptr("x"), C.byref(ar.multi([2, 0])),
                                              _stream()), "msig_rn_windows_multi")
        torch.cuda.synchronize()
        n = B * Cn * T
        for s in (0, 2):
            x = ar.view(s, "x", torch.float32).cpu().numpy()
            assert np.array_equal(x[:n].view(np.uint32), want.reshape(-1).view(np.uint32)), (n0, s)
            assert np.all(x[n:].view(np.uint8) == 0x5A)
            assert np.all(ar.view(s, "other").cpu().numpy() == 0x5A) and np.all(ar.view(s, "tail").cpu().numpy() == 0x5A)
        assert np.all(ar.mem[1].cpu().numpy() == 0x5A)


# ---- 5. trailing against expanding ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S,N,key", CASES, ids=IDS)
def test_trailing_with_k_above_n_is_expanding_on_the_device(T, S, N, key):
    _sums_, tables = _device(T, S, N, key)
    Cn = len(COLS[key])
    ex = _selected(tables[0].cpu().numpy(), Cn)
    assert np.array_equal(_selected(tables[41].cpu().numpy(), Cn).view(np.uint64), ex.view(np.uint64))
    for K in (1, 2, 7):                         # and below N: the first K windows are expanding's, the counts saturate
        tr = _selected(tables[K].cpu().numpy(), Cn)
        assert np.array_equal(tr[:K].view(np.uint64), ex[:K].view(np.uint64))
        assert list(tr[:, -1]) == [min(n + 1, K) for n in range(N)]
    if N == 40:
        assert not np.array_equal(_selected(tables[7].cpu().numpy(), Cn)[7:, :Cn], ex[7:, :Cn])


# ---- 6. batch independence -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S,key", [(T, S, key) for T, S in TS for key in COLS], ids=[f"t{T}-s{S}-{key}" for T, S in TS for key in COLS])
def test_window_sums_do_not_depend_on_the_batch(T, S, key):
    N, Cn = 40, len(COLS[key])
    whole = _device(T, S, N, key)[0].cpu().numpy()
    parts = np.concatenate([_sums(T, S, N, key, 0, 3).cpu().numpy(), _sums(T, S, N, key, 3, N - 3).cpu().numpy()])
    for sl in (slice(0, Cn), slice(MC, MC + Cn)):
        assert np.array_equal(parts[:, sl].view(np.uint64), whole[:, sl].view(np.uint64))
    assert np.all(np.isnan(whole[:, Cn:MC])) and np.all(np.isnan(whole[:, MC + Cn:]))
