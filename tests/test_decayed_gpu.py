"""The decayed running reference on the GPU, kernel level through the C ABI (include/msig_rd.h): msig_rd_stats
at its two exact anchors against msig_rn_stats, its tables against the np.longdouble restatement (tests/rd_reference.py) with the
float64 restatement's own error as the yardstick — tests/test_running_gpu.py's construction with unchanged constants — and the rows
msig_rn_windows forms from the device's own table, bit for bit.

Cases: (T, S) = (16, 4), (10, 3), a single sample (1, 1), one past the workgroup's stride (257, 5); C = 16 of 18 with one log1p bit, a
constant channel and a channel offset 1e4 from its pivot, and C = 1 (the offset channel); N = 1 and N = 40 (more than two blocks of
records loaded ahead); lambda = 0 and 1 (the anchors), 0.5, exp2(-1/3), exp2(-1/60).  The recordings are test_running_gpu's.

The statistics test prints every figure it asserts on; what they were on an MI355X is in its docstring."""
import functools

import numpy as np
import pytest
import torch

import rd_reference as RD
import rn_reference as R
import test_running_gpu as G
from multimodalsignal_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = G.DEV
EPS = G.EPS
MC = L.MAX_C
COLS = {k: G.COLS[k] for k in ("16of18", "1off")}
TS = [(16, 4), (10, 3), (1, 1), (257, 5)]
NS = [1, 40]
ANCHORS = [(1.0, 0), (0.0, 1), (-0.0, 1)]                         # lambda, msig_rn_stats' K
DECAYS = {"half": 0.5, "h3": float(np.exp2(-1.0 / 3)), "h60": float(np.exp2(-1.0 / 60))}
CASES = [(T, S, N, key) for T, S in TS for N in NS for key in COLS]
IDS = [f"t{T}-s{S}-n{N}-{key}" for T, S, N, key in CASES]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "the gpu tier needs an MI355X"


def _rd_table(T, S, N, key, lam, sums):
    _sig, dev = G._recording(T, S, N)
    tab = torch.full((N + 1, 2 * MC + 1), float("nan"), dtype=torch.float64, device=DEV)
    L.check(L.lib().msig_rd_stats(*G._head(dev, COLS[key], T, S), sums.data_ptr(), N, lam, tab.data_ptr(), G._stream()), "msig_rd_stats")
    torch.cuda.synchronize()
    assert torch.isnan(tab[N]).all(), "wrote past the table"
    return tab[:N]


def _rn_table(T, S, N, key, K, sums):
    _sig, dev = G._recording(T, S, N)
    tab = torch.full((N, 2 * MC + 1), float("nan"), dtype=torch.float64, device=DEV)
    L.check(L.lib().msig_rn_stats(*G._head(dev, COLS[key], T, S), sums.data_ptr(), N, K, tab.data_ptr(), G._stream()), "msig_rn_stats")
    torch.cuda.synchronize()
    return tab


@functools.lru_cache(maxsize=None)
def _device(T, S, N, key):
    """The window sums (one msig_rn_sums) and msig_rd_stats' table per decay — computed once, shared by the tests."""
    sums = G._sums(T, S, N, key).contiguous()
    return sums, {name: _rd_table(T, S, N, key, lam, sums) for name, lam in DECAYS.items()}


# ---- 1. the anchors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S,N,key", CASES, ids=IDS)
def test_the_anchors_are_msig_rn_stats_bit_for_bit(T, S, N, key):
    """lambda = 1: msig_rn_stats(K = 0)'s table, c_n = n + 1; lambda = 0 (and -0.0): msig_rn_stats(K = 1)'s, c_n = 1."""
    sums, _tabs = _device(T, S, N, key)
    Cn = len(COLS[key])
    for lam, K in ANCHORS:
        got, want = _rd_table(T, S, N, key, lam, sums).cpu().numpy(), _rn_table(T, S, N, key, K, sums).cpu().numpy()
        assert np.array_equal(G._selected(got, Cn).view(np.uint64), G._selected(want, Cn).view(np.uint64)), (lam, K)
        assert list(got[:, 2 * MC]) == [float(n + 1) if K == 0 else 1.0 for n in range(N)]
        assert np.all(np.isnan(got[:, Cn:MC])) and np.all(np.isnan(got[:, MC + Cn:2 * MC]))        # only the selected channels' slots


# ---- 2. the statistics ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S,N,key", CASES, ids=IDS)
def test_statistics_against_the_longdouble_restatement(T, S, N, key):
    """msig_rn_sums + msig_rd_stats against rd_reference's np.longdouble restatement, for lambda = 0.5, exp2(-1/3) and exp2(-1/60).
    The bound is tests/test_running_gpu.py's, constants unchanged: the error of a mean in units of the (weighted) std of the window's
    reference, the error of 1 / (std + 1e-8) in units of itself; per channel and statistic 8 x the float64 restatement's own error
    against np.longdouble on the same case (its largest over the case's windows) or, where that is smaller, a floor of 4 float64
    ulps — of |mean| + std for the mean, of the value for the reciprocal.  Where the reference's samples are all equal (std = 0: the
    constant channel, window 0 of T = 1) the condition is absolute, as there.  c_n is compared with the float64 restatement's exactly:
    both are one fma per window.  Two calls give the same bits.
    Measured on an MI355X over all 16 cases and the three decays: error / bound at most 0.125 for the mean
    — the device's means have the float64 restatement's bits — and at most 0.255 for 1 / (std + 1e-8) (T = 16, S = 4, N = 1, 16
    channels); every N = 40 case at or below 0.20."""
    sums, tables = _device(T, S, N, key)
    v64, vld = G._restated(T, S, N, key)
    Cn = v64.shape[1]
    worst_mean, worst_inv = 0.0, 0.0
    for name, lam in DECAYS.items():
        got = tables[name].cpu().numpy()
        m_ld, i_ld, _c = RD.stats_table(vld, T, S, lam)
        m_64, i_64, c_64 = RD.stats_table(v64, T, S, lam)
        std = RD.std_longdouble(vld, T, S, lam)
        assert np.array_equal(got[:, 2 * MC].view(np.uint64), c_64.view(np.uint64))
        assert np.all(np.isnan(got[:, Cn:MC])) and np.all(np.isnan(got[:, MC + Cn:2 * MC]))
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
        print(f"msig_rd_stats T={T} S={S} N={N} {key} decay={name}: mean error / std max {float(r_mean.max()):.3e} (float64 restatement's "
              f"{float(q_mean.max()):.3e}); inv relative error max {float(r_inv.max()):.3e} (restatement's {float(q_inv.max()):.3e}); "
              f"error / bound max: mean {ratio_mean:.3f}, inv {ratio_inv:.3f}; {int(flat.sum())} entries with std = 0")
        assert np.all(r_mean <= bound_mean), (name, r_mean.max(), yard_mean)
        assert np.all(r_inv <= bound_inv), (name, r_inv.max(), yard_inv)
        if flat.any():
            p = vld[0][None, :].repeat(N, axis=0)
            dm = np.abs(m_ld - p)
            g_mean, g_inv = got[:, :Cn][flat], got[:, MC:MC + Cn][flat]
            assert np.all(np.abs(g_mean - m_ld[flat]) <= 4 * EPS * (np.abs(m_ld[flat]) + np.abs(p[flat])))
            assert np.all(g_inv <= 1e8) and np.all(g_inv >= (1 / (np.sqrt(2 * EPS) * dm[flat] + 1e-8)).astype(np.float64) * (1 - 4 * EPS))
            assert np.all(g_inv[dm[flat] == 0] == 1e8) and np.all(g_mean[dm[flat] == 0] == p[flat][dm[flat] == 0].astype(np.float64))
        if G.CONST_COL in COLS[key]:
            c = COLS[key].index(G.CONST_COL)
            assert np.all(got[:, c] == 0.75) and np.all(got[:, MC + c] == 1e8)                      # the variance clamps at 0
        again = _rd_table(T, S, N, key, lam, sums).cpu().numpy()
        assert np.array_equal(G._selected(again, Cn).view(np.uint64), G._selected(got, Cn).view(np.uint64))
    print(f"msig_rd_stats T={T} S={S} N={N} {key}: error / bound at most {worst_mean:.3f} (mean), {worst_inv:.3f} (inv)")
    if N == 40 and T > 1:               # a reference of its own: neither expanding's nor trailing:1's table
        h3 = G._selected(tables["h3"].cpu().numpy(), Cn)
        plain = 0 if key == "1off" else COLS[key].index(G.TEMP_COL)
        for K in (0, 1):
            assert not np.array_equal(h3[5:, plain], G._selected(_rn_table(T, S, N, key, K, sums).cpu().numpy(), Cn)[5:, plain])
        assert 1.0 < h3[-1, -1] < 1 / (1 - DECAYS["h3"])


# ---- 3. the rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S,N,key", CASES, ids=IDS)
def test_rows_from_the_devices_own_table_bit_for_bit(T, S, N, key):
    """msig_rn_windows — unchanged — with msig_rd_stats' table (lambda = exp2(-1/3); for N = 40 also windows [3, 40) alone): every
    row equals the numpy statement (float32)((v - mean_b) * inv_b) with row b's record as uint32; the channel under log1p is compared
    against the library's own log1p, msig_rec_windows of that single window with row b's record, which every other channel equals too."""
    _sums, tables = _device(T, S, N, key)
    v64, _vld = G._restated(T, S, N, key)
    cols = COLS[key]
    plain = [c for c, col in enumerate(cols) if col != G.LOG_COL]
    tab = tables["h3"].contiguous()
    host = tab.cpu().numpy()
    for n0 in ((0, 3) if N > 3 else (0,)):
        got = G._rn_windows(T, S, N, key, tab[n0:].contiguous(), n0)
        want = R.rows(v64, T, S, n0, host[n0:, :len(cols)], host[n0:, MC:MC + len(cols)])
        assert got.shape == want.shape
        assert np.array_equal(got[:, plain].view(np.uint32), want[:, plain].view(np.uint32)), n0
        one = torch.stack([G._rec_windows(T, S, N, key, tab[n], n, 1)[0] for n in range(n0, N)])
        torch.cuda.synchronize()
        assert np.array_equal(got.view(np.uint32), one.cpu().numpy().view(np.uint32)), n0
    if N > 1 and T > 1:
        assert np.any(got != 0) and np.all(np.isfinite(got))
