"""Gap-tolerant running references on the GPU (include/msig_gp.h), kernel level through the C ABI and end to end.

Shapes (T, S, columns): (256, 64, 8 of 8), (200, 37, 3 of 8), (200, 300, 8 of 8: S > T), (256, 1, the log1p column alone); 12 windows.
Modes: expanding, trailing with K = 1, 2, 7 and K > N, decayed with lambda = 0, 1 and exp2(-1 / 3).  Inputs (gp_reference.plant): none
missing, sample 0 missing, +-Inf, a log1p argument of -1 and of -2, one channel missing for exactly one window, one channel missing
for the first two windows (late pivot, zero count), every channel missing for lost_after + 1 windows, 5 % of the samples dropped; live
also a gap across the ring's wrap (rings of exactly one window) and a skipped stretch.

The anchor (nothing missing: msig_rn_sums', msig_rn_stats', msig_rd_stats' and msig_rn_windows' bits), the counts and coverage
(exact), the statistics (tests/test_running_gpu.py's criterion against the np.longdouble restatement), the rows from the device's own
table, finiteness, live equals offline in every record, coverage record and row, skip equals a push of NaN rows, and LiveMonitor's
timeline against Monitor.run's with `gaps`.  The statistics test prints every figure it asserts on; what they were on an MI355X is
in its docstring."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import gp_reference as G
import lv_reference as LV
from multimodalsignal_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MC = L.MAX_C
N = G.N_WINDOWS
SHAPE_IDS = [f"t{T}-s{S}-{key}" for T, S, key in G.SHAPES]
CASES = [(T, S, key, kind) for T, S, key in G.SHAPES for kind in G.INPUTS]
CASE_IDS = [f"t{T}-s{S}-{key}-{kind}" for T, S, key, kind in CASES]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "the gpu tier needs an MI355X"


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _mode(m):
    return C.byref(L.GpMode(*m))


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64 if x.dtype == np.float64 else np.uint32)


@functools.lru_cache(maxsize=None)
def _recording(T, S, key, kind):
    sig = G.case_recording(T, S, key, kind)
    assert LV.count(sig.shape[0], T, S) == N
    return sig, torch.from_numpy(sig).to(DEV)


def _head(dev, cols, T, S):
    return dev.data_ptr(), dev.shape[0], dev.shape[1], (C.c_int32 * len(cols))(*cols), len(cols), G.mask_of(cols), T, S


def _canary(shape, dtype=torch.float64):
    return torch.full(shape, float("nan") if dtype == torch.float64 else -77.0, dtype=dtype, device=DEV)


def _gp_sums(dev, cols, T, S, pivot, n0, B):
    out = _canary((B + 1, 3 * MC))
    L.check(L.lib().msig_gp_sums(*_head(dev, cols, T, S), pivot.data_ptr(), n0, B, out.data_ptr(), _stream()), "msig_gp_sums")
    torch.cuda.synchronize()
    assert torch.isnan(out[B]).all(), "wrote past the records"
    return out[:B]


def _tables(dev, cols, T, S, n_windows):
    """pivot, window records and per mode (table, coverage) of a recording on the device: one msig_gp_pivot, one msig_gp_sums and one
    msig_gp_stats per mode.  Unselected entries keep their NaN canary."""
    lib = L.lib()
    pivot = _canary((2 * MC + 1,))
    L.check(lib.msig_gp_pivot(*_head(dev, cols, T, S), n_windows, pivot.data_ptr(), _stream()), "msig_gp_pivot")
    sums = _gp_sums(dev, cols, T, S, pivot, 0, n_windows)
    out = {}
    for name, mode in G.MODES.items():
        tab, cov = _canary((n_windows + 1, 2 * MC + 1)), _canary((n_windows + 1, MC))
        L.check(lib.msig_gp_stats(*_head(dev, cols, T, S), pivot.data_ptr(), sums.data_ptr(), n_windows, _mode(mode), tab.data_ptr(), cov.data_ptr(),
                                  _stream()), "msig_gp_stats")
        torch.cuda.synchronize()
        assert torch.isnan(tab[n_windows]).all() and torch.isnan(cov[n_windows]).all() and torch.isnan(pivot[2 * MC]), "wrote past a table"
        out[name] = (tab[:n_windows], cov[:n_windows])
    return pivot[:2 * MC], sums, out


@functools.lru_cache(maxsize=None)
def _device(T, S, key, kind):
    return _tables(_recording(T, S, key, kind)[1], G.COLS[key], T, S, N)


def _selected(rec, Cn):
    """The written entries of statistics records (..., 2 MAX_C + 1): the selected channels' mean and inv, and the count."""
    return np.concatenate([rec[..., :Cn], rec[..., MC:MC + Cn], rec[..., 2 * MC:]], axis=-1)


def _rn_table(dev, cols, T, S, mode):
    """The parent's tables for the same recording: msig_rn_sums, then msig_rn_stats or msig_rd_stats."""
    lib = L.lib()
    sums = torch.zeros((N, 2 * MC), dtype=torch.float64, device=DEV)
    tab = torch.zeros((N, 2 * MC + 1), dtype=torch.float64, device=DEV)
    L.check(lib.msig_rn_sums(*_head(dev, cols, T, S), 0, N, sums.data_ptr(), _stream()), "msig_rn_sums")
    if mode[0] == G.DECAYED:
        L.check(lib.msig_rd_stats(*_head(dev, cols, T, S), sums.data_ptr(), N, mode[2], tab.data_ptr(), _stream()), "msig_rd_stats")
    else:
        L.check(lib.msig_rn_stats(*_head(dev, cols, T, S), sums.data_ptr(), N, mode[1], tab.data_ptr(), _stream()), "msig_rn_stats")
    torch.cuda.synchronize()
    return sums.cpu().numpy(), tab


def _rows(dev, cols, T, S, table, n0, B, call="msig_gp_windows"):
    n = B * len(cols) * T
    out = _canary((n + 64,), torch.float32)
    L.check(getattr(L.lib(), call)(*_head(dev, cols, T, S), n0, B, table.data_ptr(), out.data_ptr(), _stream()), call)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[n:] == -77.0), "wrote past the batch"
    return got[:n].reshape(B, len(cols), T)


# ---- 1. the anchor: nothing missing ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S,key", G.SHAPES, ids=SHAPE_IDS)
def test_without_a_missing_sample_every_bit_is_the_parents(T, S, key):
    """Window records = msig_rn_sums' W1, W2 and N == T; every mode's table = msig_rn_stats' / msig_rd_stats'; the coverage is 1.0; the
    rows = msig_rn_windows' and msig_rn_windows_multi's — all as raw bits."""
    from multimodalsignal_amd.runtime import Arenas
    _sig, dev = _recording(T, S, key, "none")
    cols, Cn = G.COLS[key], len(G.COLS[key])
    pivot, sums, tables = _device(T, S, key, "none")
    p, s = pivot.cpu().numpy(), sums.cpu().numpy()
    assert np.all(p[MC:MC + Cn] == 1.0) and np.all(np.isnan(p[Cn:MC])) and np.all(np.isnan(p[MC + Cn:]))
    rn_sums, _tab = _rn_table(dev, cols, T, S, G.MODES["expanding"])
    for part in (0, 1):
        assert np.array_equal(_bits(s[:, part * MC:part * MC + Cn]), _bits(rn_sums[:, part * MC:part * MC + Cn]))
    assert np.all(s[:, 2 * MC:2 * MC + Cn] == T) and np.all(np.isnan(s[:, Cn:MC]))
    for name, mode in G.MODES.items():
        tab, cov = tables[name]
        _s, want = _rn_table(dev, cols, T, S, mode)
        assert np.array_equal(_bits(_selected(tab.cpu().numpy(), Cn)), _bits(_selected(want.cpu().numpy(), Cn))), name
        assert np.all(cov.cpu().numpy()[:, :Cn] == 1.0) and np.all(np.isnan(cov.cpu().numpy()[:, Cn:]))
        if name in ("expanding", "trailing2", "decayed3"):
            for n0, B in ((0, N), (3, N - 3)):
                got = _rows(dev, cols, T, S, tab[n0:].contiguous(), n0, B)
                assert np.array_equal(_bits(got), _bits(_rows(dev, cols, T, S, want[n0:].contiguous(), n0, B, "msig_rn_windows"))), (name, n0)
    tab = tables["trailing7"][0].contiguous()
    ar = Arenas(3, DEV, (("other", 1000), ("x", N * Cn * T * 4), ("tail", 256)))
    for call in ("msig_gp_windows_multi", "msig_rn_windows_multi"):
        ar.mem.fill_(0x5A)
        L.check(getattr(L.lib(), call)(*_head(dev, cols, T, S), 2, N - 2, tab[2].data_ptr(), ar.ptr("x"), C.byref(ar.multi([2, 0])), _stream()), call)
        torch.cuda.synchronize()
        x = ar.view(0, "x", torch.float32).cpu().numpy().copy()
        if call == "msig_gp_windows_multi":
            first = x
    assert np.array_equal(_bits(first), _bits(x))


# ---- 2. counts, coverage, statistics ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S,key,kind", CASES, ids=CASE_IDS)
def test_counts_coverage_and_statistics(T, S, key, kind):
    """msig_gp_pivot + msig_gp_sums + msig_gp_stats against tests/gp_reference.py.  Exact: the found flags and the pivots of the plain
    channels, N of every window and channel, the coverage N / T as raw bits, the window count of every record, (0, 0) where a channel
    has no reference yet.  The statistics: tests/test_running_gpu.py's criterion, unchanged — the error of a mean in units of the std
    of its reference's valid samples, of 1 / (std + 1e-8) in units of itself, against the np.longdouble restatement; bound, per channel
    and statistic: 8 x the float64 restatement's own error on the same case, its largest over the case's windows, or where that is
    smaller a floor of 4 ulps; where the reference's valid samples are all equal the absolute condition of that test.  The anchors on
    every input: lambda = 1 is expanding, lambda = 0 is trailing:1 and trailing with K > N is expanding, as raw bits.  Nothing is
    non-finite.
    Measured on an MI355X over all 36 cases and 8 modes: error / bound at most 0.125 for the mean — the device
    adds W1 in the float64 restatement's order — and at most 0.307 for 1 / (std + 1e-8) (T = 200, S = 37, 3 of 8, all_off)."""
    sig, _dev = _recording(T, S, key, kind)
    cols, Cn = G.COLS[key], len(G.COLS[key])
    pivot, sums, tables = _device(T, S, key, kind)
    v64, ok = G.transformed(sig, cols, G.mask_of(cols))
    p, s = pivot.cpu().numpy(), sums.cpu().numpy()
    want_p, found = G.pivot(v64, ok, T, S, N)
    plain = [c for c, col in enumerate(cols) if col != G.LOG_COL]
    assert np.array_equal(p[MC:MC + Cn], found.astype(np.float64)) and np.array_equal(_bits(p[:Cn][plain]), _bits(want_p[plain]))
    assert np.allclose(p[:Cn], want_p, rtol=1e-14, atol=0)
    W = G.window_records(v64, ok, T, S, N, want_p)
    assert np.array_equal(s[:, 2 * MC:2 * MC + Cn], W[:, 2])                                   # the counts, exactly
    assert np.array_equal(_bits(s[:, :Cn][:, plain]), _bits(W[:, 0][:, plain]))              # W1: the same additions in the same order
    assert np.all(np.isfinite(s[:, :Cn])) and np.all(np.isfinite(s[:, MC:MC + Cn]))
    worst_mean, worst_inv = 0.0, 0.0
    host = {}
    for name, mode in G.MODES.items():
        tab, cov = (t.cpu().numpy() for t in tables[name])
        host[name] = _selected(tab, Cn)
        assert np.all(np.isfinite(host[name])) and np.all(np.isfinite(cov[:, :Cn]))
        assert np.all(np.isnan(tab[:, Cn:MC])) and np.all(np.isnan(tab[:, MC + Cn:2 * MC])) and np.all(np.isnan(cov[:, Cn:]))
        y = G.yardstick(tab[:, :Cn], tab[:, MC:MC + Cn], T, S, key, kind, mode)
        assert np.array_equal(_bits(cov[:, :Cn]), _bits(y["coverage"])) and np.array_equal(_bits(cov[:, :Cn]), _bits(W[:, 2] / np.float64(T)))
        assert np.array_equal(tab[:, 2 * MC], y["n_ref"])
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio_mean = float(np.nan_to_num((y["r_mean"] / y["bound_mean"]).astype(np.float64)).max())
            ratio_inv = float(np.nan_to_num((y["r_inv"] / y["bound_inv"]).astype(np.float64)).max())
        worst_mean, worst_inv = max(worst_mean, ratio_mean), max(worst_inv, ratio_inv)
        print(f"msig_gp_stats T={T} S={S} {key} {kind} {name}: mean error / std max {float(y['r_mean'].max()):.3e} (float64 restatement's "
              f"{float(y['q_mean'].max()):.3e}); inv relative error max {float(y['r_inv'].max()):.3e} (restatement's {float(y['q_inv'].max()):.3e}); "
              f"error / bound max: mean {ratio_mean:.3f}, inv {ratio_inv:.3f}; {y['flat']} entries with std = 0, {int((~y['has']).sum())} without a reference")
        assert np.all(y["r_mean"] <= y["bound_mean"]), (name, float(y["r_mean"].max()))
        assert np.all(y["r_inv"] <= y["bound_inv"]), (name, float(y["r_inv"].max()))
        assert y["flat_ok"] and y["none_ok"], name
    print(f"msig_gp_stats T={T} S={S} {key} {kind}: error / bound at most {worst_mean:.3f} (mean), {worst_inv:.3f} (inv)")
    assert np.array_equal(_bits(host["decayed1"]), _bits(host["expanding"])) and np.array_equal(_bits(host["decayed0"]), _bits(host["trailing1"]))
    assert np.array_equal(_bits(host["trailing13"]), _bits(host["expanding"]))
    if kind == "late_pivot":                                      # windows 0 and 1 of channel 0: no valid sample, no reference, zeros
        assert np.all(s[:2, 2 * MC] == 0) and np.all(s[:2, 0] == 0) and np.all(s[:2, MC] == 0)
        assert np.all(host["expanding"][:2, 0] == 0) and np.all(host["expanding"][:2, Cn] == 0) and host["expanding"][2, Cn] > 0
    if kind == "all_off":
        for name in G.MODES:
            assert np.all(tables[name][1].cpu().numpy()[2:3 + G.LOST_AFTER, :Cn] == 0)
        assert np.all(host["trailing1"][2:3 + G.LOST_AFTER, :2 * Cn] == 0)


# ---- 3. the rows -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S,key,kind", CASES, ids=CASE_IDS)
def test_rows_from_the_devices_own_table(T, S, key, kind):
    """msig_gp_windows with the device's own table (expanding, trailing:2, decayed; all windows and windows [3, N) alone): a valid
    sample has the restatement's (float)((v - mean_b) * inv_b) bit for bit — the channel under log1p against the library's own log1p,
    i.e. msig_rn_windows with the same table, which every valid sample of every channel equals — a missing sample is exactly +0.0f,
    nothing is non-finite; msig_gp_windows_multi puts the same bits into every slot and leaves the rest of the arenas alone."""
    from multimodalsignal_amd.runtime import Arenas
    sig, dev = _recording(T, S, key, kind)
    cols, Cn = G.COLS[key], len(G.COLS[key])
    _pivot, _sums, tables = _device(T, S, key, kind)
    v64, ok = G.transformed(sig, cols, G.mask_of(cols))
    plain = [c for c, col in enumerate(cols) if col != G.LOG_COL]
    for name in ("expanding", "trailing2", "decayed3"):
        tab = tables[name][0].contiguous()
        host = tab.cpu().numpy()
        for n0 in (0, 3):
            got = _rows(dev, cols, T, S, tab[n0:].contiguous(), n0, N - n0)
            assert np.all(np.isfinite(got))
            want = G.rows(v64, ok, T, S, n0, host[n0:, :Cn], host[n0:, MC:MC + Cn])
            assert np.array_equal(_bits(got[:, plain]), _bits(want[:, plain])), (name, n0)
            valid = np.stack([ok[(n0 + b) * S:(n0 + b) * S + T].T for b in range(N - n0)])
            assert np.all(_bits(got)[~valid] == 0)                                              # +0.0f, not -0.0f
            parent = _rows(dev, cols, T, S, tab[n0:].contiguous(), n0, N - n0, "msig_rn_windows")
            assert np.array_equal(_bits(got)[valid], _bits(parent)[valid]), (name, n0)
    ar = Arenas(3, DEV, (("other", 1000), ("x", N * Cn * T * 4), ("tail", 256)))
    ar.mem.fill_(0x5A)
    B = N - 3
    L.check(L.lib().msig_gp_windows_multi(*_head(dev, cols, T, S), 3, B, tab[3].data_ptr(), ar.ptr("x"), C.byref(ar.multi([2, 0])), _stream()),
            "msig_gp_windows_multi")
    torch.cuda.synchronize()
    n = B * Cn * T
    for slot in (0, 2):
        x = ar.view(slot, "x", torch.float32).cpu().numpy()
        assert np.array_equal(_bits(x[:n]), _bits(got.reshape(-1))), slot
        assert np.all(x[n:].view(np.uint8) == 0x5A)
        assert np.all(ar.view(slot, "other").cpu().numpy() == 0x5A) and np.all(ar.view(slot, "tail").cpu().numpy() == 0x5A)
    assert np.all(ar.mem[1].cpu().numpy() == 0x5A)


# ---- 4. batch independence -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S,key", G.SHAPES, ids=SHAPE_IDS)
def test_window_records_do_not_depend_on_the_batch_or_the_grid(T, S, key):
    _sig, dev = _recording(T, S, key, "drop5")
    cols, Cn = G.COLS[key], len(G.COLS[key])
    pivot, sums, _t = _device(T, S, key, "drop5")
    whole = sums.cpu().numpy()
    parts = np.concatenate([_gp_sums(dev, cols, T, S, pivot, n0, B).cpu().numpy() for n0, B in ((0, 1), (1, 4), (5, N - 5))])
    for part in range(3):
        assert np.array_equal(_bits(parts[:, part * MC:part * MC + Cn]), _bits(whole[:, part * MC:part * MC + Cn]))
    again = _tables(dev, cols, T, S, N)
    assert np.array_equal(_bits(again[1].cpu().numpy()[:, :Cn]), _bits(whole[:, :Cn]))
    for name in G.MODES:
        assert np.array_equal(_bits(_selected(again[2][name][0].cpu().numpy(), Cn)), _bits(_selected(_t[name][0].cpu().numpy(), Cn)))


# ---- 5. live equals offline, kernel level ----------------------------------------------------------------------------------------------
POOL_SLOTS = 4                                  # sessions live in slots 0, 1 and 3: ring and state 2 are never touched


class Pool:
    """A caller-owned pool of POOL_SLOTS rings filled with 0x5A and as many session states filled with NaN (the library needs no
    initialisation), and the host's side of every open session."""

    def __init__(self, T, S, Rn, key, mode):
        from multimodalsignal_amd.live import RingBook
        self.T, self.S, self.R, self.mode, self.cols, self.RingBook = T, S, Rn, mode, G.COLS[key], RingBook
        K = mode[1] if mode[0] == G.TRAILING else 0
        self.mem = torch.full((POOL_SLOTS, Rn * 8 * 8), 0x5A, dtype=torch.uint8, device=DEV)
        self.state = torch.full((POOL_SLOTS, L.lib().msig_gp_state_bytes(K) // 8), float("nan"), dtype=torch.float64, device=DEV)
        self.book, self.next = {}, {}

    def open(self, k):
        self.book[k], self.next[k] = self.RingBook(self.R, self.T, self.S, 0), 0

    def args(self):
        return self.mem.data_ptr(), POOL_SLOTS, self.R, self.R * 8 * 8, 8

    def rows_args(self):
        return (C.c_int32 * len(self.cols))(*self.cols), len(self.cols), G.mask_of(self.cols), self.T, self.S

    def _entries(self, ks, lens):
        n = len(ks)
        return (C.c_int32 * n)(*ks), (C.c_int64 * n)(*[self.book[k].written for k in ks]), (C.c_int64 * n)(*lens), n

    def push(self, chunks):
        ks = list(chunks)
        staging = torch.cat([chunks[k] for k in ks] + [torch.zeros((1, 8), dtype=torch.float64, device=DEV)]).contiguous()
        L.check(L.lib().msig_lv_push(*self.args(), *self._entries(ks, [int(chunks[k].shape[0]) for k in ks]), staging.data_ptr(), _stream()), "msig_lv_push")

    def skip(self, counts):
        ks = list(counts)
        L.check(L.lib().msig_gp_lv_skip(*self.args(), *self._entries(ks, [counts[k] for k in ks]), _stream()), "msig_gp_lv_skip")

    def _rows(self, rows):
        B = len(rows)
        return ((C.c_int32 * B)(*[k for k, _n in rows]), (C.c_int64 * B)(*[n for _k, n in rows]), (C.c_int64 * B)(*[self.book[k].written for k, _n in rows]))

    def step(self, rows):
        """ONE msig_gp_lv_step for the mixed batch; returns its table and coverage, the last record of each a canary."""
        B = len(rows)
        table, cov = _canary((B + 1, 2 * MC + 1)), _canary((B + 1, MC))
        L.check(L.lib().msig_gp_lv_step(*self.args(), *self.rows_args(), _mode(self.mode), self.state.data_ptr(), self.state.shape[1] * 8,
                                        *self._rows(rows), (C.c_int64 * B)(*[self.next[k] for k, _n in rows]), B, table.data_ptr(), cov.data_ptr(),
                                        _stream()), "msig_gp_lv_step")
        seen = set()
        for k, _n in rows:
            self.next[k] += 0 if k in seen else sum(1 for k2, _w in rows if k2 == k)
            seen.add(k)
        return table, cov

    def windows(self, rows, table, arenas, slots):
        L.check(L.lib().msig_gp_lv_windows_multi(*self.args(), *self.rows_args(), *self._rows(rows), len(rows), table.data_ptr(), arenas.ptr("x"),
                                                 C.byref(arenas.multi(slots)), _stream()), "msig_gp_lv_windows_multi")


def _cut(Ln, cycle, gone):
    """The samples [0, Ln) as pieces (first, one past last, skipped): chunks of the cycle's lengths, cut at the skipped span."""
    out, at, i = [], 0, 0
    while at < Ln:
        end = min(Ln, at + cycle[i % len(cycle)])
        i += 1
        for a, b in ((at, end),) if gone is None else ((at, min(end, gone[0])), (max(at, gone[0]), min(end, gone[1])), (max(at, gone[1]), end)):
            if b > a:
                out.append((a, b, gone is not None and gone[0] <= a < gone[1]))
        at = end
    return out


@functools.lru_cache(maxsize=None)
def _offline(T, S, key, kind, name):
    """Table, coverage and every row of the LINEAR recording under one mode — computed once."""
    _sig, dev = _recording(T, S, key, kind)
    _p, _s, tables = _device(T, S, key, kind)
    tab, cov = tables[name]
    rows = _rows(dev, G.COLS[key], T, S, tab.contiguous(), 0, N)
    return tab.cpu().numpy(), cov.cpu().numpy(), rows


LIVE_MODES = {"8of8": ["expanding", "trailing7", "decayed3"], "3of8": ["trailing1", "trailing2", "decayed0"], "1of8": ["trailing13", "decayed1", "expanding"]}


@pytest.mark.parametrize("ring", ["t", "6s+t+41"])
@pytest.mark.parametrize("T,S,key", G.SHAPES, ids=SHAPE_IDS)
def test_live_records_coverage_and_rows_are_the_offline_ones(T, S, key, ring):
    """Three sessions of a pool of four, out of phase, in chunks of about one, two and three strides and of a few samples, through rings of exactly one window
    (every window wraps, and so does every gap) and of 6 S + T + 41 rows (one step takes several windows of a session): every
    statistics record, coverage record and row equals the offline call's on the session's linear recording as raw bits.  Session 0's
    all-channel gap is not pushed but skipped (msig_gp_lv_skip), slot 1 is closed after its first recording and reopened without
    its state being cleared, slot 3 starts on a missing sample.  Across the shapes every mode is taken."""
    from multimodalsignal_amd.runtime import Arenas
    Rn = T if ring == "t" else 6 * S + T + 41
    Cn = len(G.COLS[key])
    for name in LIVE_MODES[key]:
        pool = Pool(T, S, Rn, key, G.MODES[name])
        plan = {0: ["all_off"], 1: ["late_pivot", "drop5"], 3: ["sample0"]}
        q = max(S, T // 5)
        cycle = {0: [3 * q + 1, q, 7], 1: [q, 3 * q + 1, 5], 3: [2 * q + 3, q]}
        late = {0: 0, 1: 1, 3: 2}
        gone = (2 * S, (2 + G.LOST_AFTER) * S + T)                  # session 0's rows that are all NaN
        todo = {k: [[(kind, piece) for piece in _cut(_recording(T, S, key, kind)[1].shape[0], cycle[k], gone if kind == "all_off" else None)]
                    for kind in kinds] for k, kinds in plan.items()}
        cur, done = {k: 0 for k in plan}, {k: 0 for k in plan}
        for k in plan:
            pool.open(k)
        arenas = Arenas(3, DEV, (("other", 1000), ("x", 32 * Cn * T * 4), ("tail", 256)))          # a step takes up to 32 rows
        tick, checked, mixed, longest, skipped, reopened = 0, 0, 0, 0, 0, False
        while any(cur[k] < len(plan[k]) for k in plan):
            take = {}
            for k in plan:
                if tick >= late[k] and cur[k] < len(plan[k]):
                    take[k] = todo[k][cur[k]].pop(0)
            off = {k: 0 for k in take}
            while True:                                             # an append in segments, as live.py makes it
                seg = {k: pool.book[k].segment(take[k][1][1] - take[k][1][0] - off[k]) for k in take if take[k][1][1] - take[k][1][0] > off[k]}
                if not seg:
                    break
                data = {k: _recording(T, S, key, take[k][0])[1][take[k][1][0] + off[k]:take[k][1][0] + off[k] + a] for k, a in seg.items() if not take[k][1][2]}
                hole = {k: a for k, a in seg.items() if take[k][1][2]}
                if data:
                    pool.push(data)
                if hole:
                    pool.skip(hole)
                    skipped += sum(hole.values())
                rows = []
                for k, a in seg.items():
                    off[k] += a
                    _due, wins = pool.book[k].advance(a)
                    rows += [(k, w) for w in wins]
                if not rows:
                    continue
                assert len(rows) <= 32
                table, cov = pool.step(rows)
                arenas.mem.fill_(0x5A)
                pool.windows(rows, table, arenas, [2, 0])
                torch.cuda.synchronize()
                got, gcov = table.cpu().numpy(), cov.cpu().numpy()
                assert np.all(np.isnan(got[len(rows)])) and np.all(np.isnan(gcov[len(rows)])), "wrote past a table"
                want_rows = []
                for b, (k, w) in enumerate(rows):
                    tab, wcov, out = _offline(T, S, key, plan[k][cur[k]], name)
                    assert np.array_equal(_bits(_selected(got[b], Cn)), _bits(_selected(tab[w], Cn))), (name, tick, k, w)
                    assert np.array_equal(_bits(gcov[b, :Cn]), _bits(wcov[w, :Cn])), (name, tick, k, w)
                    assert np.all(np.isnan(got[b, Cn:MC])) and np.all(np.isnan(got[b, MC + Cn:2 * MC])) and np.all(np.isnan(gcov[b, Cn:]))
                    assert w == done[k]
                    done[k] += 1
                    want_rows.append(out[w].reshape(-1))
                ref, n = _bits(np.concatenate(want_rows)), len(rows) * Cn * T
                for s in (0, 2):
                    x = arenas.view(s, "x", torch.float32).cpu().numpy()
                    assert np.array_equal(_bits(x[:n]), ref), (name, tick, s, rows)
                    assert np.all(x[n:].view(np.uint8) == 0x5A), "wrote past the batch"
                    assert np.all(arenas.view(s, "other").cpu().numpy() == 0x5A) and np.all(arenas.view(s, "tail").cpu().numpy() == 0x5A)
                assert np.all(arenas.mem[1].cpu().numpy() == 0x5A) and np.all(pool.mem[2].cpu().numpy() == 0x5A)
                checked += len(rows)
                mixed += len({k for k, _w in rows}) > 1
                longest = max(longest, max(sum(1 for k2, _w in rows if k2 == k) for k, _w in rows))
            for k in take:                                          # a recording is through: close; slot 1 reopens with its next one
                if not todo[k][cur[k]]:
                    assert done[k] == N
                    st = pool.state[k].cpu().numpy()
                    assert st[G.STATE_NEXT] == N and st[G.STATE_NEXT + 2] == G.MODES[name][0]          # the state knows where it stands
                    cur[k], done[k] = cur[k] + 1, 0
                    if cur[k] < len(plan[k]):
                        pool.open(k)                                # the same slot, its ring and its state as they were left
                        reopened = True
            tick += 1
        assert checked == 4 * N and mixed >= 2 and reopened and skipped == gone[1] - gone[0]
        assert longest >= (2 if ring != "t" and S < T else 1)
        assert torch.isnan(pool.state[2]).all()                     # nobody's state


def test_skip_is_a_push_of_nan_rows_bit_for_bit():
    """Two sessions take the same samples, one with the stretch pushed as NaN rows, one with it skipped — the stretch crosses the
    ring's end: the two rings hold the same bytes, and the step gives the same records."""
    T, S, key = 200, 37, "3of8"
    sig, dev = _recording(T, S, key, "none")
    pool = Pool(T, S, T + 50, key, G.MODES["expanding"])
    pool.open(0), pool.open(1)
    head, hole = T + 20, 2 * T - 90                                # the hole [T + 20, 3 T - 70) wraps a ring of T + 50 rows
    nan = torch.full((hole, 8), float("nan"), dtype=torch.float64, device=DEV)
    pool.push({0: dev[:head], 1: dev[:head]})
    for k in (0, 1):
        pool.book[k].advance(head)
    pool.step([(0, 0), (1, 0)])
    at = 0
    while at < hole:
        a = pool.book[0].segment(hole - at)
        pool.push({0: nan[at:at + a]})
        pool.skip({1: a})
        rows = []
        for k in (0, 1):
            rows += [(k, w) for w in pool.book[k].advance(a)[1]]
        at += a
        if rows:
            table, cov = pool.step(rows)
            torch.cuda.synchronize()
            t, c, h = table.cpu().numpy(), cov.cpu().numpy(), len(rows) // 2
            assert np.array_equal(_bits(_selected(t[:h], 3)), _bits(_selected(t[h:2 * h], 3))) and np.array_equal(_bits(c[:h, :3]), _bits(c[h:2 * h, :3]))
    torch.cuda.synchronize()
    rings = pool.mem.cpu().numpy()
    assert np.array_equal(rings[0], rings[1]) and np.all(rings[2] == 0x5A) and np.all(rings[3] == 0x5A)
    assert np.isnan(rings[1].view(np.float64)).sum() == min(hole, T + 50) * 8
    assert np.all(rings[1].view(np.uint64)[np.isnan(rings[1].view(np.float64))] == 0x7ff8000000000000)


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------------
NAMES8 = LV.NAMES8
CHANNELS = ["chest_ECG", "chest_EDA", "chest_Resp", "wrist_BVP", "chest_ACC_x", "wrist_EDA"]
FS = 64.0
TL_SHARED = ("t_end", "mean_p", "std_p", "pred", "entropy", "mutual_info", "votes", "score", "smoothed", "state", "warmup")
TL_FIELDS = TL_SHARED + ("coverage", "valid", "lost")


@functools.lru_cache(maxsize=None)
def _models():
    return LV.models("cnn_gru_attention", len(CHANNELS), 2, 3, DEV)


def _monitors(reference, gaps, **kw):
    from multimodalsignal_amd.live import LiveMonitor
    from multimodalsignal_amd.monitor import Monitor
    common = dict(window_s=64 / FS, stride_s=16 / FS, reference=reference, eval_batch=16, channels=CHANNELS, halflife=2, on=kw.pop("on", 0.55),
                  off=kw.pop("off", 0.45), min_on=2, gaps=gaps)
    return LiveMonitor(_models(), FS, max_sessions=3, **common, **kw), Monitor(_models(), FS, **common)


def _gappy(n_windows, seed, T=64, S=16, lost_after=3):
    """(L, 8) with 3 % of the samples dropped, one channel off for a while, and two all-channel stretches, the second long enough to
    lose the wearer; the all-channel spans as (first, one past last)."""
    sig = LV.recording((n_windows - 1) * S + T + 2, seed)
    rs = np.random.RandomState(seed)
    sig[rs.rand(*sig.shape) < 0.03] = np.nan
    sig[5 * S:9 * S, 1] = np.nan
    spans = [(11 * S + 5, 12 * S + 9), (20 * S + 3, (20 + lost_after + 2) * S + T)]
    for a, b in spans:
        sig[a:b] = np.nan
    return sig, spans


def test_monitor_with_gaps_on_a_gap_free_recording_is_the_monitor_without():
    from multimodalsignal_amd.monitor import Gaps, Monitor
    sig = LV.recording(39 * 16 + 64 + 2, 501)
    dev = torch.from_numpy(sig).to(DEV)
    for reference in ("expanding", "trailing:5:2", "decayed:3"):
        common = dict(window_s=64 / FS, stride_s=16 / FS, reference=reference, eval_batch=16, channels=CHANNELS, halflife=2, on=0.55, off=0.45, min_on=2)
        want = Monitor(_models(), FS, **common).run(dev, NAMES8)
        got = Monitor(_models(), FS, gaps=Gaps(), **common).run(dev, NAMES8)
        for f in TL_SHARED:
            x, y = getattr(got, f), getattr(want, f)
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (reference, f)
        assert got.events == want.events and want.coverage is None and np.all(got.coverage == 1.0) and got.valid.all() and not got.lost.any()
        assert {k: v for k, v in got.meta.items() if k not in ("gaps", "invalid_windows", "lost_windows")} == want.meta
        assert (got.meta["gaps"], got.meta["invalid_windows"], got.meta["lost_windows"]) == ("0.75:6", 0, 0)
    stats = torch.zeros(2 * MC + 1, dtype=torch.float64, device=DEV)
    stats[MC:2 * MC] = 1.0
    common["reference"] = stats
    want, got = Monitor(_models(), FS, **common).run(dev, NAMES8), Monitor(_models(), FS, gaps=Gaps(), **common).run(dev, NAMES8)
    assert all(getattr(got, f).tobytes() == getattr(want, f).tobytes() for f in TL_SHARED) and np.all(got.coverage == 1.0)


@pytest.mark.parametrize("reference", ["expanding", "trailing:5:2", "decayed:3"])
def test_live_timeline_with_gaps_is_monitor_runs(reference):
    """Three sessions, out of phase; session "a" has its all-channel stretches skipped, "b" pushes them as NaN rows (numpy chunks),
    "c" arrives in one push; "b" is closed and "d" opened in its slot.  timeline(sid) equals Monitor.run(gaps=...) on the same samples
    with the skipped stretches as NaN rows in every field — coverage, valid and lost among them — no score or smoothed value is
    non-finite, the alarms are the ones the offline vectors imply with `lost` and `back` among them, and the updates carry each
    window's validity and coverage.  Without gaps the windows of the long stretch have no finite statistic and no finite input value: the
    defect this closes."""
    from multimodalsignal_amd.live import alarms_of_gaps, timelines_equal
    from multimodalsignal_amd.monitor import Gaps, Monitor
    T, S, gaps = 64, 16, Gaps(0.75, 3)
    recs = {k: _gappy(n, seed) for k, n, seed in (("a", 40, 601), ("b", 33, 602), ("c", 37, 603), ("d", 30, 604))}
    dev = {k: torch.from_numpy(v[0]).to(DEV) for k, v in recs.items()}
    live, mon = _monitors(reference, gaps)
    sm = mon.run(dev["a"], NAMES8).smoothed                       # thresholds these never-trained members cross
    off, on = float(np.percentile(sm, 40)), float(np.percentile(sm, 60))
    if not off < on:
        off, on = 0.45, 0.55
    live, mon = _monitors(reference, gaps, on=on, off=off)
    offline = {k: mon.run(dev[k], NAMES8) for k in recs}
    ups = {k: [] for k in recs}
    for k in ("a", "b", "c"):
        live.open(k, NAMES8)
    from multimodalsignal_amd.live import replay_pieces
    pieces = {"a": [p for i in range(0, dev["a"].shape[0], 2 * S + 5) for p in replay_pieces(i, min(i + 2 * S + 5, dev["a"].shape[0]), recs["a"][1])],
              "b": [(i, min(i + 3 * S + 1, dev["b"].shape[0]), False) for i in range(0, dev["b"].shape[0], 3 * S + 1)],
              "c": [(0, dev["c"].shape[0], False)]}
    late, tick = {"a": 0, "b": 2, "c": 5}, 0
    while any(pieces.values()):
        push, skip = {}, {}
        for k in pieces:
            if tick >= late[k] and pieces[k]:
                a, b, gone = pieces[k].pop(0)
                if gone:
                    skip[k] = b - a
                else:
                    push[k] = recs[k][0][a:b] if k == "b" else dev[k][a:b]
        for out in ([live.push(push)] if push else []) + ([live.skip(skip)] if skip else []):
            for k, u in out.items():
                ups[k] += u
        tick += 1
    assert timelines_equal(live.timeline("b"), offline["b"]) and live.timeline("b").meta == offline["b"].meta
    live.close("b")
    live.open("d", NAMES8)
    for a, b, gone in [p for i in range(0, dev["d"].shape[0], 5 * S) for p in replay_pieces(i, min(i + 5 * S, dev["d"].shape[0]), recs["d"][1])]:
        ups["d"] += live.skip("d", b - a) if gone else live.push("d", dev["d"][a:b])
    kinds = set()
    for k in ("a", "c", "d"):
        tl, want = live.timeline(k), offline[k]
        assert timelines_equal(tl, want), k
        for f in TL_FIELDS:
            x, y = getattr(tl, f), getattr(want, f)
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (k, f)
        assert tl.meta == want.meta and tl.events == want.events
        assert np.all(np.isfinite(want.score)) and np.all(np.isfinite(want.smoothed)) and np.all(np.isfinite(want.mean_p)) and np.all(np.isfinite(want.std_p))
        assert want.meta["gaps"] == "0.75:3" and want.meta["invalid_windows"] == int((~want.valid).sum()) > 0 and want.meta["lost_windows"] == int(want.lost.sum()) > 0
        assert np.array_equal(want.valid, want.coverage.min(axis=1) >= 0.75) and want.coverage.shape == (len(want.t_end), len(CHANNELS))
        assert not want.state[want.lost].any() and np.all(want.coverage[21:21 + 3] == 0)
        implied = alarms_of_gaps(want.state, want.valid, 3, mon.min_on)
        assert implied == G.alarms(want.smoothed, want.valid, on, off, mon.min_on, 3)
        assert [(a.kind, a.window, a.start_window) for a in live.alarms(k)] == implied
        kinds |= {a.kind for a in live.alarms(k)}
        assert [u.window for u in ups[k]] == list(range(len(want.t_end))) and [u.valid for u in ups[k]] == list(want.valid)
        assert np.array_equal(np.array([u.coverage for u in ups[k]]), want.coverage) and [u.smoothed for u in ups[k]] == list(want.smoothed)
    assert {"lost", "back"} <= kinds
    from multimodalsignal_amd.monitor import RecordingWindows
    plain = RecordingWindows(dev["a"], NAMES8, CHANNELS, T, S, reference)       # without gaps a window that covers the long stretch has no
    rows = plain.batch(21, 5).cpu().numpy()                         # finite statistic, and no value the models are given is finite
    assert not np.isfinite(plain.stats[21:26, :len(CHANNELS)].cpu().numpy()).any() and not np.isfinite(rows).any()
    with pytest.raises(ValueError, match="skip needs a monitor with gaps"):
        _monitors(reference, None)[0].skip("a", 5)
    with pytest.raises(ValueError):
        live.skip("a", -1)


# ---- 7. the command lines --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run_dir(tmp_path_factory):
    """A run directory of saved random state_dicts: folds S2 and S10."""
    from multimodalsignal_amd.synth import CHANNELS6
    root = tmp_path_factory.mktemp("run")
    for seed, sid in ((40, "S2"), (41, "S10")):
        d = root / f"fold_test_on_{sid}"
        d.mkdir(parents=True)
        torch.save(LV.models("cnn_gru_attention", 6, 2, 1, DEV, seed)[0].state_dict(), d / "best_model.pt")
    (root / "cv_summary.txt").write_text(f"实验配置:\nSEED: 42\nCHANNELS_TO_USE: {list(CHANNELS6)}\n", encoding="utf-8")
    return root


def test_both_command_lines_take_gaps(run_dir, tmp_path, capsys):
    """live replays the synthetic recording with planted gaps into two sessions — the all-channel stretches as skip calls — and says
    that session 0 equals Monitor.run; monitor writes the same timeline.csv with the three new columns and the same timeline.json."""
    import json
    from multimodalsignal_amd import live, monitor
    args = ["--run", str(run_dir), "--synthetic-recording", "--window-s", "8", "--stride-s", "8", "--reference", "decayed:60", "--gaps", "0.75:3",
            "--synthetic-gaps", "drop=0.05,channel=1:300:120,all=900:70,all=1500:9"]
    tl = live.main(args + ["--sessions", "2", "--chunk-s", "3", "--out", str(tmp_path / "live")])
    said = capsys.readouterr().out
    want = monitor.main(args + ["--out", str(tmp_path / "offline")])
    rows = (tmp_path / "live" / "timeline.csv").read_text().splitlines()
    n = (40 * 60 * 64 - 512) // 512 + 1
    assert len(rows) == n + 1 and rows[0] == "window,t_end_s,score,std,smoothed,state,pred,entropy,mutual_info,warmup,valid,coverage_min,lost"
    assert rows == (tmp_path / "offline" / "timeline.csv").read_text().splitlines()
    doc = json.loads((tmp_path / "offline" / "timeline.json").read_text())
    assert json.loads((tmp_path / "live" / "timeline.json").read_text()) == doc
    assert doc["gaps"] == "0.75:3" and doc["invalid_windows"] == int((~want.valid).sum()) >= 15 + 8 and doc["lost_windows"] == int(want.lost.sum()) >= 5
    line = [ln for ln in said.splitlines() if "Monitor.run" in ln]
    assert len(line) == 1 and line[0].endswith(": equal bit for bit") and "NOT" not in line[0]
    assert any(ln.startswith("gaps 0.75:3:") and f"{70 * 64 + 9 * 64} of session 0's samples were skipped" in ln and " 0 of " in ln for ln in said.splitlines())
    assert np.all(np.isfinite(tl.score)) and np.all(np.isfinite(tl.smoothed))
