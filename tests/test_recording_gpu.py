"""Windows of a continuous recording on the GPU (include/msig_rec.h, multimodalsignal_amd/monitor.py): the
batches bit for bit against msig_nr_normalise_subject on the materialised windows, the statistics against a np.longdouble
restatement (tests/rec_reference.py) with msig_nr_normalise_subject's own error as the yardstick, the monitor end to end against
Ensemble.predict on materialised windows, and Monitor.from_run's choice of checkpoints.

The statistics test prints every figure it asserts on; what they were on an MI355X is in its docstring."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

import rec_reference as R
from multimodalsignal_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = float(np.finfo(np.float64).eps)

# column 1 is the one under log1p (positive, heavy-tailed); 3 and 4 have mean >> spread; 6 is exactly constant
NAMES8 = ["chest_ECG", "chest_EDA", "chest_Resp", "chest_Temp", "chest_ACC_x", "wrist_BVP", "chest_EMG", "wrist_EDA"]
COLS = {"3of8": [5, 1, 4], "1of8": [3], "8of8": [7, 2, 0, 3, 1, 6, 5, 4]}
TS = [(T, S) for T in (256, 200) for S in (1, 37, 64, T, 300)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "the gpu tier needs an MI355X"


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _length(T, S):
    return T + 44 if S == 1 else 36 * S + T + 5          # N = 45 for S = 1, else 37; a tail no window covers


@functools.lru_cache(maxsize=None)
def _recording(T, S):
    """(L, 8) float64 with a slow drift, so that a range of windows has statistics of its own."""
    Ln = _length(T, S)
    rs = np.random.RandomState(1000 * T + S)
    spread = 0.5 + rs.rand(8)
    sig = rs.randn(Ln, 8) * spread + rs.randn(8) + 0.7 * spread * np.sin(2 * np.pi * np.arange(Ln) / Ln)[:, None]
    sig[:, 1] = np.exp(0.8 * rs.randn(Ln) + 0.5 * np.sin(2 * np.pi * np.arange(Ln) / Ln)) + 0.1
    sig[:, 3] = 33.0 + 0.05 * rs.randn(Ln) + 0.03 * np.arange(Ln) / Ln
    sig[:, 4] = 0.9 + 0.02 * rs.randn(Ln)
    sig[:, 6] = 0.75
    sig = np.ascontiguousarray(sig)
    return sig, torch.from_numpy(sig).to(DEV)


def _mask_of(cols):
    return sum(1 << c for c, col in enumerate(cols) if NAMES8[col] == "chest_EDA")


def _head(dev, cols, T, S):
    return dev.data_ptr(), dev.shape[0], dev.shape[1], (C.c_int32 * len(cols))(*cols), len(cols), _mask_of(cols), T, S


@functools.lru_cache(maxsize=None)
def _nr(T, S, key, w):
    """msig_nr_normalise_subject on the materialised windows with the mask [w0, w1): its output rows and its stats — computed once."""
    from multimodalsignal_amd.dataset import normalise_subject_device
    sig, _ = _recording(T, S)
    cols = COLS[key]
    raw = R.materialise(sig, T, S)
    ref = np.zeros(raw.shape[0], dtype=bool)
    ref[w[0]:w[1]] = True
    stats = torch.full((2 * L.MAX_C + 1,), float("nan"), dtype=torch.float64, device=DEV)
    out = normalise_subject_device(torch.from_numpy(raw).to(DEV), cols, [NAMES8[c] for c in cols], ref, stats=stats)
    torch.cuda.synchronize()
    return out.cpu().numpy(), stats


def _ranges(T, S):
    N = R.count(_length(T, S), T, S)
    return N, [(0, N), (3, 11)]


def _pieces(N):
    """16, 16 and a ragged 5 at n0 > 0; then what is left (S = 1 has 45 windows)."""
    out = [(0, 16), (16, 16), (32, 5)]
    return out + ([(37, N - 37)] if N > 37 else [])


# ---- 1. the batches, bit for bit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(COLS))
@pytest.mark.parametrize("T,S", TS, ids=[f"t{T}-s{S}" for T, S in TS])
def test_window_bits_are_msig_nr_normalise_subjects(T, S, key):
    """msig_rec_windows with the stats msig_nr_normalise_subject returned for the materialised windows gives that call's output rows
    bit for bit — for the all-window statistics and for those of windows [3, 11) — in pieces of 16, 16 and a ragged 5 at n0 > 0, and
    writes nothing beyond its batch."""
    _sig, dev = _recording(T, S)
    cols = COLS[key]
    N, ranges = _ranges(T, S)
    lib = L.lib()
    for w in ranges:
        want, stats = _nr(T, S, key, w)
        assert want.shape == (N, len(cols), T)
        for n0, B in _pieces(N):
            n = B * len(cols) * T
            out = torch.full((n + 64,), -77.0, dtype=torch.float32, device=DEV)
            L.check(lib.msig_rec_windows(*_head(dev, cols, T, S), n0, B, stats.data_ptr(), out.data_ptr(), _stream()), "msig_rec_windows")
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert np.all(got[n:] == -77.0), (w, n0, "wrote past the batch")
            assert np.array_equal(got[:n].view(np.uint32), want[n0:n0 + B].reshape(-1).view(np.uint32)), (w, n0, B)
    if "chest_EMG" in [NAMES8[c] for c in cols]:
        assert np.all(want[:, cols.index(6), :] == 0.0)
    assert np.abs(want).max() > 1.0


@pytest.mark.parametrize("T,S,key", [(256, 64, "3of8"), (200, 37, "8of8"), (200, 300, "1of8"), (256, 1, "3of8")])
def test_multi_fills_every_slot_with_the_same_bits(T, S, key):
    """msig_rec_windows_multi into arena slots 2 and 0 of three: both hold msig_rec_windows' bits, slot 1 and the rest of every arena
    stay as they were."""
    from multimodalsignal_amd.runtime import Arenas
    _sig, dev = _recording(T, S)
    cols = COLS[key]
    N, _ = _ranges(T, S)
    want, stats = _nr(T, S, key, (3, 11))
    Cn = len(cols)
    ar = Arenas(3, DEV, (("other", 1000), ("x", 16 * Cn * T * 4), ("tail", 256)))
    lib = L.lib()
    for n0, B in _pieces(N)[1:3]:
        ar.mem.fill_(0x5A)
        L.check(lib.msig_rec_windows_multi(*_head(dev, cols, T, S), n0, B, stats.data_ptr(), ar.ptr("x"), C.byref(ar.multi([2, 0])), _stream()),
                "msig_rec_windows_multi")
        torch.cuda.synchronize()
        n = B * Cn * T
        for s in (0, 2):
            x = ar.view(s, "x", torch.float32).cpu().numpy()
            assert np.array_equal(x[:n].view(np.uint32), want[n0:n0 + B].reshape(-1).view(np.uint32)), (n0, s)
            assert np.all(x[n:].view(np.uint8) == 0x5A)
            assert np.all(ar.view(s, "other").cpu().numpy() == 0x5A) and np.all(ar.view(s, "tail").cpu().numpy() == 0x5A)
        assert np.all(ar.mem[1].cpu().numpy() == 0x5A)


# ---- 2. the statistics -------------------------------------------------------------------------------------------------------------------
def _rec_stats(dev, cols, T, S, w):
    lib = L.lib()
    stats = torch.full((2 * L.MAX_C + 1,), float("nan"), dtype=torch.float64, device=DEV)
    scratch = torch.full((lib.msig_rec_scratch_bytes() // 8,), float("nan"), dtype=torch.float64, device=DEV)
    L.check(lib.msig_rec_stats(*_head(dev, cols, T, S), w[0], w[1], stats.data_ptr(), scratch.data_ptr(), _stream()), "msig_rec_stats")
    torch.cuda.synchronize()
    return stats.cpu().numpy()


@pytest.mark.parametrize("key", list(COLS))
@pytest.mark.parametrize("T,S", TS, ids=[f"t{T}-s{S}" for T, S in TS])
def test_statistics_against_longdouble(T, S, key):
    """msig_rec_stats against the np.longdouble two-pass statistics of the materialised reference windows.  Bound, per channel: the
    larger of 8 x the error msig_nr_normalise_subject's own stats show against that same reference on the same input (the project's
    "8 x the oracle's own error"), and a floor of 4 fp64 ulps — of |mean| + std for the mean, of the value for 1 / (std + 1e-8): the
    finalisation rounds about five times (two divisions, the fused variance, the square root, the sum with the pivot, the
    reciprocal), half an ulp each, before any summation error.  Two calls give the same bits.
    Measured on an MI355X over all sixty cases, in those units: the mean at most 1.22 (msig_nr's own: 1.92), 1 / (std + 1e-8) at most
    3.68 (msig_nr's own: 6.2 under the mask [3, 11), up to 8e5 where it applies its unshifted all-window sums)."""
    sig, dev = _recording(T, S)
    cols = COLS[key]
    Cn = len(cols)
    _N, ranges = _ranges(T, S)
    for w in ranges:
        mean, std = R.stats_longdouble(sig, cols, _mask_of(cols), T, S, *w)
        mean_w, std_w = R.stats_weighted_longdouble(sig, cols, _mask_of(cols), T, S, *w)
        inv = 1 / (std + np.longdouble(1e-8))
        assert np.all(np.abs(mean_w - mean) <= 4 * EPS * (np.abs(mean) + std)) and np.all(np.abs(std_w - std) <= 4 * EPS * (np.abs(mean) + std))
        got = _rec_stats(dev, cols, T, S, w)
        nr = _nr(T, S, key, w)[1].cpu().numpy()
        assert got[2 * L.MAX_C] == w[1] - w[0]
        scale = (np.abs(mean) + std).astype(np.float64)
        e_mean = np.abs(got[:Cn] - mean).astype(np.float64)
        e_inv = np.abs(got[L.MAX_C:L.MAX_C + Cn] - inv).astype(np.float64)
        o_mean = np.abs(nr[:Cn] - mean).astype(np.float64)
        o_inv = np.abs(nr[L.MAX_C:L.MAX_C + Cn] - inv).astype(np.float64)
        inv64 = inv.astype(np.float64)
        print(f"msig_rec_stats T={T} S={S} {key} windows {w}: mean error / (eps (|mean| + std)) max {(e_mean / (EPS * scale)).max():.3f} "
              f"(msig_nr's {(o_mean / (EPS * scale)).max():.3f}); 1/(std+1e-8) relative error / eps max {(e_inv / (EPS * inv64)).max():.3f} "
              f"(msig_nr's {(o_inv / (EPS * inv64)).max():.3f})")
        assert np.all(e_mean <= np.maximum(8 * o_mean, 4 * EPS * scale)), (w, e_mean, o_mean)
        assert np.all(e_inv <= np.maximum(8 * o_inv, 4 * EPS * inv64)), (w, e_inv, o_inv)
        assert np.all(np.isnan(got[Cn:L.MAX_C])) and np.all(np.isnan(got[L.MAX_C + Cn:2 * L.MAX_C]))      # only the selected channels' slots
        again = _rec_stats(dev, cols, T, S, w)
        assert np.array_equal(again[:Cn].view(np.uint64), got[:Cn].view(np.uint64))
        assert np.array_equal(again[L.MAX_C:L.MAX_C + Cn].view(np.uint64), got[L.MAX_C:L.MAX_C + Cn].view(np.uint64))


# ---- 3. the monitor end to end -----------------------------------------------------------------------------------------------------------
FIELDS = ("mean_p", "std_p", "pred", "entropy", "mutual_info", "votes")
CHANNELS = {6: ["chest_ECG", "chest_EDA", "chest_Resp", "wrist_BVP", "chest_ACC_x", "wrist_EDA"], 2: ["chest_Temp", "chest_EDA"]}


def _models(kind, Cin, K, M, seed=5):
    """Randomly initialised members (never trained), in eval mode."""
    from multimodalsignal_amd.models import CnnGruAttentionModel, CnnGruModel
    cls = CnnGruAttentionModel if kind == "cnn_gru_attention" else CnnGruModel
    out = []
    for r in range(M):
        torch.manual_seed(seed + r)
        out.append(cls(Cin, K).to(DEV).eval())
    return out


def _host(p):
    torch.cuda.synchronize()
    return {k: getattr(p, k).cpu().numpy() for k in FIELDS}


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("kind,Cin", [("cnn_gru_attention", 6), ("cnn_gru", 2)])
def test_monitor_run_is_ensemble_predict_on_the_materialised_windows(kind, Cin, M):
    from multimodalsignal_amd.ensemble import Ensemble
    T, S, K, fs = 256, 64, 2, 64.0
    models = _models(kind, Cin, K, M)
    own = torch.from_numpy(np.random.RandomState(9).randn(37, Cin, T).astype(np.float32)).to(DEV)
    before = _host(Ensemble(models, eval_batch=16).predict(own))                  # before any monitor code has run
    from multimodalsignal_amd.monitor import Monitor
    sig, dev = _recording(T, S)
    for reference, warm in (("recording", 0), ("head:7", 7)):
        mon = Monitor(models, fs, window_s=T / fs, stride_s=S / fs, reference=reference, eval_batch=16, channels=CHANNELS[Cin], halflife=2,
                      on=0.55, off=0.45, min_on=2)
        tl = mon.run(dev, NAMES8)
        rw = mon.windows(dev, NAMES8)
        assert (rw.n, rw.shape, rw.warmup) == (37, (37, Cin, T), warm)
        x = rw.materialise()
        assert x.shape == (37, Cin, T) and x.dtype == torch.float32
        want = _host(Ensemble(models, eval_batch=16).predict(x))
        for k in FIELDS:
            got = getattr(tl, k)
            assert got.dtype == want[k].dtype and np.array_equal(got.view(np.uint32), want[k].view(np.uint32)), (reference, k)
        # ... and the materialised windows are the restatement's, to fp32 rounding of the same fp64 statistics
        st = rw.stats.cpu().numpy()
        cols = [NAMES8.index(c) for c in CHANNELS[Cin]]
        ref = R.batch(sig, cols, _mask_of(cols), T, S, 0, 37, st[:Cin], st[L.MAX_C:L.MAX_C + Cin])
        assert np.abs(x.cpu().numpy() - ref).max() <= 2e-6 * max(1.0, np.abs(ref).max())
        # the host side of the timeline
        assert np.array_equal(tl.t_end, (np.arange(37) * S + T) / fs) and tl.t_end[0] == 4.0
        assert np.array_equal(tl.score, want["mean_p"][:, 1].astype(np.float64))
        assert np.array_equal(tl.smoothed, R.ema(tl.score, 2))
        state, events = R.state_and_events(tl.smoothed, tl.t_end, 0.55, 0.45, 2)
        assert np.array_equal(tl.state, state) and len(tl.events) == len(events)
        assert np.allclose(np.array(tl.events).reshape(-1, 4), np.array(events).reshape(-1, 4), rtol=1e-13, atol=0)
        assert tl.warmup.tolist() == [True] * warm + [False] * (37 - warm)
        assert tl.meta["members"] == M and tl.meta["warmup_windows"] == warm
    after = _host(Ensemble(models, eval_batch=16).predict(own))
    for k in FIELDS:
        assert np.array_equal(after[k].view(np.uint32), before[k].view(np.uint32)), k


def test_recording_windows_refuses_what_it_cannot_take():
    from multimodalsignal_amd.monitor import RecordingWindows
    _sig, dev = _recording(256, 64)
    with pytest.raises(ValueError):
        RecordingWindows(dev.cpu(), NAMES8, ["chest_ECG"], 256, 64)                # a CPU tensor: no fallback
    with pytest.raises(ValueError):
        RecordingWindows(dev.float(), NAMES8, ["chest_ECG"], 256, 64)
    with pytest.raises(ValueError):
        RecordingWindows(dev, NAMES8[:7], ["chest_ECG"], 256, 64)
    with pytest.raises(ValueError):
        RecordingWindows(dev, NAMES8, ["no_such"], 256, 64)
    with pytest.raises(ValueError):
        RecordingWindows(dev[:200], NAMES8, ["chest_ECG"], 256, 64)                # shorter than a window
    with pytest.raises(ValueError):
        RecordingWindows(dev, NAMES8, ["chest_ECG"], 256, 64, reference="head:99")
    rw = RecordingWindows(dev, NAMES8, ["chest_ECG", "chest_EDA"], 256, 64, reference=(3, 11))
    given = RecordingWindows(dev, NAMES8, ["chest_ECG", "chest_EDA"], 256, 64, reference=rw.stats)
    assert rw.mask == 0b10 and torch.equal(given.batch(5, 3), rw.batch(5, 3)) and given.warmup == 0
    with pytest.raises(RuntimeError):
        rw.batch(30, 16)                                                            # past the last window: MSIG_E_SHAPE


# ---- 4. from_run ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run_dir(tmp_path_factory):
    """A run directory of saved random state_dicts: folds S2 and S10, replica 0 and seed_1/."""
    from multimodalsignal_amd.synth import CHANNELS6
    root = tmp_path_factory.mktemp("run")
    seed = 40
    for rep in ("", "seed_1"):
        for sid in ("S2", "S10"):
            d = root / rep / f"fold_test_on_{sid}"
            d.mkdir(parents=True)
            torch.save(_models("cnn_gru_attention", 6, 2, 1, seed)[0].state_dict(), d / "best_model.pt")
            seed += 1
    (root / "cv_summary.txt").write_text(f"实验配置:\nSEED: 42\nCHANNELS_TO_USE: {list(CHANNELS6)}\n", encoding="utf-8")
    return root


def test_from_run_chooses_the_folds_members_or_replica_0_of_every_fold(run_dir):
    from multimodalsignal_amd.ensemble import Ensemble, load_members
    from multimodalsignal_amd.monitor import Monitor
    from multimodalsignal_amd.synth import CHANNELS6, make_synthetic_recording
    sig, _ = make_synthetic_recording([(1, 20.0), (2, 20.0), (1, 10.0)], fs=64.0, seed=3)
    kw = dict(fs=64.0, window_s=4, stride_s=1, eval_batch=16)
    rel = lambda mon: [str(f.relative_to(run_dir)) for f in mon.files]      # noqa: E731
    held = Monitor.from_run(run_dir, subject="S10", **kw)
    assert rel(held) == ["fold_test_on_S10/best_model.pt", "seed_1/fold_test_on_S10/best_model.pt"]
    new = Monitor.from_run(run_dir, **kw)
    assert rel(new) == ["fold_test_on_S2/best_model.pt", "fold_test_on_S10/best_model.pt"]
    assert held.channels == new.channels == list(CHANNELS6) and held.ensemble.M == new.ensemble.M == 2
    for mon in (held, new):
        tl = mon.run(sig, CHANNELS6)
        x = mon.windows(sig, CHANNELS6).materialise()
        want = _host(Ensemble(load_members(mon.files, DEV), eval_batch=16).predict(x))
        for k in FIELDS:
            assert np.array_equal(getattr(tl, k).view(np.uint32), want[k].view(np.uint32)), k
    want = _host(Ensemble.from_run(run_dir, "S10", eval_batch=16).predict(held.windows(sig, CHANNELS6).materialise()))
    assert np.array_equal(held.run(sig, CHANNELS6).mean_p, want["mean_p"])
    with pytest.raises(FileNotFoundError):
        Monitor.from_run(run_dir, subject="S3", **kw)


def test_cli_writes_the_timeline_of_the_synthetic_recording(run_dir, tmp_path, capsys):
    from multimodalsignal_amd import monitor
    tl = monitor.main(["--run", str(run_dir), "--synthetic-recording", "--window-s", "8", "--stride-s", "8", "--reference", "head:6",
                       "--out", str(tmp_path / "o")])
    n = (40 * 60 * 64 - 512) // 512 + 1
    rows = (tmp_path / "o" / "timeline.csv").read_text().splitlines()
    assert len(tl.t_end) == n and len(rows) == n + 1 and rows[0].startswith("window,t_end_s,score")
    doc = json.loads((tmp_path / "o" / "timeline.json").read_text())
    assert doc["windows"] == n and doc["members"] == 2 and doc["warmup_windows"] == 6 and doc["reference"] == "head:6"
    assert doc["note"] == monitor.SYNTHETIC_NOTE and set(doc["flagged_by_label"]) == {"1", "2", "3", "4"}
    assert sum(v["windows"] for v in doc["flagged_by_label"].values()) <= n and len(doc["events"]) == len(tl.events)
    assert "synthetic recording" in capsys.readouterr().out
