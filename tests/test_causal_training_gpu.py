"""Training under the causal references (multimodalsignal_amd/dataset.py): the acceptance test.

A subject's window file is the consecutive windows of one recording, so the device store under --norm-reference expanding |
trailing:K | decayed:H holds the very fp32 rows — and the very float64 statistics records — that RecordingWindows hands the model for
that recording under the same --reference: msig_rn_sums on the file as a recording of N T samples at stride T forms every window's
sums in the order it forms them on the recording at its real stride.  One synthetic (L, 3) recording, T = 64, S = 16, 12 windows, one
log1p column ('chest_EDA'); the window file is cut from it on the host, as preprocessing would cut it.

Also here: the float64 host store against the device store (both against the np.longdouble restatement, tests/test_running_gpu.py's
bound carried to the rows), a LOSO run under expanding that a Monitor with reference="auto" then follows, a job of two references, and
the existing references' stores, which do not change."""
import json

import numpy as np
import pytest
import torch

import rd_reference as RD
import rn_reference as R
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd import dataset

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = float(np.finfo(np.float64).eps)
MC = L.MAX_C
T, S, N = 64, 16, 12
NAMES = ["chest_Temp", "chest_EDA", "chest_ECG"]
USE = ["chest_ECG", "chest_EDA", "chest_Temp"]                      # another order than the file's: cols = [2, 1, 0], log1p bit 1
REFS = ["expanding", "trailing:5", "trailing:40", "decayed:3"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "the gpu tier needs an MI355X"


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """The recording, and a directory with its window file as subject S2 (and a second subject S3 cut from the reversed recording)."""
    root = tmp_path_factory.mktemp("causal")
    Ln = (N - 1) * S + T
    rs = np.random.RandomState(37)
    t = np.arange(Ln)
    rec = np.empty((Ln, 3))
    rec[:, 0] = 33.0 + 0.05 * rs.randn(Ln) + 0.4 * t / Ln                         # mean >> spread, drifting
    rec[:, 1] = np.exp(0.6 * rs.randn(Ln) + 0.5 * np.sin(2 * np.pi * t / Ln)) + 0.1      # positive, heavy-tailed: under log1p
    rec[:, 2] = rs.randn(Ln) * (1.0 + t / Ln) + np.where(t > Ln // 2, 1.5, 0.0)   # a level shift half way
    rec = np.ascontiguousarray(rec)
    y = np.array([1] * 4 + [2] * 4 + [3] * 2 + [1] * 2)
    for sid, r in (("S2", rec), ("S3", np.ascontiguousarray(rec[::-1]))):
        np.save(root / f"{sid}_X.npy", np.stack([r[n * S:n * S + T] for n in range(N)]))
        np.save(root / f"{sid}_y.npy", y)
    return root, rec


def _selected(rec, Cn=3):
    return np.concatenate([rec[:, :Cn], rec[:, MC:MC + Cn], rec[:, 2 * MC:]], axis=1)


def _restated(rec, ref, dtype):
    """(mean, inv, c) of the recording's 12 windows from the restatements, and — np.longdouble only — the std unit of the bound."""
    cols = [NAMES.index(c) for c in USE]
    v = R.transformed(rec, cols, 0b010, dtype)
    run = dataset.parse_reference(ref)
    if run.kind == "decayed":
        return v, RD.stats_table(v, T, S, run.decay), (RD.std_longdouble(v, T, S, run.decay) if dtype is np.longdouble else None)
    m, i, c = R.stats_table(v, T, S, run.K)
    return v, (m, i, c.astype(dtype)), (R.std_longdouble(v, T, S, run.K) if dtype is np.longdouble else None)


@pytest.mark.parametrize("ref", REFS)
def test_the_device_store_holds_the_monitors_rows_and_records(case, ref):
    """uint32 equality of the store's rows with RecordingWindows(recording, reference=ref).batch(0, 12), uint64 equality of the
    per-window table with the recording's."""
    from multimodalsignal_amd.monitor import RecordingWindows
    root, rec = case
    store = dataset.SubjectStore(root, ["S2", "S3"], USE, NAMES, device=DEV, normalise="device", reference=ref)
    rw = RecordingWindows(rec, NAMES, USE, T, S, reference=ref)
    want = rw.batch(0, N)
    torch.cuda.synchronize()
    assert rw.n == N and tuple(store.x.shape) == (2 * N, 3, T) and store.ranges == {"S2": (0, N), "S3": (N, 2 * N)}
    assert np.array_equal(store.x[:N].cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))
    table = store.reference_tables["S2"].cpu().numpy()
    assert np.array_equal(_selected(table).view(np.uint64), _selected(rw.stats.cpu().numpy()).view(np.uint64))
    assert store.reference_windows == {"S2": ("per window", False), "S3": ("per window", False)}
    # S3 is another recording: its own pivot and records
    rw3 = RecordingWindows(np.ascontiguousarray(rec[::-1]), NAMES, USE, T, S, reference=ref)
    assert np.array_equal(store.x[N:].cpu().numpy().view(np.uint32), rw3.batch(0, N).cpu().numpy().view(np.uint32))
    assert not np.array_equal(store.x[:N].cpu().numpy(), store.x[N:].cpu().numpy())
    # and normalise_subject_device(running=) alone gives the store's rows, with or without a table to fill
    raw = torch.from_numpy(np.load(root / "S2_X.npy")).to(DEV)
    alone = dataset.normalise_subject_device(raw, [NAMES.index(c) for c in USE], USE, running=dataset.parse_reference(ref))
    assert np.array_equal(alone.cpu().numpy().view(np.uint32), store.x[:N].cpu().numpy().view(np.uint32))
    with pytest.raises(ValueError):
        dataset.normalise_subject_device(raw, [0], ["chest_Temp"], ref=np.ones(N, dtype=bool), running=dataset.parse_reference(ref))


@pytest.mark.parametrize("ref", REFS)
def test_the_host_store_agrees_with_the_device_store(case, ref):
    """Host (float64 numpy, dataset.running_statistics) and device (the store's table) against the np.longdouble restatement.
    Statistics: tests/test_running_gpu.py's bound, constants unchanged — a mean's error in units of the reference's std, the
    reciprocal's in units of itself, each at most 8 x the float64 restatement's own error on this case or a floor of 4 ulps (of
    |mean| + std, of the value).  Carried to the rows r = (v - mean) inv in float64: |dr| <= bound_mean std inv + |r| bound_inv, plus
    the statement's own three roundings, 4 eps (|r| + (|v| + |mean|) inv).  The fp32 stores then differ from the np.longdouble rows'
    fp32 rounding, and from each other, by at most one fp32 ulp.  Prints the measured error / bound of both sides."""
    root, rec = case
    cols = [NAMES.index(c) for c in USE]
    v64, (m64, i64, _c64), _ = _restated(rec, ref, np.float64)
    vld, (mld, ild, _cld), std = _restated(rec, ref, np.longdouble)
    assert np.all(std > 0)
    q_mean, q_inv = np.abs(m64 - mld) / std, np.abs(i64 - ild) / ild
    b_mean = np.maximum(8 * q_mean.max(axis=0)[None, :], 4 * EPS * (np.abs(mld) + std) / std)
    b_inv = np.maximum(8 * q_inv.max(axis=0)[None, :], 4 * EPS)
    dev_store = dataset.SubjectStore(root, ["S2"], USE, NAMES, device=DEV, normalise="device", reference=ref)
    host_store = dataset.SubjectStore(root, ["S2"], USE, NAMES, device=DEV, normalise="host", reference=ref)
    table = dev_store.reference_tables["S2"].cpu().numpy()
    x = np.load(root / "S2_X.npy")[:, :, cols].copy()
    x[:, :, 1] = np.log1p(x[:, :, 1])
    hm, hi, _hc = dataset.running_statistics(x, dataset.parse_reference(ref))
    wins_ld = np.stack([vld[n * S:n * S + T] for n in range(N)])                                  # (N, T, C)
    r_ld = (wins_ld - mld[:, None, :]) * ild[:, None, :]
    b_row = (b_mean * std * ild)[:, None, :] + np.abs(r_ld) * b_inv[:, None, :] \
        + 4 * EPS * (np.abs(r_ld) + (np.abs(wins_ld) + np.abs(mld)[:, None, :]) * ild[:, None, :])
    rows64 = {"host": dataset.WesadDataset(root, ["S2"], USE, NAMES, reference=ref).data,
              "device": (x - table[:, None, :3]) * table[:, None, MC:MC + 3]}
    for side, (m, i) in (("host", (hm, hi)), ("device", (table[:, :3], table[:, MC:MC + 3]))):
        e_mean, e_inv = np.abs(m - mld) / std, np.abs(i - ild) / ild
        e_row = np.abs(rows64[side] - r_ld)
        print(f"{ref} {side}: error / bound max: mean {float((e_mean / b_mean).max()):.3f}, inv {float((e_inv / b_inv).max()):.3f}, "
              f"rows {float((e_row / b_row).max()):.3f}")
        assert np.all(e_mean <= b_mean) and np.all(e_inv <= b_inv), side
        assert np.all(e_row <= b_row), side
    want32 = r_ld.astype(np.float32).transpose(0, 2, 1)
    h32, d32 = host_store.x.cpu().numpy(), dev_store.x.cpu().numpy()
    ulp = np.spacing(np.abs(want32))
    assert np.all(np.abs(h32 - want32) <= ulp) and np.all(np.abs(d32 - want32) <= ulp) and np.all(np.abs(h32 - d32) <= ulp)
    print(f"{ref}: fp32 rows that differ between the host and the device store: {int((h32 != d32).sum())} of {h32.size}")
    assert np.array_equal(h32.view(np.uint32), np.ascontiguousarray(rows64["host"].transpose(0, 2, 1), dtype=np.float32).view(np.uint32))


@pytest.mark.parametrize("ref", ["subject", "baseline:2"])
def test_the_existing_references_store_is_what_it_was(case, ref):
    """Without a running reference the store never enters the new code: it is normalise_subject_device called directly, bit for bit."""
    root, _rec = case
    store = dataset.SubjectStore(root, ["S2", "S3"], USE, NAMES, device=DEV, normalise="device", reference=ref)
    assert store.reference_tables == {}
    cols = [NAMES.index(c) for c in USE]
    for sid, (a, b) in store.ranges.items():
        raw = torch.from_numpy(np.load(root / f"{sid}_X.npy")).to(DEV)
        mask = dataset.subject_reference(np.load(root / f"{sid}_y.npy"), ref, sid)
        want = dataset.normalise_subject_device(raw, cols, USE, mask)
        assert (mask is None) == (ref == "subject")
        assert np.array_equal(store.x[a:b].cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))
    assert store.reference_windows == ({} if ref == "subject" else {"S2": (2, False), "S3": (2, False)})


def test_a_loso_job_of_two_references_and_a_monitor_that_follows_it(tmp_path):
    """main.run_experiments, three epochs, under --norm-reference expanding and decayed:3 as one job (three subjects: the smallest
    LOSO whose folds keep a training subject — split_train_val gives the validation set one of the two that remain): it finishes,
    each configuration's cv_summary.txt says NORM_REFERENCE, normalisation.json holds both with 'per window', and a Monitor and a
    LiveMonitor built with reference="auto" resolve to the run's reference and say so in the timeline's meta."""
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.live import LiveMonitor
    from multimodalsignal_amd.monitor import Monitor
    from multimodalsignal_amd.synth import CHANNELS6, make_synthetic_recording, make_synthetic_wesad
    subs, refs = ["S2", "S3", "S4"], ["expanding", "decayed:3"]
    d = make_synthetic_wesad(tmp_path / "w", subjects=subs, windows_per_subject=20, T=256, difficulty=2.0)
    names = (d / "_channel_names.txt").read_text().split()
    base = M.default_cfg()
    base.update(data_path=d, subjects=subs, epochs=3, patience=20, batch_size=16, concurrent_folds=8, normalise="device")
    out = tmp_path / "run"
    results, _wall = M.run_experiments(out, DEV, names, {M.reference_dir(r): dict(base, norm_reference=r) for r in refs})
    assert sorted(results) == ["decayed_3", "expanding"] and all(len(v) == 3 for v in results.values())
    for r in refs:
        cv = (out / M.reference_dir(r) / "cv_summary.txt").read_text(encoding="utf-8")
        assert f"NORM_REFERENCE: {r}\n" in cv
        assert all((out / M.reference_dir(r) / f"fold_test_on_{s}" / "best_model.pt").exists() for s in subs)
    path = M.write_normalisation(out, M.normalisation({"": {r: results[M.reference_dir(r)] for r in refs}}, refs, d, subs), synthetic=True)
    doc = json.loads((out / "normalisation.json").read_text())
    assert doc["references"] == refs and doc["anchor"] == "expanding" and list(doc["sets"][""]["references"]) == refs
    assert all(doc["reference_windows"][r][s] == {"n_windows": 20, "reference_windows": "per window", "fallback": False} for r in refs for s in subs)
    assert "  decayed:3: S2 per window, S3 per window, S4 per window" in path.read_text(encoding="utf-8")
    sig, _table = make_synthetic_recording([(1, 12.0), (2, 12.0)], fs=64.0, channels=list(CHANNELS6), seed=42, difficulty=1.0)
    kw = dict(fs=64.0, window_s=4, stride_s=1, reference="auto")
    for r, want in (("expanding", "expanding:6"), ("decayed:3", "decayed:3:6")):
        mon = Monitor.from_run(out, config_name=M.reference_dir(r), **kw)
        assert mon.reference == want and mon.reference_requested == "auto"
        tl = mon.run(sig, list(CHANNELS6))
        assert tl.meta["reference"] == want and tl.meta["reference_requested"] == "auto" and tl.meta["warmup_windows"] == 6
        assert len(tl.meta["reference_window_counts"]) == len(tl.t_end) == (sig.shape[0] - 256) // 64 + 1
        live = LiveMonitor.from_run(out, config_name=M.reference_dir(r), max_sessions=1, **kw)
        assert live.reference == want and live.reference_requested == "auto"
    from multimodalsignal_amd.live import timelines_equal
    live.open(0, list(CHANNELS6))
    live.push(0, np.ascontiguousarray(sig))
    assert timelines_equal(live.timeline(0), tl) and live.timeline(0).meta == tl.meta
