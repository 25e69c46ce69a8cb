"""GPU tier of the baseline-referenced normalisation (include/msig_nr.h): msig_nr_normalise_subject against
the host rule, its two bit-for-bit identities with msig_normalise_subject, the SubjectStore on both paths, and the drivers."""
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from multimodalsignal_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# the four hard channels first, so that every C_all >= 4 has them (cf. test_trainer_gpu._raw_subject, restated here)
NAMES16 = ["chest_Temp", "chest_ACC_x", "chest_EDA", "chest_EMG", "chest_ECG", "chest_Resp", "chest_ACC_y", "chest_ACC_z",
           "wrist_ACC_x", "wrist_ACC_y", "wrist_ACC_z", "wrist_BVP", "wrist_EDA", "wrist_TEMP", "aux_0", "aux_1"]


def _raw_subject(N, T, C_all, ref, seed):
    """(N, T, C_all) float64 raw windows and their column names.  Ordinary columns have an offset and a spread of order 1; four are
    what a one-pass variance and a log1p find hard: chest_Temp 33 +- 0.05 and chest_ACC_x 0.9 +- 0.02 (mean >> spread), chest_EDA
    positive and heavy-tailed (the one column under log1p), chest_EMG exactly constant at 0.75 (variance exactly 0, here and in every
    window).  Every second window outside `ref` is moved away by 12 of the column's standard deviations (chest_EDA: in the log1p
    domain, 4 against a spread of ~0.3), so that its z-scores under the reference statistics reach 10 and more."""
    names = NAMES16[:C_all]
    rs = np.random.RandomState(seed)
    spread = 0.5 + rs.rand(C_all)
    raw = rs.randn(N, T, C_all) * spread + rs.randn(C_all)
    hard = {"chest_Temp": (33.0, 0.05), "chest_ACC_x": (0.9, 0.02)}
    for name, (m, s) in hard.items():
        if name in names:
            raw[:, :, names.index(name)] = m + s * rs.randn(N, T)
            spread[names.index(name)] = s
    if "chest_EDA" in names:
        raw[:, :, names.index("chest_EDA")] = np.exp(0.8 * rs.randn(N, T)) + 0.1
    far = [n for n in np.flatnonzero(~np.asarray(ref, dtype=bool))][::2]
    for c, name in enumerate(names):
        if name == "chest_EDA":
            raw[far, :, c] = (1.0 + raw[far, :, c]) * np.exp(4.0) - 1.0
        elif name != "chest_EMG":
            raw[far, :, c] += 12.0 * spread[c]
    if "chest_EMG" in names:
        raw[:, :, names.index("chest_EMG")] = 0.75
    return raw, names


def _mask(N, windows):
    ref = np.zeros(N, dtype=bool)
    ref[list(windows)] = True
    return ref


CASES = [
    # one workgroup of rows (448 rows), a mask that is not contiguous
    (7, 64, 5, [3, 2, 0, 1], [0, 1, 5]),
    # MSIG_MAX_C columns in a permuted order, chest_EDA (column 2) in the middle
    (9, 200, 16, [15, 3, 8, 0, 12, 5, 10, 2, 14, 6, 1, 9, 4, 13, 7, 11], [1, 2, 6]),
    # 153 600 rows > the 512 x 256 threads of one grid pass: the grid-stride loop and the reduction of 512 partials; five scattered windows
    (40, 3840, 8, [7, 2, 0, 3, 5, 1], [0, 7, 8, 21, 39]),
    # C = 1, one reference window
    (3, 64, 2, [1], [1]),
]
IDS = ["n7-t64-4of5", "n9-t200-16of16", "n40-t3840-6of8", "n3-t64-1of2"]


def _nr_call(raw, cols, names, ref, with_stats=True):
    from multimodalsignal_amd.dataset import normalise_subject_device
    stats = torch.full((2 * L.MAX_C + 1,), float("nan"), dtype=torch.float64, device=DEV) if with_stats else None
    got = normalise_subject_device(torch.from_numpy(raw).to(DEV), cols, names, ref, stats=stats)
    torch.cuda.synchronize()
    return got.cpu().numpy(), (stats.cpu().numpy() if with_stats else None)


@pytest.mark.parametrize("N,T,C_all,cols,windows", CASES, ids=IDS)
def test_kernel_matches_the_host_rule(N, T, C_all, cols, windows):
    """msig_nr_normalise_subject against dataset.normalise_subject(..., ref=mask) — float64 numpy, two passes — cast to fp32.
    Bound: |got - want| <= 2e-6 * max(1, |want|), the project's 2e-6 of this stage scaled for outputs above 1."""
    from multimodalsignal_amd.dataset import normalise_subject
    ref = _mask(N, windows)
    raw, names_all = _raw_subject(N, T, C_all, ref, seed=N + T)
    names = [names_all[c] for c in cols]
    if C_all >= 4:
        for need in ("chest_Temp", "chest_ACC_x", "chest_EDA", "chest_EMG"):
            assert need in names
        assert 0 < names.index("chest_EDA") < len(cols) - 1 and cols != sorted(cols)
    want64 = normalise_subject(raw[:, :, cols], names, ref)                    # the fancy index is a private copy
    want = want64.transpose(0, 2, 1).astype(np.float32)
    got, stats = _nr_call(raw, cols, names, ref)
    assert got.shape == (N, len(cols), T) and got.dtype == np.float32
    assert np.abs(want).max() >= 10.0, "the far windows must reach |z| >= 10"
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.maximum(1.0, np.abs(want.astype(np.float64)))
    print(f"msig_nr_normalise_subject N={N} T={T} C={len(cols)}/{C_all}: max |got - want| / max(1, |want|) = {err.max():.3e}, "
          f"max |want| = {np.abs(want).max():.2f}")
    assert err.max() <= 2e-6
    if "chest_EMG" in names:
        c = names.index("chest_EMG")
        assert np.all(got[:, c, :] == 0.0) and np.all(want[:, c, :] == 0.0)
    # the statistics the kernel applied
    v = raw[:, :, cols].copy()
    for c, name in enumerate(names):
        if name == "chest_EDA":
            v[:, :, c] = np.log1p(v[:, :, c])
    mean = np.array([np.mean(v[ref][:, :, c]) for c in range(len(cols))])
    inv = np.array([1.0 / (np.std(v[ref][:, :, c]) + 1e-8) for c in range(len(cols))])
    rel_m = np.abs(stats[:len(cols)] - mean) / np.abs(mean)
    rel_s = np.abs(stats[L.MAX_C:L.MAX_C + len(cols)] - inv) / inv
    print(f"  stats: max relative deviation of the mean {rel_m.max():.3e}, of 1 / (std + 1e-8) {rel_s.max():.3e}")
    assert rel_m.max() <= 1e-12 and rel_s.max() <= 1e-12
    assert stats[2 * L.MAX_C] == len(windows)
    # deterministic: a second call gives the same bits
    again, stats2 = _nr_call(raw, cols, names, ref)
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32)) and np.array_equal(stats2[:len(cols)], stats[:len(cols)])


@pytest.mark.parametrize("N,T,C_all,cols,windows", [CASES[0], CASES[2]], ids=[IDS[0], IDS[2]])
def test_all_and_none_selected_are_msig_normalise_subject_bit_for_bit(N, T, C_all, cols, windows):
    from multimodalsignal_amd.dataset import normalise_subject_device
    raw, names_all = _raw_subject(N, T, C_all, _mask(N, windows), seed=N + T)
    names = [names_all[c] for c in cols]
    plain = normalise_subject_device(torch.from_numpy(raw).to(DEV), cols, names)
    torch.cuda.synchronize()
    plain = plain.cpu().numpy()
    for ref, count in ((np.ones(N, dtype=bool), N), (np.zeros(N, dtype=bool), 0)):
        got, stats = _nr_call(raw, cols, names, ref)
        assert np.array_equal(got.view(np.uint32), plain.view(np.uint32)), count
        assert stats[2 * L.MAX_C] == count
    # any non-zero byte selects; a torch mask works too
    got, _ = _nr_call(raw, cols, names, torch.full((N,), True), with_stats=False)
    assert np.array_equal(got.view(np.uint32), plain.view(np.uint32))
    part, _ = _nr_call(raw, cols, names, _mask(N, windows), with_stats=False)
    assert not np.array_equal(part, plain)


def test_python_entry_refuses_what_it_cannot_take():
    from multimodalsignal_amd.dataset import normalise_subject_device
    raw = torch.zeros(4, 8, 3, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        normalise_subject_device(raw, [0], ["a"], np.ones(5, dtype=bool))
    with pytest.raises(ValueError):
        normalise_subject_device(raw, [0], ["a"], np.ones(4, dtype=bool), stats=torch.zeros(8, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        normalise_subject_device(raw, [0], ["a"], np.ones(4, dtype=bool), stats=torch.zeros(33, dtype=torch.float32, device=DEV))
    with pytest.raises(RuntimeError):
        normalise_subject_device(raw, [3], ["a"], np.ones(4, dtype=bool))            # MSIG_E_SHAPE from the library, before a launch


# ---- the store ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def store_dir(tmp_path_factory):
    """Three subjects, T = 256, all 16 columns on disk; S4 has no baseline window."""
    d = tmp_path_factory.mktemp("norm_ref_store")
    labels = {"S2": [1, 1, 2, 3, 4, 1, 2], "S3": [2, 1, 3, 1, 4, 2, 1, 1, 3], "S4": [2, 3, 4, 2, 3]}
    for i, (sid, y) in enumerate(labels.items()):
        y = np.array(y, dtype=np.int64)
        raw, names = _raw_subject(len(y), 256, 16, y == 1 if (y == 1).any() else np.ones(len(y), dtype=bool), seed=50 + i)
        np.save(d / f"{sid}_X.npy", raw)
        np.save(d / f"{sid}_y.npy", y)
    return d, list(labels), NAMES16, ["chest_Resp", "chest_Temp", "chest_EDA", "chest_EMG", "chest_ACC_x", "wrist_BVP"]


def test_store_device_path_matches_host_path(store_dir, capsys):
    from multimodalsignal_amd.dataset import SubjectStore, WesadDataset
    d, subs, names, chans = store_dir
    for reference, used in (("baseline", {"S2": (3, False), "S3": (4, False), "S4": (0, True)}),
                            ("baseline:2", {"S2": (2, False), "S3": (2, False), "S4": (0, True)})):
        capsys.readouterr()
        host = SubjectStore(d, subs, chans, names, device=DEV, normalise="host", reference=reference)
        out_host = capsys.readouterr().out
        dev = SubjectStore(d, subs, chans, names, device=DEV, normalise="device", reference=reference)
        out_dev = capsys.readouterr().out
        assert host.reference_windows == used and dev.reference_windows == used          # the device count is the kernel's own
        for out in (out_host, out_dev):
            assert out.count("Warning: subject S4 has no baseline window") == 1 and out.count("Warning") == 1
            assert f"S2: reference {reference}: {used['S2'][0]} of 7 windows" in out
        a, b = host.x.cpu().numpy().astype(np.float64), dev.x.cpu().numpy().astype(np.float64)
        err = np.abs(a - b) / np.maximum(1.0, np.abs(a))
        print(f"SubjectStore reference={reference}: device vs host max scaled difference {err.max():.3e}, max |z| {np.abs(a).max():.2f}")
        assert err.max() <= 2e-6 and np.abs(a).max() >= 10.0
        assert torch.equal(host.y, dev.y) and host.ranges == dev.ranges
        # the host store is the dataset's float64 rule, cast
        ds = WesadDataset(d, subs, chans, names, reference=reference)
        assert np.array_equal(host.x.cpu().numpy(), ds.data.transpose(0, 2, 1).astype(np.float32))
        # the subject without a baseline window has the subject rule's bits on either path
        lo, hi = host.ranges["S4"]
        for path, store in (("host", host), ("device", dev)):
            plain = SubjectStore(d, ["S4"], chans, names, device=DEV, normalise=path)
            assert torch.equal(store.x[lo:hi], plain.x), path


def test_subject_reference_is_todays_store_on_both_paths(store_dir, capsys):
    from multimodalsignal_amd.dataset import SubjectStore, normalise_subject, normalise_subject_device
    d, subs, names, chans = store_dir
    cols = [names.index(c) for c in chans]
    for path in ("host", "device"):
        capsys.readouterr()
        a = SubjectStore(d, subs, chans, names, device=DEV, normalise=path)
        b = SubjectStore(d, subs, chans, names, device=DEV, normalise=path, reference="subject")
        assert capsys.readouterr().out == "" and b.reference_windows == {}
        assert torch.equal(a.x, b.x) and torch.equal(a.y, b.y)
        # ... which is what the parent commit's store held: the unchanged per-subject calls, concatenated
        parts = []
        for sid in subs:
            raw = np.load(d / f"{sid}_X.npy")
            if path == "host":
                parts.append(torch.from_numpy(np.ascontiguousarray(normalise_subject(raw[:, :, cols], chans).transpose(0, 2, 1), dtype=np.float32)))
            else:
                parts.append(normalise_subject_device(torch.from_numpy(raw).to(DEV), cols, chans).cpu())
        assert torch.equal(a.x.cpu(), torch.cat(parts))


# ---- the drivers ------------------------------------------------------------------------------------------------------------

def _run_main(out, data, extra, limit):
    """One driver command as a child process of its own, under its own time limit."""
    env = dict(os.environ, PYTHONPATH=str(ROOT), MPLBACKEND="Agg")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "multimodalsignal_amd.main", "--synthetic", str(data), "--synthetic-windows", "24", "--samples", "256",
           "--subjects", "S2", "S3", "S4", "S5", "--epochs", "2", "--batch-size", "16", "--out", str(out), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=limit, cwd=str(ROOT))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    runs = sorted(Path(out).glob("simple_binary/run_*"))
    assert len(runs) == 1
    return runs[0], r.stdout


@pytest.fixture(scope="module")
def synth_dir(tmp_path_factory):
    from multimodalsignal_amd.synth import make_synthetic_wesad
    return make_synthetic_wesad(tmp_path_factory.mktemp("norm_ref_synth") / "w", subjects=["S2", "S3", "S4", "S5"], windows_per_subject=24, T=256,
                                difficulty=2.0)


def test_driver_two_references_in_one_job(synth_dir, tmp_path):
    subs = ["S2", "S3", "S4", "S5"]
    plain, _ = _run_main(tmp_path / "plain", synth_dir, [], 300)
    both, out = _run_main(tmp_path / "both", synth_dir, ["--norm-reference", "subject", "baseline"], 300)
    assert not (plain / "normalisation.json").exists() and "NORM_REFERENCE" not in (plain / "cv_summary.txt").read_text(encoding="utf-8")
    doc = json.loads((both / "normalisation.json").read_text())
    assert doc["references"] == ["subject", "baseline"] and doc["anchor"] == "subject" and doc["synthetic"] is True
    st = doc["sets"][""]
    assert st["n_folds"] == 4 and list(st["references"]) == ["subject", "baseline"]
    for ref in ("subject", "baseline"):
        e = st["references"][ref]
        assert [f["subject"] for f in e["folds"]] == subs
        for m in ("accuracy", "f1_score"):
            assert set(e["summary"][m]) == {"mean", "std"} and set(e["difference"][m]) == {"mean", "std", "wins", "ties", "losses"}
            assert e["difference"][m]["wins"] + e["difference"][m]["ties"] + e["difference"][m]["losses"] == 4
            assert e["summary"][m]["mean"] == pytest.approx(np.mean([f[m] for f in e["folds"]]))
        cv = (both / ref / "cv_summary.txt").read_text(encoding="utf-8")
        assert f"NORM_REFERENCE: {ref}\n" in cv and f"{e['summary']['accuracy']['mean']:.4f}" in cv
    assert st["references"]["subject"]["difference"]["accuracy"]["ties"] == 4
    for sid in subs:
        y = np.load(synth_dir / f"{sid}_y.npy")
        assert doc["reference_windows"]["baseline"][sid] == {"n_windows": 24, "reference_windows": int((y == 1).sum()), "fallback": False}
        assert doc["reference_windows"]["subject"][sid] == {"n_windows": 24, "reference_windows": 24, "fallback": False}
        assert f"{sid}: reference baseline: {int((y == 1).sum())} of 24 windows" in out
    txt = (both / "normalisation.txt").read_text(encoding="utf-8")
    assert all(s in txt for s in subs) and "wins" in txt and "not what a reference costs or gains on WESAD" in txt
    # the subject configuration of the job is the run without the flag: per-fold metrics and checkpoint bytes
    for sid in subs:
        fold = f"fold_test_on_{sid}"
        a, b = json.loads((plain / fold / "fold_result.json").read_text()), json.loads((both / "subject" / fold / "fold_result.json").read_text())
        assert (a["accuracy"], a["f1_score"]) == (b["accuracy"], b["f1_score"]), sid
        assert (plain / fold / "best_model.pt").read_bytes() == (both / "subject" / fold / "best_model.pt").read_bytes(), sid
        assert (both / "baseline" / fold / "best_model.pt").read_bytes() != (plain / fold / "best_model.pt").read_bytes(), sid


def test_driver_hierarchical_with_a_reference(synth_dir, tmp_path):
    run, _ = _run_main(tmp_path / "h", synth_dir, ["--norm-reference", "baseline:2", "--hierarchical"], 300)
    txt = (run / "hierarchical_summary.txt").read_text(encoding="utf-8")
    assert "NORM_REFERENCE: baseline:2\n" in txt and not (run / "normalisation.json").exists()


def test_driver_ablation_with_a_reference(synth_dir, tmp_path):
    run, out = _run_main(tmp_path / "a", synth_dir, ["--norm-reference", "baseline", "--ablation"], 300)
    sets = sorted(p.name for p in run.iterdir() if p.is_dir())
    assert sets == ["chest_only", "ecg_only", "eda_only", "wrist_only"]
    for s in sets:
        assert "NORM_REFERENCE: baseline\n" in (run / s / "cv_summary.txt").read_text(encoding="utf-8")
    assert "reference baseline" in out and not (run / "normalisation.json").exists()
