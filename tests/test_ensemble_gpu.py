"""Deep ensembles on the GPU (include/msig_en.h, multimodalsignal_amd/ensemble.py): the reduction against its fp64 restatement
(tests/en_reference.py) and, bit for bit, against msig_mc_reduce on the transposed stack; the fold-batch form against the single one;
Ensemble.predict over its three routes; and the driver's --seeds run."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

import en_reference as E

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
T = 256
INT = ("pred", "votes", "member_pred")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "the gpu tier needs an MI355X"


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _outputs(M, N, K, skip=()):
    shapes = dict(mean_p=(N, K), std_p=(N, K), votes=(N, K), member_pred=(N, M))
    return {name: None if name in skip else torch.full(shapes.get(name, (N,)), -77, dtype=torch.int32 if name in INT else torch.float32, device=DEV)
            for name in E.OUTS}


def _host(o):
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in o.items()}


def _reduce(stack, stride, M, N, K, skip=()):
    """msig_en_reduce on a device buffer whose member blocks are `stride` floats apart."""
    from multimodalsignal_amd import _lib as L
    o = _outputs(M, N, K, skip)
    L.check(L.lib().msig_en_reduce(stack.data_ptr(), stride, M, N, K, *(_ptr(o[n]) for n in E.OUTS), _stream()), "msig_en_reduce")
    return _host(o)


def _assert_matches(got, ref, what=""):
    for name in INT:
        assert np.array_equal(got[name], ref[name]), (what, name)
    for name in E.FLOAT_OUTS:
        err = np.abs(got[name].astype(np.float64) - ref[name])
        print(f"{what} {name}: max |got - ref| {err.max():.3e}, in units of 2 ulp + 1e-12: {(err / (2 * E.ulp32(ref[name]) + 1e-12)).max():.3f}")
        assert E.within_store_rounding(got[name], ref[name]), (what, name, float(err.max()))


# ---- 1. the reduction against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3, 16])
@pytest.mark.parametrize("M", [1, 2, 7, 256])
def test_reduce_against_the_restatement(M, K):
    N = 5
    lg = E.crafted_logits(M, N, K, 100 * M + K)
    dev = torch.as_tensor(lg).to(DEV)
    got, ref = _reduce(dev, N * K, M, N, K), E.reduce(lg)
    _assert_matches(got, ref, f"M={M} K={K}")
    assert ref["votes"][1, 0] == M and ref["pred"][1] == 0 and got["mean_p"][1, 0] == got["mean_p"][1, 1]          # the tie: first maximum
    assert got["votes"][2].max() == M and abs(float(got["mutual_info"][2])) <= 1e-12 and got["disagreement"][2] == 0.0   # all members equal
    assert np.array_equal(got["member_pred"][1], np.zeros(M, dtype=np.int32))
    if M == 1:
        assert np.all(got["disagreement"] == 0.0)
    # each window reduced alone: the same bits as in the batch
    for n in range(N):
        one = _reduce(dev[:, n:n + 1, :].contiguous(), K, M, 1, K)
        for name in E.OUTS:
            assert np.array_equal(one[name][0], got[name][n]), (n, name)
    # optional outputs left out: the others' bits are unchanged
    for skip in (("std_p", "votes", "member_pred"), ("pred", "entropy", "expected_entropy", "mutual_info", "disagreement"), E.OUTS[1:]):
        part = _reduce(dev, N * K, M, N, K, skip=skip)
        for name in E.OUTS:
            assert (part[name] is None) if name in skip else np.array_equal(part[name], got[name]), (skip, name)
    # a padded member stride: the bits of the tight stack
    stride = N * K + 3
    padded = torch.full((M, stride), float("nan"), dtype=torch.float32, device=DEV)
    padded[:, :N * K] = dev.reshape(M, N * K)
    wide = _reduce(padded, stride, M, N, K)
    for name in E.OUTS:
        assert np.array_equal(wide[name], got[name]), name


# ---- 2. the summation order: msig_mc_reduce on the transpose, bit for bit ----------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3, 16])
@pytest.mark.parametrize("M", [1, 2, 7, 256])
def test_common_outputs_are_the_monte_carlo_reduction_of_the_transpose(M, K):
    from multimodalsignal_amd import _lib as L
    N = 5
    lg = E.crafted_logits(M, N, K, 100 * M + K)
    got = _reduce(torch.as_tensor(lg).to(DEV), N * K, M, N, K)
    tr = torch.as_tensor(np.ascontiguousarray(lg.transpose(1, 0, 2)).reshape(N * M, K)).to(DEV)
    o = {k: v for k, v in _outputs(M, N, K).items() if k in E.COMMON}
    L.check(L.lib().msig_mc_reduce(tr.data_ptr(), N, M, K, *(_ptr(o[n]) for n in E.COMMON), _stream()), "msig_mc_reduce")
    mc = _host(o)
    for name in E.COMMON:
        assert np.array_equal(mc[name], got[name]), name


# ---- 3. the fold-batch form ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 3, 16])
def test_reduce_multi_is_the_single_form_on_the_gathered_stack(M):
    """The members' blocks lie 512 bytes apart in arenas visited in a non-identity order, with poison between them; all outputs live
    in one guarded buffer: nothing but the outputs is written."""
    from multimodalsignal_amd import _lib as L
    N, K, stride_b = 5, 3, 512
    lg = E.crafted_logits(M, N, K, 7 + M)
    slots = [(11 * i + 5) % 17 for i in range(M)]                 # 5, 16, 10, ...: distinct (11 and 17 are coprime), not increasing, with gaps
    assert len(set(slots)) == M and (M == 1 or slots != sorted(slots))
    arenas = torch.full((17, stride_b // 4), float("nan"), dtype=torch.float32, device=DEV)
    for z, s in enumerate(slots):
        arenas[s, :N * K] = torch.as_tensor(lg[z]).reshape(-1).to(DEV)
    before = arenas.clone()
    m = L.Multi()
    m.n, m.stride_bytes, m.form_folds = M, stride_b, 1
    for z, s in enumerate(slots):
        m.slot[z] = s
    # one guarded buffer for every output (4-byte elements): [guard | out | guard | out | ... | guard]
    sizes = dict(mean_p=N * K, std_p=N * K, votes=N * K, member_pred=N * M)
    GUARD, at, where = 64, 64, {}
    for name in E.OUTS:
        where[name] = (at, sizes.get(name, N))
        at += sizes.get(name, N) + GUARD
    buf = torch.full((at,), -77, dtype=torch.int32, device=DEV)
    ptrs = [buf.data_ptr() + 4 * where[name][0] for name in E.OUTS]
    L.check(L.lib().msig_en_reduce_multi(arenas.data_ptr(), C.byref(m), N, K, *ptrs, _stream()), "msig_en_reduce_multi")
    torch.cuda.synchronize()
    single = _reduce(torch.as_tensor(lg).to(DEV), N * K, M, N, K)
    host = buf.cpu().numpy()
    written = np.zeros(at, dtype=bool)
    for name in E.OUTS:
        o, n = where[name]
        written[o:o + n] = True
        got = host[o:o + n] if name in INT else host[o:o + n].view(np.float32)
        assert np.array_equal(got.reshape(single[name].shape), single[name]), name
    assert np.all(host[~written] == -77)                                           # every byte outside the outputs
    assert torch.equal(arenas.view(torch.int32), before.view(torch.int32))         # the logits and the poison between them


# ---- 4. Ensemble.predict ----------------------------------------------------------------------------------------------------------------
CONFIGS = {"full": dict(), "embedded": dict(gru_hidden_size=32, gru_num_layers=1)}
CASES = [("cnn_gru_attention", "full", 6, 3), ("cnn_gru", "full", 6, 2), ("cnn_gru_attention", "full", 2, 2), ("cnn_gru", "embedded", 2, 3)]


def _case(B, Cin, K, seed):
    rs = np.random.RandomState(seed)
    x = (rs.randn(B, Cin, T) * (0.5 + rs.rand(1, Cin, 1)) + rs.randn(1, Cin, 1)).astype(np.float32)
    return torch.as_tensor(x), torch.as_tensor(rs.randint(0, K, size=(B,)).astype(np.int64))


def _trained(kind, config, Cin, K, seed):
    """A model after two real train steps (its BatchNorm running statistics have moved), as test_mc_dropout_gpu.py's helper."""
    from multimodalsignal_amd.models import CnnGruAttentionModel, CnnGruModel
    torch.manual_seed(seed)
    cls = CnnGruAttentionModel if kind == "cnn_gru_attention" else CnnGruModel
    m = cls(Cin, K, dropout=0.5, **CONFIGS[config]).to(DEV).train()
    opt = torch.optim.SGD(m.parameters(), lr=0.05)
    for s in range(2):
        x, y = _case(16, Cin, K, 50 + s + seed)
        opt.zero_grad()
        torch.nn.CrossEntropyLoss()(m(x.to(DEV)), y.to(DEV)).backward()
        opt.step()
    return m.eval()


@functools.lru_cache(maxsize=None)
def _members(kind, config, Cin, K):
    """Three members, the windows and the members' own eval logits (N, K) each — computed once per case."""
    from multimodalsignal_amd.uncertainty import eval_logits
    models = [_trained(kind, config, Cin, K, 11 + r) for r in range(3)]
    x = _case(37, Cin, K, 900 + Cin)[0].to(DEV)
    logits = [eval_logits(m, x).cpu().numpy() for m in models]
    return models, x, logits


def _fields(p):
    torch.cuda.synchronize()
    return {name: getattr(p, name).cpu().numpy() for name in E.OUTS}


@pytest.mark.parametrize("kind,config,Cin,K", CASES)
def test_ensemble_predict(kind, config, Cin, K):
    from multimodalsignal_amd.ensemble import Ensemble
    models, x, logits = _members(kind, config, Cin, K)
    N = x.shape[0]
    state = [({k: v.clone() for k, v in m.state_dict().items()}, m.engine().bn_state.clone(), m.engine().bn_count.clone()) for m in models]
    rng, cpu_rng = torch.cuda.get_rng_state(DEV), torch.get_rng_state()
    # N = 37 in pieces of 16: two full pieces and a ragged one of 5
    p = Ensemble(models, eval_batch=16).predict(x)
    got = _fields(p)
    assert (p.n, p.members) == (N, 3) and got["member_pred"].shape == (N, 3)
    _assert_matches(got, E.reduce(np.stack(logits)), f"{kind} {config} C={Cin} K={K}")
    assert len({lg.tobytes() for lg in logits}) == 3 and float(got["std_p"].max()) > 0          # the members differ
    single = _fields(Ensemble(models, batched=False, eval_batch=16).predict(x))
    whole = _fields(Ensemble(models, eval_batch=1024).predict(x))
    for name in E.OUTS:
        assert np.array_equal(single[name], got[name]) and np.array_equal(whole[name], got[name]), name
    # one member: the model's own eval prediction, no mutual information, no disagreement
    one = _fields(Ensemble(models[:1], eval_batch=16).predict(x))
    assert np.array_equal(one["pred"], logits[0].argmax(axis=1)) and np.array_equal(one["member_pred"][:, 0], one["pred"])
    assert float(np.abs(one["mutual_info"]).max()) <= 1e-12 and np.all(one["disagreement"] == 0.0) and float(one["std_p"].max()) == 0.0
    # seventeen members (the three, repeated): more than a fold batch holds, so the logits go through the (M, N, K) stack
    idx = [i % 3 for i in range(17)]
    many = Ensemble([models[i] for i in idx], eval_batch=16)
    got17 = _fields(many.predict(x))
    _assert_matches(got17, E.reduce(np.stack([logits[i] for i in idx])), "M=17")
    single17 = _fields(Ensemble([models[i] for i in idx], batched=False, eval_batch=16).predict(x))
    for name in E.OUTS:
        assert np.array_equal(single17[name], got17[name]), name
    # nothing of the models, their BatchNorm state or torch's RNG has moved
    for m, (sd, bn, cnt) in zip(models, state):
        after = m.state_dict()
        assert set(after) == set(sd) and all(torch.equal(after[k], sd[k]) for k in sd)
        assert torch.equal(m.engine().bn_state, bn) and torch.equal(m.engine().bn_count, cnt) and m.training is False
    assert torch.equal(torch.cuda.get_rng_state(DEV), rng) and torch.equal(torch.get_rng_state(), cpu_rng)


def test_ensemble_refuses_mixed_members():
    from multimodalsignal_amd.ensemble import Ensemble
    a, b = _members("cnn_gru_attention", "full", 6, 3)[0][0], _members("cnn_gru", "full", 6, 2)[0][0]
    with pytest.raises(ValueError):
        Ensemble([a, b])
    with pytest.raises(ValueError):
        Ensemble([])
    with pytest.raises(ValueError):
        Ensemble([a]).predict(torch.zeros(2, 6, T))                    # a CPU tensor: no fallback


# ---- 5. the driver ----------------------------------------------------------------------------------------------------------------------
EXTRA = lambda name: name.startswith("seed_") or name.startswith("seeds.") or name == "ensemble_result.json"


def _tree(run):
    return sorted(str(p.relative_to(run)) for p in run.rglob("*") if not any(EXTRA(part) for part in p.relative_to(run).parts))


def test_driver_seed_replicas_and_ensembles(tmp_path, capsys):
    """Three subjects: the smallest LOSO the command line runs, two epochs.  cv_summary.txt is compared without its wall-clock
    line, the checkpoints tensor by tensor."""
    from multimodalsignal_amd import ensemble as EN
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.dataset import DeviceLoader, SubjectStore
    from multimodalsignal_amd.synth import CHANNELS6, make_synthetic_wesad
    subs = ["S2", "S3", "S4"]
    d = make_synthetic_wesad(tmp_path / "w", subjects=subs, windows_per_subject=12, T=256, difficulty=2.0)
    common = ["--synthetic", str(d), "--samples", "256", "--subjects", *subs, "--epochs", "2", "--batch-size", "16"]
    M.main(common + ["--out", str(tmp_path / "plain")])
    M.main(common + ["--seeds", "3", "--out", str(tmp_path / "s3")])
    M.main(common + ["--seeds", "2", "--out", str(tmp_path / "s2")])
    M.main(common + ["--seeds", "2", "--model", "cnn_gru_attention", "cnn_gru", "--out", str(tmp_path / "pair")])
    out = capsys.readouterr().out
    runs = {k: sorted((tmp_path / k).glob("simple_binary/run_*"))[0] for k in ("plain", "s3", "s2", "pair")}
    cut = lambda text: text[:text.index("LOSO wall-clock")]
    load = lambda run, rel: torch.load(run / rel / "best_model.pt", map_location="cpu")
    same = lambda a, b: set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    # replica 0 is the run without the flag
    assert cut((runs["s3"] / "cv_summary.txt").read_text(encoding="utf-8")) == cut((runs["plain"] / "cv_summary.txt").read_text(encoding="utf-8"))
    assert _tree(runs["s3"]) == _tree(runs["plain"])
    assert not any(EXTRA(part) for p in runs["plain"].rglob("*") for part in p.relative_to(runs["plain"]).parts)
    for s in subs:
        fold = f"fold_test_on_{s}"
        assert same(load(runs["s3"], fold), load(runs["plain"], fold)), s
        assert not same(load(runs["s3"], f"seed_1/{fold}"), load(runs["s3"], fold)), s
        assert not same(load(runs["s3"], f"seed_2/{fold}"), load(runs["s3"], f"seed_1/{fold}")), s
        # fewer seeds: the same replicas
        assert same(load(runs["s2"], fold), load(runs["s3"], fold)) and same(load(runs["s2"], f"seed_1/{fold}"), load(runs["s3"], f"seed_1/{fold}")), s
        assert sorted(p.name for p in (runs["s3"] / "seed_1" / fold).iterdir()) == sorted(
            p.name for p in (runs["s3"] / fold).iterdir() if p.name != "ensemble_result.json")
    assert not (runs["s2"] / "seed_2").exists() and not (runs["s3"] / "seed_1" / "cv_summary.txt").exists()
    # seeds.json is complete
    doc = json.loads((runs["s3"] / "seeds.json").read_text())
    assert doc["settings"] == {"seeds": 3, "stride": 1_000_003} and doc["note"] == EN.SYNTHETIC_NOTE and doc["pairs"] == []
    c = doc["configurations"][""]
    assert c["seeds"] == 3 and c["n_folds"] == 3 and [f["subject"] for f in c["folds"]] == subs
    for m in ("accuracy", "f1_score"):
        assert len(c[m]["per_seed"]) == 3 and c[m]["std"] is not None and c[m]["mean"] == pytest.approx(np.mean(c[m]["per_seed"]))
    cv = (runs["s3"] / "cv_summary.txt").read_text(encoding="utf-8")
    assert f"{c['accuracy']['per_seed'][0]:.4f}" in cv                                     # seed 0's LOSO mean is the summary's
    row_keys = {"n", "accuracy", "f1_score", "nll", "brier", "ece", "mean_disagreement", "entropy_correct", "entropy_wrong",
                "mutual_information_correct", "mutual_information_wrong", "auroc_entropy", "selective_accuracy"}
    for key in ("ensemble", "mean_member"):
        assert set(c[key]["pooled"]) == row_keys and c[key]["pooled"]["n"] == 36 and set(c[key]["loso_mean"]) == {"accuracy", "f1_score"}
        assert set(c[key]["pooled"]["selective_accuracy"]) == {"100", "90", "80", "50"}
    assert c["mean_member"]["loso_mean"]["accuracy"] == pytest.approx(c["accuracy"]["mean"])
    # per fold: three member accuracies (the replicas' own test passes), and the ensemble recomputed from the checkpoints
    store = SubjectStore(d, subs, list(CHANNELS6), [ln.strip() for ln in open(d / "_channel_names.txt") if ln.strip()],
                         classification_mode="stress_binary", device=DEV)
    for s, f in zip(subs, c["folds"]):
        per = json.loads((runs["s3"] / f"fold_test_on_{s}" / "ensemble_result.json").read_text())
        assert len(f["member_accuracy"]) == 3 and len(f["epochs"]) == 3 and f["n"] == 12 and per["members"] == 3
        for r in range(3):
            rel = f"fold_test_on_{s}" if r == 0 else f"seed_{r}/fold_test_on_{s}"
            assert f["member_accuracy"][r] == json.loads((runs["s3"] / rel / "fold_result.json").read_text())["accuracy"]
        assert per["seeds"] == [42 + subs.index(s) + r * 1_000_003 for r in range(3)]
        ds = store.view([s])
        ld = DeviceLoader(ds, 1024, False, DEV)
        idx = ld.index if ld.index is not None else torch.arange(len(ds), device=DEV)
        x, y = ld.store.index_select(0, idx), ld.store_y.index_select(0, idx).cpu().numpy()
        ens = EN.Ensemble.from_run(runs["s3"], s)
        assert ens.M == 3
        pred = ens.predict(x).pred.cpu().numpy()
        assert float((pred == y).mean()) == f["ensemble_accuracy"] == per["ensemble"]["accuracy"], s
        assert np.array_equal(pred, np.asarray(per["windows"]["mean_p"]).argmax(axis=1))
    txt = (runs["s3"] / "seeds.txt").read_text(encoding="utf-8")
    assert EN.SYNTHETIC_NOTE in txt and "ensemble" in txt and "mean member" in txt and all(s in txt for s in subs)
    assert "ensemble of 3 seeds over 12 windows" in out
    # two model kinds: the pair table over seeds
    pdoc = json.loads((runs["pair"] / "seeds.json").read_text())
    assert list(pdoc["configurations"]) == ["cnn_gru_attention", "cnn_gru"] and len(pdoc["pairs"]) == 1
    pair = pdoc["pairs"][0]
    assert (pair["a"], pair["b"]) == ("cnn_gru_attention", "cnn_gru") and len(pair["accuracy"]["per_seed_difference"]) == 2
    assert pair["accuracy"]["wins"] + pair["accuracy"]["losses"] + pair["accuracy"]["ties"] == 2 and pair["accuracy"]["ensemble_difference"] is not None
    assert (runs["pair"] / "comparison.json").exists() and (runs["pair"] / "cnn_gru" / "seed_1" / "fold_test_on_S2" / "best_model.pt").exists()
    assert EN.Ensemble.from_run(runs["pair"], "S3", config_name="cnn_gru").kind == "cnn_gru"
