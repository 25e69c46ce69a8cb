"""Monte-Carlo dropout on the GPU (include/msig_mc.h, multimodalsignal_amd/uncertainty.py): the two kernels against their restatement
(tests/mc_reference.py), the trunk against an eval forward bit for bit, the tail against the oracle's pieces fed the GPU trunk's own
output, dropout 0, reproducibility and the absence of side effects, and the driver's --mc-dropout stage."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

import mc_reference as R
from gpu_common import rel_err, stage_tol

pytestmark = pytest.mark.gpu

CONFIGS = {"full": dict(), "embedded": dict(gru_hidden_size=32, gru_num_layers=1)}
CASES = [("cnn_gru_attention", "full"), ("cnn_gru", "full"), ("cnn_gru_attention", "embedded"), ("cnn_gru", "embedded")]
DEV = torch.device("cuda:0")
C_, K, T, TP = 6, 3, 256, 16


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "the gpu tier needs an MI355X"


def _case(B, seed):
    rs = np.random.RandomState(seed)
    x = (rs.randn(B, C_, T) * (0.5 + rs.rand(1, C_, 1)) + rs.randn(1, C_, 1)).astype(np.float32)
    y = rs.randint(0, K, size=(B,)).astype(np.int64)
    return torch.as_tensor(x), torch.as_tensor(y)


def _trained(kind, config, dropout=0.5):
    """A model whose BatchNorm running statistics are no longer the initial ones (two training steps), as
    tests/test_attribute_gpu.py's helper of the same name makes it."""
    from multimodalsignal_amd.models import CnnGruAttentionModel, CnnGruModel
    torch.manual_seed(7 + C_)
    cls = CnnGruAttentionModel if kind == "cnn_gru_attention" else CnnGruModel
    m = cls(C_, K, dropout=dropout, **CONFIGS[config]).to(DEV).train()
    opt = torch.optim.SGD(m.parameters(), lr=0.05)
    for s in range(2):
        x, y = _case(16, 50 + s)
        opt.zero_grad()
        torch.nn.CrossEntropyLoss()(m(x.to(DEV)), y.to(DEV)).backward()
        opt.step()
    return m


@functools.lru_cache(maxsize=None)
def _shared_model(kind, config, dropout=0.5):
    return _trained(kind, config, dropout).eval()


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---- 1. the replication kernel alone --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [128, 16 * 128, 301])
@pytest.mark.parametrize("N,S", [(3, 5), (1, 1), (5, 7)])
def test_expand_against_the_restatement(N, S, row):
    """row 128 and 2048: the 16-byte form (one tile, two tiles); 301: the element-wise form with a ragged tile.  Each also from
    buffers that start 4 bytes off a 16-byte boundary (the element-wise form whatever the row length)."""
    from multimodalsignal_amd import _lib as L
    GUARD = 1024
    rs = np.random.RandomState(1000 * N + 10 * S + row)
    src = rs.randn(N, row).astype(np.float32)
    want = R.expand(src, S)
    for off in (0, 1):
        sbuf = torch.zeros(N * row + 4, dtype=torch.float32, device=DEV)
        s = sbuf[off:off + N * row]
        s.copy_(torch.as_tensor(src).reshape(-1))
        dbuf = torch.full((N * S * row + GUARD + 4,), -777.0, dtype=torch.float32, device=DEV)
        d = dbuf[off:]
        assert s.data_ptr() % 16 == 4 * off and d.data_ptr() % 16 == 4 * off
        L.check(L.lib().msig_mc_expand(s.data_ptr(), d.data_ptr(), N, S, row, _stream()), "msig_mc_expand")
        torch.cuda.synchronize()
        assert np.array_equal(d[:N * S * row].cpu().numpy().reshape(N * S, row), want), off
        assert bool((d[N * S * row:] == -777.0).all()) and bool((dbuf[:off] == -777.0).all())          # the guard bands are untouched


# ---- 2. the reduction kernel alone ----------------------------------------------------------------------------------------------------
OUTS = ("mean_p", "std_p", "pred", "entropy", "expected_entropy", "mutual_info", "votes")


def _reduce(logits, N, S, K_, skip=()):
    from multimodalsignal_amd import _lib as L
    o = {}
    for name in OUTS:
        shape, dt = ((N, K_) if name in ("mean_p", "std_p", "votes") else (N,)), (torch.int32 if name in ("pred", "votes") else torch.float32)
        o[name] = None if name in skip else torch.full(shape, -77, dtype=dt, device=DEV)
    L.check(L.lib().msig_mc_reduce(logits.data_ptr(), N, S, K_, *(_ptr(o[n]) for n in OUTS), _stream()), "msig_mc_reduce")
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in o.items()}


def _reduce_logits(N, S, K_, seed):
    """Window 0: one saturated row (a logit gap of 60); window 1: an exact two-way tie for the maximum in every sample; window 2:
    all samples equal; the others generic."""
    rs = np.random.RandomState(seed)
    lg = (3.0 * rs.randn(N, S, K_)).astype(np.float32)
    lg[0, 0, :] = 0.0
    lg[0, 0, K_ - 1] = 60.0
    lg[1, :, 0] = lg[1].max(axis=1) + 1.0
    lg[1, :, 1] = lg[1, :, 0]
    lg[2, :, :] = lg[2, 0, :]
    return lg.reshape(N * S, K_)


def _assert_reduce_matches(got, ref, what=""):
    assert np.array_equal(got["votes"], ref["votes"]) and np.array_equal(got["pred"], ref["pred"]), what
    for name in ("mean_p", "std_p", "entropy", "expected_entropy", "mutual_info"):
        err = np.abs(got[name].astype(np.float64) - ref[name])
        print(f"{what} {name}: max |got - ref| {err.max():.3e}, in units of 2 ulp + 1e-12: {(err / (2 * R.ulp32(ref[name]) + 1e-12)).max():.3f}")
        assert R.within_store_rounding(got[name], ref[name]), (what, name, float(err.max()))


@pytest.mark.parametrize("K_", [2, 3, 16])
@pytest.mark.parametrize("S", [1, 2, 7, 256])
def test_reduce_against_the_restatement(S, K_):
    N = 5
    lg = _reduce_logits(N, S, K_, 100 * S + K_)
    dev = torch.as_tensor(lg).to(DEV)
    got, ref = _reduce(dev, N, S, K_), R.reduce(lg, N, S, K_)
    _assert_reduce_matches(got, ref, f"S={S} K={K_}")
    assert ref["votes"][1, 0] == S and ref["pred"][1] == 0 and got["mean_p"][1, 0] == got["mean_p"][1, 1]          # the tie: first maximum
    assert got["votes"][2].max() == S and abs(float(got["mutual_info"][2])) <= 1e-12                                   # all samples equal
    # each window reduced alone: the same bits as in the batch
    for n in range(N):
        one = _reduce(dev[n * S:(n + 1) * S].clone(), 1, S, K_)
        for name in OUTS:
            assert np.array_equal(one[name][0], got[name][n]), (n, name)
    # optional outputs left out: the others' bits are unchanged
    for skip in (("std_p", "votes"), ("pred", "entropy", "expected_entropy", "mutual_info"), OUTS[1:]):
        part = _reduce(dev, N, S, K_, skip=skip)
        for name in OUTS:
            assert (part[name] is None) if name in skip else np.array_equal(part[name], got[name]), (skip, name)


# ---- 3. the trunk = the front of an eval forward, bit for bit --------------------------------------------------------------------------
def _trunk_region(m, x, poison=True):
    """The region the trunk leaves for the tail — H0 (N, TP, 128), one layer: FEAT (N, 128) — after msig_mc_trunk, and the same
    region after an eval-mode forward of the same windows in the same workspace (poisoned before each call)."""
    from multimodalsignal_amd import _lib as L
    eng = m.engine()
    if m.embedded:
        eng.scatter()
    name, shape = ("FEAT", (x.shape[0], 128)) if m.embedded else ("H0", (x.shape[0], TP, 128))
    b = eng._batch(x, None, False, 0.0, 0, 0)
    eng.region(name, torch.float32, shape).fill_(float("nan"))
    L.check(L.lib().msig_mc_trunk(C.byref(b), L.MC_KINDS[m.kind], _stream()), "msig_mc_trunk")
    mine = eng.region(name, torch.float32, shape).clone()
    if not poison:
        return mine, None
    eng.region(name, torch.float32, shape).fill_(float("nan"))
    eng.forward(x, None, training=False)
    m._bump_token()
    return mine, eng.region(name, torch.float32, shape).clone()


@pytest.mark.parametrize("kind,config", CASES)
def test_trunk_is_the_front_of_an_eval_forward_bit_for_bit(kind, config):
    m = _shared_model(kind, config)
    x = _case(5, 31)[0].to(DEV)
    bn = m.engine().bn_state.clone(), m.engine().bn_count.clone()
    mine, full = _trunk_region(m, x)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(mine).all()) and float(mine.abs().max()) > 0 and torch.equal(mine, full)
    assert torch.equal(m.engine().bn_state, bn[0]) and torch.equal(m.engine().bn_count, bn[1])
    assert not torch.equal(bn[0][:16], torch.zeros(16, device=DEV))                  # the running statistics have moved


# ---- 4. the tail against the oracle's pieces -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tail_reference(kind, config, N, S, chunk, seed):
    """(x, reference logits in fp64 (N, S, K), own = the fp32 reference tail's disagreement with it), from the GPU trunk's own output:
    the trunk is pinned by test 3, and MaxPool near-ties stay out of this comparison."""
    from multimodalsignal_amd import uncertainty as U
    m = _shared_model(kind, config)
    x = _case(N, 400 + N)[0].to(DEV)
    src = _trunk_region(m, x, poison=False)[0].cpu().numpy()
    named = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    thr = 128
    r64, r32 = [], []
    for j, i, nb in U.chunk_plan(N, S, chunk):
        r64.append(R.tail(named, src[i:i + nb], S, seed, j, thr, torch.float64).reshape(nb, S, K))
        r32.append(R.tail(named, src[i:i + nb], S, seed, j, thr, torch.float32).reshape(nb, S, K))
    r64, r32 = np.concatenate(r64), np.concatenate(r32)
    return x, r64, rel_err(r32, r64)


@pytest.mark.parametrize("chunk", [None, 2])
@pytest.mark.parametrize("N,S", [(3, 5), (5, 7), (4, 128)])
@pytest.mark.parametrize("kind,config", CASES[:3])
def test_tail_against_the_oracle(kind, config, N, S, chunk):
    """(3, 5): 15 rows, a ragged batch tile; (5, 7): 35 rows, three tiles; (4, 128): 512 rows = 32 tiles, from where on layer 1 runs in
    its wave-specialised form (in chunks of 2 windows: 16 tiles, the projection + recurrence form); chunk None: all windows in one wide batch, chunk 2: wide
    batches of 2, 2(, 1) windows under the keys of j = 0, 1(, 2)."""
    seed = 5
    m = _shared_model(kind, config)
    x, ref, own = _tail_reference(kind, config, N, S, chunk, seed)
    p = m.predict_mc(x, samples=S, seed=seed, chunk=chunk, return_samples=True)
    torch.cuda.synchronize()
    got = p.samples.cpu().numpy()
    err, tol = rel_err(got, ref), stage_tol("logits", own)
    print(f"{kind} {config} N={N} S={S} chunk={chunk}: logits err {err:.3e} own {own:.3e} tol {tol:.3e}")
    assert got.shape == (N, S, K) and err <= tol, (err, own, tol)
    red = R.reduce(got.reshape(N * S, K), N, S, K)
    out = dict(mean_p=p.mean, std_p=p.std, pred=p.pred, entropy=p.entropy, expected_entropy=p.expected_entropy,
               mutual_info=p.mutual_information, votes=p.votes)
    _assert_reduce_matches({k: v.cpu().numpy() for k, v in out.items()}, red, "outputs")
    # the samples of a window differ: a mask shared between them could not pass
    ref_std = R.reduce(ref.reshape(N * S, K), N, S, K)["std_p"]
    assert np.all(ref_std.max(axis=1) > 0) and bool((p.std.amax(dim=1) > 0).all())
    assert all(len({got[n, s].tobytes() for s in range(S)}) > 1 for n in range(N))


# ---- 5. dropout 0 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,config", CASES[:3])
def test_without_dropout_every_sample_is_the_eval_forward(kind, config):
    """(N, S) = (5, 7): 35 rows, layer 1 in its projection + recurrence form like the eval forward of 5 windows; (4, 128): 512 rows =
    32 batch tiles, where layer 1 changes over to the wave-specialised kernel — the forms agree in every bit."""
    m = _shared_model(kind, config, 0.0)
    for N, S, chunk in ((5, 7, None), (5, 7, 2), (4, 128, None)):
        x = _case(N, 51)[0].to(DEV)
        with torch.no_grad():
            ev = m(x)
        p = m.predict_mc(x, samples=S, seed=1, chunk=chunk, return_samples=True)
        torch.cuda.synchronize()
        assert torch.equal(p.samples, ev[:, None, :].expand(N, S, K))                      # bit for bit, whatever the batching
        onehot = torch.zeros((N, K), dtype=torch.int32, device=DEV)
        onehot[torch.arange(N, device=DEV), torch.argmax(ev, dim=1)] = S
        assert torch.equal(p.votes, onehot) and torch.equal(p.pred.long(), torch.argmax(ev, dim=1))
        assert float(p.mutual_information.abs().max()) <= 1e-12 and float(p.std.max()) <= 1e-7


# ---- 6. reproducibility and isolation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["full", "embedded"])
def test_reproducible_and_without_side_effects(config):
    from multimodalsignal_amd import _lib as L
    m = _trained("cnn_gru_attention", config)
    x = _case(5, 61)[0].to(DEV)
    with torch.no_grad():
        ev = m.eval()(x)
    m.train()
    eng = m.engine()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    bn, cnt = eng.bn_state.clone(), eng.bn_count.clone()
    step, seed_, next_key = m._step, m._seed, L.dropout_key(m._seed, m._step + 1, 1)
    rng, cpu_rng = torch.cuda.get_rng_state(DEV), torch.get_rng_state()
    a = m.predict_mc(x, samples=4, seed=3, chunk=2, return_samples=True)
    b = m.predict_mc(x, samples=4, seed=3, chunk=2, return_samples=True)
    c = m.predict_mc(x, samples=4, seed=4, chunk=2, return_samples=True)
    d = m.predict_mc(x, samples=4, seed=3, chunk=5, return_samples=True)
    torch.cuda.synchronize()
    for name in ("mean", "std", "pred", "entropy", "expected_entropy", "mutual_information", "votes", "samples"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert not torch.equal(a.samples, c.samples)                                           # another seed: other masks
    assert torch.equal(a.samples[:2], d.samples[:2]) and not torch.equal(a.samples[2:], d.samples[2:])      # the chunk is part of the result
    after = m.state_dict()
    assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert torch.equal(eng.bn_state, bn) and torch.equal(eng.bn_count, cnt)
    assert all(int(after[f"cnn_encoder.{i}.num_batches_tracked"]) == 2 for i in (1, 5))
    assert m.training is True and m._step == step and m._seed == seed_ and L.dropout_key(m._seed, m._step + 1, 1) == next_key
    assert torch.equal(torch.cuda.get_rng_state(DEV), rng) and torch.equal(torch.get_rng_state(), cpu_rng)
    with torch.no_grad():
        assert torch.equal(m.eval()(x), ev)                                                # a following eval forward: the bits it had


# ---- 7. the driver ----------------------------------------------------------------------------------------------------------------------
def test_driver_mc_dropout_after_loso(tmp_path, capsys):
    """Three subjects: the smallest LOSO the command line runs (a fold needs a training and a validation subject beside its test
    subject), two epochs.  cv_summary.txt is compared without its wall-clock line, the checkpoints tensor by tensor."""
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd import uncertainty as U
    from multimodalsignal_amd.synth import make_synthetic_wesad
    subs = ["S2", "S3", "S4"]
    d = make_synthetic_wesad(tmp_path / "w", subjects=subs, windows_per_subject=12, T=256, difficulty=2.0)
    common = ["--synthetic", str(d), "--samples", "256", "--subjects", *subs, "--epochs", "2", "--batch-size", "16"]
    M.main(common + ["--mc-dropout", "4", "--out", str(tmp_path / "mc")])
    M.main(common + ["--out", str(tmp_path / "plain")])
    runs = {k: sorted((tmp_path / k).glob("simple_binary/run_*"))[0] for k in ("mc", "plain")}
    cut = lambda text: text[:text.index("LOSO wall-clock")]
    assert cut((runs["mc"] / "cv_summary.txt").read_text(encoding="utf-8")) == cut((runs["plain"] / "cv_summary.txt").read_text(encoding="utf-8"))
    for s in subs:
        ck = [torch.load(runs[k] / f"fold_test_on_{s}" / "best_model.pt", map_location="cpu") for k in ("mc", "plain")]
        assert set(ck[0]) == set(ck[1]) and all(torch.equal(ck[0][k], ck[1][k]) for k in ck[0]), s
    assert sorted(p.name for p in runs["plain"].iterdir()) == sorted(p.name for p in runs["mc"].iterdir() if not p.name.startswith("uncertainty"))
    assert not (runs["plain"] / "uncertainty.json").exists() and not (runs["plain"] / "fold_test_on_S2" / "uncertainty_result.json").exists()
    doc = json.loads((runs["mc"] / "uncertainty.json").read_text())
    assert [f["subject"] for f in doc["folds"]] == subs and doc["n_folds"] == 3 and doc["note"] == U.SYNTHETIC_NOTE
    assert doc["settings"] == {"samples": 4, "seed": 0, "dropout": 0.5}
    keys = {"n", "accuracy_eval", "accuracy_mc", "entropy_correct", "entropy_wrong", "mutual_information_correct", "mutual_information_wrong",
            "auroc_entropy", "selective_accuracy", "ece_eval", "ece_mc"}
    assert set(doc["pooled"]) == keys and doc["pooled"]["n"] == 36
    for s, fold in zip(subs, doc["folds"]):
        per = json.loads((runs["mc"] / f"fold_test_on_{s}" / "uncertainty_result.json").read_text())
        assert {k: v for k, v in per.items() if k != "windows"} == fold and keys <= set(fold)
        assert per["subject"] == s and per["n"] == 12 and per["samples"] == 4 and per["seed"] == 0 and per["chunk"] == 512
        assert set(per["selective_accuracy"]) == {"100", "90", "80", "50"} and per["selective_accuracy"]["100"] == per["accuracy_mc"]
        assert all(len(per["windows"][k]) == 12 for k in U.WINDOW_KEYS) and all(h >= 0 for h in per["windows"]["entropy"])
        assert 0.0 <= per["ece_eval"] <= 1.0 and 0.0 <= per["ece_mc"] <= 1.0
        assert per["auroc_entropy"] is None or 0.0 <= per["auroc_entropy"] <= 1.0
    txt = (runs["mc"] / "uncertainty.txt").read_text(encoding="utf-8")
    assert U.SYNTHETIC_NOTE in txt and all(s in txt for s in subs) and "pooled" in txt
    assert "Monte-Carlo dropout over 12 windows, 4 samples" in capsys.readouterr().out
