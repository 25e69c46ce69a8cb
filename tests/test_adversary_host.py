"""Subject-adversarial training (include/msig_da.h), host tier: tests/da_reference.py pinned to torch's autograd through a
gradient-reversal Function and torch.optim.Adam in float64; the lambda schedule, the domain-table builder, the discriminator's
initialisation, the command line and the batch-size limit."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import da_reference as R
from multimodalsignal_amd import adversary as A
from multimodalsignal_amd import main as M


class _Reverse(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, lam):
        ctx.lam = lam
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return -ctx.lam * g, None


def _labels(B, S, seed, unlabelled=0.2):
    rs = np.random.RandomState(seed)
    d = rs.randint(0, S, size=B)
    d[rs.rand(B) < unlabelled] = -1
    return d.astype(np.int64)


def _torch_run(flat0, S, feats, dfeats, ds, lam, lam_rev, lr, wd):
    """The same steps with torch: D as leaves of the flat layout's tensors, L_dom in the two-label form, Adam(weight_decay=wd)."""
    P = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in R.split(flat0, S).items()}
    opt = torch.optim.Adam([P[k] for k in R.KEYS], lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    out = []
    for f_np, df_np, d_np in zip(feats, dfeats, ds):
        f = torch.tensor(f_np, dtype=torch.float64, requires_grad=True)
        d = torch.tensor(d_np)
        n = lam * float((d >= 0).sum()) + (1.0 - lam) * float((d.flip(0) >= 0).sum())
        if n == 0.0:
            out.append(dict(loss=0.0, dfeat=df_np.copy()))
            continue
        z = F.linear(torch.relu(F.linear(_Reverse.apply(f, lam_rev), P["W0"], P["b0"])), P["W3"], P["b3"])
        loss = (lam * F.cross_entropy(z, d, ignore_index=-1, reduction="sum")
                + (1.0 - lam) * F.cross_entropy(z, d.flip(0), ignore_index=-1, reduction="sum")) / n
        opt.zero_grad()
        loss.backward()
        opt.step()
        out.append(dict(loss=float(loss.detach()), dfeat=df_np + f.grad.numpy()))
    state = {k: opt.state[P[k]] for k in R.KEYS if P[k] in opt.state}
    return P, state, out


@pytest.mark.parametrize("lam", [1.0, 0.3])
@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("B", [1, 5, 21])
@pytest.mark.parametrize("S", [2, 11, 16])
def test_restatement_equals_torch_autograd_and_adam(S, B, steps, lam):
    rs = np.random.RandomState(100 * S + B)
    flat0 = A.SubjectAdversary.initial_parameters(S, seed=S + B).double().numpy()
    feats = [rs.randn(B, 128) for _ in range(steps)]
    dfeats = [rs.randn(B, 128) for _ in range(steps)]
    ds = [_labels(B, S, 7 * s + B) for s in range(steps)]
    if B > 1:
        ds[0][0] = 0                                                # at least one labelled row in the first step
    lam_rev, lr, wd = 0.7, 1e-2, 1e-3
    P = R.split(flat0, S)
    Mo, Vo = R.zeros_like(P), R.zeros_like(P)
    mine = []
    for t, (f, df, d) in enumerate(zip(feats, dfeats, ds), 1):
        # torch's Adam counts only the steps it took: a batch without a labelled row is no step of either
        r = R.step(P, Mo, Vo, f, df, d, lam=lam, lam_rev=lam_rev, lr=lr, t=1 + sum(1 for m in mine if m["n"] > 0), weight_decay=wd)
        P, Mo, Vo = r["params"], r["exp_avg"], r["exp_avg_sq"]
        mine.append(r)
    Pt, state, theirs = _torch_run(flat0, S, feats, dfeats, ds, lam, lam_rev, lr, wd)
    for r, w in zip(mine, theirs):
        assert abs(r["loss"] - w["loss"]) <= 1e-12 * max(1.0, abs(w["loss"]))
        assert np.abs(r["dfeat"] - w["dfeat"]).max() <= 1e-12 * max(1.0, np.abs(w["dfeat"]).max())
    for k in R.KEYS:
        assert np.abs(P[k] - Pt[k].detach().numpy()).max() <= 1e-12, k
        if k in state:
            assert np.abs(Mo[k] - state[k]["exp_avg"].numpy()).max() <= 1e-12, k
            assert np.abs(Vo[k] - state[k]["exp_avg_sq"].numpy()).max() <= 1e-12, k


def test_restatement_without_a_labelled_row_changes_nothing_and_counts_nothing():
    S, B = 4, 6
    P = R.split(A.SubjectAdversary.initial_parameters(S, 1).numpy(), S)
    Z = R.zeros_like(P)
    rs = np.random.RandomState(0)
    f, df = rs.randn(B, 128), rs.randn(B, 128)
    r = R.step(P, Z, Z, f, df, np.full(B, -1), lam=0.3, lam_rev=0.5, dtype=np.float32)
    assert r["n"] == 0.0 and not r["stats"].any() and np.array_equal(r["dfeat"], df.astype(np.float32))
    for k in R.KEYS:
        assert np.array_equal(r["params"][k], P[k].astype(np.float32))


def test_restatement_statistics_and_clamped_labels():
    S, B = 3, 9
    P = R.split(A.SubjectAdversary.initial_parameters(S, 2).numpy(), S)
    Z = R.zeros_like(P)
    rs = np.random.RandomState(1)
    dom = np.array([0, 1, 2, -1, 7, -5, 2, 1, 0], dtype=np.int32)       # 7 and -5 are outside [-1, S): read as -1
    d = R.labels(dom, None, S)
    assert d.tolist() == [0, 1, 2, -1, -1, -1, 2, 1, 0]
    assert R.labels(dom, np.array([8, 4, 2]), S).tolist() == [0, -1, 2]
    r = R.step(P, Z, Z, rs.randn(B, 128), np.zeros((B, 128)), d, lam=0.4)
    assert r["stats"][2] == 6 and 0 <= r["stats"][1] <= 6
    assert abs(r["n"] - 6.0) < 1e-6                                   # the flip is a permutation: n = labelled rows, whatever lam
    assert abs(r["stats"][0] - r["n"] * r["loss"]) <= 1e-12 * r["stats"][0]
    assert not r["dfeat"].any()                                       # lam_rev = 0: dfeat untouched


def test_lambda_schedule():
    a = A.SubjectAdversary(4, lam=0.5, schedule="ganin", gamma=10.0)
    total = 200
    v = [a.lam_at(s, total) for s in range(1, total + 1)]
    assert v[0] == 0.0
    assert all(v[i] < v[i + 1] for i in range(len(v) - 1))
    assert 0.49 < v[-1] < 0.5
    assert abs(a.lam_at(101, total) - 0.5 * (2.0 / (1.0 + math.exp(-5.0)) - 1.0)) < 1e-15
    c = A.SubjectAdversary(4, lam=0.5, schedule="constant")
    assert [c.lam_at(s, total) for s in (1, 50, 200)] == [0.5] * 3
    assert A.SubjectAdversary(4, lam=0.0).lam_at(77, 100) == 0.0
    with pytest.raises(ValueError):
        A.SubjectAdversary(4, schedule="linear")
    with pytest.raises(ValueError):
        A.SubjectAdversary(4, lam=-0.1)
    for S in (1, 17):
        with pytest.raises(ValueError):
            A.SubjectAdversary(S)


class _View:
    """A StoreView's fields as domain_table reads them."""
    def __init__(self, n_store, index, ordinals):
        self.store = type("S", (), {"x": np.zeros((n_store, 1, 1))})()
        self.index_host, self.subject_ordinals = np.asarray(index), np.asarray(ordinals, dtype=np.int32)


def test_domain_table():
    # a store of three subjects at [0, 4), [4, 6), [6, 9); the fold trains on the third and the first, in that order
    view = _View(9, [6, 7, 8, 0, 1, 2, 3], A.subject_ordinals([3, 4]))
    t = A.domain_table(view)
    assert t.dtype == np.int32 and t.tolist() == [1, 1, 1, 1, -1, -1, 0, 0, 0]
    own = type("D", (), {"subject_ordinals": A.subject_ordinals([2, 0, 3])})()      # a WesadDataset: its own store, an empty subject
    assert A.domain_table(own).tolist() == [0, 0, 2, 2, 2]


def test_initialisation_is_deterministic_and_leaves_the_global_rng_alone():
    torch.manual_seed(5)
    before = torch.get_rng_state().clone()
    a = A.SubjectAdversary.initial_parameters(11, seed=3)
    assert torch.equal(torch.get_rng_state(), before)
    torch.manual_seed(99)
    b = A.SubjectAdversary.initial_parameters(11, seed=3)
    assert torch.equal(a, b) and not torch.equal(a, A.SubjectAdversary.initial_parameters(11, seed=4))
    lay = A.flat_layout(11)
    assert lay == R.layout(11) and a.numel() == lay[-1] == 8192 + 64 + 704 + 12
    assert float(a[:8256].abs().max()) <= 1.0 / math.sqrt(128) and float(a[8256:8256 + 704 + 11].abs().max()) <= 1.0 / math.sqrt(64)
    assert float(a[:8192].std()) > 0.04 and float(a[-1]) == 0.0                         # uniform, and the padding stays zero


def test_state_dict_round_trip():
    a, b = A.SubjectAdversary(5, seed=1), A.SubjectAdversary(5, seed=2)
    a.step = 17
    a.exp_avg.fill_(0.25)
    b.load_state_dict(a.state_dict())
    assert torch.equal(a.params, b.params) and torch.equal(a.exp_avg, b.exp_avg) and b.step == 17
    with pytest.raises(ValueError):
        A.SubjectAdversary(6).load_state_dict(a.state_dict())


def _cfg(argv):
    ap = M.build_parser()
    return M.build_cfg(M.parse_args(ap, argv), ["cnn_gru_attention"])


def test_command_line_and_config():
    assert "adversary" not in _cfg([]) and "adversary" not in M.trainer_config(_cfg([]), 0)
    c = _cfg(["--subject-adversarial"])
    assert c["adversary"] == dict(lam=0.1, schedule="ganin", gamma=10.0, lr_mult=1.0, seed=None)
    assert M.trainer_config(c, 0)["adversary"] == c["adversary"]
    c = _cfg(["--subject-adversarial", "0", "--adversary-schedule", "constant", "--adversary-lr-mult", "2.5"])
    assert (c["adversary"]["lam"], c["adversary"]["schedule"], c["adversary"]["lr_mult"]) == (0.0, "constant", 2.5)
    assert "lambda=0 " in M.adversary_line(c) and M.adversary_line(_cfg([])) is None
    for bad in (["--adversary-schedule", "constant"], ["--adversary-lr-mult", "2"], ["--subject-adversarial", "-1"],
                ["--subject-adversarial", "nan"], ["--subject-adversarial", "0.1", "--adversary-schedule", "linear"]):
        with pytest.raises(SystemExit):
            _cfg(bad)
    assert A.settings(None) is None
    for bad in ("0.1", dict(lam="0.1"), dict(lambda_=0.1), dict(schedule="x"), dict(lr_mult=float("inf"))):
        with pytest.raises(ValueError):
            A.settings(bad)


def test_batch_sizes_above_256_are_refused_before_training():
    _cfg(["--subject-adversarial", "--batch-size", "256"])
    with pytest.raises(ValueError, match="at most 256"):
        _cfg(["--subject-adversarial", "0", "--batch-size", "257"])
    assert _cfg(["--batch-size", "4096"])["batch_size"] == 4096          # without the flag nothing is refused


def test_fold_record_and_report(tmp_path):
    hist = [dict(epoch=1, domain_acc=0.30, domain_loss=1.4, adversary_lambda=0.0), dict(epoch=2, domain_acc=0.26, domain_loss=1.39, adversary_lambda=0.05)]
    rec = A.fold_record(dict(subject="S2", accuracy=0.9, history=hist, adversary_domains=4))
    assert rec["chance"] == 0.25 and rec["first_domain_acc"] == 0.30 and rec["last_domain_acc"] == 0.26 and rec["final_lambda"] == 0.05
    assert A.fold_record(dict(subject="S2", history=[dict(epoch=1)])) is None
    path = A.write_adversary(tmp_path, [rec], A.settings(dict(lam=0.0)), synthetic=True)
    import json
    doc = json.loads((tmp_path / "adversary.json").read_text())
    assert doc["probe"] is True and doc["folds"][0]["S"] == 4 and abs(doc["pooled"]["test_accuracy"] - 0.9) < 1e-12
    text = path.read_text()
    assert "probe" in text and "no subject shift" in text and "S2" in text
