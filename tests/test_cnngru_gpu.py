"""The cnn_gru baseline on the MI355X (include/msig_cg.h, models.CnnGruModel).

C <= 3: the attention model's gate is exactly 0.5 (sigmoidf_fast(0) = rcp(1 + exp(0)) is exact) and every scaling by it is a power of
two, so the baseline on x equals the attention model on 2x in every bit — forward, backward (dx_cg(x) = 2 dx_attn(2x)), fused steps
and fold batches.  C >= 4: the fp64 oracle with its gate patched to s = 1 (the oracle itself is not edited).  Then fold
independence, the launches the baseline saves, and the comparison driver."""
import ctypes as C
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_common import grad_tol, rel_err, split_named, stage_tol, to_t
from oracle import cnn_gru_oracle as O
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd.models import CnnGruAttentionModel, CnnGruModel
from multimodalsignal_amd.runtime import Engine, FoldArena

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CONFIGS = {"full": dict(), "embedded": dict(gru_hidden_size=32, gru_num_layers=1)}
LR, WD, P = 1e-3, 1e-4, 0.5


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _x(B, C_, T, seed):
    """Inputs away from the subnormal range: |x| >= 1e-3."""
    rs = np.random.RandomState(seed)
    x = (rs.randn(B, C_, T) * (0.5 + rs.rand(1, C_, 1)) + rs.randn(1, C_, 1)).astype(np.float32)
    x = np.where(np.abs(x) < 1e-3, np.float32(1e-3), x)
    y = rs.randint(0, 3, size=(B,)).astype(np.int64)
    return torch.as_tensor(x, device=DEV), torch.as_tensor(y, device=DEV)


def _pair(C_, config, seed=5):
    """An attention model and a baseline with the same non-gate weights and the same dropout seed."""
    torch.manual_seed(seed)
    att = CnnGruAttentionModel(C_, 3, **CONFIGS[config]).to(DEV)
    cg = CnnGruModel(C_, 3, **CONFIGS[config]).to(DEV)
    cg.load_state_dict({k: v for k, v in att.state_dict().items() if k not in L.GATE_KEYS})
    with torch.no_grad():                        # running statistics away from the initial (0, 1), for the eval-mode forward
        for m in (att, cg):
            for i, ch in ((1, 16), (5, 32)):
                g = torch.Generator().manual_seed(i)
                m.cnn_encoder[i].running_mean.copy_(torch.rand(ch, generator=g) - 0.5)
                m.cnn_encoder[i].running_var.copy_(0.5 + torch.rand(ch, generator=g))
    att.set_dropout_seed(77)
    cg.set_dropout_seed(77)
    return att, cg


def _grads_and_dx(model, x, y):
    xl = x.clone().requires_grad_(True)
    for p in model.parameters():
        p.grad = None
    logits = model(xl)
    loss = F.cross_entropy(logits, y)
    loss.backward()
    return logits.detach(), loss.detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}, xl.grad


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("C_", [1, 2, 3])
def test_bit_identity_with_attention_on_2x_forward_backward(C_, config):
    att, cg = _pair(C_, config)
    x, y = _x(64, C_, 640, seed=C_)
    for mode in ("train", "eval"):
        for m in (att, cg):
            m.train(mode == "train")
        la, lossa, ga, dxa = _grads_and_dx(att, 2 * x, y)
        lc, lossc, gc, dxc = _grads_and_dx(cg, x, y)
        torch.cuda.synchronize()
        assert torch.equal(_bits(la), _bits(lc)), mode
        assert torch.equal(_bits(lossa), _bits(lossc)), mode
        for k, v in cg.state_dict().items():
            assert torch.equal(_bits(att.state_dict()[k]), _bits(v)), (mode, k)          # BN running statistics and the weights
        assert sorted(gc) == sorted(k for k in ga if k not in L.GATE_KEYS)
        for k in gc:
            assert torch.equal(_bits(ga[k]), _bits(gc[k])), (mode, k)
        assert torch.equal(dxc, 2 * dxa), mode
        assert dxc.abs().max() > 0


def _engines(C_, config, seed=5):
    att, cg = _pair(C_, config, seed)
    return att.engine(), cg.engine()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("C_", [1, 2, 3])
def test_bit_identity_fused_train_steps(C_, config, weighted):
    ea, ec = _engines(C_, config)
    assert ea.layout == ec.layout                                 # C < 4: the two layouts are the same
    cw = torch.tensor([0.5, 2.0, 1.25], device=DEV) if weighted else None
    for s in (1, 2, 3):
        x, y = _x(64, C_, 512, seed=10 + s)
        ea.train_step(2 * x, y, LR, weight_decay=WD, step=s, dropout_p=P, seed=9, class_weight=cw)
        ec.train_step(x, y, LR, weight_decay=WD, step=s, dropout_p=P, seed=9, class_weight=cw)
        torch.cuda.synchronize()
        assert torch.equal(_bits(ea.region("LOSS", torch.float32, (4,))), _bits(ec.region("LOSS", torch.float32, (4,)))), s
    for name in ("params", "grads", "exp_avg", "exp_avg_sq", "bn_state", "bn_count", "loss_acc"):
        assert torch.equal(_bits(getattr(ea, name)), _bits(getattr(ec, name))), name


def _arena_run(kind, n, B, T, C_, config, data, cw=None, steps=3, scale=1.0, seed=5):
    """n folds of one kind in one FoldArena: `steps` fused multi steps, then one evaluation pass."""
    hidden, layers = (32, 1) if config == "embedded" else (64, 2)
    arena = FoldArena(C_, 3, DEV, n, B, T, gru_hidden=hidden, gru_layers=layers, kind=kind)
    for f in range(n):
        att, cg = _pair(C_, config, seed + f)
        model = att if kind == "cnn_gru_attention" else cg
        model._engine = arena.engine(f)
        model.engine()
        if layers == 1:
            model._engine.scatter()
        if cw is not None:
            arena.set_class_weight(f, cw[f])
    lib = L.lib()
    train = lib.msig_cg_train_step_multi if kind == "cnn_gru" else lib.msig_cw_train_step_multi
    fwd = lib.msig_cg_forward_multi if kind == "cnn_gru" else lib.msig_cw_forward_multi
    cwp = arena.ptr("cw") if cw is not None else None
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    for s in range(1, steps + 1):
        for f in range(n):
            x, y = data[f][s - 1]
            arena.view(f, "x", torch.float32)[:x.numel()].copy_((scale * x).reshape(-1))
            arena.view(f, "y", torch.int64)[:B].copy_(y)
        m = arena.multi(list(range(n)), key_gru=[L.dropout_key(100 + f, s, 1) for f in range(n)],
                        key_head=[L.dropout_key(100 + f, s, 2) for f in range(n)], lr=[LR] * n, steps=[s] * n)
        L.check(train(C.byref(arena.batch(B, True, P)), C.byref(m), cwp, arena.ptr("exp_avg"), arena.ptr("exp_avg_sq"), 0.9, 0.999, 1e-8,
                      WD, s, st), "train_step_multi")
    L.check(fwd(C.byref(arena.batch(B, False, 0.0)), C.byref(arena.multi(list(range(n)))), cwp, st), "forward_multi")
    torch.cuda.synchronize()
    return arena


def _fold_data(n, B, C_, T, steps=3):
    return [[_x(B, C_, T, seed=1000 * f + s) for s in range(steps)] for f in range(n)]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_bit_identity_fold_batch(config, weighted):
    n, B, T, C_ = 3, 64, 512, 2
    data = _fold_data(n, B, C_, T)
    cw = [(0.5, 2.0, 1.0), (1.0, 1.0, 1.0), (3.0, 0.25, 1.0)] if weighted else None
    a = _arena_run("cnn_gru_attention", n, B, T, C_, config, data, cw, scale=2.0)
    c = _arena_run("cnn_gru", n, B, T, C_, config, data, cw)
    assert a.off == c.off and a.stride == c.stride
    for name in ("params", "grads", "exp_avg", "exp_avg_sq", "bn_state", "bn_count", "acc"):
        o, nb = a.off[name]
        assert torch.equal(a.mem[:, o:o + nb], c.mem[:, o:o + nb]), name
    off = L.workspace_layout(B, C_, T, 3, False)
    for region in ("LOGITS", "PRED"):
        o0, o1 = a.off["ws"][0] + off[L.WS[region]], a.off["ws"][0] + off[L.WS[region] + 1]
        assert torch.equal(a.mem[:, o0:o1], c.mem[:, o0:o1]), region


# ---- C >= 4: the fp64 oracle with s = 1 ---------------------------------------------------------------------------------------
def _hip_pool_choice(eng, st64, B, T):
    """MaxPool near-ties (two candidates equal to within fp32 resolution): the oracle adopts the HIP path's decision, recomputed
    from ITS conv outputs and BatchNorm constants — only there (gpu_common.run_case's rule; everywhere else the oracle's own
    argmax stands)."""
    L1, _, L2, _ = O.stage_lengths(T)
    choice, n = {}, 0
    for stage, yname, sname, CH, Lc in (("pool1", "Y1", "BN1_STAT", 16, L1), ("pool2", "Y2", "BN2_STAT", 32, L2)):
        yh = eng.region(yname, torch.float32, (B, Lc, CH)).cpu().double().permute(0, 2, 1)
        stt = eng.region(sname, torch.float32, (4, CH)).cpu().double()
        zh = (yh * stt[2][None, :, None] + stt[3][None, :, None]).float()
        ch_hip = O.first_argmax(O.pool_windows(torch.clamp_min(zh, 0)))
        win = O.pool_windows(torch.clamp_min(st64["bn" + stage[-1]].detach(), 0))
        ch_ref = O.first_argmax(win)
        top = win.max(dim=3).values
        hip_val = win.gather(3, ch_hip.to(torch.int64)[..., None]).squeeze(3)
        near = (ch_hip != ch_ref) & ((top - hip_val) <= 4e-6 * torch.clamp_min(top.abs(), 1e-3))
        n += int(near.sum())
        choice[stage] = torch.where(near, ch_hip, ch_ref)
    assert n <= 8, f"{n} adopted pooling decisions"
    return choice if n else None


def _oracle(named, x, y, dtype, training, fw, loss_fn=None, pool_choice=None):
    """(dL/dx, {param: dL/dparam}, stages) of the oracle with x as a leaf."""
    p, b = split_named(to_t(named, dtype))
    leaf = {k: v.detach().clone().requires_grad_(v.numel() > 0) for k, v in p.items()}
    xl = x.to(dtype).clone().requires_grad_(True)
    st, _ = O.forward(leaf, b, xl, training=training, pool_choice=pool_choice, **fw)
    loss = O.cross_entropy(st["logits"], y) if loss_fn is None else loss_fn(st["logits"])
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items()}
    return xl.grad.detach(), grads, st


@pytest.fixture
def no_gate(monkeypatch):
    """The oracle's ChannelAttention replaced by the identity (s = 1): the baseline's reference, without editing oracle/."""
    def gate(x, W1, W2):
        B, C_, _ = x.shape
        return x.mean(dim=2), torch.zeros(B, 0, dtype=x.dtype), torch.ones(B, C_, dtype=x.dtype)
    monkeypatch.setattr(O, "channel_gate", gate)


def _named(model):
    """The model's parameters and buffers plus zero-size gate tensors (the oracle's forward reads the keys)."""
    named = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    C_ = model.in_channels
    named["channel_attention.fc.0.weight"] = torch.zeros(0, C_)
    named["channel_attention.fc.2.weight"] = torch.zeros(C_, 0)
    return named


@pytest.mark.parametrize("C_,T,config", [(6, 3840, "full"), (6, 3840, "embedded"), (12, 1000, "full"), (5, 1002, "full"),
                                         (12, 1001, "embedded")])
def test_against_fp64_oracle(no_gate, C_, T, config):
    torch.manual_seed(C_ + T)
    model = CnnGruModel(C_, 3, **CONFIGS[config]).to(DEV)
    model.set_dropout_seed(31)
    x, y = _x(64, C_, T, seed=T)
    named = _named(model)                                      # before the step: the weights and running statistics it starts from
    model.train()
    logits, loss, grads, dx = _grads_and_dx(model, x, y)
    torch.cuda.synchronize()
    fw = dict(dropout_p=0.5, seed=model._seed, step=model._step)
    xc, yc = x.cpu(), y.cpu()
    dx64, g64, st64 = _oracle(named, xc, yc, torch.float64, True, fw)
    choice = _hip_pool_choice(model._engine, st64, 64, T)
    if choice is not None:
        dx64, g64, st64 = _oracle(named, xc, yc, torch.float64, True, fw, pool_choice=choice)
    dx32, g32, st32 = _oracle(named, xc, yc, torch.float32, True, fw, pool_choice=choice)
    eng = model._engine
    L1, P1, L2, TP = O.stage_lengths(T)
    stages = {"conv1": eng.region("Y1", torch.float32, (64, L1, 16)).cpu().permute(0, 2, 1),
              "pool1": eng.region("P1", torch.float32, (64, P1, 16)).cpu().permute(0, 2, 1),
              "pool2": eng.region("P2", torch.float32, (64, TP, 32)).cpu().permute(0, 2, 1),
              "feat": eng.region("FEAT", torch.float32, (64, 128)).cpu(), "logits": logits.cpu()}
    for k, got in stages.items():
        if k == "feat" and config == "embedded":
            got = torch.cat([got[:, :32], got[:, 64:96]], dim=1)
        ref, own = st64[k].detach().numpy(), rel_err(st32[k].detach().numpy(), st64[k].detach().numpy())
        assert rel_err(got.numpy(), ref) <= stage_tol(k, own), (k, rel_err(got.numpy(), ref), own)
    loss64 = float(O.cross_entropy(st64["logits"].detach(), yc))
    assert abs(float(loss) - loss64) <= 2e-6 * max(abs(loss64), 1e-6)
    assert sorted(grads) == sorted(k for k in g64 if k not in L.GATE_KEYS)
    for k, g in grads.items():
        ref = g64[k].numpy()
        own = rel_err(g32[k].numpy(), ref)
        assert rel_err(g.cpu().numpy(), ref) <= grad_tol(k, own), (k, rel_err(g.cpu().numpy(), ref), own)
    own = rel_err(dx32.numpy(), dx64.numpy())
    assert rel_err(dx.cpu().numpy(), dx64.numpy()) <= grad_tol("x", own), ("dx", own)


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_autograd_input_gradient(no_gate, mode):
    """torch.autograd.grad(model(x)[:, 1].sum(), x) through CnnGruModel, after model.train() and model.eval()."""
    C_, T = 6, 1024
    torch.manual_seed(4)
    model = CnnGruModel(C_, 3).to(DEV)
    model.set_dropout_seed(8)
    model.train(mode == "train")
    x, y = _x(32, C_, T, seed=3)
    named = _named(model)
    xl = x.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(model(xl)[:, 1].sum(), xl)
    torch.cuda.synchronize()
    fw = dict(dropout_p=0.5, seed=model._seed, step=model._step) if mode == "train" else {}
    loss_fn = lambda lg: lg[:, 1].sum()
    dx64, _, st64 = _oracle(named, x.cpu(), y.cpu(), torch.float64, mode == "train", fw, loss_fn)
    choice = _hip_pool_choice(model._engine, st64, 32, T)
    if choice is not None:
        dx64, _, _ = _oracle(named, x.cpu(), y.cpu(), torch.float64, mode == "train", fw, loss_fn, choice)
    dx32, _, _ = _oracle(named, x.cpu(), y.cpu(), torch.float32, mode == "train", fw, loss_fn, choice)
    own = rel_err(dx32.numpy(), dx64.numpy())
    assert rel_err(g.cpu().numpy(), dx64.numpy()) <= grad_tol("x", own)


# ---- fold independence, launches ------------------------------------------------------------------------------------------------
def test_fold_batch_equals_single_model_steps():
    n, B, T, C_ = 4, 64, 512, 6
    data = _fold_data(n, B, C_, T)
    arena = _arena_run("cnn_gru", n, B, T, C_, "full", data)
    for f in range(n):
        _, cg = _pair(C_, "full", 5 + f)
        e = cg.engine()
        for s in (1, 2, 3):
            x, y = data[f][s - 1]
            e.train_step(x, y, LR, weight_decay=WD, step=s, dropout_p=P, seed=100 + f)      # the same dropout keys as the arena's
        torch.cuda.synchronize()
        for name in ("params", "exp_avg", "exp_avg_sq", "bn_state"):
            o, nb = arena.off[name]
            got = arena.mem[f, o:o + nb].view(torch.float32)[:getattr(e, name).numel()]
            assert torch.equal(_bits(got), _bits(getattr(e, name))), (f, name)


def _launches(fn):
    torch.cuda.synchronize()
    L.profile_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        return L.profile_report()
    finally:
        L.profile_enable(False)


def test_launches_saved():
    C_, B, T = 6, 64, 3840
    x, y = _x(B, C_, T, seed=1)
    ec, ea = Engine(C_, 3, DEV, kind="cnn_gru"), Engine(C_, 3, DEV)
    ev_c = _launches(lambda: ec.forward(x, y, training=False))
    ev_a = _launches(lambda: ea.forward(x, y, training=False))
    assert "gate" not in ev_c and "gate_eo" not in ev_c and "gate" in ev_a
    assert sum(c for c, _ in ev_c.values()) == sum(c for c, _ in ev_a.values()) - 1          # one launch fewer per eval batch
    keep = _launches(lambda: ec.forward(x, y, training=False, keep_for_backward=True))
    assert keep.get("gate_eo", (0,))[0] == 1 and "gate" not in keep
    st_c = _launches(lambda: ec.train_step(x, y, LR, step=1, dropout_p=P, seed=1))
    st_a = _launches(lambda: ea.train_step(x, y, LR, step=1, dropout_p=P, seed=1))
    assert "gate_bwd" not in st_c and "gate" not in st_c and st_c["gate_eo"][0] == 1
    assert "gate_bwd" in st_a
    assert sum(c for c, _ in st_c.values()) == sum(c for c, _ in st_a.values()) - 1


# ---- the comparison driver ------------------------------------------------------------------------------------------------------
def _fold_results(run, subs):
    out = {}
    for s in subs:
        info = json.loads((run / f"fold_test_on_{s}" / "fold_result.json").read_text())
        hist = [{k: v for k, v in h.items() if k != "seconds"} for h in info["history"]]          # wall time is not a result
        out[s] = (info["accuracy"], info["f1_score"], info["epochs"], hist)
    return out


def test_comparison_driver(tmp_path):
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.synth import make_synthetic_wesad
    subs = ["S2", "S3", "S4", "S5"]
    d = make_synthetic_wesad(tmp_path / "w", subjects=subs, windows_per_subject=30, T=256, difficulty=2.0, window_spread=3)
    common = ["--synthetic", str(d), "--samples", "256", "--subjects", *subs, "--epochs", "3", "--patience", "1", "2", "--batch-size", "16"]
    M.main(common + ["--model", "cnn_gru_attention", "cnn_gru", "--out", str(tmp_path / "both")])
    M.main(common + ["--model", "cnn_gru_attention", "--out", str(tmp_path / "one")])
    (both,) = sorted((tmp_path / "both").glob("simple_binary/run_*"))
    (one,) = sorted((tmp_path / "one").glob("simple_binary/run_*"))
    for kind in ("cnn_gru_attention", "cnn_gru"):
        text = (both / kind / "cv_summary.txt").read_text(encoding="utf-8")
        assert f"MODEL_TO_USE: {kind}\n" in text and f"MODEL_PARAMS: {{'{kind}': {{" in text
    assert "MODEL_TO_USE: cnn_gru_attention\n" in (one / "cv_summary.txt").read_text(encoding="utf-8")
    assert _fold_results(both / "cnn_gru_attention", subs) == _fold_results(one, subs)       # the kinds do not interact
    cmp = json.loads((both / "comparison.json").read_text())
    st = cmp["sets"][""]
    assert st["n_folds"] == 4 and st["gate_hidden_width"] == 6 // 4
    cg = _fold_results(both / "cnn_gru", subs)
    for f in st["folds"]:
        assert f["cnn_gru"]["accuracy"] == pytest.approx(cg[f["subject"]][0])
    assert "cnn_gru_attention wins" in (both / "comparison.txt").read_text(encoding="utf-8")


def test_hierarchical_baseline(tmp_path):
    """--hierarchical --model cnn_gru: M1 and M2 are baselines (no gate in their checkpoints), the fold-batched driver gives the
    sequential driver's results, and hierarchical_summary.txt names the kind."""
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.synth import make_synthetic_wesad
    subs = ["S2", "S3", "S4", "S5"]
    d = make_synthetic_wesad(tmp_path / "w", subjects=subs, windows_per_subject=40, T=256, difficulty=2.0)
    names = (d / "_channel_names.txt").read_text().split()
    M.main(["--synthetic", str(d), "--samples", "256", "--subjects", *subs, "--epochs", "3", "--patience", "1", "2", "--batch-size", "16",
            "--hierarchical", "--model", "cnn_gru", "--out", str(tmp_path / "cli")])
    (run,) = sorted((tmp_path / "cli").glob("simple_binary/run_*"))
    text = (run / "hierarchical_summary.txt").read_text(encoding="utf-8")
    assert "MODEL_TO_USE: cnn_gru\n" in text
    for tag, hid in (("model_m1", 64), ("model_m2", 32)):
        sd = torch.load(run / "fold_test_on_S3" / tag / "best_model.pt", weights_only=True, map_location="cpu")
        assert not any(k.startswith("channel_attention") for k in sd) and sd["gru.weight_hh_l0"].shape[1] == hid
    cfg = M.default_cfg()
    cfg.update(data_path=d, subjects=subs, epochs=3, patience=[1, 2], batch_size=16, model="cnn_gru")
    res_b, _ = M.run_hierarchical_experiment(tmp_path / "batched", DEV, names, cfg)
    res_s, _ = M.run_hierarchical_experiment(tmp_path / "seq", DEV, names, dict(cfg, concurrent_folds=1))
    assert res_b == res_s
    for s in subs:
        fb = json.loads((tmp_path / "batched" / f"fold_test_on_{s}" / "fold_result.json").read_text())
        fs = json.loads((tmp_path / "seq" / f"fold_test_on_{s}" / "fold_result.json").read_text())
        assert fb == fs, s
    att = M.default_cfg()
    att.update(data_path=d, subjects=subs, epochs=3, patience=[1, 2], batch_size=16)
    M.run_hierarchical_experiment(tmp_path / "att", DEV, names, att)
    assert "MODEL_TO_USE" not in (tmp_path / "att" / "hierarchical_summary.txt").read_text(encoding="utf-8")
