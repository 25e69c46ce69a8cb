"""Input gradients and eval-mode backward through CnnGruAttentionModel (msig_batch.dx / keep_for_backward, ABI 5) against the
autograd of the oracle with x as a leaf: fp64 is the reference, the fp32 run of the same oracle the yardstick of fp32 arithmetic
on the case ("own" error, as tests/gpu_common.py does for the parameter gradients)."""
import numpy as np
import pytest
import torch

from gpu_common import GRAD_FLOOR, grad_tol, rel_err, split_named, to_t
from oracle import cnn_gru_oracle as O

pytestmark = pytest.mark.gpu

CONFIGS = {"full": dict(), "embedded": dict(gru_hidden_size=32, gru_num_layers=1)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tier needs an MI355X"
    return torch.device("cuda:0")


def _model(C, K, config, dropout, dev, seed=0):
    from multimodalsignal_amd.models import CnnGruAttentionModel
    torch.manual_seed(seed)
    return CnnGruAttentionModel(C, K, dropout=dropout, **CONFIGS[config]).to(dev)


def _case(B, C, K, T, seed):
    rs = np.random.RandomState(seed)
    x = (rs.randn(B, C, T) * (0.5 + rs.rand(1, C, 1)) + rs.randn(1, C, 1)).astype(np.float32)
    y = rs.randint(0, K, size=(B,)).astype(np.int64)
    return torch.as_tensor(x), torch.as_tensor(y)


def _hip_pool_choice(eng, st64, B, T):
    """MaxPool near-ties (two candidates equal to within fp32 resolution): the oracle adopts the HIP path's decision, recomputed
    from ITS conv outputs and BatchNorm constants — only there (the rule of gpu_common.run_case; everywhere else the oracle's own
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


def _check_against_oracle(m, named, x, y, xgrad, training, fw, loss_fn=None, params=True):
    dx64, g64, st64 = _oracle(named, x, y, torch.float64, training, fw, loss_fn)
    choice = _hip_pool_choice(m._engine, st64, x.shape[0], x.shape[2])
    if choice is not None:
        dx64, g64, st64 = _oracle(named, x, y, torch.float64, training, fw, loss_fn, choice)
    dx32, g32, _ = _oracle(named, x, y, torch.float32, training, fw, loss_fn, choice)
    own = rel_err(dx32.numpy(), dx64.numpy())
    err = rel_err(xgrad, dx64.numpy())
    assert err <= grad_tol("x", own), ("dx", err, own)
    if params:
        for k, p in m.named_parameters():
            if p.numel():
                own_k = rel_err(g32[k].numpy(), g64[k].numpy())
                assert rel_err(p.grad.cpu().numpy(), g64[k].numpy()) <= grad_tol(k, own_k), (k, own_k)


SHAPES = [(4, 256), (5, 511), (64, 3840)]


@pytest.mark.parametrize("dropout", [0.0, 0.5])
@pytest.mark.parametrize("config", ["full", "embedded"])
@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("C", [1, 3, 6, 16])
def test_train_mode_input_gradient_against_oracle(C, B, T, config, dropout, dev):
    K = 2 + (C + B) % 2                  # both class counts over the matrix
    m = _model(C, K, config, dropout, dev, seed=C + B).train()
    seed = 1000 + C
    m.set_dropout_seed(seed)
    x, y = _case(B, C, K, T, 10 * C + B)
    named = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    xd = x.to(dev).requires_grad_(True)
    loss = torch.nn.CrossEntropyLoss()(m(xd), y.to(dev))
    loss.backward()
    assert xd.grad is not None and xd.grad.shape == x.shape
    _check_against_oracle(m, named, x, y, xd.grad.cpu().numpy(), True, dict(dropout_p=dropout, seed=seed, step=1), params=False)


def test_train_mode_odd_conv_length_uses_the_positionwise_staging(dev):
    """T = 301: L1 = 151 is not a multiple of 4, so the dx kernel stages dy1 position by position instead of by quads."""
    B, C, K, T = 6, 3, 2, 301
    m = _model(C, K, "full", 0.0, dev, seed=3).train()
    x, y = _case(B, C, K, T, 5)
    named = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    xd = x.to(dev).requires_grad_(True)
    torch.nn.CrossEntropyLoss()(m(xd), y.to(dev)).backward()
    _check_against_oracle(m, named, x, y, xd.grad.cpu().numpy(), True, dict(dropout_p=0.0, seed=0, step=1))


def _trained(C, K, config, dev, T=256):
    """A model whose BatchNorm running statistics are no longer the initial ones (two training steps)."""
    m = _model(C, K, config, 0.5, dev, seed=7 + C).train()
    opt = torch.optim.SGD(m.parameters(), lr=0.05)
    for s in range(2):
        x, y = _case(16, C, K, T, 50 + s)
        opt.zero_grad()
        torch.nn.CrossEntropyLoss()(m(x.to(dev)), y.to(dev)).backward()
        opt.step()
    return m


@pytest.mark.parametrize("config", ["full", "embedded"])
@pytest.mark.parametrize("C,B,T", [(6, 8, 512), (3, 5, 511), (16, 64, 3840)])
def test_eval_mode_backward_against_oracle(C, B, T, config, dev):
    K = 3
    m = _trained(C, K, config, dev).eval()
    x, y = _case(B, C, K, T, 99 + C)
    named = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ref_logits = m(x.to(dev)).clone()
    bn_before = {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
    m.zero_grad()
    xd = x.to(dev).requires_grad_(True)
    logits = m(xd)
    assert torch.equal(logits.detach(), ref_logits)                  # kept for the backward or not: the same bits
    torch.nn.CrossEntropyLoss()(logits, y.to(dev)).backward()
    torch.cuda.synchronize()
    for k, v in bn_before.items():
        assert torch.equal(m.state_dict()[k], v), k                 # forward and backward leave the running statistics alone
    _check_against_oracle(m, named, x, y, xd.grad.cpu().numpy(), False, dict(dropout_p=0.0, seed=0, step=0))


@pytest.mark.parametrize("config", ["full", "embedded"])
def test_eval_mode_saliency_map_with_autograd_grad(config, dev):
    """torch.autograd.grad(model(x)[:, 1].sum(), x) after model.eval(): an arbitrary upstream gradient, no loss, no .grad."""
    C, K, B, T = 6, 3, 7, 640
    m = _trained(C, K, config, dev).eval()
    x, y = _case(B, C, K, T, 123)
    named = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    xd = x.to(dev).requires_grad_(True)
    (g,) = torch.autograd.grad(m(xd)[:, 1].sum(), xd)
    _check_against_oracle(m, named, x, y, g.cpu().numpy(), False, dict(dropout_p=0.0, seed=0, step=0),
                          loss_fn=lambda logits: logits[:, 1].sum(), params=False)


def test_eval_mode_keeps_for_backward_only_when_autograd_may_ask(dev):
    from multimodalsignal_amd.runtime import Engine
    C, K, B, T = 6, 2, 4, 256
    m = _model(C, K, "full", 0.5, dev).eval()
    x, _ = _case(B, C, K, T, 1)
    with torch.no_grad():
        m(x.to(dev))
    assert m._engine._last[2] is False                              # a plain evaluation: no stash, the evaluation workspace
    for p in m.parameters():
        p.requires_grad_(False)
    out = m(x.to(dev))                                               # nothing requires grad: nothing kept either
    assert m._engine._last[2] is False and not out.requires_grad
    for p in m.parameters():
        p.requires_grad_(True)
    m(x.to(dev).requires_grad_(True))
    assert m._engine._last[2] == Engine.EVAL_KEEP                  # autograd may ask: the forward keeps, in a workspace of its own


def test_train_mode_parameter_gradients_do_not_depend_on_x_requires_grad(dev):
    """Asking for dx adds ONE launch (conv1_bwd_dx) and changes no other bit; not asking launches what the parameter-only
    backward always launched."""
    from multimodalsignal_amd import _lib as L
    C, K, B, T = 6, 2, 64, 3840
    x, y = _case(B, C, K, T, 17)
    runs = []
    for want_dx in (False, True):
        m = _model(C, K, "full", 0.5, dev, seed=11).train()
        m.set_dropout_seed(5)
        xd = x.to(dev).requires_grad_(want_dx)
        torch.cuda.synchronize()
        L.profile_enable(True)
        try:
            torch.nn.CrossEntropyLoss()(m(xd), y.to(dev)).backward()
            torch.cuda.synchronize()
            prof = L.profile_report()
        finally:
            L.profile_enable(False)
        runs.append((prof, {k: p.grad.clone() for k, p in m.named_parameters() if p.numel()}, xd.grad))
    (p0, g0, dx0), (p1, g1, dx1) = runs
    assert dx0 is None and dx1 is not None
    assert "conv1_bwd_dx" not in p0 and p1.pop("conv1_bwd_dx")[0] == 1
    assert {k: v[0] for k, v in p0.items()} == {k: v[0] for k, v in p1.items()}
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


def test_eval_mode_input_gradient_is_per_window(dev):
    """Eval mode: a window's gradient depends on that window alone — dx of 2048 windows at once equals the 64-window slices."""
    C, K, B, T = 6, 2, 2048, 512
    m = _trained(C, K, "full", dev).eval()
    x, y = _case(B, C, K, T, 31)
    xd = x.to(dev)

    def dx_of(xs, ys):
        xs = xs.clone().requires_grad_(True)
        torch.nn.CrossEntropyLoss(reduction="sum")(m(xs), ys).backward()
        return xs.grad

    full = dx_of(xd, y.to(dev))
    parts = torch.cat([dx_of(xd[i:i + 64], y[i:i + 64].to(dev)) for i in range(0, B, 64)])
    assert rel_err(full.cpu().numpy(), parts.cpu().numpy()) <= GRAD_FLOOR
