"""Weight averaging (include/msig_wa.h) on the GPU.  Every comparison is exact: the update is three fp32 roundings per
element, restated in numpy by tests/wa_reference.py; a fold of a fold batch has the bits of its single call; the train step does not
know the shadow exists; the shadow is evaluated by the existing forward.

Shapes: C in {2, 6} (C = 2: the gate's hidden width C // 4 is 0, the degenerate gate), K = 2, T = 256, B = 5, 3 or 4 arenas — the
smallest at which float4 tails, arena strides and the degenerate gate occur."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import wa_reference as R
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd import averaging as AV
from multimodalsignal_amd.runtime import EmbeddedEngine, Engine, FoldArena
from oracle import cnn_gru_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
K, T, B, LR = 2, 256, 5, 1e-3
COEFS = (0.0, 1.0, 2.0 ** -10, 0.1, 0.9)
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-42, -3.0e38], np.float32)


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _raw(t):
    """The bytes of a device tensor, as a numpy array."""
    return t.detach().contiguous().view(torch.uint8).cpu().numpy()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_raw(a), _raw(b))


def _values(n, seed):
    """n fp32 values: seeded normal numbers with zeros, +-inf, NaN, a denormal and a huge value spread through them."""
    rs = np.random.RandomState(seed)
    v = rs.randn(n).astype(np.float32)
    pos = rs.permutation(n)[:min(n // 2, 3 * len(SPECIAL))] if n > 4 else np.array([seed % 4, (seed + 2) % 4])
    v[pos] = SPECIAL[(np.arange(len(pos)) + seed) % len(SPECIAL)]
    return v


def _same_as_reference(got, want):
    """Bit for bit, except where the reference is NaN: there the position alone counts."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def _wa(n_flat, p, s, a, bn=None):
    w = L.Wa()
    w.n_flat, w.params, w.avg_params = n_flat, p.data_ptr(), s.data_ptr()
    if bn is not None:
        w.bn_state, w.bn_count, w.avg_bn_state, w.avg_bn_count = (t.data_ptr() for t in bn)
    w.coef[0] = a
    return w


def _update(n_flat, p, s, a, bn=None):
    L.check(L.lib().msig_wa_update(C.byref(_wa(n_flat, p, s, a, bn)), _stream()), "msig_wa_update")


# ---- 1. the kernel against the numpy restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bn", [True, False], ids=["bn", "null-bn"])
@pytest.mark.parametrize("a", COEFS)
@pytest.mark.parametrize("n_flat", [4, 1028, "layout"])
def test_update_equals_the_reference_bit_for_bit(n_flat, a, with_bn):
    n = L.param_layout(2, K)[-1] if n_flat == "layout" else n_flat
    a = float(np.float32(a))
    p_h, s_h = _values(n, 1), _values(n, 2)
    bp_h, bs_h = _values(L.BN_STATE_FLOATS, 3), _values(L.BN_STATE_FLOATS, 4)
    p, s = torch.as_tensor(p_h).to(DEV), torch.as_tensor(s_h).to(DEV)
    bn = None
    if with_bn:
        bn = (torch.as_tensor(bp_h).to(DEV), torch.tensor([7, 2 ** 40 + 3], dtype=torch.int64, device=DEV), torch.as_tensor(bs_h).to(DEV),
              torch.tensor([-1, 5], dtype=torch.int64, device=DEV))
    _update(n, p, s, a, bn)
    torch.cuda.synchronize()
    assert np.array_equal(_raw(p), torch.as_tensor(p_h).view(torch.uint8).numpy())               # the model is only read
    if a == 0.0 or a == 1.0:                                                                      # nothing, or a 32-bit copy: NaN payloads included
        assert np.array_equal(s.cpu().numpy().view(np.uint32), (s_h if a == 0.0 else p_h).view(np.uint32))
    assert _same_as_reference(s.cpu().numpy(), R.update(s_h, p_h, a))
    if with_bn:
        assert np.array_equal(_raw(bn[0]), torch.as_tensor(bp_h).view(torch.uint8).numpy()) and bn[1].tolist() == [7, 2 ** 40 + 3]
        assert _same_as_reference(bn[2].cpu().numpy(), R.update(bs_h, bp_h, a))
        assert bn[3].tolist() == ([-1, 5] if a == 0.0 else [7, 2 ** 40 + 3])


# ---- 2. a fold batch against its single calls -----------------------------------------------------------------------------------------
SHADOW = ("avg_params", "avg_bn_state", "avg_bn_count")


def _filled_arena(Cc, n=4, seed=0, **kw):
    """Arenas whose every byte is seeded noise, with finite floats in the buffers the update reads as numbers."""
    arena = FoldArena(Cc, K, DEV, n, B, T, averaging=True, **kw)
    g = torch.Generator(device="cpu").manual_seed(seed)
    arena.mem.copy_(torch.randint(0, 256, tuple(arena.mem.shape), dtype=torch.uint8, generator=g))
    for slot in range(n):
        for name in ("params", "bn_state", "avg_params", "avg_bn_state"):
            v = arena.view(slot, name, torch.float32)
            v.copy_(torch.as_tensor(_values(v.numel(), 10 * slot + len(name) + seed)))
    return arena


def _single(arena, slot, a):
    """The single call on copies of arena `slot`'s buffers: (avg_params, avg_bn_state, avg_bn_count) after it."""
    t = {name: arena.view(slot, name, torch.int64 if name.endswith("count") else torch.float32).clone()
         for name in ("params", "bn_state", "bn_count") + SHADOW}
    _update(arena.n_flat, t["params"], t["avg_params"], a, (t["bn_state"], t["bn_count"], t["avg_bn_state"], t["avg_bn_count"]))
    return [t[name] for name in SHADOW]


@pytest.mark.parametrize("Cc", [2, 6])
def test_fold_batch_equals_single_calls_and_touches_nothing_else(Cc):
    arena = _filled_arena(Cc, grad_clip=(Cc == 6))
    names = list(arena.off)
    assert names[-3:] == list(SHADOW) and ("gc" in names) == (Cc == 6)                # after every other region, "gc" included
    for coefs in ((0.25, 0.9), (0.5, 0.0), (1.0, float(np.float32(0.1)))):
        before = arena.mem.clone()
        want = {slot: _single(arena, slot, a) for slot, a in zip((2, 0), coefs)}
        L.check(L.lib().msig_wa_update_multi(C.byref(arena.wa([2, 0], coefs)), C.byref(arena.multi([2, 0])), _stream()), "msig_wa_update_multi")
        torch.cuda.synchronize()
        for slot, a in zip((2, 0), coefs):
            for name, w in zip(SHADOW, want[slot]):
                assert _same(arena.view(slot, name, w.dtype), w), (coefs, slot, name)
            if a == 0.0:
                assert torch.equal(arena.mem[slot], before[slot]), (coefs, slot)     # nothing of that fold is written
        assert torch.equal(arena.mem[1], before[1]) and torch.equal(arena.mem[3], before[3])
        lo = arena.off["avg_params"][0]
        assert torch.equal(arena.mem[:, :lo], before[:, :lo])                         # every region but the three shadow regions
        pads = [(o + nb, (o + nb + 255) // 256 * 256) for o, nb in (arena.off[n_] for n_ in SHADOW)]
        assert all(torch.equal(arena.mem[:, a0:a1], before[:, a0:a1]) for a0, a1 in pads)      # nor the padding between them


def test_arenas_without_averaging_are_what_they_were():
    plain, avg = FoldArena(6, K, DEV, 3, B, T, grad_clip=True), FoldArena(6, K, DEV, 3, B, T, grad_clip=True, averaging=True)
    assert list(avg.off)[:len(plain.off)] == list(plain.off) and all(avg.off[k] == plain.off[k] for k in plain.off)
    assert avg.stride > plain.stride and not any(k.startswith("avg_") for k in plain.off)
    with pytest.raises(RuntimeError):
        plain.wa([0], [0.5])
    with pytest.raises(ValueError):
        plain.batch(B, False, 0.0, shadow=True)
    with pytest.raises(ValueError):
        avg.batch(B, True, 0.5, shadow=True)
    with pytest.raises(ValueError):
        avg.wa([0, 1], [0.5, 1.5])


# ---- 3. repeated and concurrent runs --------------------------------------------------------------------------------------------------
def test_repeated_and_concurrent_runs_give_the_same_bits():
    n = L.param_layout(6, K)[-1]
    p, s0 = torch.as_tensor(_values(n, 5)).to(DEV), torch.as_tensor(_values(n, 6)).to(DEV)
    bn0 = (torch.as_tensor(_values(96, 7)).to(DEV), torch.tensor([3, 4], dtype=torch.int64, device=DEV), torch.as_tensor(_values(96, 8)).to(DEV),
           torch.zeros(2, dtype=torch.int64, device=DEV))
    outs = []
    busy, side = torch.randn(2048, 2048, device=DEV), torch.cuda.Stream(DEV)
    for run in range(3):
        s, bn = s0.clone(), tuple(t.clone() for t in bn0)
        torch.cuda.synchronize()
        if run == 2:                                        # beside a busy second stream
            with torch.cuda.stream(side):
                for _ in range(8):
                    busy = torch.tanh(busy @ busy * 1e-3)
        for a in (0.9, 0.1, 0.01):
            _update(n, p, s, float(np.float32(a)), bn)
        torch.cuda.synchronize()
        outs.append((_raw(s), _raw(bn[2]), bn[3].tolist()))
    for o in outs[1:]:
        assert np.array_equal(o[0], outs[0][0]) and np.array_equal(o[1], outs[0][1]) and o[2] == outs[0][2] == [3, 4]


# ---- 4. the training step is untouched ------------------------------------------------------------------------------------------------
def _data(Cc, seed, rows=B):
    rs = np.random.RandomState(seed)
    y = rs.randint(0, K, size=rows).astype(np.int64)
    y[:K] = np.arange(K)
    return torch.as_tensor(rs.randn(rows, Cc, T).astype(np.float32)).to(DEV), torch.as_tensor(y).to(DEV)


def _engine(Cc, hidden=64, layers=2, seed=3, storage_engine=None):
    params = O.init_params(Cc, K, seed=seed, hidden=hidden, layers=layers)
    e = storage_engine
    if e is None:
        e = EmbeddedEngine(Cc, K, DEV, hidden) if layers == 1 else Engine(Cc, K, DEV)
    if layers == 1:
        for k, v in e.small_views().items():
            v.copy_(params[k])
        e.scatter()
    else:
        e.load_named(params)
    return e


def _four_steps(e, Cc, ema, snaps=None):
    if ema:
        e.average_update(1.0)
    for s in (1, 2, 3, 4):
        x, y = _data(Cc, 20 + s)
        e.train_step(x, y, LR, weight_decay=1e-4, step=s, dropout_p=0.5, seed=7)
        if ema:
            e.average_update(AV.ema_coef(s - 1))
        if snaps is not None:
            snaps.append((e.params.cpu().numpy().copy(), e.bn_state.cpu().numpy().copy(), e.bn_count.tolist()))
    torch.cuda.synchronize()
    return e


@pytest.mark.parametrize("Cc", [2, 6])
@pytest.mark.parametrize("model", [(64, 2), (32, 1)], ids=["depth2", "embedded"])
def test_train_steps_are_the_same_with_and_without_the_shadow_and_the_shadow_is_the_replay(model, Cc):
    """Four train steps with EMA on and off from the same seeds: parameters, gradients, BatchNorm state and Adam moments are
    byte-identical, and (test 5, the engine path) the shadow is the reference's replay of the four snapshots — in the padded
    layout for the embedded model, whose padding stays bitwise +0.0."""
    hidden, layers = model
    snaps = []
    init = _engine(Cc, hidden, layers)
    p0, b0 = init.params.cpu().numpy().copy(), init.bn_state.cpu().numpy().copy()
    on, off = _four_steps(_engine(Cc, hidden, layers), Cc, True, snaps), _four_steps(_engine(Cc, hidden, layers), Cc, False)
    for name in ("params", "grads", "exp_avg", "exp_avg_sq", "bn_state", "bn_count", "loss_acc"):
        assert _same(getattr(on, name), getattr(off, name)), name
    assert off.avg_params is None
    assert np.array_equal(on.avg_params.cpu().numpy().view(np.uint32), R.replay_ema(p0, [s[0] for s in snaps]).view(np.uint32))
    assert np.array_equal(on.avg_bn_state.cpu().numpy().view(np.uint32), R.replay_ema(b0, [s[1] for s in snaps]).view(np.uint32))
    assert on.avg_bn_count.tolist() == snaps[-1][2] == [4, 4]
    assert not np.array_equal(on.avg_params.cpu().numpy(), snaps[-1][0])                # an average, not the last iterate
    if layers == 1:
        pad = on.avg_params[on.padding]
        assert pad.numel() > 0 and int(pad.view(torch.int32).count_nonzero()) == 0       # bitwise +0.0


def _profiled(fn):
    L.profile_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        return {k: v[0] for k, v in L.profile_report().items()}
    finally:
        L.profile_enable(False)


def test_the_update_is_exactly_one_more_launch_per_training_step():
    Cc = 6
    x, y = _data(Cc, 4)
    reports = []
    for ema in (False, True):
        e = _engine(Cc)
        if ema:
            e.average_update(1.0)
        e.train_step(x, y, LR, step=1, dropout_p=0.5, seed=7)              # workspaces exist before the count starts

        def step():
            e.train_step(x, y, LR, step=2, dropout_p=0.5, seed=7)
            if ema:
                e.average_update(AV.ema_coef(1))
        reports.append(_profiled(step))
    plain, with_ema = reports
    assert "wa_update" not in plain and sum(plain.values()) > 5
    assert with_ema == {**plain, "wa_update": 1}
    e = _engine(Cc)
    assert _profiled(lambda: e.average_update(0.0)) == {}                   # a = 0: no launch at all


# ---- 5./7./8./9. the trainers ---------------------------------------------------------------------------------------------------------
SUBS = ["S2", "S3", "S4", "S5"]


def _dataset(tmp_path, windows=10, spread=0):
    from multimodalsignal_amd.synth import make_synthetic_wesad
    d = make_synthetic_wesad(tmp_path / "w", subjects=SUBS, windows_per_subject=windows, T=T, difficulty=2.0, window_spread=spread)
    return d, (d / "_channel_names.txt").read_text().split()


def _cfg(d, averaging, **kw):
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.synth import CHANNELS6
    cfg = M.default_cfg()
    cfg.update(data_path=d, channels=list(CHANNELS6), subjects=SUBS, epochs=1, batch_size=B, patience=20, averaging=averaging)
    cfg.update(kw)
    return cfg


def _preps(tmp_path, tag, d, names, cfg, folds=(0, 1, 2, 3)):
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.dataset import SubjectStore
    store = SubjectStore(d, SUBS, cfg["channels"], names, classification_mode=cfg["mode"], device=DEV)
    return [M.prepare_fold(k, SUBS[k], tmp_path / tag, DEV, names, cfg, store) for k in folds]


def _record_engine_updates(monkeypatch):
    """Records (engine, a, params, bn_state) of every Engine.average_update with a > 0, after the call (the model is only read)."""
    log = []
    for cls in (Engine, EmbeddedEngine):
        orig = cls.average_update

        def wrapped(self, a, _orig=orig, _cls=cls):
            _orig(self, a)
            if a > 0 and type(self) is _cls:
                log.append((self, float(a), self.params.cpu().numpy().copy(), self.bn_state.cpu().numpy().copy()))
        monkeypatch.setattr(cls, "average_update", wrapped)
    return log


def _record_multi_updates(monkeypatch, holder):
    """Records (slot, a, params, bn_state) for every fold with a > 0 of every msig_wa_update_multi (holder["lt"]: the LockstepTrainer)."""
    log, lib = [], L.lib()
    orig = lib.msig_wa_update_multi

    def wrapped(w, m, st):
        rc = orig(w, m, st)
        arena = holder["lt"].arena
        for z in range(m._obj.n):
            if w._obj.coef[z] > 0:
                slot = m._obj.slot[z]
                log.append((slot, float(w._obj.coef[z]), arena.view(slot, "params", torch.float32).cpu().numpy().copy(),
                            arena.view(slot, "bn_state", torch.float32).cpu().numpy().copy()))
        return rc
    monkeypatch.setattr(lib, "msig_wa_update_multi", wrapped)
    return log


def _check_ema_replay(records, eng):
    """records: [(a, params, bn_state)] of one fold in order — the initial copy, then one update per train step."""
    assert len(records) >= 5 and records[0][0] == 1.0
    assert [r[0] for r in records[1:]] == [float(R.ema_coef(t)) for t in range(len(records) - 1)]
    assert np.array_equal(eng.avg_params.cpu().numpy().view(np.uint32), R.replay_ema(records[0][1], [r[1] for r in records[1:]]).view(np.uint32))
    assert np.array_equal(eng.avg_bn_state.cpu().numpy().view(np.uint32), R.replay_ema(records[0][2], [r[2] for r in records[1:]]).view(np.uint32))
    assert _same(eng.avg_bn_count, eng.bn_count) and int(eng.bn_count[0]) == len(records) - 1


@pytest.mark.parametrize("embedded", [False, True], ids=["depth2", "embedded"])
def test_trainer_and_lockstep_shadows_are_the_replay_of_their_snapshots(tmp_path, monkeypatch, embedded):
    """One epoch of at least four steps with EMA on, through Trainer.train and through LockstepTrainer: each fold's shadow equals the
    reference's replay of the parameter snapshots taken after each of its train steps, with the schedule's coefficients."""
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.multifold import LockstepTrainer
    d, names = _dataset(tmp_path)
    kw = dict(model_params=dict(M.M2_MODEL_PARAMS)) if embedded else {}
    cfg = _cfg(d, {"mode": "ema"}, **kw)
    log = _record_engine_updates(monkeypatch)
    (p,) = _preps(tmp_path, "seq", d, names, cfg, folds=(1,))
    info = M.train_fold(p, DEV)
    eng = p["model"].engine()
    _check_ema_replay([r[1:] for r in log if r[0] is eng], eng)
    assert info["averaging"]["updates"] == len(log) - 1 and info["averaging"]["iterates"] == 0 and "val_loss_avg" not in info["history"][0]
    if embedded:
        assert int(eng.avg_params[eng.padding].view(torch.int32).count_nonzero()) == 0
    seq_shadow = (eng.avg_params.clone(), eng.avg_bn_state.clone())
    holder = {}
    mlog = _record_multi_updates(monkeypatch, holder)
    preps = _preps(tmp_path, "lock", d, names, cfg, folds=(0, 1, 2))
    holder["lt"] = LockstepTrainer(preps, DEV)
    infos = holder["lt"].run()
    for slot, pp in enumerate(preps):
        e = pp["model"].engine()
        _check_ema_replay([r[1:] for r in mlog if r[0] == slot], e)
        if embedded:
            assert int(e.avg_params[e.padding].view(torch.int32).count_nonzero()) == 0
    assert _same(preps[1]["model"].engine().avg_params, seq_shadow[0]) and _same(preps[1]["model"].engine().avg_bn_state, seq_shadow[1])
    a, b = dict(infos[1]), dict(info)
    for i in (a, b):
        i.pop("seconds"), i.pop("train_windows_per_s"), [h.pop("seconds") for h in i["history"]]
    assert json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)


def test_swa_is_the_mean_of_the_epoch_end_iterates_and_falls_back_to_the_final_weights(tmp_path, monkeypatch):
    from multimodalsignal_amd import main as M
    d, names = _dataset(tmp_path)
    (probe,) = _preps(tmp_path, "probe", d, names, _cfg(d, None), folds=(0,))
    n_train = len(probe["loaders"][0].dataset)
    bs = (n_train + 1) // 2                                                        # two steps per epoch
    log = _record_engine_updates(monkeypatch)
    cfg = _cfg(d, {"mode": "swa", "start_epoch": 2, "bn": "average"}, epochs=3, batch_size=bs)
    (p,) = _preps(tmp_path, "swa", d, names, cfg, folds=(0,))
    info = M.train_fold(p, DEV)
    eng = p["model"].engine()
    assert len(p["loaders"][0]) == 2 and info["epochs"] == 3
    assert [r[1] for r in log] == [1.0, 0.5] and info["averaging"]["iterates"] == 2
    assert np.array_equal(eng.avg_params.cpu().numpy().view(np.uint32), R.replay_swa([r[2] for r in log]).view(np.uint32))
    assert np.array_equal(eng.avg_bn_state.cpu().numpy().view(np.uint32), R.replay_swa([r[3] for r in log]).view(np.uint32))
    assert eng.avg_bn_count.tolist() == [6, 6]
    # a fold that early-stops before start_epoch: its end-of-training weights — not the restored checkpoint — are its single iterate
    del log[:]
    cfg = _cfg(d, {"mode": "swa", "start_epoch": 10, "bn": "average"}, epochs=4, batch_size=bs, patience=1)
    (p,) = _preps(tmp_path, "early", d, names, cfg, folds=(0,))
    info = M.train_fold(p, DEV)
    eng = p["model"].engine()
    assert info["averaging"]["iterates"] == 0 and info["epochs"] < 10 and len(log) == 1 and log[0][1] == 1.0
    assert np.array_equal(eng.avg_params.cpu().numpy().view(np.uint32), log[0][2].view(np.uint32))
    assert np.array_equal(eng.avg_bn_state.cpu().numpy().view(np.uint32), log[0][3].view(np.uint32))
    saved = torch.load(p["fold_dir"] / "averaged_model.pt", weights_only=True)
    assert all(torch.equal(saved[k], v.cpu()) for k, v in eng.named_param_views(eng.avg_params).items())


def test_recompute_equals_a_hand_built_adapter(tmp_path):
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.adapt import BnAdapter
    d, names = _dataset(tmp_path)
    for tag, bn in (("avg", "average"), ("rec", "recompute")):
        (p,) = _preps(tmp_path, tag, d, names, _cfg(d, {"mode": "ema", "bn": bn}, epochs=2), folds=(2,))
        M.train_fold(p, DEV)
        eng = p["model"].engine()
        if bn == "average":
            averaged = (eng.avg_params.clone(), eng.avg_bn_state.clone())
            continue
        assert _same(eng.avg_params, averaged[0]) and not _same(eng.avg_bn_state, averaged[1])      # the weights are the same run's
        fresh = M.make_model(_cfg(d, None), eng.C, K, dict(M.MODEL_PARAMS["cnn_gru_attention"])).to(DEV)
        fresh.load_state_dict(p["trainer"].averager.state_dict())
        x = AV.training_windows(p["loaders"][0])
        want = BnAdapter([dict(model=fresh, x=x)], alpha=1.0).adapted_state(0)
        assert _same(eng.avg_bn_state, want)
        assert _same(eng.avg_bn_count, eng.bn_count)


@pytest.mark.parametrize("averaging", [{"mode": "ema", "validate": True, "decay": 0.9, "warmup": 2},
                                       {"mode": "swa", "start_epoch": 2, "validate": True}], ids=["ema", "swa-recompute"])
def test_lockstep_equals_sequential_with_folds_of_unequal_size(tmp_path, averaging):
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.multifold import LockstepTrainer, lockstep_compatible
    d, names = _dataset(tmp_path, windows=14, spread=4)
    out = {}
    for mode in ("seq", "lock"):
        cfg = _cfg(d, averaging, epochs=4, patience=[1, 2, 4, 4])
        preps = _preps(tmp_path, mode, d, names, cfg)
        if mode == "seq":
            infos = [M.train_fold(p, DEV) for p in preps]
        else:
            assert lockstep_compatible(preps)
            infos = LockstepTrainer(preps, DEV).run()
        out[mode] = []
        for p, i in zip(preps, infos):
            e = p["model"].engine()
            i = dict(i)
            i.pop("seconds"), i.pop("train_windows_per_s"), [h.pop("seconds") for h in i["history"]]
            assert json.loads((p["fold_dir"] / "fold_result.json").read_text())["averaging"] == i["averaging"]
            out[mode].append((i, e.avg_params.clone(), e.avg_bn_state.clone(), e.avg_bn_count.clone(),
                              torch.load(p["fold_dir"] / "averaged_model.pt", weights_only=True), len(p["loaders"][0])))
    assert len({o[5] for o in out["seq"]}) > 1, "the folds should take different numbers of steps per epoch for this test to bite"
    for (ia, pa, ba, ca, wa, _), (ib, pb, bb, cb, wb, _) in zip(out["seq"], out["lock"]):
        assert json.dumps(ia, sort_keys=True) == json.dumps(ib, sort_keys=True)
        assert _same(pa, pb) and _same(ba, bb) and _same(ca, cb)
        assert list(wa) == list(wb) and all(torch.equal(wa[k], wb[k]) for k in wa)
        assert all({"val_loss_avg", "val_acc_avg", "val_f1_avg"} <= set(h) for h in ia["history"])
        if averaging["mode"] == "swa":
            assert ia["history"][0]["val_loss_avg"] is None and (len(ia["history"]) < 2 or ia["history"][1]["val_loss_avg"] is not None)
        else:
            assert all(h["val_loss_avg"] is not None for h in ia["history"])


def test_folds_of_a_batch_must_share_one_averaging_setting(tmp_path):
    from multimodalsignal_amd.multifold import LockstepTrainer
    d, names = _dataset(tmp_path)
    preps = _preps(tmp_path, "a", d, names, _cfg(d, {"mode": "ema"}), folds=(0,)) + _preps(tmp_path, "b", d, names, _cfg(d, {"mode": "swa"}), folds=(1,))
    with pytest.raises(ValueError, match="averaging setting"):
        LockstepTrainer(preps, DEV)


# ---- 6. evaluation under the shadow ----------------------------------------------------------------------------------------------------
def _fresh_forward(sd, Cc, x, y, hidden=64, layers=2):
    from multimodalsignal_amd.models import CnnGruAttentionModel
    m = CnnGruAttentionModel(Cc, K, gru_hidden_size=hidden, gru_num_layers=layers).to(DEV)
    m.load_state_dict(sd)
    m.eval()
    e = m.engine()
    e.loss_acc.zero_()
    e.forward(x, y, training=False)
    rows = x.shape[0]
    return (e.region("LOGITS", torch.float32, (rows, K)).clone(), e.region("LOSS", torch.float32, (1,)).clone(),
            e.region("PRED", torch.int32, (rows,)).clone(), e.loss_acc.clone())


@pytest.mark.parametrize("Cc", [2, 6])
@pytest.mark.parametrize("model", [(64, 2), (32, 1)], ids=["depth2", "embedded"])
def test_forward_under_the_shadow_is_a_fresh_model_with_the_averaged_state(model, Cc):
    hidden, layers = model
    e = _engine(Cc, hidden, layers)
    x, y = _data(Cc, 99, rows=7)
    e.forward(x, y, training=False)
    own_before = e.region("LOGITS", torch.float32, (7, K)).clone()
    _four_steps(e, Cc, True)
    av = AV.WeightAverager({"mode": "ema"}).bind(e)
    assert av.start_coef() == 1.0
    sd = av.state_dict()
    want = _fresh_forward(sd, Cc, x, y, hidden, layers)
    e.loss_acc.zero_()
    e.forward(x, y, training=False, shadow=True)
    got = (e.region("LOGITS", torch.float32, (7, K)).clone(), e.region("LOSS", torch.float32, (1,)).clone(),
           e.region("PRED", torch.int32, (7,)).clone(), e.loss_acc.clone())
    assert all(_same(g, w) for g, w in zip(got, want))
    # the model's own forward does not know the shadow exists
    plain = _four_steps(_engine(Cc, hidden, layers), Cc, False)
    e.forward(x, y, training=False)
    plain.forward(x, y, training=False)
    assert _same(e.region("LOGITS", torch.float32, (7, K)), plain.region("LOGITS", torch.float32, (7, K)))
    assert not _same(e.region("LOGITS", torch.float32, (7, K)), got[0]) and not _same(own_before, got[0])
    with pytest.raises(ValueError):
        e.forward(x, y, training=True, shadow=True)
    with pytest.raises(RuntimeError):
        plain.forward(x, y, shadow=True)                    # no shadow yet


def test_forward_multi_under_the_shadows_equals_fresh_models():
    Cc, n, rows = 6, 3, 7
    arena = FoldArena(Cc, K, DEV, n, B, T, eval_batch=rows, averaging=True)
    engs = [_engine(Cc, seed=10 + f, storage_engine=arena.engine(f)) for f in range(n)]
    for f, e in enumerate(engs):
        _four_steps(e, Cc, True)
    x, y = _data(Cc, 77, rows=rows)
    for f in range(n):
        arena.view(f, "x", torch.float32)[:x.numel()].copy_(x.reshape(-1))
        arena.view(f, "y", torch.int64)[:rows].copy_(y)
    slots = [2, 0, 1]
    off = L.workspace_layout(rows, Cc, T, K, False)
    outs = {}
    for shadow in (False, True):
        arena.across("acc", 0, torch.float64, 2).zero_()
        desc, m, s = arena.batch(rows, False, 0.0, shadow=shadow), arena.multi(slots), arena.soft(slots, 0.0)
        L.check(L.lib().msig_st_forward_multi(C.byref(desc), C.byref(m), C.byref(s), _stream()), "msig_st_forward_multi")
        torch.cuda.synchronize()
        outs[shadow] = (arena.across("ws", off[L.WS["LOGITS"]], torch.float32, rows * K).clone(),
                        arena.across("ws", off[L.WS["PRED"]], torch.int32, rows).clone(), arena.across("acc", 0, torch.float64, 2).clone())
    for f, e in enumerate(engs):
        av = AV.WeightAverager({"mode": "ema"}).bind(e)
        av.start_coef()
        logits, _, pred, acc = _fresh_forward(av.state_dict(), Cc, x, y)
        assert _same(outs[True][0][f].view(rows, K), logits) and _same(outs[True][1][f], pred) and _same(outs[True][2][f], acc), f
        own = _fresh_forward({k: v.clone() for k, v in {**e.named_param_views(), **e.bn_views()}.items()}, Cc, x, y)
        assert _same(outs[False][0][f].view(rows, K), own[0]) and not _same(outs[False][0][f], outs[True][0][f]), f


# ---- 10. the driver ---------------------------------------------------------------------------------------------------------------------
def _fold_results(run):
    out = {}
    for s in SUBS:
        info = json.loads((run / f"fold_test_on_{s}" / "fold_result.json").read_text())
        info.pop("seconds"), info.pop("train_windows_per_s"), [h.pop("seconds") for h in info["history"]]
        out[s] = info
    return out


def test_driver_writes_the_averaging_table_and_leaves_the_loso_run_alone(tmp_path, capsys):
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.models import CnnGruAttentionModel
    from multimodalsignal_amd.synth import make_synthetic_wesad
    d = make_synthetic_wesad(tmp_path / "w", subjects=SUBS, windows_per_subject=150, T=256, difficulty=2.0)
    common = ["--synthetic", str(d), "--samples", "256", "--subjects", *SUBS, "--epochs", "2", "--patience", "1", "--batch-size", "16"]
    M.main(common + ["--weight-average", "ema", "--out", str(tmp_path / "avg")])
    M.main(common + ["--out", str(tmp_path / "plain")])
    runs = {k: sorted((tmp_path / k).glob("simple_binary/run_*"))[0] for k in ("avg", "plain")}
    cut = lambda text: text[:text.index("LOSO wall-clock")]
    a_txt, p_txt = (cut((runs[k] / "cv_summary.txt").read_text(encoding="utf-8")) for k in ("avg", "plain"))
    assert a_txt.replace("WEIGHT AVERAGING: mode=ema decay=0.99 warmup=10 bn=average\n", "") == p_txt and a_txt != p_txt
    fa, fp = _fold_results(runs["avg"]), _fold_results(runs["plain"])
    for s in SUBS:
        assert "averaging" not in fp[s] and {k: v for k, v in fa[s].items() if k != "averaging"} == fp[s], s
        fd = runs["avg"] / f"fold_test_on_{s}"
        assert not (runs["plain"] / f"fold_test_on_{s}" / "averaged_model.pt").exists()
        best_a = torch.load(fd / "best_model.pt", weights_only=True, map_location="cpu")
        best_p = torch.load(runs["plain"] / f"fold_test_on_{s}" / "best_model.pt", weights_only=True, map_location="cpu")
        assert list(best_a) == list(best_p) and all(torch.equal(best_a[k], best_p[k]) for k in best_a)
        sd = torch.load(fd / "averaged_model.pt", weights_only=True, map_location="cpu")
        m = CnnGruAttentionModel(6, 2)
        m.load_state_dict(sd)                                                       # strict: the reference's keys, all of them
        assert set(sd) == set(best_a) and any(not torch.equal(sd[k], best_a[k]) for k in sd)
    assert sorted(p.name for p in runs["plain"].iterdir()) == sorted(p.name for p in runs["avg"].iterdir() if not p.name.startswith("averaging"))
    doc = json.loads((runs["avg"] / "averaging.json").read_text())
    assert [f["subject"] for f in doc["folds"]] == SUBS and doc["n_folds"] == 4 and doc["note"] == AV.SYNTHETIC_NOTE
    assert doc["settings"] == AV.settings({"mode": "ema"})
    for f in doc["folds"]:
        r = fa[f["subject"]]
        assert f["before"] == {"accuracy": r["accuracy"], "f1_score": r["f1_score"]}
        assert f["after"] == {"accuracy": r["averaging"]["accuracy"], "f1_score": r["averaging"]["f1_score"]}
        assert f["updates"] == r["averaging"]["updates"] > 0 and f["val_loss"] > 0 and f["val_loss_avg"] > 0
    txt = (runs["avg"] / "averaging.txt").read_text(encoding="utf-8")
    assert AV.SYNTHETIC_NOTE in txt and all(s in txt for s in SUBS) and "mean paired difference" in txt and "not known" in txt
    assert "Weight-averaging table written to" in capsys.readouterr().out
