"""GPU tier: the HIP path against the fp64 oracle over WINDOW LENGTHS (tests/window_lengths.py; DESIGN.md "Window lengths").

Every other parity test with T % 4 != 0 fits one conv1 chunk (L1 <= 256), every multi-chunk length there is a multiple of 8, and
T % 8 == 4 occurs nowhere: the scalar staging of stage_x_chunk, conv1_bwd's non-prefetch staging at a compile-time channel count and
conv1_bwd_dx's position-wise staging have never run in a second chunk, a segment of several chunks or a whole-window item.  Here
every residue T % 16 runs inside one chunk, the chunk crossings of conv1 (256) and conv2 (128) run at unaligned lengths, and the GRU
sequence is 2, 5, 6, 7 and 8 steps long.  The tolerances are the project's own, unchanged (gpu_common.stage_tol / grad_tol, OWN_CAP,
run_case's cap of 8 adopted near-ties); the cases and seeds are window_lengths' tables, which tests/test_window_lengths_host.py
holds, with the oracle alone, to: `own` <= OWN_CAP, a live gate MLP, at most 8 fp32 / fp64 pooling disagreements, every path reached.
The plain window gather at window_floats % 4 != 0 (element by element) is held to index_select bit for bit, alone and under the
drivers.  Negative controls: make negctl LENGTH=k, tools/negative_controls.sh length, profiles/length_negative_control.log."""
import ctypes as Ct

import numpy as np
import pytest
import torch

import window_lengths as WL
from oracle import cnn_gru_oracle as O
from test_parity_gpu import FORMS
from test_trained_regimes_gpu import OWN_CAP, assert_own_capped, oracle_stages64, run_case_own

pytestmark = pytest.mark.gpu
FORM_PAIRS = dict(FORMS, auto=("auto", "auto"))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tier needs an MI355X"
    return torch.device("cuda:0")


@pytest.fixture
def kernel_forms():
    from multimodalsignal_amd import _lib as L
    yield L.set_kernel_form
    L.set_kernel_form("auto", "auto")


def check_case(eng, rep, ref, own):
    from gpu_common import failures, format_report
    print("\n" + format_report(rep))
    assert_own_capped(own)
    if eng.C >= 4:
        for k in ("channel_attention.fc.0.weight", "channel_attention.fc.2.weight"):
            assert float(ref[1][k].abs().max()) > 0, f"the gate MLP is dead: the oracle's gradient of {k} is exactly zero"
    assert bool(torch.isfinite(eng.grads).all()), "a gradient of the HIP path is not finite"
    assert not failures(rep), format_report(rep)


def stage_case(case, table, dev, kernel_forms, monkeypatch, tmp_path):
    from multimodalsignal_amd.runtime import Engine
    kernel_forms(*FORM_PAIRS[case.form])
    params, x, y = WL.build_case(case)
    eng = Engine(case.C, case.K, dev)
    rep, ref, own = run_case_own(monkeypatch, tmp_path, eng, params, x, y, tag=f"length_{table}_{case.form}", dropout_p=case.p, **WL.FW)
    check_case(eng, rep, ref, own)


@pytest.mark.parametrize("case", WL.RESIDUES, ids=WL.case_id)
def test_every_residue_of_the_window_length_against_oracle(case, dev, kernel_forms, monkeypatch, tmp_path):
    """T = 272 .. 287, one conv1 chunk each: the four low bits of T decide whether each of the four stride-2 stages ends on a padded
    window; T % 4 selects the staging of x, T % 8 the staging of conv1's backward."""
    stage_case(case, "residue", dev, kernel_forms, monkeypatch, tmp_path)


@pytest.mark.parametrize("case", WL.CROSSINGS, ids=WL.case_id)
def test_chunk_crossings_at_unaligned_lengths_against_oracle(case, dev, kernel_forms, monkeypatch, tmp_path):
    """Unaligned lengths and T % 8 == 4 across the chunk borders of conv1 (256 positions of L1) and conv2 (128 of L2): last chunks of
    one and two positions, conv1_bwd's segments of one and of two chunks, and its whole-window items at B >= 256."""
    stage_case(case, "crossing", dev, kernel_forms, monkeypatch, tmp_path)


@pytest.mark.parametrize("case", WL.SHORT, ids=WL.case_id)
def test_short_gru_sequences_against_oracle(case, dev, kernel_forms, monkeypatch, tmp_path):
    """T' = 2, 5, 6, 7, 8 under both shipped form sets: gru_bwd_b6's prologue stages steps 0 - 3 and prefetches two steps ahead,
    gru_bwd_b3 pairs steps — short sequences are where their clamps do the work.  Three batch tiles, the last with one row."""
    assert O.stage_lengths(case.T)[-1] == WL.SHORT_T[case.T]
    stage_case(case, "short", dev, kernel_forms, monkeypatch, tmp_path)


@pytest.mark.parametrize("forms", [("auto", "auto"), ("ws", "b6")], ids=["auto", "ws_b6"])
def test_fold_batch_at_an_unaligned_length_against_oracle(forms, dev, kernel_forms, monkeypatch, tmp_path):
    """ONE msig_train_step_multi over three folds at T = 1027 (built as test_fold_batch_input_regimes_against_oracle builds its
    launch); the folds differ in parameters, inputs and dropout seeds, and every fold is held to the oracle."""
    from multimodalsignal_amd import _lib as L
    from multimodalsignal_amd.runtime import FoldArena
    kernel_forms(*forms)
    (B, Cc, K, T, p), step, NF = WL.FOLD_SHAPE, WL.FOLD_STEP, len(WL.FOLD_CASES)
    arena = FoldArena(Cc, K, dev, NF, B, T)
    engines, cases = [arena.engine(s) for s in range(NF)], []
    for f in range(NF):
        params, x, y, seed = WL.fold_case(f)
        engines[f].load_named({k: torch.as_tensor(v) for k, v in params.items()})
        arena.view(f, "x", torch.float32)[:x.size].copy_(torch.as_tensor(x).reshape(-1))
        arena.view(f, "y", torch.int64)[:B].copy_(torch.as_tensor(y))
        engines[f].workspace(B, T, True)
        engines[f]._last = (B, T, True)
        cases.append((params, x, y, seed))
    m = arena.multi(list(range(NF)), key_gru=[L.dropout_key(c[3], step, 1) for c in cases],
                    key_head=[L.dropout_key(c[3], step, 2) for c in cases], lr=[1e-3] * NF, steps=[step] * NF)
    desc = arena.batch(B, True, p)
    done = []

    def launch(phase):
        if phase == "fwd" and not done:
            st = Ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            L.check(L.lib().msig_train_step_multi(Ct.byref(desc), Ct.byref(m), arena.ptr("exp_avg"), arena.ptr("exp_avg_sq"),
                                                  0.9, 0.999, 1e-8, 1e-4, step, st), "msig_train_step_multi")
            done.append(1)

    for f, (params, x, y, seed) in enumerate(cases):
        rep, ref, own = run_case_own(monkeypatch, tmp_path, engines[f], params, x, y, launch=launch, tag=f"length_multi_{forms[1]}",
                                     dropout_p=p, seed=seed, step=step)
        check_case(engines[f], rep, ref, own)


def test_eval_mode_at_an_unaligned_length_with_foreign_running_statistics(dev):
    """Engine.forward(training=False) at T = 1027 with running statistics that are no golden file's own against the fp64 oracle's
    eval-mode logits; bn_state and bn_count are untouched."""
    from gpu_common import rel_err, split_named, stage_tol, to_t
    from multimodalsignal_amd.runtime import Engine
    params, x = WL.eval_case()
    B, C, T = x.shape
    K = params["classifier.3.weight"].shape[0]
    ref = oracle_stages64(params, x, training=False)["logits"]
    p32, b32 = split_named(to_t(params))
    with torch.no_grad():
        st32, _ = O.forward(p32, {**O.init_buffers(), **b32}, torch.as_tensor(x), training=False)
    own = rel_err(st32["logits"].numpy(), ref)
    assert own <= OWN_CAP, own
    eng = Engine(C, K, dev)
    eng.load_named({k: torch.as_tensor(v) for k, v in params.items()})
    before, count = eng.bn_state.clone(), eng.bn_count.clone()
    assert float(before[:16].abs().min()) == 3.0 and float(before[16:32].min()) == pytest.approx(1e-3)      # the statistics did load
    eng.forward(torch.as_tensor(x).to(dev), None, training=False)
    torch.cuda.synchronize()
    got = eng.region("LOGITS", torch.float32, (B, K)).cpu().numpy()
    err, tol = rel_err(got, ref), stage_tol("logits", own)
    print(f"eval logits err={err:.3e} tol={tol:.1e} own={own:.2e}")
    assert np.isfinite(got).all() and err <= tol, (err, tol, own)
    assert torch.equal(before, eng.bn_state) and torch.equal(count, eng.bn_count)


@pytest.mark.parametrize("B,C,T,training,mseed", WL.XGRAD_CASES, ids=[f"{c[2]}-{'train' if c[3] else 'eval'}" for c in WL.XGRAD_CASES])
def test_input_gradient_at_unaligned_multi_item_lengths(B, C, T, training, mseed, dev):
    """dL/dx and every parameter gradient through CnnGruAttentionModel and autograd, by tests/test_input_grad_gpu.py's comparison,
    where conv1_bwd_dx runs more than one item per window: position-wise staging with the scalar store (1027) and with the pair
    store (1028), quads with the scalar store (1031); 1027 in eval mode too."""
    import test_input_grad_gpu as IG
    K = WL.xgrad_classes(C, B)
    m = IG._model(C, K, "full", 0.5, dev, seed=mseed)
    m = m.train() if training else m.eval()
    m.set_dropout_seed(1000 + C)
    named, x, y = WL.module_case("cnn_gru_attention", B, C, K, T, mseed, 10 * C + B)
    for k, v in m.state_dict().items():
        assert torch.equal(v.cpu(), named[k]), k                      # the model the host file judged
    xd = x.to(dev).requires_grad_(True)
    torch.nn.CrossEntropyLoss()(m(xd), y.to(dev)).backward()
    torch.cuda.synchronize()
    assert xd.grad is not None and xd.grad.shape == x.shape and bool(torch.isfinite(xd.grad).all()) and float(xd.grad.abs().max()) > 0
    fw = dict(dropout_p=0.5, seed=1000 + C, step=1) if training else dict(dropout_p=0.0, seed=0, step=0)
    IG._check_against_oracle(m, named, x, y, xd.grad.cpu().numpy(), training, fw)


def test_cnn_gru_kind_at_an_unaligned_multi_chunk_length_against_oracle(dev, monkeypatch):
    """The cnn_gru kind (conv1_fwd_kernel<CT, false>: ungated taps) at T = 1027 through test_channel_class_range_gpu's helper for that
    kind: stages, loss, every gradient and dL/dx."""
    import test_channel_class_range_gpu as RC
    RC.test_cnn_gru_kind_against_oracle(*WL.CNN_GRU_CASE, dev, monkeypatch)


# ---- the plain window gather at window_floats % 4 != 0 ----------------------------------------------------------------------------------
GATHER_ROWS = [[3, 6, 3, 0, 5], [1, 1, 2, 6, 4]]
POISON = 0x7FC12345                                                   # a NaN payload no copy produces


def _store(C, T, dev):
    rs = np.random.RandomState(C * 10000 + T)
    x = rs.randn(7, C, T).astype(np.float32)
    x[0, 0, :3] = [-0.0, np.float32(1e-42), -np.inf]                   # bits a copy keeps and arithmetic may not
    return torch.as_tensor(x).to(dev), torch.as_tensor(rs.randint(0, 4, size=7).astype(np.int64)).to(dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("C,T", [(3, 251), (6, 251), (1, 4099)])
def test_plain_gather_copies_unaligned_windows_bit_for_bit(C, T, dev):
    """window_floats % 4 = 1, 2, 3: rows and labels of msig_gather_windows equal store.index_select bit for bit, with a repeated
    index, into an output that starts 4 bytes off a 16-byte boundary; the poisoned elements before and behind the output survive."""
    from multimodalsignal_amd import _lib as L
    W = C * T
    assert W % 4 == {(3, 251): 1, (6, 251): 2, (1, 4099): 3}[C, T]
    store, labels = _store(C, T, dev)
    idx = torch.tensor(GATHER_ROWS[0], device=dev)
    B = len(GATHER_ROWS[0])
    buf = torch.full((B * W + 9,), POISON, dtype=torch.int32, device=dev).view(torch.float32)
    out = buf[1:1 + B * W]
    oy = torch.full((B + 1,), -7, dtype=torch.int64, device=dev)
    assert out.data_ptr() % 16 == 4
    st = Ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L.check(L.lib().msig_gather_windows(store.data_ptr(), labels.data_ptr(), idx.data_ptr(), B, W, out.data_ptr(), oy.data_ptr(), st),
            "msig_gather_windows")
    torch.cuda.synchronize()
    assert torch.equal(_bits(out).view(B, C, T), _bits(store.index_select(0, idx)))
    assert torch.equal(oy[:B], labels.index_select(0, idx)) and int(oy[B]) == -7
    guard = _bits(buf)
    assert int(guard[0]) == POISON and bool((guard[1 + B * W:] == POISON).all())


@pytest.mark.parametrize("C,T", [(3, 251), (6, 251), (1, 4099)])
def test_plain_gather_fold_batch_copies_unaligned_windows_bit_for_bit(C, T, dev):
    """msig_gather_windows_multi over two folds in arenas [2, 0] of three, idx rows further apart than B: each arena's x / y are
    index_select's bits; every other byte of the arenas keeps the pattern it had."""
    from multimodalsignal_amd import _lib as L
    W, B, slots, row_stride = C * T, len(GATHER_ROWS[0]), [2, 0], 9
    store, labels = _store(C, T, dev)
    idx = torch.full((2, row_stride), 10 ** 6, dtype=torch.int64, device=dev)          # the padding is never read
    for z, r in enumerate(GATHER_ROWS):
        idx[z, :B] = torch.tensor(r, device=dev)
    xbytes, x_off = B * W * 4, 512
    y_off = (x_off + xbytes + 256 + 255) // 256 * 256
    stride = (y_off + 8 * B + 256 + 255) // 256 * 256
    mem = torch.full((3, stride), 0xAB, dtype=torch.uint8, device=dev)
    before = mem.clone()
    m = L.Multi()
    m.n, m.stride_bytes = 2, stride
    for z, s in enumerate(slots):
        m.slot[z] = s
    st = Ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L.check(L.lib().msig_gather_windows_multi(store.data_ptr(), labels.data_ptr(), idx.data_ptr(), row_stride, B, W, mem.data_ptr() + x_off,
                                              mem.data_ptr() + y_off, Ct.byref(m), st), "msig_gather_windows_multi")
    torch.cuda.synchronize()
    touched = torch.zeros_like(mem, dtype=torch.bool)
    for z, s in enumerate(slots):
        rows = torch.tensor(GATHER_ROWS[z], device=dev)
        assert torch.equal(mem[s, x_off:x_off + xbytes].view(torch.int32), _bits(store.index_select(0, rows)).flatten()), z
        assert torch.equal(mem[s, y_off:y_off + 8 * B].view(torch.int64), labels.index_select(0, rows)), z
        touched[s, x_off:x_off + xbytes] = True
        touched[s, y_off:y_off + 8 * B] = True
    assert torch.equal(mem[~touched], before[~touched])


def test_drivers_train_on_windows_whose_float_count_is_no_multiple_of_four(tmp_path, dev):
    """Six channels at 251 samples (C * T % 4 == 2): three folds, two epochs, dropout on — the fold batch
    (msig_gather_windows_multi) gives the sequential loop's (msig_gather_windows) history, final parameters and test metrics bit
    for bit, as test_augment_gpu.test_lockstep_equals_sequential_with_augmentation compares them."""
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.dataset import SubjectStore
    from multimodalsignal_amd.multifold import LockstepTrainer, lockstep_compatible
    from multimodalsignal_amd.synth import make_synthetic_wesad, CHANNELS6
    from test_augment_gpu import _fold_numbers
    subs = ["S2", "S3", "S4"]
    d = make_synthetic_wesad(tmp_path / "w", subjects=subs, windows_per_subject=20, T=251, difficulty=4.0)
    names = (d / "_channel_names.txt").read_text().split()
    out = {}
    for mode in ("seq", "lock"):
        base = M.default_cfg()
        base.update(data_path=d, channels=list(CHANNELS6), subjects=subs, epochs=2, patience=20, batch_size=16)
        store = SubjectStore(d, subs, base["channels"], names, classification_mode=base["mode"], device=dev)
        preps = [M.prepare_fold(k, subs[k], tmp_path / mode, dev, names, base, store) for k in range(3)]
        assert all(tuple(p["loaders"][0].store.shape[1:]) == (6, 251) for p in preps)
        if mode == "seq":
            infos = [M.train_fold(p, dev) for p in preps]
        else:
            assert lockstep_compatible(preps)
            infos = LockstepTrainer(preps, dev).run()
        torch.cuda.synchronize(dev)
        out[mode] = _fold_numbers(infos, preps)
    (h_s, m_s, w_s), (h_l, m_l, w_l) = out["seq"], out["lock"]
    assert h_s == h_l and m_s == m_l
    assert all(len(h) == 2 and all(np.isfinite(e["train_loss"]) for e in h) for h in h_s)
    for a, b in zip(w_s, w_l):
        for k in a:
            assert torch.equal(a[k], b[k]), k
