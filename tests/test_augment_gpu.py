"""Window augmentation inside the training gather (include/msig_aug.h) on the GPU: the kernel against the numpy restatement
(tests/aug_reference.py) bit for bit, switched off against the plain gather, a fold batch against single calls, `Augment.apply` and
`DeviceLoader(augment=...)`, fold batches against the sequential loop, and one driver run with --augment."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import aug_reference as R
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd.augment import Augment

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KEYS = [R.dropout_key(11, s, R.STREAM_ID) for s in (1, 2, 977)]
# (3, 200), (6, 512), (16, 16): odd channel counts, a workgroup of 64 / 128 threads with idle lanes; (2, 1040): two workgroups per
# (row, channel), the second partly filled; (2, 8200): more than 8 x 256 float4 per channel — the strided loop; (1, 64): one channel
SHAPES = [(3, 200), (6, 512), (16, 16), (2, 1040), (2, 8200), (1, 64)]
IDX = [3, 10, 3, 0, 7]          # B = 5 out of 11 windows, window 3 twice


def _configs(T):
    return {"scale": dict(scale=0.3), "jitter": dict(jitter=0.2), "mask_T": dict(mask_prob=0.7, mask_max=T),
            "mask_1": dict(mask_prob=0.7, mask_max=1), "chandrop": dict(chan_drop=0.6),
            "all": dict(scale=0.1, jitter=0.05, mask_prob=0.5, mask_max=max(1, T // 4), chan_drop=0.3)}


def _store(Cn, T, n=11, seed=0):
    rs = np.random.RandomState(seed)
    x = rs.randn(n, Cn, T).astype(np.float32)
    x[3, 0, :5] = -0.0
    x[0, Cn - 1, -3:] = 0.0
    return x, rs.randint(0, 3, size=n).astype(np.int64)


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _gather(store_d, labels_d, idx_d, key, **kw):
    B, (Cn, T) = idx_d.numel(), store_d.shape[1:]
    ox = torch.full((B, Cn, T), float("nan"), device=DEV)
    oy = torch.full((B,), -7, dtype=torch.int64, device=DEV)
    a = Augment(**kw).struct([key])
    L.check(L.lib().msig_aug_gather_windows(store_d.data_ptr(), labels_d.data_ptr(), idx_d.data_ptr(), B, Cn, T, ox.data_ptr(), oy.data_ptr(),
                                            C.byref(a), _stream()), "msig_aug_gather_windows")
    return ox, oy


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(got, want_np):
    return torch.equal(_bits(got.cpu()), _bits(torch.from_numpy(np.ascontiguousarray(want_np))))


@pytest.mark.parametrize("name", ["scale", "jitter", "mask_T", "mask_1", "chandrop", "all"])
@pytest.mark.parametrize("Cn,T", SHAPES)
def test_kernel_equals_the_restatement_bit_for_bit(Cn, T, name):
    kw = _configs(T)[name]
    x, y = _store(Cn, T)
    xd, yd, idx = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), torch.tensor(IDX, device=DEV)
    seen = []
    for key in KEYS:
        ox, oy = _gather(xd, yd, idx, key, **kw)
        want = R.augment(x, IDX, key, **kw)
        assert _same_bits(ox, want), (name, Cn, T, key, float((ox.cpu() - torch.from_numpy(want)).abs().max()))
        assert torch.equal(oy.cpu(), torch.from_numpy(y[IDX]))
        seen.append(ox.cpu())
        if name in ("scale", "jitter", "all"):
            assert not torch.equal(seen[-1][0], seen[-1][2])          # window 3 twice in the batch: the draws are keyed by the row
    if Cn == 1 and name == "chandrop":          # a window's only channel is the one that stays
        assert all(torch.equal(_bits(s), _bits(torch.from_numpy(x[IDX]))) for s in seen)
        return
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    assert not torch.equal(seen[0], torch.from_numpy(x[IDX]))


def test_off_is_the_plain_gather():
    Cn, T = 6, 512
    x, y = _store(Cn, T)
    xd, yd, idx = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), torch.tensor(IDX, device=DEV)
    plain = torch.full((5, Cn, T), float("nan"), device=DEV)
    py = torch.zeros(5, dtype=torch.int64, device=DEV)
    L.check(L.lib().msig_gather_windows(xd.data_ptr(), yd.data_ptr(), idx.data_ptr(), 5, Cn * T, plain.data_ptr(), py.data_ptr(), _stream()), "gather")
    ox, oy = _gather(xd, yd, idx, KEYS[0])
    assert torch.equal(_bits(ox), _bits(plain)) and torch.equal(oy, py)
    assert torch.signbit(ox[0, 0, :5]).all()                      # window 3's -0.0 came through
    # one transform at 0, the other three on: exactly the three (the one is skipped, not run with a neutral value) — and it matters
    full = _configs(T)["all"]
    all4, _ = _gather(xd, yd, idx, KEYS[0], **full)
    for off in (dict(scale=0.0), dict(jitter=0.0), dict(mask_prob=0.0, mask_max=0), dict(chan_drop=0.0)):
        kw = dict(full, **off)
        got, _ = _gather(xd, yd, idx, KEYS[0], **kw)
        assert _same_bits(got, R.augment(x, IDX, KEYS[0], **kw)), off
        assert not torch.equal(_bits(got), _bits(all4)), off
    # scale alone keeps -0.0: the gain is positive at this sigma and nothing is added
    sc, _ = _gather(xd, yd, idx, KEYS[0], scale=0.1)
    assert torch.signbit(sc[0, 0, :5]).all()


def test_fold_batch_equals_single_calls():
    """Three folds in arenas [2, 0, 1] of four, idx rows further apart than B, a key per fold: each arena's x / y are the single
    call's with that fold's key; every other byte of the arenas keeps the pattern it had."""
    Cn, T, B, slots, row_stride = 6, 512, 5, [2, 0, 1], 9
    kw = _configs(T)["all"]
    x, y = _store(Cn, T)
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    rows = [[3, 10, 3, 0, 7], [1, 1, 2, 9, 4], [10, 8, 6, 5, 0]]
    idx = torch.full((3, row_stride), 10 ** 6, dtype=torch.int64, device=DEV)          # the padding is never read
    for z, r in enumerate(rows):
        idx[z, :B] = torch.tensor(r, device=DEV)
    xbytes, x_off = B * Cn * T * 4, 512
    y_off = x_off + xbytes + 256
    stride = (y_off + 8 * B + 256 + 255) // 256 * 256
    mem = torch.full((4, stride), 0xAB, dtype=torch.uint8, device=DEV)
    before = mem.clone()
    m = L.Multi()
    m.n, m.stride_bytes = 3, stride
    for z, s in enumerate(slots):
        m.slot[z] = s
    a = Augment(**kw).struct(KEYS)
    L.check(L.lib().msig_aug_gather_windows_multi(xd.data_ptr(), yd.data_ptr(), idx.data_ptr(), row_stride, B, Cn, T, mem.data_ptr() + x_off,
                                                  mem.data_ptr() + y_off, C.byref(m), C.byref(a), _stream()), "msig_aug_gather_windows_multi")
    touched = torch.zeros_like(mem, dtype=torch.bool)
    for z, s in enumerate(slots):
        one_x, one_y = _gather(xd, yd, torch.tensor(rows[z], device=DEV), KEYS[z], **kw)
        assert torch.equal(mem[s, x_off:x_off + xbytes].view(torch.int32), _bits(one_x).flatten()), z
        assert torch.equal(mem[s, y_off:y_off + 8 * B].view(torch.int64), one_y), z
        assert _same_bits(one_x, R.augment(x, rows[z], KEYS[z], **kw))
        touched[s, x_off:x_off + xbytes] = True
        touched[s, y_off:y_off + 8 * B] = True
    assert torch.equal(mem[~touched], before[~touched])


class _Windows:
    """The least a DeviceLoader needs of a dataset."""

    def __init__(self, x, y):
        self.x, self.labels = torch.from_numpy(x).to(DEV), y
        self.y = torch.from_numpy(y).to(DEV)

    def __len__(self):
        return len(self.labels)

    def device_tensors(self, device):
        return self.x, self.y


def _epoch(loader):
    return [(xb.clone(), yb.clone()) for xb, yb in loader]


def test_apply_equals_the_loaders_batch():
    from multimodalsignal_amd.dataset import DeviceLoader
    x, y = _store(6, 512, n=11)
    ds, aug = _Windows(x, y), Augment(**_configs(512)["all"])
    ld = DeviceLoader(ds, 4, False, DEV, seed=5, augment=aug)
    assert (ld.aug_seed, ld.aug_step) == (5, 0)
    batches = _epoch(ld) + _epoch(ld)                                  # 3 + 3 batches (4, 4, 3 windows): steps 1..6
    assert ld.aug_step == 6
    for k, (xb, yb) in enumerate(batches):
        i = (k % 3) * 4
        src = ds.x[i:i + 4].clone()
        keep = src.clone()
        got = aug.apply(src, 5, k + 1)
        assert torch.equal(_bits(got), _bits(xb)), k
        assert torch.equal(_bits(src), _bits(keep)) and got.data_ptr() != src.data_ptr()
        assert torch.equal(yb.cpu(), torch.from_numpy(y[i:i + 4]))
        assert _same_bits(xb, R.augment(x, list(range(i, min(i + 4, 11))), R.dropout_key(5, k + 1, R.STREAM_ID), **_configs(512)["all"]))
    with pytest.raises(ValueError):
        aug.apply(ds.x[:, :, :510], 5, 1)
    with pytest.raises(ValueError):
        DeviceLoader(ds, 4, True, DEV, seed=5, augment=Augment(mask_prob=0.5, mask_max=513))


def test_loader_determinism():
    from multimodalsignal_amd.dataset import DeviceLoader
    x, y = _store(6, 512, n=11)
    ds, aug = _Windows(x, y), Augment(scale=0.1, jitter=0.05)
    a, b, c = (DeviceLoader(ds, 4, True, DEV, seed=s, augment=aug) for s in (5, 5, 6))
    for _ in range(2):
        ea, eb, ec = _epoch(a), _epoch(b), _epoch(c)
        assert all(torch.equal(_bits(p[0]), _bits(q[0])) and torch.equal(p[1], q[1]) for p, q in zip(ea, eb))
        assert not all(torch.equal(_bits(p[0]), _bits(q[0])) for p, q in zip(ea, ec))
    # the same windows in the same order, an epoch later: other draws
    fixed = DeviceLoader(ds, 4, False, DEV, seed=5, augment=aug)
    e1, e2 = _epoch(fixed), _epoch(fixed)
    assert all(torch.equal(p[1], q[1]) and not torch.equal(p[0], q[0]) for p, q in zip(e1, e2))
    # validation-style loaders are what they were; all four at 0 is no augmentation at all
    for ld in (DeviceLoader(ds, 4, False, DEV), DeviceLoader(ds, 4, False, DEV, augment=None), DeviceLoader(ds, 4, False, DEV, augment=Augment())):
        assert ld.augment is None
        assert torch.equal(_bits(torch.cat([xb for xb, _ in _epoch(ld)])), _bits(ds.x))


def _fold_numbers(infos, preps):
    hist = [[{k: v for k, v in h.items() if k != "seconds"} for h in i["history"]] for i in infos]
    metrics = [(i["subject"], i["accuracy"], i["f1_score"], i["epochs"]) for i in infos]
    weights = [{k: v.detach().cpu().clone() for k, v in p["model"].state_dict().items()} for p in preps]
    return hist, metrics, weights


def test_lockstep_equals_sequential_with_augmentation(tmp_path):
    """Three folds with training sets of unequal size, C = 6, T = 512, B = 16, two epochs, dropout on: the fold batch
    (msig_aug_gather_windows_multi, a key per fold) gives the sequential loop's history, final parameters and test metrics bit for
    bit, with augmentation and without; and augmentation changes the numbers."""
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.dataset import SubjectStore
    from multimodalsignal_amd.multifold import LockstepTrainer, lockstep_compatible
    from multimodalsignal_amd.synth import make_synthetic_wesad, CHANNELS6
    subs = ["S2", "S3", "S4", "S5", "S6"]
    d = make_synthetic_wesad(tmp_path / "w", subjects=subs, windows_per_subject=14, T=512, difficulty=4.0, window_spread=4)
    names = (d / "_channel_names.txt").read_text().split()
    spec = "scale=0.1,jitter=0.05,mask=0.5:64,chandrop=0.1"
    out = {}
    for aug in (spec, None):
        for mode in ("seq", "lock"):
            base = M.default_cfg()
            base.update(data_path=d, channels=list(CHANNELS6), subjects=subs, epochs=2, patience=20, batch_size=16)
            if aug:
                base["augment"] = aug
            store = SubjectStore(d, subs, base["channels"], names, classification_mode=base["mode"], device=DEV)
            preps = [M.prepare_fold(k, subs[k], tmp_path / f"{mode}{bool(aug)}", DEV, names, base, store) for k in range(3)]
            assert all((p["loaders"][0].augment == Augment.parse(spec)) if aug else (p["loaders"][0].augment is None) for p in preps)
            assert all(p["loaders"][i].augment is None for p in preps for i in (1, 2))
            if mode == "seq":
                infos = [M.train_fold(p, DEV) for p in preps]
            else:
                assert lockstep_compatible(preps)
                infos = LockstepTrainer(preps, DEV).run()
            torch.cuda.synchronize(DEV)
            out[aug, mode] = _fold_numbers(infos, preps)
            out[aug, mode, "steps"] = [p["loaders"][0].aug_step for p in preps]
            sizes = [len(p["loaders"][0].dataset) for p in preps]
    assert len(set(sizes)) > 1, sizes
    for aug in (spec, None):
        (h_s, m_s, w_s), (h_l, m_l, w_l) = out[aug, "seq"], out[aug, "lock"]
        assert h_s == h_l and m_s == m_l, aug
        assert out[aug, "seq", "steps"] == out[aug, "lock", "steps"]
        for a, b in zip(w_s, w_l):
            for k in a:
                assert torch.equal(a[k], b[k]), (aug, k)
    assert out[spec, "seq", "steps"] == [2 * (-(-n // 16)) for n in sizes] and out[None, "seq", "steps"] == [0, 0, 0]
    assert [h[0]["train_loss"] for h in out[spec, "seq"][0]] != [h[0]["train_loss"] for h in out[None, "seq"][0]]


def test_folds_of_a_batch_must_share_the_augmentation(tmp_path):
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.dataset import SubjectStore
    from multimodalsignal_amd.multifold import LockstepTrainer
    from multimodalsignal_amd.synth import make_synthetic_wesad, CHANNELS6
    subs = ["S2", "S3", "S4"]
    d = make_synthetic_wesad(tmp_path / "w", subjects=subs, windows_per_subject=8, T=256)
    names = (d / "_channel_names.txt").read_text().split()
    base = M.default_cfg()
    base.update(data_path=d, channels=list(CHANNELS6), subjects=subs, epochs=1, patience=20, batch_size=16)
    store = SubjectStore(d, subs, base["channels"], names, classification_mode=base["mode"], device=DEV)
    preps = [M.prepare_fold(k, subs[k], tmp_path / "r", DEV, names, dict(base, augment=f"scale=0.{k + 1}"), store) for k in range(2)]
    with pytest.raises(ValueError, match="share one augmentation"):
        LockstepTrainer(preps, DEV)


def test_driver_run_with_augment(tmp_path):
    from multimodalsignal_amd import main as M
    subs = ["S2", "S3", "S4", "S5"]
    spec = "scale=0.1,jitter=0.05,mask=0.5:64,chandrop=0.1"
    common = ["--synthetic", str(tmp_path / "w"), "--synthetic-windows", "12", "--samples", "256", "--subjects", *subs, "--epochs", "2",
              "--batch-size", "16"]
    losses = {}
    for tag, extra in (("aug", ["--augment", spec]), ("plain", [])):
        results, _ = M.main(common + extra + ["--out", str(tmp_path / tag)])
        assert [r["subject"] for r in results] == subs
        run = next((tmp_path / tag).glob("*/run_*"))
        txt = (run / "cv_summary.txt").read_text(encoding="utf-8")
        assert (f"AUGMENT: {spec}\n" in txt) == (tag == "aug") and ("AUGMENT" in txt) == (tag == "aug")
        infos = [json.loads((run / f"fold_test_on_{s}" / "fold_result.json").read_text()) for s in subs]
        losses[tag] = [[h["train_loss"] for h in i["history"]] for i in infos]
        assert all(len(l) == 2 and all(np.isfinite(l)) for l in losses[tag])
    assert all(a != p for a, p in zip(losses["aug"], losses["plain"]))
