"""The cases of tests/golden/gru_forms.npz: every GRU kernel form at the smallest shapes at which a weight-fragment prologue or a rung
of the forward launcher can go wrong — shared by tests/golden/make_gru_forms_golden.py (which records them once, from the library as
it was before the GRU prologues, the forward launch ladder and the stamp report each became one piece of source) and
tests/test_gru_forms_golden_gpu.py (which compares bits).  Nothing here is imported by the product.

Recorded per output tensor: the SHA-256 of its bytes and its first 64 elements as integers of the element's width.

Shapes.  C = 3, K = 3, dropout 0.5 under one fixed key.  The window lengths T give StageDims.TP = 1, 5, 6, 7 recurrent steps: the
one-step recurrence, every remainder of the depth-3 prefetch rotations of gru_fwd_ws / gru_fwd_rec, odd and even step counts of
gru_bwd_b3's two-step dW pairing.  B = 17 is two batch tiles, the second with one live row; B = 40 three tiles, the last ragged.
Every form set meets all four step counts and both batch sizes: the batch size of a (form, step count) pair alternates."""
import ctypes as C
import functools
import hashlib

import numpy as np

CH, K, P = 3, 3, 0.5
SEED, STEP = 7, 2                                     # the fixed dropout key: dropout_key(SEED, STEP, .)
T_OF_TP = {1: 16, 5: 80, 6: 96, 7: 112}
BATCHES = (17, 40)
FORMS = {"ws6": ("ws", "b6"), "split": ("split", "split"), "ws": ("ws", "b4"), "ws5": ("ws", "b5"), "b3": ("b3", "b3"),
         "fp32": ("fp32", "b3"), "auto": ("auto", "auto")}      # tests/test_parity_gpu.py FORMS, and the library's own choice
FWD_FORMS = ("split", "ws", "b3", "fp32", "auto")     # one forward without keeping (STASH = false) each
FOLD_FORMS = (("ws", "b4"), ("ws", "b5"), ("ws", "b6"), ("ws", "b3"), ("split", "split"), ("auto", "auto"))
NF, FOLD_B, FOLD_TP = 3, 16, 5                        # the FOLDS = true instantiations: three folds of one tile
ONE_LAYER_FORMS = ("split", "ws6")
MANY = dict(B=3100, C=6, K=2, T=64)                   # 194 tiles: the >= 192-tile selection, no GI region in the workspace
LR, WD = 1e-3, 1e-4


def batch_of(form, tp):
    return BATCHES[(list(FORMS).index(form) + list(T_OF_TP).index(tp)) % 2]


def record(t):
    """A device tensor -> (sha256 digest as 32 uint8, first 64 elements as same-width integers)."""
    a = t.detach().contiguous().cpu().numpy()
    flat = a.reshape(-1).view({1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize])
    return np.frombuffer(hashlib.sha256(flat.tobytes()).digest(), dtype=np.uint8).copy(), flat[:64].copy()


@functools.lru_cache(maxsize=None)
def _params(Cc, Kk, seed):
    from oracle import cnn_gru_oracle as O
    return {k: v.clone() for k, v in O.init_params(Cc, Kk, seed=seed).items()}


def _batch(torch, dev, B, Cc, Kk, T, seed):
    rs = np.random.RandomState(seed)
    x = (rs.randn(B, Cc, T) * (0.5 + rs.rand(1, Cc, 1)) + 0.3 * rs.randn(1, Cc, 1)).astype(np.float32)
    y = rs.randint(0, Kk, size=B).astype(np.int64)
    return torch.as_tensor(x).to(dev), torch.as_tensor(y).to(dev)


def _engine(dev, Cc=CH, Kk=K, seed=11):
    from multimodalsignal_amd.runtime import Engine
    e = Engine(Cc, Kk, dev)
    e.load_named(_params(Cc, Kk, seed))
    return e


def _tp(T):
    from oracle import cnn_gru_oracle as O
    return O.stage_lengths(T)[3]


def _gru_regions(torch, e, B, T, backward, two_layers=True, key=None):
    """What the GRU launches of the last call (or of the workspace `key`) wrote, as far as the binding reads it.  The one-layer model
    leaves H1 unwritten and DH0 written at its last position only."""
    TP = _tp(T)
    out = {"H0": e.region("H0", shape=(B, TP, 128), key=key), "FEAT": e.region("FEAT", shape=(B, 128), key=key)}
    if two_layers:
        out["H1"] = e.region("H1", shape=(B, TP, 64), key=key)
    if backward:
        out["DX0"] = e.region("DX0", shape=(2, B, TP, 32), key=key)
        if two_layers:
            out["DH0"] = e.region("DH0", shape=(B, TP, 128), key=key)
    return out


def _pinned(L, forms):
    class Pin:
        def __enter__(self):
            L.set_kernel_form(*forms)

        def __exit__(self, *exc):
            L.set_kernel_form("auto", "auto")
    return Pin()


def separate_case(L, torch, dev, forms, B, T, Cc=CH, Kk=K, layers=2):
    """msig_forward (training, dropout) and msig_backward as two calls: the three-vector stash under every form."""
    e = _engine(dev, Cc, Kk)
    e.gru_layers = layers
    x, y = _batch(torch, dev, B, Cc, Kk, T, 1000 * B + T)
    with _pinned(L, forms):
        b = e.forward(x, y, training=True, dropout_p=P, seed=SEED, step=STEP)
        e.backward(b)
    torch.cuda.synchronize()
    out = _gru_regions(torch, e, B, T, True, layers == 2)
    out["grads"] = e.grads
    return {k: record(v) for k, v in out.items()}


def fused_case(L, torch, dev, forms, B, T):
    """One msig_train_step: under ("ws", "b6") the forward stores r, z only (stash_skip_hn = 1) and gru_bwd_b6 recomputes W_hn h."""
    e = _engine(dev)
    x, y = _batch(torch, dev, B, CH, K, T, 1000 * B + T)
    with _pinned(L, forms):
        e.train_step(x, y, LR, weight_decay=WD, step=STEP, dropout_p=P, seed=SEED)
    torch.cuda.synchronize()
    return {"params": record(e.params), "loss": record(e.region("LOSS")[:3])}


def eval_case(L, torch, dev, fwd, B, T):
    """An evaluation forward that keeps nothing: the STASH = false instantiations."""
    e = _engine(dev)
    x, y = _batch(torch, dev, B, CH, K, T, 1000 * B + T)
    with _pinned(L, (fwd, "auto")):
        e.forward(x, y, training=False)
    torch.cuda.synchronize()
    out = _gru_regions(torch, e, B, T, False)
    out["LOGITS"] = e.region("LOGITS", shape=(B, K))
    return {k: record(v) for k, v in out.items()}


def fold_case(L, torch, dev, forms):
    """One msig_train_step_multi of NF folds with their own weights, inputs and dropout keys: blockIdx.z = fold."""
    from multimodalsignal_amd.runtime import FoldArena
    B, T = FOLD_B, T_OF_TP[FOLD_TP]
    with _pinned(L, forms):
        arena = FoldArena(CH, K, dev, NF, B, T)
        engines = [arena.engine(f) for f in range(NF)]     # once: building a fold's engine zeroes its buffers
        for f, e in enumerate(engines):
            e.load_named(_params(CH, K, 20 + f))
            e.workspace(B, T, True)                        # the layout region() reads by, before anything is written
            x, y = _batch(torch, dev, B, CH, K, T, 50 + f)
            arena.view(f, "x", torch.float32)[:x.numel()].copy_(x.reshape(-1))
            arena.view(f, "y", torch.int64)[:B].copy_(y)
        m = arena.multi(list(range(NF)), key_gru=[L.dropout_key(100 + f, STEP, 1) for f in range(NF)],
                        key_head=[L.dropout_key(100 + f, STEP, 2) for f in range(NF)], lr=[LR] * NF, steps=[STEP] * NF)
        desc = arena.batch(B, True, P)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        L.check(L.lib().msig_train_step_multi(C.byref(desc), C.byref(m), arena.ptr("exp_avg"), arena.ptr("exp_avg_sq"),
                                              0.9, 0.999, 1e-8, WD, STEP, st), "msig_train_step_multi")
    torch.cuda.synchronize()
    out = {}
    for f, e in enumerate(engines):
        for k, v in _gru_regions(torch, e, B, T, True, key=(B, T, True)).items():
            out[f"fold{f}.{k}"] = record(v)
        for k in ("params", "grads", "acc"):
            out[f"fold{f}.{k}"] = record(arena.view(f, k))
    return out


def all_cases():
    """(key, callable(L, torch, dev) -> {output: (sha, head)}) for every case."""
    cases = []
    for form, forms in FORMS.items():
        for tp, T in T_OF_TP.items():
            B = batch_of(form, tp)
            cases.append((f"separate/{form}/tp{tp}_b{B}", lambda L, t, d, fo=forms, B=B, T=T: separate_case(L, t, d, fo, B, T)))
    for tp, T in T_OF_TP.items():
        B = batch_of("ws6", tp)
        cases.append((f"fused/ws6/tp{tp}_b{B}", lambda L, t, d, B=B, T=T: fused_case(L, t, d, FORMS["ws6"], B, T)))
    for fwd in FWD_FORMS:
        cases.append((f"eval/{fwd}", lambda L, t, d, fwd=fwd: eval_case(L, t, d, fwd, 17, T_OF_TP[5])))
    for forms in FOLD_FORMS:
        cases.append((f"folds/{forms[0]}_{forms[1]}", lambda L, t, d, fo=forms: fold_case(L, t, d, fo)))
    for form in ONE_LAYER_FORMS:
        cases.append((f"one_layer/{form}", lambda L, t, d, fo=FORMS[form]: separate_case(L, t, d, fo, 17, T_OF_TP[6], layers=1)))
    cases.append(("many_tiles/auto", lambda L, t, d: separate_case(L, t, d, FORMS["auto"], MANY["B"], MANY["T"], MANY["C"], MANY["K"])))
    return cases
