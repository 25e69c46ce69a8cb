"""The cases of tests/golden/member_stats.npz: inputs regenerated from a fixed numpy seed, and the library calls that turn them into the
recorded outputs — shared by tests/golden/make_member_stats_golden.py (which records them once, from the library as it was before the
three reductions became one) and tests/test_member_stats_golden_gpu.py (which compares bits).  Nothing here is imported by the product."""
import ctypes as C

import numpy as np

N = 7
CASES = ((1, 2), (2, 5), (17, 16), (64, 3), (256, 16))          # (M, K): stacked and window-major
MULTI_CASES = ((3, 2), (3, 5), (3, 16))                         # (M, K): members in arenas SLOTS of N_ARENAS
SLOTS, N_ARENAS = (3, 0, 2), 4
TEMPERATURES = (1.0 / 64.0, 1.0, 4.0, 64.0)
MULTI_TEMPERATURE = 4.0
PAD = 12                                                        # floats of poison between the member blocks of a stack
EN_OUTS = ("mean_p", "std_p", "pred", "entropy", "expected_entropy", "mutual_info", "votes", "member_pred", "disagreement")
MC_OUTS = EN_OUTS[:7]
OPTIONAL_OUTS = EN_OUTS[1:]                                      # every output but mean_p may be NULL
INT_OUTS = ("pred", "votes", "member_pred")


def logits(M, K, n=N):
    """(M, n, K) fp32, member-major.  Window 0 generic; 1 an exact two-way tie for the maximum in every member's row; 2 all members
    equal, with that tie (so the MEAN ties too); 3 member 0 saturated at -80 / +80 (its tempered probabilities underflow to 0 at
    T = 1/64); 4 member 0 at -400 / +400 (exp(-800) is 0 in fp64: the untempered p ln p branch); 5 member m votes for class m % K —
    the votes split as evenly as M and K allow; the rest generic."""
    rs = np.random.RandomState(1000 * M + K)
    lg = (3.0 * rs.randn(n, M, K)).astype(np.float32)
    lg[1, :, 0] = lg[1].max(axis=1) + 1.0
    lg[1, :, 1] = lg[1, :, 0]
    lg[2, :, :] = lg[1, 0, :]
    lg[3, 0, :], lg[3, 0, K - 1] = -80.0, 80.0
    lg[4, 0, :], lg[4, 0, K - 1] = -400.0, 400.0
    lg[5] = (0.25 * rs.randn(M, K)).astype(np.float32)
    lg[5, np.arange(M), np.arange(M) % K] += 5.0
    return np.ascontiguousarray(lg.transpose(1, 0, 2))


def _outputs(torch, dev, names, M, n, K, skip=None):
    o = {}
    for name in names:
        shape = (n, K) if name in ("mean_p", "std_p", "votes") else (n, M) if name == "member_pred" else (n,)
        o[name] = None if name == skip else torch.full(shape, -77, dtype=torch.int32 if name in INT_OUTS else torch.float32, device=dev)
    return o


def _bits(torch, o):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().view(np.int32) for k, v in o.items() if v is not None}


def _ptr(t):
    return None if t is None else t.data_ptr()


def _multi(L, stride_bytes):
    m = L.Multi()
    m.n, m.stride_bytes, m.form_folds = len(SLOTS), stride_bytes, 1
    for z, s in enumerate(SLOTS):
        m.slot[z] = s
    return m


def run(L, torch, dev, M, K, n=N, multi=False, skip=None):
    """Every call of one case: {"mc/<out>", "en/<out>", "kd/<T>"} or, multi, {"en_multi/<out>", "kd_multi"} -> int32 views of what
    the library wrote.  skip: the name of one optional output to pass as NULL (mean_p is never optional)."""
    lib, st = L.lib(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lg, got = logits(M, K, n), {}
    q = torch.full((n, K), -77, dtype=torch.float32, device=dev)
    if multi:
        stride = (n * K * 4 + 255) // 256 * 256
        arenas = torch.full((N_ARENAS, stride // 4), float("nan"), dtype=torch.float32, device=dev)
        for z, s in enumerate(SLOTS):
            arenas[s, :n * K] = torch.as_tensor(lg[z]).reshape(-1).to(dev)
        m = _multi(L, stride)
        o = _outputs(torch, dev, EN_OUTS, M, n, K, skip)
        L.check(lib.msig_en_reduce_multi(arenas.data_ptr(), C.byref(m), n, K, *(_ptr(o[k]) for k in EN_OUTS), st), "msig_en_reduce_multi")
        got.update({f"en_multi/{k}": v for k, v in _bits(torch, o).items()})
        L.check(lib.msig_kd_teacher_multi(arenas.data_ptr(), C.byref(m), n, K, MULTI_TEMPERATURE, q.data_ptr(), st), "msig_kd_teacher_multi")
        got.update({"kd_multi": _bits(torch, {"q": q})["q"]})
        return got
    wide = torch.as_tensor(np.ascontiguousarray(lg.transpose(1, 0, 2)).reshape(n * M, K)).to(dev)
    o = _outputs(torch, dev, MC_OUTS, M, n, K, skip)
    L.check(lib.msig_mc_reduce(wide.data_ptr(), n, M, K, *(_ptr(o[k]) for k in MC_OUTS), st), "msig_mc_reduce")
    got.update({f"mc/{k}": v for k, v in _bits(torch, o).items()})
    stack = torch.full((M, n * K + PAD), float("nan"), dtype=torch.float32, device=dev)
    stack[:, :n * K] = torch.as_tensor(lg).reshape(M, n * K).to(dev)
    o = _outputs(torch, dev, EN_OUTS, M, n, K, skip)
    L.check(lib.msig_en_reduce(stack.data_ptr(), n * K + PAD, M, n, K, *(_ptr(o[k]) for k in EN_OUTS), st), "msig_en_reduce")
    got.update({f"en/{k}": v for k, v in _bits(torch, o).items()})
    if skip is None:
        for T in TEMPERATURES:
            q.fill_(-77)
            L.check(lib.msig_kd_teacher(stack.data_ptr(), n * K + PAD, M, n, K, T, q.data_ptr(), st), "msig_kd_teacher")
            got[f"kd/{T!r}"] = _bits(torch, {"q": q})["q"]
    return got


def case_key(M, K, multi):
    return f"{'slots' if multi else 'stack'}_M{M}_K{K}"


def all_cases():
    return [(M, K, False) for M, K in CASES] + [(M, K, True) for M, K in MULTI_CASES]

