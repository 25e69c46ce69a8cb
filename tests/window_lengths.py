"""Window lengths for the parity tests (tests/test_window_lengths_host.py, tests/test_window_lengths_gpu.py; DESIGN.md "Window lengths").

The front-end kernels branch on the window length T more than on anything else (csrc/frontend.hip):
  gate_kernel, stage_x_chunk   T % 4 == 0: 16-byte loads, whole-vector zero padding      | sample by sample, scalar clamp and padding
  conv1_fwd_kernel<CT>, C <= 8 T % 4 == 0: register-prefetch pipeline                    | stage_x_chunk<true> + per-item weight staging
  conv1_bwd_kernel<CT>, C <= 8 T % 8 == 0 && 2 P1 == L1 && L1 >= 8: quad prefetch        | stage_x_chunk<false> + routed_load per position
  conv1_bwd_dx_kernel          L1 % 4 == 0: quads;  T % 2 == 0: float2 store             | position-wise staging; scalar store, t + 1 < T guard
and they walk a window in chunks: conv1 forward, backward and backward-dx 256 positions of L1, conv2 forward and backward 128 of L2;
with B < 256 conv1_bwd cuts a window into SEG segments of CPS = ceil(nchunk / 8) chunks.  Every other parity test with T % 4 != 0 has
L1 <= 256 (one chunk), every multi-chunk T is a multiple of 8, and T % 8 == 4 occurs nowhere.  paths() restates the kernels' predicates;
the tables below are the ONE place that fixes shapes and seeds.  The host file proves from the oracle alone that every case is
well-conditioned (`own` <= OWN_CAP, few fp32 / fp64 pooling disagreements, a live gate MLP) and that the tables reach every path; the
GPU file holds the HIP path to the project's unchanged tolerances on exactly those cases.  Nothing here is imported by the product.

Inputs are the usual ones: oracle.init_params(C, K, seed) and unit-scale noise with a per-channel spread and offset, as
tests/test_parity_gpu.py::test_random_shapes_with_dropout draws them."""
from collections import namedtuple

import numpy as np
import torch

from oracle import cnn_gru_oracle as O

Paths = namedtuple("Paths", "x_vec fwd_pipe bwd_pipe dx_quads dx_pair_store n1 n2 cps seg")


def paths(B, C, T):
    """The kernels' own predicates on (B, C, T), from O.stage_lengths(T) = (L1, P1, L2, T')."""
    L1, P1, L2, _ = O.stage_lengths(T)
    x_vec = T % 4 == 0
    n1, n2 = -(-L1 // 256), -(-L2 // 128)
    cps = n1 if B >= 256 else (n1 + 7) // 8                       # conv1_bwd_cps
    return Paths(x_vec=x_vec, fwd_pipe=C <= 8 and x_vec, bwd_pipe=C <= 8 and T % 8 == 0 and 2 * P1 == L1 and L1 >= 8,
                 dx_quads=L1 % 4 == 0, dx_pair_store=T % 2 == 0, n1=n1, n2=n2, cps=cps, seg=-(-n1 // cps))   # conv1_bwd_segs


def base_input(B, C, K, T, xseed):
    rs = np.random.RandomState(xseed)
    x = (rs.randn(B, C, T) * (0.5 + rs.rand(1, C, 1)) + rs.randn(1, C, 1)).astype(np.float32)
    y = rs.randint(0, K, size=(B,)).astype(np.int64)
    return x, y


# ---- seeds ---------------------------------------------------------------------------------------------------------------------------
# oracle.init_params seed: at C = 6 the gate MLP's one hidden unit is dead under most seeds; 82 can be live (test_trained_regimes_gpu).
# Whether it is live also depends on the inputs' per-channel offsets (its pre-activation is W1 . mean_t x), i.e. on the input seed:
# the default is 7 B + T as everywhere; XSEED holds the (B, C, T) at which that default leaves the unit dead for every window (both
# channel_attention gradients exactly zero), found with tests/test_window_lengths_host.py and frozen here.
def pseed(C):
    return 82 if C == 6 else 100 + C


XSEED = {(2, 6, 513): 4527, (2, 6, 1020): 2034, (2, 6, 1023): 5037, (2, 9, 1027): 2041, (3, 6, 274): 1295, (3, 6, 275): 2296,
         (3, 6, 276): 1297, (3, 6, 279): 2300, (3, 6, 282): 1303, (3, 6, 284): 1305, (3, 6, 285): 2306, (3, 6, 287): 1308,
         (3, 9, 276): 1297,      # the first of 7 B + T + 1000 k that is live
         (3, 6, 277): 2298,      # 298: live, but `own` of channel_attention.fc.0.weight is 2.5e-5 in the oracle itself; 1298 dead
         # live under the default, but with pre-activations at ReLU's kink (gate_kink below): at (2, 6, 1027) they are 0.0022 and 0.0050,
         # sums of terms of order 1, and the bound on dW2 is 9.5e-5 (the HIP path's dW2 was 2.2e-5 off there, every other stage and
         # gradient within 1.1e-6); at (257, 6, 1027) the bound is 3.7e-6 and 4.2e-6 under 2826 and 3826, 4826 and 5826 are dead
         (2, 6, 1027): 2041, (257, 6, 1027): 6826}


def xseed(B, C, T):
    return XSEED.get((B, C, T), 7 * B + T)


Case = namedtuple("Case", "B C K T p form pseed xseed")


def _case(B, C, T, K=2, p=0.5, form="auto"):
    return Case(B, C, K, T, p, form, pseed(C), xseed(B, C, T))


def case_id(c):
    return f"{c.B}-{c.C}-{c.K}-{c.T}-{c.form}"


def build_case(c):
    """(params, x, y) of a Case."""
    params = {k: v.numpy() for k, v in O.init_params(c.C, c.K, seed=c.pseed).items()}
    x, y = base_input(c.B, c.C, c.K, c.T, c.xseed)
    return params, x, y


# ---- the frozen case tables ----------------------------------------------------------------------------------------------------------
FW = dict(seed=1234, step=3)          # the dropout stream of the stage cases, as test_random_shapes_with_dropout has it

# every residue T % 16 inside ONE conv1 chunk (L1 = 136 .. 144): B = 3, C = 6; the generic CT == 0 instantiation (C = 9) at an odd T
# and at T % 8 == 4, C = 2 (no gate MLP) at T % 4 == 3 and T % 4 == 2
RESIDUES = ([_case(3, 6, 272 + r) for r in range(16)] + [_case(3, 9, 272 + r) for r in (1, 4)] + [_case(3, 2, 272 + r) for r in (3, 6)])

# chunk crossings (L1, P1, L2, T' from O.stage_lengths; the host file asserts them)
CROSSING_LENGTHS = {513: (257, 129, 65, 33),          # a second conv1 chunk of one position
                    516: (258, 129, 65, 33),          # T % 8 == 4
                    1020: (510, 255, 128, 64),        # T % 8 == 4, exactly one conv2 chunk
                    1023: (512, 256, 128, 64),        # odd
                    1025: (513, 257, 129, 65),        # a third conv1 chunk of one position, a second conv2 chunk of one position
                    1027: (514, 257, 129, 65),
                    1028: (514, 257, 129, 65),        # T % 8 == 4
                    1030: (515, 258, 129, 65),        # T % 4 == 2
                    2100: (1050, 525, 263, 132),      # five conv1 chunks, three conv2 chunks: SEG = 5, CPS = 1
                    4100: (2050, 1025, 513, 257),     # T % 8 == 4, nine chunks: CPS = 2, SEG = 5, the last segment one chunk of two positions
                    4099: (2050, 1025, 513, 257)}     # the same, odd
CROSSINGS = ([_case(2, 6, T) for T in (513, 516, 1020, 1023, 1025, 1027)] + [_case(2, 9, 1027), _case(2, 3, 1028), _case(2, 6, 1030),
             _case(2, 3, 2100), _case(2, 2, 4100), _case(2, 3, 4099),
             _case(256, 3, 516), _case(257, 6, 1027)])      # whole-window conv1_bwd items (B >= 256: CPS = nchunk); 257: a ragged last batch tile

# short GRU sequences: B = 33 (three batch tiles, the last with one row), C = 3, K = 3, both shipped form sets; T' = 2, 5, 6, 7, 8
SHORT_T = {30: 2, 75: 5, 93: 6, 110: 7, 125: 8}
SHORT = [_case(33, 3, T, K=3, form=f) for T in SHORT_T for f in ("ws6", "split")]

# one msig_train_step_multi over three folds: (init_params seed, input seed, dropout seed) per fold
FOLD_SHAPE, FOLD_STEP = (5, 6, 2, 1027, 0.5), 2
FOLD_CASES = [(82, 1060, 1000), (82, 1064, 1001), (82, 1067, 1002)]

# Engine.forward(training=False) with foreign running statistics: B, C, K, T, init_params seed, input seed
EVAL_CASE = (5, 6, 2, 1027, 82, 1060)

# dL/dx through CnnGruAttentionModel and autograd: B, C, T, training, torch.manual_seed of the model (nn's initialisation, as
# tests/test_input_grad_gpu.py builds it); the input seed is 10 C + B as there
XGRAD_CASES = [(3, 6, 1027, True, 9),        # odd: scalar store, position-wise staging, three dx items
               (3, 6, 1028, True, 9),        # pair store, position-wise staging, multi-item
               (3, 6, 1031, True, 11),       # L1 = 516: quads with an odd T (model seeds 9 and 10: the gate MLP is dead on this input)
               (3, 6, 1027, False, 9)]
CNN_GRU_CASE = (3, 6, 2, 1027)               # B, C, K, T: test_channel_class_range_gpu's helper of the ungated kind


def fold_case(f):
    B, C, K, T, p = FOLD_SHAPE
    ps, xs, seed = FOLD_CASES[f]
    params = {k: v.numpy() for k, v in O.init_params(C, K, seed=ps).items()}
    x, y = base_input(B, C, K, T, xs)
    return params, x, y, seed


def eval_case():
    """(params with foreign running statistics, x): means of +-3, variances of 1e-3, 1 and 50, drawn as
    tests/test_input_regimes_host.py::eval_case draws them."""
    B, C, K, T, ps, xs = EVAL_CASE
    params = {k: v.numpy() for k, v in O.init_params(C, K, seed=ps).items()}
    x, _ = base_input(B, C, K, T, xs)
    rs = np.random.RandomState(7)
    for idx, ch in ((1, 16), (5, 32)):
        params[f"cnn_encoder.{idx}.running_mean"] = rs.choice([-3.0, 3.0], size=ch).astype(np.float32)
        params[f"cnn_encoder.{idx}.running_var"] = rs.choice([1e-3, 1.0, 50.0], size=ch).astype(np.float32)
    return params, x


def module_case(kind, B, C, K, T, model_seed, xs):
    """(state_dict as the oracle reads it, x, y) of a case that runs through the nn.Modules: nn's initialisation under
    torch.manual_seed(model_seed), running statistics included (the eval-mode input-gradient case runs on means of 0 and variances of
    1: under eval_case's foreign statistics `own` of its weight gradients is 1.2e-5 .. 7.6e-5 in the oracle itself, model seeds 9 .. 19)."""
    from multimodalsignal_amd.models import CnnGruAttentionModel, CnnGruModel
    torch.manual_seed(model_seed)
    m = (CnnGruAttentionModel(C, K, dropout=0.5) if kind == "cnn_gru_attention" else CnnGruModel(C, K))
    named = {k: v.detach().clone() for k, v in m.state_dict().items()}
    if kind == "cnn_gru":
        named["channel_attention.fc.0.weight"], named["channel_attention.fc.2.weight"] = torch.zeros(0, C), torch.zeros(C, 0)
    x, y = base_input(B, C, K, T, xs)
    return named, torch.as_tensor(x), torch.as_tensor(y)


# ---- the gate MLP's ReLU kink ---------------------------------------------------------------------------------------------------------
# The hidden pre-activation a[b, j] = sum_c W1[j, c] mean_t x[b, c] is a sum of terms of order 1 that can cancel to almost nothing, and
# dW2[c, j] = sum_b (ds s (1 - s))[b, c] relu(a[b, j]) is LINEAR in it: any fp32 evaluation of a (a mean over T samples, C products,
# C - 1 additions) is off by about 2 u sum_c |W1[j, c] mean[b, c]|, u = 2^-24, and dW2 inherits that absolute error — two correct fp32
# implementations then disagree by more than the gradient tolerance although every `own` is small (the fp32 ORACLE's error in a is
# one draw of that rounding, not its size).  A case is well-conditioned here when that first-order bound moves dW2 by at most half of
# gpu_common.GRAD_FLOOR relative to its largest element, and when no a[b, j] is within the bound of zero (its sign decides dW1).
KINK_U = 2.0 ** -24
KINK_MAX = 3e-6


def gate_kink(named, st64, ds64=None):
    """(relative first-order error bound of dW2 from rounding the pre-activations — with ds64 = dL/d gate_s, else the plain condition
    number max sum |terms| / |a| times 2 u, which bounds it for any ds —, smallest |a| / bound over windows and units)."""
    W1 = np.abs(np.asarray(named["channel_attention.fc.0.weight"], dtype=np.float64))            # (Cr, C)
    mean, pre, s = (np.asarray(st64[k], dtype=np.float64) for k in ("gate_mean", "gate_pre", "gate_s"))
    delta = 2.0 * KINK_U * np.einsum("jc,bc->bj", W1, np.abs(mean))                              # (B, Cr)
    margin = float((np.abs(pre) / delta).min())
    if ds64 is None:
        return float((delta / np.abs(pre)).max()), margin
    dz2 = np.abs(np.asarray(ds64, dtype=np.float64) * s * (1.0 - s))                             # (B, C)
    dW2 = np.einsum("bc,bj->cj", np.asarray(ds64, dtype=np.float64) * s * (1.0 - s), np.maximum(pre, 0.0))
    err = np.einsum("bc,bj->cj", dz2, delta * (pre > -delta))
    return float(err.max() / np.abs(dW2).max()), margin


def xgrad_classes(C, B):
    return 2 + (C + B) % 2
