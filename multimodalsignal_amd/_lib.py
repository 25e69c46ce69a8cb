"""ctypes binding of libmsig_hip.so (include/msig.h, include/msig_cw.h, include/msig_cg.h, include/msig_ft.h, include/msig_gc.h,
include/msig_aug.h, include/msig_st.h, include/msig_ab.h, include/msig_at.h, include/msig_mc.h, include/msig_da.h, include/msig_wa.h, include/msig_en.h, include/msig_kd.h, include/msig_sam.h, include/msig_dro.h, include/msig_sc.h, include/msig_nr.h,
include/msig_rec.h, include/msig_lv.h, include/msig_rn.h, include/msig_rd.h).

There is deliberately no fallback: if the shared library is missing the import
of anything that computes raises, and every launcher raises RuntimeError on a
non-zero status.  PyTorch is used only to own device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("MSIG_LIB", _HERE / "libmsig_hip.so"))

# ---- mirrors of the enums in include/msig.h (tests/test_cabi.py checks them against the header)
P_GATE_W1, P_GATE_W2, P_CONV1_W, P_BN1_G, P_BN1_B, P_CONV2_W, P_BN2_G, P_BN2_B, P_GRU = range(9)
P_CLS0_W, P_CLS0_B, P_CLS3_W, P_CLS3_B, NPARAM = P_GRU + 16, P_GRU + 17, P_GRU + 18, P_GRU + 19, P_GRU + 20

WS_NAMES = [
    "GATE_MEAN", "GATE_PRE", "GATE_S", "Y1", "BN1_PART", "BN1_STAT", "P1", "Y2", "BN2_PART", "BN2_STAT", "P2",
    "H0", "H1", "STASH0", "STASH1", "STASH1R", "FEAT", "HID", "LOGITS", "PROBS", "PRED", "LOSS", "DLOGITS",
    "DFEAT", "DH0", "DX0", "DY2", "DP1", "DS", "BNB_PART", "BNB_STAT", "GRAD_PART", "GI", "POOLC1", "POOLC2", "G1W", "GATE_EO",
]
WS = {n: i for i, n in enumerate(WS_NAMES)}
NWS = len(WS_NAMES)
BN_STATE_FLOATS = 96
MAX_C, MAX_K = 16, 16

# state_dict key of every parameter tensor, in msig_param order (== nn.Module.parameters() order)
PARAM_KEYS = (
    ["channel_attention.fc.0.weight", "channel_attention.fc.2.weight", "cnn_encoder.0.weight",
     "cnn_encoder.1.weight", "cnn_encoder.1.bias", "cnn_encoder.4.weight", "cnn_encoder.5.weight",
     "cnn_encoder.5.bias"]
    + [f"gru.{w}_l{layer}{sfx}" for layer in (0, 1) for sfx in ("", "_reverse")
       for w in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    + ["classifier.0.weight", "classifier.0.bias", "classifier.3.weight", "classifier.3.bias"]
)
assert len(PARAM_KEYS) == NPARAM

# Model kinds (main.py --model).  "cnn_gru" is the baseline without ChannelAttention (include/msig_cg.h): the same tensors minus
# the gate's two, which have zero size in its flat layout.
MODEL_KINDS = ("cnn_gru_attention", "cnn_gru")
GATE_KEYS = ("channel_attention.fc.0.weight", "channel_attention.fc.2.weight")


def check_kind(kind: str) -> str:
    if kind not in MODEL_KINDS:
        raise ValueError(f"model kind must be one of {MODEL_KINDS}, got {kind!r}")
    return kind


def param_keys(kind: str = "cnn_gru_attention"):
    """(msig_param index, state_dict key) of every parameter tensor the model kind has, in flat-buffer order."""
    check_kind(kind)
    return [(i, k) for i, k in enumerate(PARAM_KEYS) if kind == "cnn_gru_attention" or k not in GATE_KEYS]

ERRORS = {-1: "MSIG_E_NULL (required pointer is NULL)", -2: "MSIG_E_SHAPE (unsupported B/C/T/K or mode)",
          -3: "MSIG_E_ALIGN (buffer not 16-byte aligned)", -4: "MSIG_E_WORKSPACE (workspace too small)",
          -5: "MSIG_E_FORM (fwd_form / bwd_form is not a kernel form this call can run)"}


class Shape(C.Structure):
    _fields_ = [("B", C.c_int32), ("C", C.c_int32), ("T", C.c_int32), ("K", C.c_int32)]


class Batch(C.Structure):
    _fields_ = [
        ("shape", Shape), ("training", C.c_int32), ("bn_momentum", C.c_float), ("bn_eps", C.c_float),
        ("dropout_thr", C.c_int32), ("key_gru", C.c_uint32), ("key_head", C.c_uint32),
        ("x", C.c_void_p), ("labels", C.c_void_p), ("params", C.c_void_p), ("grads", C.c_void_p),
        ("bn_state", C.c_void_p), ("bn_count", C.c_void_p), ("ws", C.c_void_p), ("ws_bytes", C.c_int64),
        ("gru_layers", C.c_int32), ("fwd_form", C.c_int16), ("bwd_form", C.c_int16),
        ("loss_acc", C.c_void_p),
        ("keep_for_backward", C.c_int32), ("dx", C.c_void_p),          # ABI 5
    ]


MAX_FOLDS = 16
ABI_VERSION = 5       # include/msig.h MSIG_ABI_VERSION
CW_ABI_VERSION = 1    # include/msig_cw.h MSIG_CW_ABI_VERSION (class-weighted CrossEntropy)
CG_ABI_VERSION = 1    # include/msig_cg.h MSIG_CG_ABI_VERSION (the cnn_gru baseline)
FT_ABI_VERSION = 1    # include/msig_ft.h MSIG_FT_ABI_VERSION (window embeddings, classifier-only head epochs)
GC_ABI_VERSION = 1    # include/msig_gc.h MSIG_GC_ABI_VERSION (gradient-norm clipping inside the fused train steps)
AUG_ABI_VERSION = 1   # include/msig_aug.h MSIG_AUG_ABI_VERSION (window augmentation inside the training gather)
AUG_STREAM_ID = 3     # msig_aug.h MSIG_AUG_STREAM_ID: msig_dropout_key's stream of the augmentation keys (1, 2: GRU and head dropout)
ST_ABI_VERSION = 1    # include/msig_st.h MSIG_ST_ABI_VERSION (label smoothing and mixup in the criterion and the training gather)
ST_STREAM_ID = 4      # msig_st.h MSIG_ST_STREAM_ID: msig_dropout_key's stream of the mixup draws
FT_MAX_BATCH, FT_MAX_N = 256, 1 << 24
FT_KINDS = {"cnn_gru_attention": 0, "cnn_gru": 1}      # MSIG_FT_KIND_*
AB_ABI_VERSION = 1    # include/msig_ab.h MSIG_AB_ABI_VERSION (label-free BatchNorm adaptation)
AB_ACC_DOUBLES = 98   # msig_ab.h MSIG_AB_ACC_DOUBLES: fp64 values of one model's accumulator
AB_N1, AB_N2, AB_SUM1, AB_SQ1, AB_SUM2, AB_SQ2 = 0, 1, 2, 18, 34, 66      # msig_ab.h MSIG_AB_*: the accumulator's slots
AT_ABI_VERSION = 1    # include/msig_at.h MSIG_AT_ABI_VERSION (integrated-gradients attribution: path points and their reduction)
AT_MAX_POINTS = 256   # msig_at.h MSIG_AT_MAX_POINTS: path points per window
AT_BASE_ZERO, AT_BASE_CHANNEL, AT_BASE_SHARED, AT_BASE_OWN = range(4)      # msig_at.h MSIG_AT_BASE_*: what the baseline pointer holds
MC_ABI_VERSION = 1    # include/msig_mc.h MSIG_MC_ABI_VERSION (Monte-Carlo dropout: trunk, expand, tail, reduce)
MC_MAX_SAMPLES = 256  # msig_mc.h MSIG_MC_MAX_SAMPLES: stochastic passes per window
MC_KINDS = {"cnn_gru_attention": 0, "cnn_gru": 1}      # MSIG_MC_KIND_*
DA_ABI_VERSION = 1    # include/msig_da.h MSIG_DA_ABI_VERSION (subject-adversarial training: the discriminator's step)
DA_MAX_BATCH = 256    # msig_da.h MSIG_DA_MAX_BATCH: rows of one discriminator step
WA_ABI_VERSION = 1    # include/msig_wa.h MSIG_WA_ABI_VERSION (weight averaging: the shadow's update)
EN_ABI_VERSION = 1    # include/msig_en.h MSIG_EN_ABI_VERSION (deep ensembles: the reduction of the members' logits)
EN_MAX_MEMBERS = 256  # msig_en.h MSIG_EN_MAX_MEMBERS: members of one ensemble
KD_ABI_VERSION = 1    # include/msig_kd.h MSIG_KD_ABI_VERSION (distillation: the teacher table and the train step's distillation term)
KD_MAX_MEMBERS = 256  # msig_kd.h MSIG_KD_MAX_MEMBERS: members of one teacher
KD_MIN_T, KD_MAX_T = 1.0 / 64.0, 64.0      # msig_kd.h: the temperature's range
SAM_ABI_VERSION = 1   # include/msig_sam.h MSIG_SAM_ABI_VERSION (sharpness-aware minimisation: perturbation, restore, the two-pass train step)
SAM_NORM_SUM, SAM_NORM_MAX, SAM_NORM_LAST, SAM_SHARP_SUM, SAM_SHARP_LAST, SAM_STEPS = range(6)      # msig_sam.h: the state's statistics
SAM_NSTAT = 8         # msig_sam.h MSIG_SAM_NSTAT: float64 statistics at the head of a model's SAM state
DRO_ABI_VERSION = 1   # include/msig_dro.h MSIG_DRO_ABI_VERSION (group-DRO: the group weights and the per-row rescale of the train step's gradient)
DRO_MAX_GROUPS = 64   # msig_dro.h MSIG_DRO_MAX_GROUPS: groups of one fold
DRO_MAX_BATCH = 2048  # msig_dro.h MSIG_DRO_MAX_BATCH: rows of one step with the term
DRO_STATS = 3 * DRO_MAX_GROUPS + 2      # msig_dro.h MSIG_DRO_STATS: T_g, W_g, n_g per group, the robust loss's sum, the steps
SC_ABI_VERSION = 1    # include/msig_sc.h MSIG_SC_ABI_VERSION (supervised contrastive loss on the feature inside the train steps)
SC_MAX_BATCH = 2048   # msig_sc.h MSIG_SC_MAX_BATCH: rows of one step with the term
SC_STATS = 4          # msig_sc.h MSIG_SC_STATS: sum of the anchors' losses, anchors, anchors whose nearest row is a positive, steps
SC_POSITIVES = {"class": 0, "cross-subject": 1}      # MSIG_SC_POS_*
NR_ABI_VERSION = 1    # include/msig_nr.h MSIG_NR_ABI_VERSION (per-subject normalisation with the statistics of reference windows)
REC_ABI_VERSION = 1   # include/msig_rec.h MSIG_REC_ABI_VERSION (statistics and normalised window batches straight from a continuous recording)
LV_ABI_VERSION = 1    # include/msig_lv.h MSIG_LV_ABI_VERSION (a pool of sample rings and window batches whose rows come from different sessions)
LV_MAX_SESSIONS = 4096        # MSIG_LV_MAX_SESSIONS
RN_ABI_VERSION = 1    # include/msig_rn.h MSIG_RN_ABI_VERSION (causal running references: a statistics record per window, offline and live)
RN_MAX_K = 4096               # MSIG_RN_MAX_K
RD_ABI_VERSION = 1    # include/msig_rd.h MSIG_RD_ABI_VERSION (the exponentially decayed running reference, offline and live)
GP_ABI_VERSION = 1    # include/msig_gp.h MSIG_GP_ABI_VERSION (gap-tolerant running references: missing samples, offline and live)
GP_EXPANDING, GP_TRAILING, GP_DECAYED = 0, 1, 2      # msig_gp_mode.kind
RS_ABI_VERSION = 1    # include/msig_rs.h MSIG_RS_ABI_VERSION (causal polyphase FIR resampling, offline and in front of the live rings)
RS_MAX_RATIO = 4096           # MSIG_RS_MAX_RATIO: L and M at most
RS_MAX_HALF = 1 << 22         # MSIG_RS_MAX_HALF
MX_ABI_VERSION = 1    # include/msig_mx.h MSIG_MX_ABI_VERSION (mixed-rate streams: a sample rate per column group, offline and live)
MX_MAX_GROUPS = 8             # MSIG_MX_MAX_GROUPS: column groups (streams) of a session at most
RD_MAX_H = 1 << 20            # half-life of a decayed reference in windows at most (the host's limit: the library takes any decay in [0, 1])


class Sc(C.Structure):
    """msig_sc (include/msig_sc.h): the supervised contrastive term of a launch — which rows are positives, the temperature, the
    subject table and the batch's store positions (cross-subject mode), the scratch, the optional statistics, (fold batch) the bytes
    between the folds' grp, scratch and stats, and a weight per fold."""
    _fields_ = [("positives", C.c_int32), ("tau", C.c_float), ("grp", C.c_void_p), ("idx", C.c_void_p), ("idx_row_stride", C.c_int64),
                ("scratch", C.c_void_p), ("stats", C.c_void_p), ("stride_bytes", C.c_int64), ("weight", C.c_float * MAX_FOLDS)]


class Multi(C.Structure):
    """msig_multi (include/msig.h): a fold batch — arenas `stride_bytes` apart, per-fold dropout keys, learning rates and optimiser step counts."""
    _fields_ = [("n", C.c_int32), ("slot", C.c_int32 * MAX_FOLDS), ("stride_bytes", C.c_int64),
                ("key_gru", C.c_uint32 * MAX_FOLDS), ("key_head", C.c_uint32 * MAX_FOLDS), ("lr", C.c_float * MAX_FOLDS),
                ("form_folds", C.c_int32), ("step", C.c_int64 * MAX_FOLDS)]


class GpMode(C.Structure):
    """msig_gp_mode (include/msig_gp.h): the running reference of a gap-tolerant call — kind GP_EXPANDING, GP_TRAILING (K windows) or
    GP_DECAYED (decay = lambda)."""
    _fields_ = [("kind", C.c_int32), ("K", C.c_int32), ("decay", C.c_double)]


class MxGroup(C.Structure):
    """msig_mx_group (include/msig_mx.h): one column group of a mixed-rate session — its ratio (1, 1, 0: the identity), its columns of a
    ring row, its taps' offset into the tap table and its tail inside a session's tail block (offsets in doubles)."""
    _fields_ = [("L", C.c_int32), ("M", C.c_int32), ("half", C.c_int32), ("col0", C.c_int32), ("ncols", C.c_int32), ("reserved", C.c_int32),
                ("h_off", C.c_int64), ("tail_rows", C.c_int64), ("tail_off", C.c_int64)]


class FtHead(C.Structure):
    """msig_ft_head (include/msig_ft.h): consecutive classifier-only train steps on cached features, one launch."""
    _fields_ = [("K", C.c_int32), ("N", C.c_int32), ("n_order", C.c_int32), ("batch", C.c_int32), ("first_step", C.c_int32),
                ("n_steps", C.c_int32), ("dropout_thr", C.c_int32), ("reserved", C.c_int32), ("cls_offset", C.c_int64),
                ("step0", C.c_int64), ("seed", C.c_uint64), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
                ("eps", C.c_float), ("weight_decay", C.c_float), ("reserved_f", C.c_float),
                ("feat", C.c_void_p), ("labels", C.c_void_p), ("order", C.c_void_p), ("params", C.c_void_p), ("exp_avg", C.c_void_p),
                ("exp_avg_sq", C.c_void_p), ("class_weight", C.c_void_p), ("loss_acc", C.c_void_p)]


class FtMulti(C.Structure):
    """msig_ft_multi (include/msig_ft.h): the folds of one head-epoch launch — arenas `stride_bytes` apart, per-fold learning rate,
    first optimiser step count and dropout seed."""
    _fields_ = [("n", C.c_int32), ("slot", C.c_int32 * MAX_FOLDS), ("reserved", C.c_int32), ("stride_bytes", C.c_int64),
                ("lr", C.c_float * MAX_FOLDS), ("step0", C.c_int64 * MAX_FOLDS), ("seed", C.c_uint64 * MAX_FOLDS)]


GC_KINDS = {"cnn_gru_attention": 0, "cnn_gru": 1}      # MSIG_GC_KIND_*
GC_SUM, GC_MAX, GC_CLIPPED, GC_LAST, GC_NSTAT = range(5)      # msig_gc.h: the statistics at the head of a model's clip state


class GcClip(C.Structure):
    """msig_gc_clip (include/msig_gc.h): the clip of a train step — model kind, optional class weights, the caller-owned clip state
    and max_norm per fold of the launch."""
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("class_weight", C.c_void_p), ("state", C.c_void_p),
                ("state_bytes", C.c_int64), ("max_norm", C.c_double * MAX_FOLDS)]


class Aug(C.Structure):
    """msig_aug (include/msig_aug.h): the augmentation of a gather launch — the four transforms' parameters and a key per fold."""
    _fields_ = [("scale_sigma", C.c_float), ("jitter_sigma", C.c_float), ("mask_prob", C.c_float), ("chan_drop_prob", C.c_float),
                ("mask_max", C.c_int32), ("reserved", C.c_int32), ("key", C.c_uint32 * MAX_FOLDS)]


class St(C.Structure):
    """msig_st (include/msig_st.h): the soft targets of a launch — model kind, label smoothing, optional class weights, an optional
    msig_gc_clip (by address: `make_st` keeps it alive) and the mixup weight of every fold."""
    _fields_ = [("kind", C.c_int32), ("smoothing", C.c_float), ("class_weight", C.c_void_p), ("clip", C.c_void_p),
                ("lam", C.c_float * MAX_FOLDS)]


class Da(C.Structure):
    """msig_da (include/msig_da.h): the subject discriminator of a launch — its size and Adam constants, the domain table and the
    batch's store positions, its parameter / moment / statistics buffers (per fold `stride_bytes` apart) and every fold's reversal
    weight, learning rate and step count."""
    _fields_ = [("S", C.c_int32), ("weight_decay", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("dom", C.c_void_p), ("idx", C.c_void_p), ("idx_row_stride", C.c_int64), ("params", C.c_void_p), ("exp_avg", C.c_void_p),
                ("exp_avg_sq", C.c_void_p), ("stats", C.c_void_p), ("stride_bytes", C.c_int64), ("lambda", C.c_float * MAX_FOLDS),
                ("lr", C.c_float * MAX_FOLDS), ("step", C.c_int64 * MAX_FOLDS)]


class Kd(C.Structure):
    """msig_kd (include/msig_kd.h): the distillation term of a launch — its weight and temperature, the teacher table and the
    batch's store positions, the optional statistics, and (fold batch) the bytes between the folds' tables and statistics."""
    _fields_ = [("alpha", C.c_float), ("temperature", C.c_float), ("q", C.c_void_p), ("idx", C.c_void_p), ("idx_row_stride", C.c_int64),
                ("stats", C.c_void_p), ("stride_bytes", C.c_int64)]


class Dro(C.Structure):
    """msig_dro (include/msig_dro.h): the group-DRO term of a launch — group count, step size, the frozen flag, the group table and the
    batch's store positions, the weights q, the optional statistics, and (fold batch) the bytes between the folds' q, grp and stats."""
    _fields_ = [("G", C.c_int32), ("eta", C.c_float), ("frozen", C.c_int32), ("grp", C.c_void_p), ("idx", C.c_void_p),
                ("idx_row_stride", C.c_int64), ("q", C.c_void_p), ("stats", C.c_void_p), ("stride_bytes", C.c_int64)]


class Sam(C.Structure):
    """msig_sam (include/msig_sam.h): the sharpness-aware step of a launch — model kind, SAM or ASAM, rho and eta, and the caller-owned
    state (fold slot 0's in a fold batch)."""
    _fields_ = [("kind", C.c_int32), ("adaptive", C.c_int32), ("rho", C.c_float), ("eta", C.c_float), ("state", C.c_void_p),
                ("state_bytes", C.c_int64)]


class Wa(C.Structure):
    """msig_wa (include/msig_wa.h): the weight-averaging update of a launch — the model's parameters and BatchNorm state, the shadow's
    (in a fold batch both are fold slot 0's, msig_multi.stride_bytes apart) and every fold's coefficient."""
    _fields_ = [("n_flat", C.c_int64), ("params", C.c_void_p), ("bn_state", C.c_void_p), ("bn_count", C.c_void_p),
                ("avg_params", C.c_void_p), ("avg_bn_state", C.c_void_p), ("avg_bn_count", C.c_void_p), ("coef", C.c_float * MAX_FOLDS)]


def make_st(kind: str, smoothing: float, class_weight=None, clip: "GcClip" = None, lams=(1.0,)) -> St:
    """msig_st of model kind `kind` with the given smoothing, class-weight device pointer, clip and per-fold lam."""
    s = St()
    s.kind, s.smoothing, s.class_weight = GC_KINDS[check_kind(kind)], float(smoothing), class_weight
    s._clip = clip                      # the struct holds only its address
    s.clip = C.addressof(clip) if clip is not None else None
    for i in range(MAX_FOLDS):
        s.lam[i] = float(lams[i]) if i < len(lams) else 1.0
    return s


_lib = None


def _loaded_hip_runtime() -> str:
    """Path of the libamdhip64 this process has ALREADY mapped (torch's bundled copy once torch is imported), else the soname for
    the loader's search path.  MSIG_HIP_RUNTIME overrides.  dlopen of that path returns the mapped object; RTLD_GLOBAL then makes
    its symbols visible to libmsig_hip.so, which names no HIP runtime of its own."""
    override = os.environ.get("MSIG_HIP_RUNTIME")
    if override:
        return override
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                path = line.rsplit(None, 1)[-1]
                if "libamdhip64" in os.path.basename(path):
                    return path
    except OSError:
        pass
    return "libamdhip64.so.7"


def lib() -> C.CDLL:
    """Loads libmsig_hip.so once.  Raises (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `make -C multimodalsignal_amd/csrc` "
                "(or python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
        # libmsig_hip.so has no DT_NEEDED on the HIP runtime (csrc/Makefile: -no-hip-rt): it binds to the copy this process already
        # uses.  torch first — its wheel bundles its own libamdhip64 — then that very object, found BY PATH in /proc/self/maps
        # (_loaded_hip_runtime: dlopen of a mapped path returns the mapped object), is promoted to the global symbol scope, where
        # the loader resolves this library's hip* symbols.  Not by soname: a soname lookup walks the search path and may return
        # /opt/rocm's copy — a second runtime in the process, round 3's hipErrorNoDevice (build() + smoke() in one process).  Only
        # a process with no runtime mapped at all falls back to the soname (ld.so.conf has /opt/rocm/lib on this image).
        import torch  # noqa: F401
        rt = _loaded_hip_runtime()
        try:
            C.CDLL(rt, mode=C.RTLD_GLOBAL)
        except OSError as e:
            raise RuntimeError(f"cannot open the HIP runtime {rt!r} ({e}): libmsig_hip.so binds to the libamdhip64 the process already uses; "
                               "set MSIG_HIP_RUNTIME=/path/to/libamdhip64.so to name it explicitly") from e
        L = C.CDLL(str(LIB_PATH))
        vp, i64p = C.c_void_p, C.POINTER(C.c_int64)
        L.msig_abi_version.restype = C.c_int
        L.msig_struct_bytes.argtypes = [C.c_int32]
        L.msig_struct_bytes.restype = C.c_int64
        if L.msig_abi_version() != ABI_VERSION or L.msig_struct_bytes(0) != C.sizeof(Batch) or L.msig_struct_bytes(1) != C.sizeof(Multi):
            raise RuntimeError(f"{LIB_PATH} is ABI {L.msig_abi_version()} with msig_batch / msig_multi of {L.msig_struct_bytes(0)} / "
                               f"{L.msig_struct_bytes(1)} bytes; this binding is ABI {ABI_VERSION} with {C.sizeof(Batch)} / {C.sizeof(Multi)}: "
                               "rebuild the library (make -C multimodalsignal_amd/csrc)")
        L.msig_stage_lengths.argtypes = [C.c_int, C.POINTER(C.c_int32)]
        L.msig_param_layout.argtypes = [C.c_int, C.c_int, i64p]
        L.msig_workspace_layout.argtypes = [C.POINTER(Shape), C.c_int, i64p]
        L.msig_workspace_bytes.argtypes = [C.POINTER(Shape), C.c_int]
        L.msig_workspace_bytes.restype = C.c_int64
        for name in ("msig_frontend_fwd", "msig_gru_fwd", "msig_head_ce_fwd", "msig_gru_bwd", "msig_frontend_bwd",
                     "msig_forward"):
            getattr(L, name).argtypes = [C.POINTER(Batch), vp]
        for name in ("msig_head_ce_bwd", "msig_backward"):
            getattr(L, name).argtypes = [C.POINTER(Batch), vp, vp]
        L.msig_adam_step.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float,
                                     C.c_float, C.c_int64, vp]
        L.msig_train_step.argtypes = [C.POINTER(Batch), vp, vp, C.c_float, C.c_float, C.c_float, C.c_float,
                                      C.c_float, C.c_int64, vp]
        L.msig_dropout_key.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
        L.msig_dropout_key.restype = C.c_uint32
        L.msig_gather_windows.argtypes = [vp, vp, vp, C.c_int32, C.c_int64, vp, vp, vp]
        L.msig_normalise_scratch_bytes.restype = C.c_int64
        L.msig_normalise_subject.argtypes = [vp, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_uint32, vp, vp, vp]
        L.msig_channel_attention.argtypes = [vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp]
        L.msig_profile_enable.argtypes = [C.c_int]
        L.msig_forward_multi.argtypes = [C.POINTER(Batch), C.POINTER(Multi), vp]
        L.msig_train_step_multi.argtypes = [C.POINTER(Batch), C.POINTER(Multi), vp, vp, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int64, vp]
        L.msig_gather_windows_multi.argtypes = [vp, vp, vp, C.c_int64, C.c_int32, C.c_int64, vp, vp, C.POINTER(Multi), vp]
        L.msig_profile_report.argtypes = [C.c_char_p, C.c_int64]
        L.msig_profile_report.restype = C.c_int64
        # include/msig_cw.h, exported by the same library: the forward / train-step calls with a class-weight vector
        L.msig_cw_abi_version.restype = C.c_int
        if L.msig_cw_abi_version() != CW_ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} has msig_cw.h ABI {L.msig_cw_abi_version()}; this binding is {CW_ABI_VERSION}: rebuild the library")
        f32, i64 = C.c_float, C.c_int64
        L.msig_cw_forward.argtypes = [C.POINTER(Batch), vp, vp]
        L.msig_cw_train_step.argtypes = [C.POINTER(Batch), vp, vp, vp, f32, f32, f32, f32, f32, i64, vp]
        L.msig_cw_forward_multi.argtypes = [C.POINTER(Batch), C.POINTER(Multi), vp, vp]
        L.msig_cw_train_step_multi.argtypes = [C.POINTER(Batch), C.POINTER(Multi), vp, vp, vp, f32, f32, f32, f32, i64, vp]
        # include/msig_cg.h, exported by the same library: the cnn_gru baseline (no ChannelAttention)
        L.msig_cg_abi_version.restype = C.c_int
        if L.msig_cg_abi_version() != CG_ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} has msig_cg.h ABI {L.msig_cg_abi_version()}; this binding is {CG_ABI_VERSION}: rebuild the library")
        L.msig_cg_param_layout.argtypes = [C.c_int, C.c_int, i64p]
        L.msig_cg_forward.argtypes = [C.POINTER(Batch), vp, vp]
        L.msig_cg_backward.argtypes = [C.POINTER(Batch), vp, vp]
        L.msig_cg_train_step.argtypes = [C.POINTER(Batch), vp, vp, vp, f32, f32, f32, f32, f32, i64, vp]
        L.msig_cg_forward_multi.argtypes = [C.POINTER(Batch), C.POINTER(Multi), vp, vp]
        L.msig_cg_train_step_multi.argtypes = [C.POINTER(Batch), C.POINTER(Multi), vp, vp, vp, f32, f32, f32, f32, i64, vp]
        # include/msig_ft.h, exported by the same library: window embeddings and the classifier-only head epoch
        L.msig_ft_abi_version.restype = C.c_int
        L.msig_ft_struct_bytes.argtypes = [C.c_int32]
        L.msig_ft_struct_bytes.restype = C.c_int64
        if (L.msig_ft_abi_version() != FT_ABI_VERSION or L.msig_ft_struct_bytes(0) != C.sizeof(FtHead)
                or L.msig_ft_struct_bytes(1) != C.sizeof(FtMulti)):
            raise RuntimeError(f"{LIB_PATH} has msig_ft.h ABI {L.msig_ft_abi_version()} with msig_ft_head / msig_ft_multi of "
                               f"{L.msig_ft_struct_bytes(0)} / {L.msig_ft_struct_bytes(1)} bytes; this binding is {FT_ABI_VERSION} with "
                               f"{C.sizeof(FtHead)} / {C.sizeof(FtMulti)}: rebuild the library")
        L.msig_ft_features.argtypes = [C.POINTER(Batch), C.c_int, vp, vp]
        L.msig_ft_features_multi.argtypes = [C.POINTER(Batch), C.POINTER(Multi), C.c_int, vp, C.c_int64, vp]
        L.msig_ft_head_epoch.argtypes = [C.POINTER(FtHead), vp]
        L.msig_ft_head_epoch_multi.argtypes = [C.POINTER(FtHead), C.POINTER(FtMulti), vp]
        # include/msig_ab.h, exported by the same library: label-free BatchNorm adaptation (kind: FT_KINDS)
        L.msig_ab_abi_version.restype = C.c_int
        if L.msig_ab_abi_version() != AB_ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} has msig_ab.h ABI {L.msig_ab_abi_version()}; this binding is {AB_ABI_VERSION}: rebuild the library")
        L.msig_ab_accumulate.argtypes = [C.POINTER(Batch), C.c_int, C.c_int, vp, vp]
        L.msig_ab_accumulate_multi.argtypes = [C.POINTER(Batch), C.POINTER(Multi), C.c_int, C.c_int, vp, vp]
        L.msig_ab_commit.argtypes = [vp, C.c_int, C.c_float, vp, vp, vp]
        L.msig_ab_commit_multi.argtypes = [vp, C.c_int, C.c_float, vp, vp, C.POINTER(Multi), vp]
        # include/msig_at.h, exported by the same library: the path points of integrated gradients and the reduction of their gradients
        L.msig_at_abi_version.restype = C.c_int
        if L.msig_at_abi_version() != AT_ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} has msig_at.h ABI {L.msig_at_abi_version()}; this binding is {AT_ABI_VERSION}: rebuild the library")
        L.msig_at_path.argtypes = [vp, vp, C.c_int32, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp]
        L.msig_at_reduce.argtypes = [vp, vp, vp, C.c_int32, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp]
        # include/msig_mc.h, exported by the same library: Monte-Carlo dropout (an eval forward cut at the first dropout site)
        L.msig_mc_abi_version.restype = C.c_int
        if L.msig_mc_abi_version() != MC_ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} has msig_mc.h ABI {L.msig_mc_abi_version()}; this binding is {MC_ABI_VERSION}: rebuild the library")
        L.msig_mc_trunk.argtypes = [C.POINTER(Batch), C.c_int32, vp]
        L.msig_mc_tail.argtypes = [C.POINTER(Batch), C.c_int32, vp]
        L.msig_mc_expand.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int64, vp]
        L.msig_mc_reduce.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp]
        # include/msig_gc.h, exported by the same library: the train steps with gradient-norm clipping
        L.msig_gc_abi_version.restype = C.c_int
        L.msig_gc_struct_bytes.restype = C.c_int64
        if L.msig_gc_abi_version() != GC_ABI_VERSION or L.msig_gc_struct_bytes() != C.sizeof(GcClip):
            raise RuntimeError(f"{LIB_PATH} has msig_gc.h ABI {L.msig_gc_abi_version()} with msig_gc_clip of {L.msig_gc_struct_bytes()} bytes; "
                               f"this binding is {GC_ABI_VERSION} with {C.sizeof(GcClip)}: rebuild the library")
        L.msig_gc_state_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        L.msig_gc_state_bytes.restype = C.c_int64
        L.msig_gc_train_step.argtypes = [C.POINTER(Batch), C.POINTER(GcClip), vp, vp, f32, f32, f32, f32, f32, i64, vp]
        L.msig_gc_train_step_multi.argtypes = [C.POINTER(Batch), C.POINTER(Multi), C.POINTER(GcClip), vp, vp, f32, f32, f32, f32, i64, vp]
        # include/msig_aug.h, exported by the same library: the gathers with on-device window augmentation
        L.msig_aug_abi_version.restype = C.c_int
        L.msig_aug_struct_bytes.restype = C.c_int64
        if L.msig_aug_abi_version() != AUG_ABI_VERSION or L.msig_aug_struct_bytes() != C.sizeof(Aug):
            raise RuntimeError(f"{LIB_PATH} has msig_aug.h ABI {L.msig_aug_abi_version()} with msig_aug of {L.msig_aug_struct_bytes()} bytes; "
                               f"this binding is {AUG_ABI_VERSION} with {C.sizeof(Aug)}: rebuild the library")
        i32 = C.c_int32
        L.msig_aug_gather_windows.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, C.POINTER(Aug), vp]
        L.msig_aug_gather_windows_multi.argtypes = [vp, vp, vp, i64, i32, i32, i32, vp, vp, C.POINTER(Multi), C.POINTER(Aug), vp]
        # include/msig_st.h, exported by the same library: soft targets (label smoothing, mixup)
        L.msig_st_abi_version.restype = C.c_int
        L.msig_st_struct_bytes.restype = C.c_int64
        if L.msig_st_abi_version() != ST_ABI_VERSION or L.msig_st_struct_bytes() != C.sizeof(St):
            raise RuntimeError(f"{LIB_PATH} has msig_st.h ABI {L.msig_st_abi_version()} with msig_st of {L.msig_st_struct_bytes()} bytes; "
                               f"this binding is {ST_ABI_VERSION} with {C.sizeof(St)}: rebuild the library")
        L.msig_st_forward.argtypes = [C.POINTER(Batch), C.POINTER(St), vp]
        L.msig_st_forward_multi.argtypes = [C.POINTER(Batch), C.POINTER(Multi), C.POINTER(St), vp]
        L.msig_st_train_step.argtypes = [C.POINTER(Batch), C.POINTER(St), vp, vp, f32, f32, f32, f32, f32, i64, vp]
        L.msig_st_train_step_multi.argtypes = [C.POINTER(Batch), C.POINTER(Multi), C.POINTER(St), vp, vp, f32, f32, f32, f32, i64, vp]
        L.msig_st_gather_windows.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, C.POINTER(Aug), C.POINTER(f32), vp]
        L.msig_st_gather_windows_multi.argtypes = [vp, vp, vp, i64, i32, i32, i32, vp, vp, C.POINTER(Multi), C.POINTER(Aug), C.POINTER(f32), vp]
        # include/msig_da.h, exported by the same library: the subject discriminator's step, alone and inside the train steps
        L.msig_da_abi_version.restype = C.c_int
        L.msig_da_struct_bytes.restype = C.c_int64
        if L.msig_da_abi_version() != DA_ABI_VERSION or L.msig_da_struct_bytes() != C.sizeof(Da):
            raise RuntimeError(f"{LIB_PATH} has msig_da.h ABI {L.msig_da_abi_version()} with msig_da of {L.msig_da_struct_bytes()} bytes; "
                               f"this binding is {DA_ABI_VERSION} with {C.sizeof(Da)}: rebuild the library")
        L.msig_da_param_floats.argtypes = [i32]
        L.msig_da_param_floats.restype = C.c_int64
        L.msig_da_step.argtypes = [C.POINTER(Da), vp, vp, i32, f32, vp]
        L.msig_da_step_multi.argtypes = [C.POINTER(Da), C.POINTER(Multi), vp, vp, i32, C.POINTER(f32), vp]
        L.msig_da_train_step.argtypes = [C.POINTER(Batch), C.POINTER(St), C.POINTER(Da), vp, vp, f32, f32, f32, f32, f32, i64, vp]
        L.msig_da_train_step_multi.argtypes = [C.POINTER(Batch), C.POINTER(Multi), C.POINTER(St), C.POINTER(Da), vp, vp, f32, f32, f32, f32,
                                               i64, vp]
        # include/msig_wa.h, exported by the same library: the weight-averaging update of a shadow model
        L.msig_wa_abi_version.restype = C.c_int
        L.msig_wa_struct_bytes.restype = C.c_int64
        if L.msig_wa_abi_version() != WA_ABI_VERSION or L.msig_wa_struct_bytes() != C.sizeof(Wa):
            raise RuntimeError(f"{LIB_PATH} has msig_wa.h ABI {L.msig_wa_abi_version()} with msig_wa of {L.msig_wa_struct_bytes()} bytes; "
                               f"this binding is {WA_ABI_VERSION} with {C.sizeof(Wa)}: rebuild the library")
        L.msig_wa_update.argtypes = [C.POINTER(Wa), vp]
        L.msig_wa_update_multi.argtypes = [C.POINTER(Wa), C.POINTER(Multi), vp]
        # include/msig_en.h, exported by the same library: the reduction of ensemble members' logits
        L.msig_en_abi_version.restype = C.c_int
        if L.msig_en_abi_version() != EN_ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} has msig_en.h ABI {L.msig_en_abi_version()}; this binding is {EN_ABI_VERSION}: rebuild the library")
        L.msig_en_reduce.argtypes = [vp, i64, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.msig_en_reduce_multi.argtypes = [vp, C.POINTER(Multi), i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        # include/msig_kd.h, exported by the same library: the teacher table and the train steps with the distillation term
        L.msig_kd_abi_version.restype = C.c_int
        L.msig_kd_struct_bytes.restype = C.c_int64
        if L.msig_kd_abi_version() != KD_ABI_VERSION or L.msig_kd_struct_bytes() != C.sizeof(Kd):
            raise RuntimeError(f"{LIB_PATH} has msig_kd.h ABI {L.msig_kd_abi_version()} with msig_kd of {L.msig_kd_struct_bytes()} bytes; "
                               f"this binding is {KD_ABI_VERSION} with {C.sizeof(Kd)}: rebuild the library")
        L.msig_kd_teacher.argtypes = [vp, i64, i32, i32, i32, f32, vp, vp]
        L.msig_kd_teacher_multi.argtypes = [vp, C.POINTER(Multi), i32, i32, f32, vp, vp]
        L.msig_kd_apply.argtypes = [C.POINTER(Kd), vp, vp, i32, i32, f32, vp]
        L.msig_kd_apply_multi.argtypes = [C.POINTER(Kd), C.POINTER(Multi), vp, vp, i32, i32, C.POINTER(f32), vp]
        L.msig_kd_train_step.argtypes = [C.POINTER(Batch), C.POINTER(St), C.POINTER(Da), C.POINTER(Kd), vp, vp, f32, f32, f32, f32, f32, i64, vp]
        L.msig_kd_train_step_multi.argtypes = [C.POINTER(Batch), C.POINTER(Multi), C.POINTER(St), C.POINTER(Da), C.POINTER(Kd), vp, vp, f32, f32,
                                               f32, f32, i64, vp]
        # include/msig_sam.h, exported by the same library: the perturbation, the restore and the two-pass train steps
        L.msig_sam_abi_version.restype = C.c_int
        L.msig_sam_struct_bytes.restype = C.c_int64
        if L.msig_sam_abi_version() != SAM_ABI_VERSION or L.msig_sam_struct_bytes() != C.sizeof(Sam):
            raise RuntimeError(f"{LIB_PATH} has msig_sam.h ABI {L.msig_sam_abi_version()} with msig_sam of {L.msig_sam_struct_bytes()} bytes; "
                               f"this binding is {SAM_ABI_VERSION} with {C.sizeof(Sam)}: rebuild the library")
        L.msig_sam_state_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        L.msig_sam_state_bytes.restype = C.c_int64
        L.msig_sam_perturb.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.POINTER(Sam), vp]
        L.msig_sam_restore.argtypes = [vp, vp, vp, vp, i32, C.c_int, C.c_int, C.POINTER(Sam), vp]
        L.msig_sam_train_step.argtypes = [C.POINTER(Batch), C.POINTER(St), C.POINTER(Kd), C.POINTER(Sam), vp, vp, f32, f32, f32, f32, f32, i64, vp]
        L.msig_sam_train_step_multi.argtypes = [C.POINTER(Batch), C.POINTER(Multi), C.POINTER(St), C.POINTER(Kd), C.POINTER(Sam), vp, vp, f32, f32,
                                                f32, f32, i64, vp]
        # include/msig_dro.h, exported by the same library: the group-DRO term and the train steps with it
        L.msig_dro_abi_version.restype = C.c_int
        L.msig_dro_struct_bytes.restype = C.c_int64
        if L.msig_dro_abi_version() != DRO_ABI_VERSION or L.msig_dro_struct_bytes() != C.sizeof(Dro):
            raise RuntimeError(f"{LIB_PATH} has msig_dro.h ABI {L.msig_dro_abi_version()} with msig_dro of {L.msig_dro_struct_bytes()} bytes; "
                               f"this binding is {DRO_ABI_VERSION} with {C.sizeof(Dro)}: rebuild the library")
        L.msig_dro_apply.argtypes = [C.POINTER(Dro), vp, vp, vp, f32, vp, i32, i32, vp]
        L.msig_dro_apply_multi.argtypes = [C.POINTER(Dro), C.POINTER(Multi), vp, vp, vp, f32, vp, i32, i32, vp]
        L.msig_dro_train_step.argtypes = [C.POINTER(Batch), C.POINTER(St), C.POINTER(Da), C.POINTER(Kd), C.POINTER(Sam), C.POINTER(Dro), vp, vp,
                                          f32, f32, f32, f32, f32, i64, vp]
        L.msig_dro_train_step_multi.argtypes = [C.POINTER(Batch), C.POINTER(Multi), C.POINTER(St), C.POINTER(Da), C.POINTER(Kd), C.POINTER(Sam),
                                                C.POINTER(Dro), vp, vp, f32, f32, f32, f32, i64, vp]
        # include/msig_sc.h, exported by the same library: the supervised contrastive term and the train steps with it
        L.msig_sc_abi_version.restype = C.c_int
        L.msig_sc_struct_bytes.restype = C.c_int64
        if L.msig_sc_abi_version() != SC_ABI_VERSION or L.msig_sc_struct_bytes() != C.sizeof(Sc):
            raise RuntimeError(f"{LIB_PATH} has msig_sc.h ABI {L.msig_sc_abi_version()} with msig_sc of {L.msig_sc_struct_bytes()} bytes; "
                               f"this binding is {SC_ABI_VERSION} with {C.sizeof(Sc)}: rebuild the library")
        L.msig_sc_scratch_bytes.argtypes = [i32]
        L.msig_sc_scratch_bytes.restype = C.c_int64
        L.msig_sc_apply.argtypes = [C.POINTER(Sc), vp, vp, vp, i32, i32, vp]
        L.msig_sc_apply_multi.argtypes = [C.POINTER(Sc), C.POINTER(Multi), vp, vp, vp, i32, i32, vp]
        L.msig_sc_train_step.argtypes = [C.POINTER(Batch), C.POINTER(St), C.POINTER(Da), C.POINTER(Kd), C.POINTER(Sam), C.POINTER(Dro),
                                         C.POINTER(Sc), vp, vp, f32, f32, f32, f32, f32, i64, vp]
        L.msig_sc_train_step_multi.argtypes = [C.POINTER(Batch), C.POINTER(Multi), C.POINTER(St), C.POINTER(Da), C.POINTER(Kd), C.POINTER(Sam),
                                               C.POINTER(Dro), C.POINTER(Sc), vp, vp, f32, f32, f32, f32, i64, vp]
        # include/msig_nr.h, exported by the same library: per-subject normalisation with the statistics of reference windows
        L.msig_nr_abi_version.restype = C.c_int
        if L.msig_nr_abi_version() != NR_ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} has msig_nr.h ABI {L.msig_nr_abi_version()}; this binding is {NR_ABI_VERSION}: rebuild the library")
        L.msig_nr_scratch_bytes.restype = C.c_int64
        L.msig_nr_normalise_subject.argtypes = [vp, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_uint32, vp, vp, vp,
                                                vp, vp]
        # include/msig_rec.h, exported by the same library: statistics and window batches of a continuous recording
        L.msig_rec_abi_version.restype = C.c_int
        if L.msig_rec_abi_version() != REC_ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} has msig_rec.h ABI {L.msig_rec_abi_version()}; this binding is {REC_ABI_VERSION}: rebuild the library")
        L.msig_rec_scratch_bytes.restype = C.c_int64
        L.msig_rec_count.argtypes = [i64, i64, i64]
        L.msig_rec_count.restype = C.c_int64
        rec = [vp, i64, i32, C.POINTER(i32), i32, C.c_uint32, i64, i64]      # sig, L, C_all, cols, C, log1p_mask, T, S
        L.msig_rec_stats.argtypes = rec + [i64, i64, vp, vp, vp]
        L.msig_rec_windows.argtypes = rec + [i64, i32, vp, vp, vp]
        L.msig_rec_windows_multi.argtypes = rec + [i64, i32, vp, vp, C.POINTER(Multi), vp]
        # include/msig_lv.h, exported by the same library: sample rings of many sessions and mixed window batches
        L.msig_lv_abi_version.restype = C.c_int
        if L.msig_lv_abi_version() != LV_ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} has msig_lv.h ABI {L.msig_lv_abi_version()}; this binding is {LV_ABI_VERSION}: rebuild the library")
        pool = [vp, i32, i64, i64, i32]                                       # pool, sessions, R, ring_bytes, C_all
        L.msig_lv_push.argtypes = pool + [C.POINTER(i32), C.POINTER(i64), C.POINTER(i64), i32, vp, vp]
        L.msig_lv_windows_multi.argtypes = pool + [C.POINTER(i32), i32, C.c_uint32, i64, i64, C.POINTER(i32), C.POINTER(i64), C.POINTER(i64), i32,
                                                   vp, vp, C.POINTER(Multi), vp]
        # include/msig_rn.h, exported by the same library: window sums, a statistics record per window, batches with a record per row
        L.msig_rn_abi_version.restype = C.c_int
        if L.msig_rn_abi_version() != RN_ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} has msig_rn.h ABI {L.msig_rn_abi_version()}; this binding is {RN_ABI_VERSION}: rebuild the library")
        L.msig_rn_state_bytes.argtypes = [i32]
        L.msig_rn_state_bytes.restype = C.c_int64
        L.msig_rn_sums.argtypes = rec + [i64, i64, vp, vp]
        L.msig_rn_stats.argtypes = rec + [vp, i64, i32, vp, vp]
        L.msig_rn_windows.argtypes = rec + [i64, i32, vp, vp, vp]
        L.msig_rn_windows_multi.argtypes = rec + [i64, i32, vp, vp, C.POINTER(Multi), vp]
        rows = [C.POINTER(i32), i32, C.c_uint32, i64, i64]                    # cols, C, log1p_mask, T, S
        L.msig_rn_lv_step.argtypes = pool + rows + [i32, vp, i64, C.POINTER(i32), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), i32, vp, vp]
        L.msig_rn_lv_windows_multi.argtypes = pool + rows + [C.POINTER(i32), C.POINTER(i64), C.POINTER(i64), i32, vp, vp, C.POINTER(Multi), vp]
        # include/msig_rd.h, exported by the same library: the decayed reference's statistics table and its live step
        L.msig_rd_abi_version.restype = C.c_int
        if L.msig_rd_abi_version() != RD_ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} has msig_rd.h ABI {L.msig_rd_abi_version()}; this binding is {RD_ABI_VERSION}: rebuild the library")
        L.msig_rd_stats.argtypes = rec + [vp, i64, C.c_double, vp, vp]
        L.msig_rd_lv_step.argtypes = pool + rows + [C.c_double, vp, i64, C.POINTER(i32), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), i32, vp, vp]
        # include/msig_gp.h, exported by the same library: pivot, window records, statistics and coverage tables, rows and the live step
        # of recordings and sessions with missing samples
        L.msig_gp_abi_version.restype = C.c_int
        L.msig_gp_struct_bytes.restype = C.c_int64
        if L.msig_gp_abi_version() != GP_ABI_VERSION or L.msig_gp_struct_bytes() != C.sizeof(GpMode):
            raise RuntimeError(f"{LIB_PATH} has msig_gp.h ABI {L.msig_gp_abi_version()} with msig_gp_mode of {L.msig_gp_struct_bytes()} bytes; "
                               f"this binding is {GP_ABI_VERSION} with {C.sizeof(GpMode)}: rebuild the library")
        L.msig_gp_state_bytes.argtypes = [i32]
        L.msig_gp_state_bytes.restype = C.c_int64
        L.msig_gp_pivot.argtypes = rec + [i64, vp, vp]
        L.msig_gp_sums.argtypes = rec + [vp, i64, i64, vp, vp]
        L.msig_gp_stats.argtypes = rec + [vp, vp, i64, C.POINTER(GpMode), vp, vp, vp]
        L.msig_gp_windows.argtypes = rec + [i64, i32, vp, vp, vp]
        L.msig_gp_windows_multi.argtypes = rec + [i64, i32, vp, vp, C.POINTER(Multi), vp]
        L.msig_gp_lv_step.argtypes = pool + rows + [C.POINTER(GpMode), vp, i64, C.POINTER(i32), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), i32, vp,
                                                    vp, vp]
        L.msig_gp_lv_windows_multi.argtypes = pool + rows + [C.POINTER(i32), C.POINTER(i64), C.POINTER(i64), i32, vp, vp, C.POINTER(Multi), vp]
        L.msig_gp_lv_skip.argtypes = pool + [C.POINTER(i32), C.POINTER(i64), C.POINTER(i64), i32, vp]
        # include/msig_rs.h, exported by the same library: the polyphase FIR resampler, offline and fused with the ring append
        L.msig_rs_abi_version.restype = C.c_int
        if L.msig_rs_abi_version() != RS_ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} has msig_rs.h ABI {L.msig_rs_abi_version()}; this binding is {RS_ABI_VERSION}: rebuild the library")
        ratio = [vp, i32, i32, i32]                                           # h, L, M, half
        L.msig_rs_out_count.argtypes = [i64, i32, i32, i32]
        L.msig_rs_out_count.restype = C.c_int64
        L.msig_rs_resample.argtypes = [vp, i64, i32] + ratio + [vp, i64, vp]
        L.msig_rs_lv_push.argtypes = pool + [vp, i64, i64] + ratio + [C.POINTER(i32), C.POINTER(i64), C.POINTER(i64), i32, vp, vp]
        # include/msig_mx.h, exported by the same library: a rate per column group in front of the rings and offline
        L.msig_mx_abi_version.restype = C.c_int
        L.msig_mx_struct_bytes.restype = C.c_int64
        if L.msig_mx_abi_version() != MX_ABI_VERSION or L.msig_mx_struct_bytes() != C.sizeof(MxGroup):
            raise RuntimeError(f"{LIB_PATH} has msig_mx.h ABI {L.msig_mx_abi_version()} with msig_mx_group of {L.msig_mx_struct_bytes()} bytes; "
                               f"this binding is {MX_ABI_VERSION} with {C.sizeof(MxGroup)}: rebuild the library")
        L.msig_mx_resample.argtypes = [vp, i64, vp, C.POINTER(MxGroup), vp, i64, i32, vp]
        L.msig_mx_lv_push.argtypes = pool + [vp, i64, vp, C.POINTER(MxGroup), i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64), C.POINTER(i64), i32,
                                             vp, vp]
        _lib = L
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        msg = ERRORS.get(rc, f"hipError_t {rc}" if rc > 0 else f"error {rc}")
        raise RuntimeError(f"{what} failed: {msg}")


def stage_lengths(T: int):
    out = (C.c_int32 * 4)()
    check(lib().msig_stage_lengths(T, out), "msig_stage_lengths")
    return tuple(int(v) for v in out)


def param_layout(Cin: int, K: int, kind: str = "cnn_gru_attention"):
    """Offsets (floats) of the NPARAM tensors in the flat buffer; last entry = total.  kind "cnn_gru": msig_cg_param_layout (the
    gate's two tensors have zero size)."""
    off = (C.c_int64 * (NPARAM + 1))()
    if check_kind(kind) == "cnn_gru":
        check(lib().msig_cg_param_layout(Cin, K, off), "msig_cg_param_layout")
    else:
        check(lib().msig_param_layout(Cin, K, off), "msig_param_layout")
    return [int(v) for v in off]


def param_shapes(Cin: int, K: int, kind: str = "cnn_gru_attention"):
    G, H = 192, 64
    Cr = Cin // 4 if check_kind(kind) == "cnn_gru_attention" else 0
    shapes = [(Cr, Cin), (Cin, Cr), (16, Cin, 7), (16,), (16,), (32, 16, 5), (32,), (32,)]
    for layer in (0, 1):
        for _ in range(2):
            shapes += [(G, 128 if layer else 32), (G, H), (G,), (G,)]
    shapes += [(64, 128), (64,), (K, 64), (K,)]
    return shapes


def workspace_layout(B: int, Cin: int, T: int, K: int, training: bool):
    sh = Shape(B, Cin, T, K)
    off = (C.c_int64 * (NWS + 1))()
    check(lib().msig_workspace_layout(C.byref(sh), int(training), off), "msig_workspace_layout")
    return [int(v) for v in off]


def dropout_key(seed: int, step: int, stream_id: int) -> int:
    return int(lib().msig_dropout_key(seed & (2 ** 64 - 1), step & (2 ** 64 - 1), stream_id))


def _fmix32_np(h):
    import numpy as np
    h = h.astype(np.uint64)
    h ^= h >> np.uint64(16); h = (h * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13); h = (h * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    return h


def dropout_keys(seed: int, steps, stream_id: int):
    """msig_dropout_key for an array of steps at once (same mixing; tests/test_host_logic.py checks it against the C function)."""
    import numpy as np
    steps = np.asarray(steps, dtype=np.uint64)
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    a = (steps * np.uint64(0x9E3779B9)) & np.uint64(0xFFFFFFFF)
    b = np.uint64((stream_id * 0x7F4A7C15) & 0xFFFFFFFF)
    inner = _fmix32_np((a + b + hi) & np.uint64(0xFFFFFFFF))
    return _fmix32_np(lo ^ inner).astype(np.uint32)


def dropout_threshold(p: float) -> int:
    return int(round(float(p) * 256.0))


def check_class_weight(values, K: int):
    """The host-side checks of a class-weight vector (include/msig_cw.h), made before anything is launched: exactly K finite,
    non-negative numbers.  Returns them as a float64 numpy array; raises ValueError otherwise."""
    import numpy as np
    try:
        w = np.asarray(values, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"class weights must be {K} numbers: {e}") from None
    if w.ndim != 1 or w.size != K:
        raise ValueError(f"class weights must be {K} numbers (one per class), got shape {tuple(w.shape)}")
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError(f"class weights must be finite and non-negative, got {w.tolist()}")
    return w


def gc_state_bytes(Cin: int, K: int, kind: str = "cnn_gru_attention") -> int:
    """Bytes of one model's clip state (include/msig_gc.h msig_gc_state_bytes)."""
    n = int(lib().msig_gc_state_bytes(Cin, K, GC_KINDS[check_kind(kind)]))
    if n < 0:
        check(n, "msig_gc_state_bytes")
    return n


def sam_state_bytes(Cin: int, K: int, kind: str = "cnn_gru_attention") -> int:
    """Bytes of one model's SAM state (include/msig_sam.h msig_sam_state_bytes)."""
    n = int(lib().msig_sam_state_bytes(Cin, K, GC_KINDS[check_kind(kind)]))
    if n < 0:
        check(n, "msig_sam_state_bytes")
    return n


def da_param_floats(S: int) -> int:
    """Floats of a subject discriminator's parameter buffer for S domains (include/msig_da.h msig_da_param_floats)."""
    n = int(lib().msig_da_param_floats(int(S)))
    if n < 0:
        check(n, "msig_da_param_floats")
    return n


def check_max_grad_norm(value) -> float:
    """The host-side check of a max_norm (include/msig_gc.h): a number > 0, +infinity allowed (no clipping).  ValueError otherwise."""
    if isinstance(value, (str, bytes, bool)):          # float("1") would pass: a string is not a number here
        raise ValueError(f"max_grad_norm must be a positive number, got {value!r}")
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"max_grad_norm must be a positive number, got {value!r}") from None
    if not v > 0.0:
        raise ValueError(f"max_grad_norm must be a positive number, got {value!r}")
    return v


def check_label_smoothing(value) -> float:
    """The host-side check of a label smoothing (include/msig_st.h): None or a number with 0 <= eps < 1 as the C calls see it (fp32).
    Returns the float (0.0 for None); ValueError otherwise."""
    if value is None:
        return 0.0
    if isinstance(value, (str, bytes, bool)):
        raise ValueError(f"label_smoothing must be a number in [0, 1), got {value!r}")
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"label_smoothing must be a number in [0, 1), got {value!r}") from None
    if not 0.0 <= v < 1.0 or C.c_float(v).value >= 1.0:
        raise ValueError(f"label_smoothing must be a number in [0, 1), got {value!r}")
    return v


def check_mix_lambda(value) -> float:
    """The host-side check of a mixup weight (include/msig_st.h): None (1.0, no mixing) or a number in [0, 1].  ValueError otherwise."""
    if value is None:
        return 1.0
    if isinstance(value, (str, bytes, bool)):
        raise ValueError(f"mix_lambda must be a number in [0, 1], got {value!r}")
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"mix_lambda must be a number in [0, 1], got {value!r}") from None
    if not 0.0 <= v <= 1.0:
        raise ValueError(f"mix_lambda must be a number in [0, 1], got {value!r}")
    return C.c_float(v).value


def check_distill(alpha, temperature):
    """The host-side checks of a distillation setting (include/msig_kd.h): alpha a number in [0, 1] and the temperature one in
    [1/64, 64], returned as the fp32 values the calls will see.  ValueError otherwise."""
    out = []
    for name, value, lo, hi in (("alpha", alpha, 0.0, 1.0), ("temperature", temperature, KD_MIN_T, KD_MAX_T)):
        if isinstance(value, (str, bytes, bool)):
            raise ValueError(f"a distillation {name} must be a number in [{lo:g}, {hi:g}], got {value!r}")
        try:
            v = float(value)
        except (TypeError, ValueError):
            raise ValueError(f"a distillation {name} must be a number in [{lo:g}, {hi:g}], got {value!r}") from None
        if not lo <= v <= hi:
            raise ValueError(f"a distillation {name} must be a number in [{lo:g}, {hi:g}], got {value!r}")
        out.append(C.c_float(v).value)
    return tuple(out)


def check_average_coef(value) -> float:
    """The host-side check of a weight-averaging coefficient (include/msig_wa.h): a number in [0, 1], returned as the fp32 value the
    call will see.  ValueError otherwise."""
    if isinstance(value, (str, bytes, bool)):
        raise ValueError(f"an averaging coefficient must be a number in [0, 1], got {value!r}")
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"an averaging coefficient must be a number in [0, 1], got {value!r}") from None
    if not 0.0 <= v <= 1.0:
        raise ValueError(f"an averaging coefficient must be a number in [0, 1], got {value!r}")
    return C.c_float(v).value


FORM_AUTO = -1
FWD_FORMS = {"auto": -1, "split": 0, "fused": 1, "b3": 1, "fp32": 2, "ws": 3}       # msig.h MSIG_FWD_*
BWD_FORMS = {"auto": -1, "split": 0, "fused": 1, "b3": 2, "b4": 3, "b5": 4, "b6": 5}                   # msig.h MSIG_BWD_*

# Kernel forms are per call in the C ABI (msig_batch.fwd_form / bwd_form = enumerator + 1, 0 = the library's default).  This
# binding keeps a default pair that runtime.Engine / FoldArena put into every descriptor they build (diagnostics / tests).
_default_forms = [0, 0]


def set_kernel_form(fwd="auto", bwd="auto"):
    """Default GRU kernel forms of the descriptors this binding builds from now on; "auto" = the library picks by batch size."""
    _default_forms[0], _default_forms[1] = FWD_FORMS[fwd] + 1, BWD_FORMS[bwd] + 1


def apply_forms(b: "Batch", fwd=None, bwd=None):
    """Writes the kernel forms into a descriptor: the given names, else the binding's defaults (set_kernel_form)."""
    b.fwd_form = _default_forms[0] if fwd is None else FWD_FORMS[fwd] + 1
    b.bwd_form = _default_forms[1] if bwd is None else BWD_FORMS[bwd] + 1
    return b


def profile_enable(on: bool):
    check(lib().msig_profile_enable(int(on)), "msig_profile_enable")


def profile_report():
    """{kernel name: (launches, total_ms)} for everything launched since profile_enable(True)."""
    buf = C.create_string_buffer(1 << 16)
    n = lib().msig_profile_report(buf, len(buf))
    if n < 0:
        raise RuntimeError(f"msig_profile_report failed: {n}")
    out = {}
    for line in buf.value.decode().splitlines():
        name, cnt, ms = line.split()
        out[name] = (int(cnt), float(ms))
    return out
