/* msig_gc.h — gradient-norm clipping inside the fused and fold-batched train steps of libmsig_hip.so.
 *
 * msig_train_step and its msig_cw_* / msig_cg_* siblings reduce every weight-gradient partial and apply Adam to the reduced element
 * in the same thread of their last launch, so a caller has no point at which torch.nn.utils.clip_grad_norm_ could run.  The calls
 * below are those train steps with the clip between the reduction and the update:
 *     torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm, norm_type=2); optimizer.step()
 * They stand beside msig.h, msig_cw.h, msig_cg.h and msig_ft.h, which are unchanged; libmsig_hip.so exports all of them.
 *
 * Semantics, for each model of a launch:
 *     g      the reduced fp32 gradient of every parameter element: the value the unclipped step leaves in msig_batch.grads
 *     N      = sqrt(sum g^2) over every parameter tensor, the squares accumulated in fp64 in ONE fixed order that depends on the
 *              model's shape alone (not on the folds of the launch, their companions or the stream)
 *     coef   = (float)q with q = max_norm / (N + 1e-6) in fp64, q > 1 replaced by 1 (a NaN q stays NaN, as torch's clamp keeps it)
 *     g'     = g * coef, one fp32 multiplication, stored to msig_batch.grads (torch clips .grad in place)
 *     Adam   on g' with the arithmetic of the unclipped step; L2 weight decay is added inside Adam, after the clip, as in torch
 * max_norm = +infinity switches the clip off: coef = 1 and every bit of the step is the unclipped step's.  Non-finite norms get no
 * special case (torch's error_if_nonfinite=False).
 *
 * Clip state: caller-owned DEVICE memory of msig_gc_state_bytes(C, K, kind) bytes per model, 8-byte aligned.  Its first
 * MSIG_GC_NSTAT doubles are running statistics that every clipped step of the model updates (one thread, stream order) and the
 * caller zeroes when it starts a new count (an epoch):
 *     [MSIG_GC_SUM]  += N      [MSIG_GC_MAX] = max(itself, N)      [MSIG_GC_CLIPPED] += (N > max_norm)      [MSIG_GC_LAST] = N
 * (N before the clip).  The rest is scratch of the step (the per-workgroup sums of squares).  In a fold batch fold z's state lies at
 * state + m->slot[z] * m->stride_bytes — in its own arena, like every other buffer.
 *
 * Conventions, argument checks, MSIG_E_* codes and "nothing launched on error" are the counterpart's (msig_train_step[_multi],
 * msig_cw_*, msig_cg_*), plus the clip's own, checked before the counterpart's (in a fold batch: after msig_multi's own checks, which
 * say how many folds there are): NULL msig_gc_clip or state -> MSIG_E_NULL; a kind that is not MSIG_GC_KIND_*, or a max_norm of a fold
 * of the launch that is NaN or <= 0 -> MSIG_E_SHAPE; state not 8-byte aligned -> MSIG_E_ALIGN; state_bytes below msig_gc_state_bytes
 * -> MSIG_E_WORKSPACE.
 */
#ifndef MSIG_GC_H
#define MSIG_GC_H
#include "msig.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSIG_GC_ABI_VERSION 1

#define MSIG_GC_KIND_ATTENTION 0      /* CnnGruAttentionModel: msig.h's parameter layout, msig_train_step / msig_cw_train_step */
#define MSIG_GC_KIND_CNN_GRU 1        /* the cnn_gru baseline: msig_cg.h's layout, msig_cg_train_step */

enum { MSIG_GC_SUM = 0, MSIG_GC_MAX = 1, MSIG_GC_CLIPPED = 2, MSIG_GC_LAST = 3, MSIG_GC_NSTAT = 4 };

typedef struct msig_gc_clip {
  int32_t kind;                         /* MSIG_GC_KIND_* of every model of the launch */
  int32_t reserved;                     /* write 0 (not read) */
  const float* class_weight;            /* msig_cw.h's semantics (device, K floats, 4-byte aligned); NULL = the unweighted criterion */
  void* state;                          /* device: the clip state of the model (of fold slot 0 in a fold batch) */
  int64_t state_bytes;                  /* bytes available per model at `state` */
  double max_norm[MSIG_MAX_FOLDS];      /* per fold of the launch ([0] for a single model): > 0, +infinity = no clipping */
} msig_gc_clip;

int msig_gc_abi_version(void);
int64_t msig_gc_struct_bytes(void);     /* sizeof(msig_gc_clip) of the build */

/* Bytes of one model's clip state (a multiple of 8), or a negative MSIG_E_* for an unsupported C / K / kind. */
int64_t msig_gc_state_bytes(int C, int K, int kind);

/* msig_train_step / msig_cw_train_step / msig_cg_train_step with the clip. */
int msig_gc_train_step(const msig_batch* b, const msig_gc_clip* g, float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2,
                       float eps, float weight_decay, int64_t step, void* stream);

/* msig_train_step_multi / msig_cw_train_step_multi / msig_cg_train_step_multi with the clip; fold z is clipped to g->max_norm[z]. */
int msig_gc_train_step_multi(const msig_batch* b, const msig_multi* m, const msig_gc_clip* g, float* exp_avg, float* exp_avg_sq,
                             float beta1, float beta2, float eps, float weight_decay, int64_t step, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSIG_GC_H */
