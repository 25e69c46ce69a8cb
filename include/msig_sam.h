/* msig_sam.h — sharpness-aware minimisation (SAM, Foret et al. 2021; ASAM, Kwon et al. 2021) inside the fused and fold-batched
 * train steps of libmsig_hip.so.
 *
 * Per batch SAM takes the gradient g at w, steps to w + e with e = rho g / ||g||, takes the gradient there, and applies the optimiser
 * AT w with that second gradient.  msig_*_train_step reduces the weight-gradient partials and applies Adam in the same thread of its
 * last launch, and a fold batch has no per-fold host step at all, so the method cannot be added from outside.  The calls below are
 * msig_kd_train_step[_multi] run twice over one batch with three more launches: the perturbation (two) between the passes and the
 * restore (one) before the second pass's Adam.  They stand beside msig.h and its companions, which are unchanged; libmsig_hip.so
 * exports all of them.
 *
 * Perturbation (msig_sam_perturb).  g is the reduced fp32 gradient in `grads`, p a parameter element.  Every
 * fp32 operation is one rounding, never an FMA:
 *     SAM    u = g                                     ASAM   t = fadd(fabsf(p), eta),  u = fmul(t, g)
 *     N      = sqrt(sum (double)u (double)u) over the elements of every parameter tensor, accumulated in fp64 in ONE fixed order that
 *              depends on (C, K, kind) alone — not on the folds of the launch, their companions or the stream
 *     coef   = (float)(rho / (N + 1e-12)), the quotient in fp64, rounded once
 *     e      = fmul(coef, u)                           ASAM   e = fmul(coef, fmul(t, u))
 *     backup = p,  p = fadd(p, e)
 * The kernels walk the tensors by their (offset, length) table: the padding between tensors of `grads`, which nobody writes, is
 * never read, and the padding of `params` is copied to the backup and left as it is.  The same launch copies bn_state, bn_count and
 * ws_loss[0..2] into the state and one thread updates, in stream order,
 *     [MSIG_SAM_NORM_SUM] += N      [MSIG_SAM_NORM_MAX] = max(itself, N)      [MSIG_SAM_NORM_LAST] = N
 * Two launches: the per-workgroup sums of squares, then the rest.
 *
 * Restore (msig_sam_restore), one launch: p = backup for EVERY element of the padded layout (bit exact); bn_state and bn_count from
 * the state — the running statistics and num_batches_tracked of a SAM step are those of the pass at w, updated once;
 *     d = ws_loss[1] / B - saved[1] / B in fp64      (mean CE at w + e minus mean CE at w)
 *     [MSIG_SAM_SHARP_SUM] += d      [MSIG_SAM_SHARP_LAST] = d      [MSIG_SAM_STEPS] += 1
 * and ws_loss[0..2] is rewritten with the saved triple.
 *
 * State: caller-owned DEVICE memory of msig_sam_state_bytes(C, K, kind) bytes per model, 8-byte aligned, in this order:
 * MSIG_SAM_NSTAT doubles of statistics (every SAM step updates them; the caller zeroes them when it starts a new count, an epoch,
 * as with msig_gc.h's clip state), the per-workgroup sums of squares, a backup of the parameters (padded-layout length), a backup of
 * the 96 BatchNorm floats and the two counters, three floats of MSIG_WS_LOSS (and one of padding).  In a fold batch fold z's state
 * lies at state + m->slot[z] * m->stride_bytes, in its own arena like every other buffer.
 *
 * msig_sam_train_step[_multi] — what the call leaves.  Pass 1 is the training forward with the head unfused, the distillation term
 * if `kd` is given, the backward and the reduction WITHOUT Adam; then the perturbation; pass 2 is the whole train step on the same
 * batch with the same dropout keys (one mask and one function in both passes — implementations that redraw dropout in pass 2
 * differ), head unfused, with the restore after its backward and before its reduction + Adam launch.  msig_st.clip clips pass 2's
 * gradient.  After the call:
 *     grads                          pass 2's gradient (at w + e), clipped if a clip is on
 *     params, both moments           Adam applied at w with that gradient
 *     MSIG_WS_LOSS, msig_batch.loss_acc (both entries), msig_kd.stats, bn_state, bn_count      pass 1's: a batch counts once, at w
 *     MSIG_WS_LOGITS, MSIG_WS_PROBS, MSIG_WS_PRED and every other workspace region             pass 2's
 * No host synchronisation: the call is capturable like the other steps.  A NULL msig_sam, or one with rho == 0 (after its checks),
 * makes the call msig_kd_train_step[_multi] (da = NULL) itself: the same launches, the fused head where it applies.  The subject
 * adversary (msig_da.h) is out of scope — its launch advances the discriminator's own Adam, and two passes would advance it twice —
 * so these calls take no msig_da.
 *
 * Checks, all before any launch (in a fold batch msig_multi's own checks come first), then the counterpart's: NULL msig_sam where
 * one is required, NULL state (stand-alone calls: any NULL pointer) -> MSIG_E_NULL; a kind that is not MSIG_GC_KIND_* or differs from
 * msig_st.kind, adaptive outside {0, 1}, rho NaN or negative, eta NaN or negative, (stand-alone calls) unsupported C / K, B < 1 ->
 * MSIG_E_SHAPE; a state that is not 8-byte aligned (stand-alone calls: params / grads not 16, bn_state / ws_loss not 4, bn_count
 * not 8) -> MSIG_E_ALIGN; state_bytes below msig_sam_state_bytes -> MSIG_E_WORKSPACE.
 */
#ifndef MSIG_SAM_H
#define MSIG_SAM_H
#include "msig.h"
#include "msig_gc.h"
#include "msig_st.h"
#include "msig_kd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSIG_SAM_ABI_VERSION 1

enum { MSIG_SAM_NORM_SUM, MSIG_SAM_NORM_MAX, MSIG_SAM_NORM_LAST,      /* N of pass 1 (above)               */
       MSIG_SAM_SHARP_SUM, MSIG_SAM_SHARP_LAST,                       /* mean CE at w+e minus mean CE at w */
       MSIG_SAM_STEPS, MSIG_SAM_NSTAT = 8 };

typedef struct msig_sam {
  int32_t kind;          /* MSIG_GC_KIND_*; must equal msig_st.kind                         */
  int32_t adaptive;      /* 0 = SAM, 1 = ASAM                                               */
  float   rho;           /* >= 0, of the launch; 0 = off                                    */
  float   eta;           /* ASAM only: T_w = |w| + eta, eta >= 0 (0.01 is the paper's)      */
  void*   state;         /* device, 8-byte aligned; fold z: state + slot[z] * m->stride_bytes */
  int64_t state_bytes;
} msig_sam;

int     msig_sam_abi_version(void);
int64_t msig_sam_struct_bytes(void);    /* sizeof(msig_sam) of the build */

/* Bytes of one model's state (a multiple of 8), or a negative MSIG_E_* for an unsupported C / K / kind. */
int64_t msig_sam_state_bytes(int C, int K, int kind);

/* The perturbation alone on caller-owned buffers of one model: params / grads in the padded layout of (C, K, s->kind), 16-byte
 * aligned; bn_state (96 floats), bn_count (2 x int64) and ws_loss (3 floats) are only read. */
int msig_sam_perturb(float* params, const float* grads, float* bn_state, int64_t* bn_count, const float* ws_loss,
                     int C, int K, const msig_sam* s, void* stream);
/* The restore alone: undoes the msig_sam_perturb that filled s->state.  B: rows of the batch whose summed losses ws_loss[1] holds. */
int msig_sam_restore(float* params, float* bn_state, int64_t* bn_count, float* ws_loss, int32_t B, int C, int K,
                     const msig_sam* s, void* stream);

/* msig_kd_train_step[_multi] (da = NULL) as a SAM step; kd may be NULL. */
int msig_sam_train_step(const msig_batch* b, const msig_st* s, const msig_kd* kd, const msig_sam* sam, float* exp_avg, float* exp_avg_sq,
                        float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, void* stream);
int msig_sam_train_step_multi(const msig_batch* b, const msig_multi* m, const msig_st* s, const msig_kd* kd, const msig_sam* sam,
                              float* exp_avg, float* exp_avg_sq, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSIG_SAM_H */
