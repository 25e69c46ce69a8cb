/* msig_dro.h — group-DRO: adversarial group weights on the objective inside the fused and fold-batched train steps of libmsig_hip.so.
 *
 * Every train step minimises the mean loss over a fold's pooled windows; a LOSO run is judged on a subject the model has not seen,
 * and the folds that pull the mean down fit a few training subjects much worse than the rest.  Group-DRO (Sagawa et al.,
 * "Distributionally Robust Neural Networks for Group Shifts", ICLR 2020, the online algorithm) keeps one weight q_g per group —
 * here a fold's training subjects, or its (subject, class) pairs — raises it with the group's loss and descends sum_g q_g L_g.
 * That is a per-row rescale of MSIG_WS_DLOGITS, which is written and consumed inside one msig_*_train_step[_multi] call.  The train
 * steps below are msig_kd.h's / msig_sam.h's with ONE more launch between the criterion and the head's backward (before the
 * distillation term's).  It stands beside msig.h and its companions, which are unchanged; libmsig_hip.so exports all of them.
 *
 * One step of one fold.  B rows, logits z (B, K) fp32, labels y, class weights w (1 when none), smoothing eps;
 * dlogits is what the criterion left in MSIG_WS_DLOGITS (msig_st.h's gradient with lam = 1).  The group table grp holds one int32 per
 * store position: row b's group is g_b = grp[idx[b]] (idx: the int64 store positions the batch was gathered from, as msig_da.idx) or
 * grp[b] when idx is NULL.  G groups, 1 <= G <= MSIG_DRO_MAX_GROUPS; a g_b outside [0, G) means the row is in no group (so does a
 * label outside [0, K): such a row has m_b = t_b = 0).  q: G fp32 weights that sum to 1, the caller's, persistent across steps.
 * eta >= 0 is the launch's.
 *     m_b  = w[y_b]
 *     t_b  = (1-eps) w[y_b] l_b(y_b) + (eps/K) sum_c w_c l_b(c)
 *            l_b(c) = -ln softmax(z_b)_c, in fp64 from the fp32 z: (z_c - max) - ln sum exp(z_c - max); 1-eps and eps/K from the fp32
 *            eps widened to fp64; the sum over c in increasing c
 *     W    = sum_b m_b                  all B rows, increasing b, fp64 (the criterion's W)
 *     W_g  = sum_{b: g_b = g} m_b       T_g = sum_{b: g_b = g} t_b     n_g = rows     increasing b, fp64
 *     g is present iff n_g > 0 and W_g > 0;      L_g = T_g / W_g
 *     update (unless frozen):  q'_g = q_g * exp(eta * L_g) for present g, q'_g = q_g otherwise;
 *                              Z = sum_g q'_g in increasing g;   q_g <- (float)(q'_g / Z)
 *     r_b  = (float)((double)q_{g_b} * W / W_{g_b})    with the stored fp32 q after the update;
 *            r_b = 0 for a row in no group or in a group that is not present
 *     dlogits[b][c] = fmul(r_b, dlogits[b][c])         one rounding, in place; nothing else of the workspace is written
 * Because dL_g/dz_b = (W / W_g) dlogits_b for b in g, the result is d/dz sum_{g present} q_g L_g with q held constant: the q-weighted
 * sum of per-group F.cross_entropy(z[g], y[g], weight=w, label_smoothing=eps).  If no group is present NOTHING is written (not
 * dlogits, not q, not stats).  If every row is in one group and q = [1.0], r_b is exactly 1.0f (x / x; W and W_0 are the same sum in
 * the same order): dlogits keeps its bits and a train step has the bits of the step without the term.
 *
 * What a step REPORTS — MSIG_WS_LOSS, msig_batch.loss_acc, probabilities, argmax, the correct count — stays the criterion's, as with
 * distillation.  The term reports into stats (optional, double[MSIG_DRO_STATS], accumulated like msig_batch.loss_acc), for g with
 * n_g > 0:
 *     [g] += T_g      [64 + g] += W_g      [128 + g] += n_g      [192] += sum_{g present} q_g L_g (the updated q, increasing g)
 *     [193] += 1
 * Frozen (msig_dro.frozen != 0): q is read only and no stats are written; on the q an updating call left behind it gives that call's
 * dlogits bit for bit.  The second pass of a sharpness-aware step uses it.
 *
 * Fold batches.  Fold z of a launch reads its logits, labels, class weights and dlogits in model arena msig_multi.slot[z]
 * (msig_multi.stride_bytes apart) and its q, grp and stats at slot[z] * msig_dro.stride_bytes from the given pointers.  idx is shared:
 * fold z reads idx + z * idx_row_stride.  One workgroup per fold, every sum over the fold's own rows in one fixed order: a fold of a
 * fold batch has the bits of its single call.
 *
 * Checks, all before any launch (in a fold batch msig_multi's own checks come first), in this order: NULL msig_dro where one is
 * required, NULL grp / q / logits / labels / dlogits -> MSIG_E_NULL; G outside 1..MSIG_DRO_MAX_GROUPS, eta NaN or negative, K outside
 * 2..MSIG_MAX_K, B outside 1..MSIG_DRO_MAX_BATCH (the kernel keeps a row's term, mass and group in LDS so that the group sums run in
 * row order), smoothing NaN or outside [0, 1), (train steps) a msig_st.lam of the launch that is not 1 — a row blended from two
 * subjects has no group —, idx_row_stride < B in a fold batch with idx -> MSIG_E_SHAPE; q / grp / logits / dlogits / class weights
 * not 4-byte aligned, stats / idx / labels not 8, or (fold batch) a stride_bytes that is not a positive multiple of 256 ->
 * MSIG_E_ALIGN.  In the train-step calls da and sam both non-NULL -> MSIG_E_SHAPE, and a NULL msig_dro makes the call
 * msig_sam_train_step[_multi] when sam is given, else msig_kd_train_step[_multi]: the same launches, the fused head where it applies.
 * With the term the head runs unfused whatever B is: head_fwd, ce, dro_apply, kd_apply when distilling, head_bwd.  The distillation
 * term is mixed into the rescaled gradient as before, and the clip norm of msig_st.clip covers the result.
 */
#ifndef MSIG_DRO_H
#define MSIG_DRO_H
#include "msig.h"
#include "msig_st.h"
#include "msig_da.h"
#include "msig_kd.h"
#include "msig_sam.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSIG_DRO_ABI_VERSION 1
#define MSIG_DRO_MAX_GROUPS 64
#define MSIG_DRO_MAX_BATCH 2048
#define MSIG_DRO_STATS (3 * MSIG_DRO_MAX_GROUPS + 2)

typedef struct msig_dro {
  int32_t G;                       /* groups of every fold of the launch */
  float eta;                       /* step size of the weights, of the launch */
  int32_t frozen;                  /* != 0: q is read only, no stats */
  const int32_t* grp;              /* device: one int32 per store position */
  const int64_t* idx;              /* device store positions of the batch's rows, or NULL */
  int64_t idx_row_stride;          /* fold batch: elements between the folds' rows of idx */
  float* q;                        /* device float[G] */
  double* stats;                   /* device double[MSIG_DRO_STATS], or NULL */
  int64_t stride_bytes;            /* fold batch: bytes between the folds' q, grp and stats (positive multiple of 256) */
} msig_dro;

int msig_dro_abi_version(void);
int64_t msig_dro_struct_bytes(void);     /* sizeof(msig_dro) of the build */

/* The term alone on caller-owned buffers: logits / dlogits (B, K) fp32, labels int64[B], class_weight K floats or NULL. */
int msig_dro_apply(const msig_dro* dro, const float* logits, const int64_t* labels, const float* class_weight, float smoothing,
                   float* dlogits, int32_t B, int32_t K, void* stream);
int msig_dro_apply_multi(const msig_dro* dro, const msig_multi* m, const float* logits, const int64_t* labels, const float* class_weight,
                         float smoothing, float* dlogits, int32_t B, int32_t K, void* stream);

/* msig_kd_train_step[_multi] (sam NULL) or msig_sam_train_step[_multi] with the term above between the criterion and the head's
 * backward.  da, kd, sam and dro may each be NULL. */
int msig_dro_train_step(const msig_batch* b, const msig_st* s, const msig_da* da, const msig_kd* kd, const msig_sam* sam, const msig_dro* dro,
                        float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                        void* stream);
int msig_dro_train_step_multi(const msig_batch* b, const msig_multi* m, const msig_st* s, const msig_da* da, const msig_kd* kd,
                              const msig_sam* sam, const msig_dro* dro, float* exp_avg, float* exp_avg_sq, float beta1, float beta2,
                              float eps, float weight_decay, int64_t step, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSIG_DRO_H */
