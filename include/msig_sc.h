/* msig_sc.h — supervised contrastive loss on the classifier's 128-d feature inside the fused and fold-batched train steps of
 * libmsig_hip.so.
 *
 * Every other training-time option of the library acts on the logits, the weights or a discriminator.  This one is metric learning
 * on the embedding itself (Khosla et al., "Supervised Contrastive Learning", NeurIPS 2020): windows of the same class are pulled
 * together on the unit sphere and all others pushed apart — in its cross-subject form only windows of the same class from DIFFERENT
 * people count as positives.  Its gradient is one more addend of MSIG_WS_DFEAT, which is written and consumed inside one
 * msig_*_train_step[_multi] call; the train steps below are msig_dro.h's with TWO more launches between the head's launch and the GRU
 * backward (after the adversary's launch when both are on).  The term has no parameters, no moments and no state: it stands beside
 * msig.h and its companions, which are unchanged; libmsig_hip.so exports all of them.
 *
 * One step of one fold.  Rows b < B have a feature f_b (128 fp32), a label y_b (msig_batch.labels) and, in
 * cross-subject mode, a group g_b = grp[idx[b]] (idx: the int64 store positions the batch was gathered from, as msig_dro.idx) or
 * grp[b] when idx is NULL.  A row is VALID iff 0 <= y_b < K and, in cross-subject mode, g_b >= 0.  tau: the launch's temperature;
 * w: the fold's weight.
 *     z_b   = f_b / max(||f_b||_2, 1e-12)                      fp32
 *     s_ij  = (z_i . z_j) / tau
 *     class mode:          A(i) = { j != i, both valid }               P(i) = { j in A(i) : y_j = y_i }
 *     cross-subject mode:  A(i) = { j != i, both valid, not (y_j = y_i and g_j = g_i) }
 *                          P(i) = { j != i, both valid, y_j = y_i, g_j != g_i }
 *                          (a same-subject same-class row is neither a positive nor a negative)
 *     lse_i = ln sum_{a in A(i)} exp(s_ia)                     with the row maximum subtracted
 *     i is an anchor iff |P(i)| > 0;  N_a = number of anchors
 *     L_i   = lse_i - (1/|P(i)|) sum_{p in P(i)} s_ip
 *     L     = (1/N_a) sum_anchors L_i
 *     C_ij  = [i anchor] ( exp(s_ij - lse_i)[j in A(i)] - [j in P(i)]/|P(i)| ) / N_a
 *     dz_i  = (1/tau) sum_j (C_ij + C_ji) z_j
 *     df_i  = ( dz_i - z_i (z_i . dz_i) ) / max(||f_i||, 1e-12)
 *     if w != 0:  dfeat_i = fadd(dfeat_i, fmul(w, df_i))       two roundings, never an FMA
 * df is dL/df exactly (the closed form of autograd through the normalisation, the similarities and the log-sum-exp).
 *
 * w = 0 is a probe: the loss and the statistics are measured, dfeat is not touched, and a train step leaves the model the bits of
 * the step without the term.  N_a = 0: NOTHING is written (not dfeat, not stats).
 *
 * Two launches, grid (ceil(B / 32), 1, folds).  Each row i is owned by exactly one workgroup, which walks the columns j in increasing
 * order in tiles of 64; the similarities and the contraction G . Z run on the exact-fp32 matrix instruction.  sum L_i and the
 * statistics are fp64 sums in increasing i.  Every sum depends on the fold's own rows alone: a fold of a fold batch has the bits of
 * its single call.
 *
 * The term reports into stats (optional, double[MSIG_SC_STATS], accumulated like msig_batch.loss_acc):
 *     [0] += sum_anchors L_i      [1] += N_a
 *     [2] += the number of anchors whose largest s_ia over A(i) is a positive (the first maximum on ties)
 *     [3] += 1
 * What a step REPORTS — MSIG_WS_LOSS, msig_batch.loss_acc, probabilities, argmax, the correct count — stays the criterion's.
 *
 * Scratch is the caller's: msig_sc_scratch_bytes(B) bytes per fold, 16-byte aligned.  It holds the normalised rows and the per-row
 * statistics between the two launches; its contents mean nothing before or after a call.  The workspace layout of msig.h does not
 * change.
 *
 * The embedded 32-unit model keeps its feature in the first columns of MSIG_WS_FEAT and exact zeros in the rest.  Zero columns add
 * nothing to a norm or a dot product and get df = 0 (dz's zero columns minus z's zero columns), so the term works on it unchanged
 * and the padding of MSIG_WS_DFEAT stays exactly zero.
 *
 * Fold batches.  Fold z of a launch reads its feature, labels and dfeat in model arena msig_multi.slot[z] (msig_multi.stride_bytes
 * apart) and its grp, scratch and stats at slot[z] * msig_sc.stride_bytes from the given pointers; weight[z] is its weight.  idx is
 * shared: fold z reads idx + z * idx_row_stride.
 *
 * Checks, all before any launch (in a fold batch msig_multi's own checks come first), in this order: NULL msig_sc where one is
 * required, NULL scratch / feat / dfeat / labels, a NULL grp in cross-subject mode -> MSIG_E_NULL; positives outside {0, 1}, tau NaN
 * or outside [1e-3, 1e3], a weight of the launch NaN or negative, B outside 1..MSIG_SC_MAX_BATCH, K outside 2..MSIG_MAX_K, (train
 * steps) a msig_st.lam of the launch that is not 1 — a row blended from two windows has no label to contrast —, idx_row_stride < B in
 * a fold batch with idx -> MSIG_E_SHAPE; feat / dfeat / scratch not 16-byte aligned, stats / idx / labels not 8, grp not 4, or (fold
 * batch) a stride_bytes that is not a positive multiple of 256 -> MSIG_E_ALIGN.  In the train-step calls the term's checks follow
 * msig_dro.h's; a NULL msig_sc makes the call msig_dro_train_step[_multi], launch for launch and bit for bit.  The head stays fused
 * where it was; under msig_sam.h the term runs in both passes, the second with no stats.  The clip norm of msig_st.clip covers the
 * term, because it flows through MSIG_WS_DFEAT.
 */
#ifndef MSIG_SC_H
#define MSIG_SC_H
#include "msig_dro.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSIG_SC_ABI_VERSION 1
#define MSIG_SC_MAX_BATCH 2048
#define MSIG_SC_STATS 4
#define MSIG_SC_POS_CLASS 0
#define MSIG_SC_POS_CROSS_SUBJECT 1

typedef struct msig_sc {
  int32_t positives;               /* MSIG_SC_POS_* of the launch */
  float tau;                       /* temperature of the launch */
  const int32_t* grp;              /* device: one int32 per store position (cross-subject mode; else unused, may be NULL) */
  const int64_t* idx;              /* device store positions of the batch's rows, or NULL */
  int64_t idx_row_stride;          /* fold batch: elements between the folds' rows of idx */
  void* scratch;                   /* device: msig_sc_scratch_bytes(B) bytes */
  double* stats;                   /* device double[MSIG_SC_STATS], or NULL */
  int64_t stride_bytes;            /* fold batch: bytes between the folds' grp, scratch and stats (positive multiple of 256) */
  float weight[MSIG_MAX_FOLDS];    /* per fold of the launch; 0 = probe */
} msig_sc;

int msig_sc_abi_version(void);
int64_t msig_sc_struct_bytes(void);      /* sizeof(msig_sc) of the build */
int64_t msig_sc_scratch_bytes(int32_t B);      /* per fold; MSIG_E_SHAPE for B outside 1..MSIG_SC_MAX_BATCH */

/* The term alone on caller-owned buffers: feat / dfeat (B, 128) fp32, labels int64[B]. */
int msig_sc_apply(const msig_sc* sc, const float* feat, const int64_t* labels, float* dfeat, int32_t B, int32_t K, void* stream);
int msig_sc_apply_multi(const msig_sc* sc, const msig_multi* m, const float* feat, const int64_t* labels, float* dfeat, int32_t B,
                        int32_t K, void* stream);

/* msig_dro_train_step[_multi] with the term above between the head's launch and the GRU backward.  da, kd, sam, dro and sc may each
 * be NULL. */
int msig_sc_train_step(const msig_batch* b, const msig_st* s, const msig_da* da, const msig_kd* kd, const msig_sam* sam, const msig_dro* dro,
                       const msig_sc* sc, float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2, float eps, float weight_decay,
                       int64_t step, void* stream);
int msig_sc_train_step_multi(const msig_batch* b, const msig_multi* m, const msig_st* s, const msig_da* da, const msig_kd* kd,
                             const msig_sam* sam, const msig_dro* dro, const msig_sc* sc, float* exp_avg, float* exp_avg_sq, float beta1,
                             float beta2, float eps, float weight_decay, int64_t step, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSIG_SC_H */
