/* msig_kd.h — knowledge distillation: a dense per-row teacher target inside the fused and fold-batched train steps of
 * libmsig_hip.so, and the kernel that builds the teacher table from an ensemble's logits.
 *
 * A LOSO run with --seeds S trains S replicas of every fold and evaluates them as a deep ensemble (include/msig_en.h, DESIGN.md
 * section 23): S forwards per window.  Distillation (Hinton et al., 2015) trains ONE student against the ensemble's tempered
 * probabilities as well as the labels.  msig_st.h expresses two hard labels per row; a dense K-vector per row has no route into the
 * criterion, and MSIG_WS_DLOGITS is written and consumed inside one msig_*_train_step[_multi] call.  The train steps below are
 * msig_da.h's with ONE more launch between the criterion and the head's backward, where MSIG_WS_LOGITS and MSIG_WS_DLOGITS are both
 * complete.  It stands beside msig.h and its companions, which are unchanged; libmsig_hip.so exports all of them.
 *
 * One step of one fold.  B rows, logits z (B, K), the launch's weight alpha in [0, 1] and temperature T in
 * [1/64, 64], the teacher table q: K fp32 probabilities per store position.  Row b's teacher row is q_b = q[idx[b]] (idx: the int64
 * store positions the batch was gathered from, as msig_da.idx) or q[b] when idx is NULL.  With msig_st.h's partner rule and the
 * fold's mixup weight lam:
 *     qm_b   = fadd(fmul(lam, q_b), fmul(1.f - lam, q_{B-1-b}))          (lam == 1: q_b itself)
 *     s_b    = softmax(z_b / T)
 *     L_kd   = (T^2 / B) sum_b sum_c qm_bc (ln qm_bc - ln s_bc)          0 ln 0 = 0
 *     L      = (1 - alpha) L_hard + alpha L_kd                           L_hard: msig_st.h's L (weights, smoothing, mixup)
 *     dL/dz[b][c] = (1 - alpha) dL_hard/dz[b][c] + alpha (T / B) (s_bc - qm_bc)
 * Class weights and smoothing do not touch the KD term and its mean is over B.  The launch rewrites dlogits in place, in fp32, every
 * operation a single rounding and never an FMA:
 *     u_c = z_c / T,  m = max_c u_c,  e_c = expf(u_c - m),  S = sum_c e_c in increasing c,  s_c = e_c / S
 *     dlogits[b][c] = fadd(fmul(1.f - alpha, dlogits[b][c]), fmul(kappa, fsub(s_c, qm_c))),   kappa = (float)((double)alpha * T / B)
 * and nothing else of the workspace.  What a step REPORTS — MSIG_WS_LOSS, msig_batch.loss_acc, probabilities, argmax, the correct
 * count — stays the criterion's against the labels.  The KD term reports into stats (optional, double[3], accumulated like
 * msig_batch.loss_acc):
 *     [0] += B L_kd      [1] += rows whose first argmax of z equals the first argmax of qm      [2] += B
 * The row terms are fp64 (ln s_c = (u_c - m) - ln S), each thread sums its rows in increasing row order, the sums are reduced per
 * wave and the wave sums added in wave order by one thread: one owner and one order per fold, and a fold's values depend on its own
 * rows alone, so a fold of a fold batch has the bits of its single call.
 *
 * Fold batches.  Fold z of a launch reads its logits in model arena msig_multi.slot[z] (msig_multi.stride_bytes apart) and its
 * teacher table and stats at slot[z] * msig_kd.stride_bytes from the given pointers.  idx is shared: fold z reads
 * idx + z * idx_row_stride, as the gather does.  alpha and T are the launch's; lam is per fold.
 *
 * Checks, all before any launch (in a fold batch msig_multi's own checks come first): NULL msig_kd where one is required, NULL q /
 * logits / dlogits -> MSIG_E_NULL; alpha NaN or outside [0, 1], T NaN or outside [1/64, 64], K outside 2..MSIG_MAX_K, B < 1, lam NaN
 * or outside [0, 1], idx_row_stride < B in a fold batch with idx -> MSIG_E_SHAPE; q / logits / dlogits not 4-byte aligned, stats /
 * idx not 8, or (fold batch) a stride_bytes that is not a positive multiple of 256 -> MSIG_E_ALIGN.  In the train-step calls a NULL
 * msig_kd, or one with alpha == 0 (after its checks), makes the call msig_da_train_step[_multi] itself: the same launches, the fused
 * head where it applies.  With alpha > 0 the head runs unfused whatever B is.  The clip norm of msig_st.clip covers the distilled
 * gradient.
 */
#ifndef MSIG_KD_H
#define MSIG_KD_H
#include "msig.h"
#include "msig_st.h"
#include "msig_da.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSIG_KD_ABI_VERSION 1
#define MSIG_KD_MAX_MEMBERS 256

typedef struct msig_kd {
  float alpha, temperature;        /* of the launch */
  const float* q;                  /* device: (positions, K) fp32 */
  const int64_t* idx;              /* device store positions of the batch's rows, or NULL */
  int64_t idx_row_stride;          /* fold batch: elements between the folds' rows of idx */
  double* stats;                   /* device double[3], or NULL */
  int64_t stride_bytes;            /* fold batch: bytes between the folds' q and stats (positive multiple of 256) */
} msig_kd;

int msig_kd_abi_version(void);
int64_t msig_kd_struct_bytes(void);     /* sizeof(msig_kd) of the build */

/* The teacher table.  Per window n over its M rows of logits (row n of every member's (N, K) block), in fp64:
 *     p_m = softmax(logits of member m, window n, each divided by T), max-subtracted
 *     q[n] = (sum_m p_m) / M, summed in increasing m, rounded to fp32 once on store
 * At T = 1 these are msig_en_reduce's statements for mean_p and q carries its bits.  The argument conventions and checks are
 * msig_en_reduce[_multi]'s (include/msig_en.h): member m's block starts member_stride_floats after member m - 1's; in the multi form
 * member z's block is at (const char*)logits0 + m->slot[z] * m->stride_bytes, members in the order of m->slot, M = m->n.
 * MSIG_E_NULL: logits or q NULL.  MSIG_E_SHAPE: M outside 1..MSIG_KD_MAX_MEMBERS (multi: MSIG_MAX_FOLDS), K outside 2..MSIG_MAX_K,
 * N < 1, M * N >= 2^31, member_stride_floats < N * K (multi: stride_bytes < 4 * N * K), T NaN or outside [1/64, 64].
 * MSIG_E_ALIGN: a pointer that is not 4-byte aligned. */
int msig_kd_teacher(const float* logits, int64_t member_stride_floats, int32_t M, int32_t N, int32_t K, float T, float* q, void* stream);
int msig_kd_teacher_multi(const float* logits0, const msig_multi* m, int32_t N, int32_t K, float T, float* q, void* stream);

/* The distillation term alone on caller-owned logits / dlogits ((B, K) fp32 each).  lam: the mixup weight, host value(s). */
int msig_kd_apply(const msig_kd* kd, const float* logits, float* dlogits, int32_t B, int32_t K, float lam, void* stream);
int msig_kd_apply_multi(const msig_kd* kd, const msig_multi* m, const float* logits, float* dlogits, int32_t B, int32_t K, const float* lam,
                        void* stream);

/* msig_da_train_step[_multi] with the term above between the criterion and the head's backward (its lam: msig_st.lam).  da may be
 * NULL. */
int msig_kd_train_step(const msig_batch* b, const msig_st* s, const msig_da* da, const msig_kd* kd, float* exp_avg, float* exp_avg_sq,
                       float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, void* stream);
int msig_kd_train_step_multi(const msig_batch* b, const msig_multi* m, const msig_st* s, const msig_da* da, const msig_kd* kd,
                             float* exp_avg, float* exp_avg_sq, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSIG_KD_H */
