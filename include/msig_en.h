/* msig_en.h — deep ensembles: the reduction of M independently trained members' logits to per-window statistics, in libmsig_hip.so.
 *
 * A LOSO run with --seeds S trains S seed replicas of every fold.  Averaging their probabilities on the test
 * subject is a deep ensemble (Lakshminarayanan et al., 2017).  The members are ordinary models and their eval forwards are the
 * ordinary calls (msig_forward / msig_cg_forward and the *_multi forms); what this header adds is the one kernel that turns the
 * members' logits into the ensemble's prediction and its uncertainty — msig_mc_reduce's definitions (include/msig_mc.h) with
 * "sample s" read as "member m", for logits that lie MEMBER-major (one (N, K) block per member, where each member's forward left
 * it) instead of window-major, plus what only distinct members have: each member's own prediction and their pairwise disagreement.
 *
 * The calls stand beside msig.h and its companions, which are unchanged.
 *
 * Conventions are msig.h's: device pointers, asynchronous on `stream`, no allocation, no state; 0 = ok, > 0 a hipError_t of a
 * launch, < 0 an MSIG_E_* argument error found BEFORE anything is launched.
 */
#ifndef MSIG_EN_H
#define MSIG_EN_H
#include "msig.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSIG_EN_ABI_VERSION 1
#define MSIG_EN_MAX_MEMBERS 256

int msig_en_abi_version(void);

/* Per window n, over its M rows of logits (row n of every member's (N, K) block), everything in fp64 and rounded to fp32 once on
 * store:
 *   p_m     = softmax(logits of member m, window n), max-subtracted
 *   mean_p  (N, K)  mu = (sum_m p_m) / M, summed in increasing m
 *   std_p   (N, K)  sqrt((sum_m (p_m - mu)^2) / M), the population standard deviation over the members
 *   pred    (N)     first argmax of mu
 *   entropy (N)     H(mu) = -sum_k mu_k ln mu_k, 0 ln 0 = 0, in nats
 *   expected_entropy (N)  (sum_m H(p_m)) / M, in increasing m
 *   mutual_info (N) H(mu) - expected entropy, not clamped (the two are computed separately: it may be a rounding below zero)
 *   votes   (N, K) int32: the number of members whose first maximal logit is k
 *   member_pred (N, M) int32: member m's first maximal logit
 *   disagreement (N) the share of unordered member pairs whose member_pred differ: 1 - sum_k v_k (v_k - 1) / (M (M - 1)) from the
 *                   integer votes with one fp64 division; 0 for M = 1
 * Member m's block starts member_stride_floats after member m - 1's (>= N * K; N * K for a contiguous (M, N, K) stack).  Any output
 * but mean_p may be NULL, and leaving one out changes no other output's bits.  One workgroup owns a window, every sum has one owner
 * and one order: a window's bits depend on its own M rows alone — not on N, the grid, the stride or where the blocks lie.  On a
 * contiguous stack the outputs msig_mc_reduce also has carry the bits msig_mc_reduce gives on the window-major transpose
 * (N, M, K) of the same logits.
 * MSIG_E_NULL: logits or mean_p NULL.  MSIG_E_SHAPE: M outside 1..MSIG_EN_MAX_MEMBERS, K outside 2..MSIG_MAX_K, N < 1,
 * M * N >= 2^31, member_stride_floats < N * K.  MSIG_E_ALIGN: a pointer that is not 4-byte aligned. */
int msig_en_reduce(const float* logits, int64_t member_stride_floats, int32_t M, int32_t N, int32_t K, float* mean_p, float* std_p,
                   int32_t* pred, float* entropy, float* expected_entropy, float* mutual_info, int32_t* votes, int32_t* member_pred,
                   float* disagreement, void* stream);

/* The same where a fold-batch forward (msig_forward_multi and its companions) left the logits: member z's (N, K) block is at
 * (const char*)logits0 + m->slot[z] * m->stride_bytes — logits0 is WS_LOGITS of arena 0 — and M = m->n (1..MSIG_MAX_FOLDS).  Members
 * are taken in the order of m->slot, which need not be increasing; only n, slot and stride_bytes of `m` are read beyond msig_multi's
 * own checks (n, distinct non-negative slots, stride_bytes a positive multiple of 256, form_folds), which come first.  The bits are
 * msig_en_reduce's on the gathered stack.  MSIG_E_SHAPE also when stride_bytes < 4 * N * K. */
int msig_en_reduce_multi(const float* logits0, const msig_multi* m, int32_t N, int32_t K, float* mean_p, float* std_p, int32_t* pred,
                         float* entropy, float* expected_entropy, float* mutual_info, int32_t* votes, int32_t* member_pred,
                         float* disagreement, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSIG_EN_H */
