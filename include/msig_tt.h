/* msig_tt.h — label-free entropy-minimisation adaptation to a new subject (TENT / information maximisation) in libmsig_hip.so.
 *
 * After a LOSO run the label-free companion of msig_ab.h that MOVES parameters: every weight stays frozen except the tensors a
 * selection names (by default the scale and shift of the two BatchNorm layers), and those descend the Shannon entropy of the model's
 * own predictions on the new subject's unlabelled windows (test-time entropy minimisation: Wang et al., ICLR 2021), optionally with
 * the diversity term of information maximisation (Liang et al., ICML 2020) against collapse onto one class.  The model runs in EVAL
 * mode throughout — running-statistic BatchNorm, no dropout; the batch-statistic form of TENT is out of scope: the whole recording
 * is there, msig_ab.h supplies whole-set statistics, and a prediction never depends on its batch companions.  The reference has no
 * such step.  The calls stand beside msig.h, msig_ft.h and msig_ab.h, which are unchanged.
 *
 * The objective.  One batch of one model: logits z (B, K) fp32 and a diversity weight div >= 0.  ALL
 * arithmetic is fp64; each output element is rounded once to fp32.
 *     m_b   = max_k z_bk
 *     lp_bk = z_bk - m_b - ln sum_k exp(z_bk - m_b)
 *     p_bk  = exp(lp_bk)
 *     H_b   = - sum_k p_bk lp_bk
 *     q_k   = (1/B) sum_b p_bk
 *     lq_k  = ln q_k                      (0 where q_k == 0)
 *     Hq    = - sum_k q_k lq_k
 *     L     = (1/B) sum_b H_b - div * Hq
 *     c_b   = sum_k p_bk lq_k
 *     dlogits_bj = [ - p_bj (lp_bj + H_b) + div * p_bj (lq_j - c_b) ] / B            = dL/dz_bj exactly
 * div = 0 is TENT.  The sums over b run in ONE fixed order that depends on B and K alone (per thread in increasing row order, the
 * threads of a wave by a butterfly, the waves in wave order): one workgroup per model, grid (1, 1, folds), no atomics; a fold of a
 * fold batch has the bits of its single call.  Limits: B in 1..MSIG_TT_MAX_BATCH, K in 2..MSIG_MAX_K.
 * Non-finite logits are NOT handled: a NaN or an infinity in a row propagates into that row's dlogits and, through q, into every
 * row's when div > 0, and into the statistics.  Nothing is read or written out of bounds for any input.
 *
 * Conventions are msig.h's: device pointers, asynchronous on `stream`, no allocation, no state; 0 = ok, > 0 a hipError_t of a
 * launch, < 0 an MSIG_E_* argument error found BEFORE anything is launched.  In a *_multi call every pointer is fold 0's and fold z's
 * buffer sits m->slot[z] * m->stride_bytes further on — parameters, gradients, both Adam moments, logits, dlogits and the
 * statistics alike.
 */
#ifndef MSIG_TT_H
#define MSIG_TT_H
#include "msig.h"
#include "msig_ft.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSIG_TT_ABI_VERSION 1
#define MSIG_TT_MAX_BATCH 2048      /* rows of one objective launch (and so of one step) */

/* ---- statistics --------------------------------------------------------------------------------------------------------------
 * Optional (NULL = unused): MSIG_TT_STATS fp64 values per model, caller-owned, 8-byte aligned, accumulated like
 * msig_batch.loss_acc — one thread adds, in stream order; the caller zeroes them when a pass starts:
 *   [MSIG_TT_S_ENT]  += sum_b H_b        [MSIG_TT_S_ROWS]  += B
 *   [MSIG_TT_S_HQ]   += Hq               [MSIG_TT_S_STEPS] += 1
 *   [MSIG_TT_S_P + k]    += sum_b p_bk                              (k < K; the other slots are not touched)
 *   [MSIG_TT_S_PRED + k] += rows whose FIRST argmax is k
 * The mean objective of a pass is S_ENT / S_ROWS - div * S_HQ / S_STEPS. */
#define MSIG_TT_S_ENT   0
#define MSIG_TT_S_ROWS  1
#define MSIG_TT_S_HQ    2
#define MSIG_TT_S_STEPS 3
#define MSIG_TT_S_P     4
#define MSIG_TT_S_PRED  20
#define MSIG_TT_STATS   36

int msig_tt_abi_version(void);
int64_t msig_tt_struct_bytes(void);      /* sizeof(msig_tt) as this library was compiled */

/* dlogits (B, K) fp32 = dL/dz of the objective above from logits (B, K) fp32; stats optional.  dlogits may not alias logits.
 * Checks, in this order: logits or dlogits NULL -> MSIG_E_NULL (_multi: m NULL -> MSIG_E_NULL, then msig_multi's own checks);
 * B outside 1..MSIG_TT_MAX_BATCH, K outside 2..MSIG_MAX_K, diversity negative or not finite -> MSIG_E_SHAPE; logits or dlogits not
 * 4-byte aligned, stats not 8-byte aligned -> MSIG_E_ALIGN. */
int msig_tt_objective(const float* logits, int32_t B, int32_t K, float diversity, float* dlogits, double* stats, void* stream);
int msig_tt_objective_multi(const float* logits, int32_t B, int32_t K, float diversity, float* dlogits, double* stats,
                            const msig_multi* m, void* stream);

/* ---- the selective Adam -------------------------------------------------------------------------------------------------------
 * torch.optim.Adam's update (the arithmetic of msig_adam_step, bit for bit) on the tensors t of the flat parameter layout whose
 * bit (1u << t) is set in `select`, t an msig_param of msig.h; kind: MSIG_FT_KIND_* — msig_param_layout or msig_cg_param_layout
 * (whose gate tensors are empty: their bits select nothing).  params, grads, exp_avg and exp_avg_sq are all in the FULL flat
 * layout.  A selected tensor is updated over its slot of the layout, [offset t, offset t + 1): with every bit set the call is
 * msig_adam_step over the whole buffer.  Elements of unselected tensors are never written, and neither are their moments.
 * Checks, in this order: a NULL pointer -> MSIG_E_NULL (_multi: m first, then msig_multi's own checks); C or K out of range, a
 * kind that is not MSIG_FT_KIND_*, select == 0 or with a bit at or above MSIG_NPARAM, step < 1 (_multi: m->step[z] < 0)
 * -> MSIG_E_SHAPE; a pointer not 16-byte aligned -> MSIG_E_ALIGN.
 * _multi: learning rate and step count per fold, m->lr[z] and m->step[z] (0 = the call's `step`), as msig_train_step_multi. */
#define MSIG_TT_SELECT_BN   ((1u << MSIG_P_BN1_G) | (1u << MSIG_P_BN1_B) | (1u << MSIG_P_BN2_G) | (1u << MSIG_P_BN2_B))
#define MSIG_TT_SELECT_GATE ((1u << MSIG_P_GATE_W1) | (1u << MSIG_P_GATE_W2))
#define MSIG_TT_SELECT_ALL  ((1u << MSIG_NPARAM) - 1u)
int msig_tt_adam(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int32_t C, int32_t K, int32_t kind,
                 uint32_t select, float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, void* stream);
int msig_tt_adam_multi(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int32_t C, int32_t K, int32_t kind,
                       uint32_t select, float beta1, float beta2, float eps, float weight_decay, int64_t step, const msig_multi* m,
                       void* stream);

/* ---- the step -----------------------------------------------------------------------------------------------------------------
 * What one adaptation step needs beyond its msig_batch. */
typedef struct msig_tt {
  int32_t  kind;           /* MSIG_FT_KIND_*: which model's front end and parameter layout                                     */
  uint32_t select;         /* the tensors Adam updates (MSIG_TT_SELECT_*)                                                        */
  float    diversity;      /* div >= 0; 0 = plain entropy minimisation                                                           */
  float    beta1, beta2, eps, weight_decay;      /* Adam's                                                                       */
  float*   exp_avg;        /* both moments in the full flat layout, 16-byte aligned; only the selected tensors' are touched      */
  float*   exp_avg_sq;
  double*  stats;          /* optional: MSIG_TT_STATS doubles                                                                    */
} msig_tt;

/* One adaptation step of the model(s) of `b`, a descriptor with training = 0, keep_for_backward = 1 and dx = NULL (any other
 * combination of the three: MSIG_E_SHAPE).  In order:
 *   1. the eval forward (msig_forward's launches: running-statistic BatchNorm, no dropout);
 *   2. the objective launch on MSIG_WS_LOGITS, which writes MSIG_WS_DLOGITS;
 *   3. the arithmetic of msig_backward with dlogits = NULL, its one column reduction included: b->grads, every tensor;
 *   4. the selective Adam on b->params.
 * The result is, bit for bit, msig_forward -> msig_tt_objective -> msig_backward -> msig_tt_adam (with msig_cg.h's calls for
 * MSIG_FT_KIND_CNN_GRU).  b->bn_state and b->bn_count are never written.  b->labels may be NULL; when given they are read only by
 * the head's own criterion, so that b->loss_acc reports the online CrossEntropy and correct count — dlogits and every updated bit
 * are the same with and without labels.  b->params is written although msig_batch declares it const.
 * Checks, all before the first launch, in this order: b or t NULL -> MSIG_E_NULL (_multi: m NULL, then msig_multi's own checks);
 * training != 0, keep_for_backward == 0 or dx != NULL -> MSIG_E_SHAPE; kind, select (as msig_tt_adam), diversity negative or not
 * finite, B > MSIG_TT_MAX_BATCH -> MSIG_E_SHAPE; a NULL moment -> MSIG_E_NULL; step < 1 (_multi: m->step[z] < 0) -> MSIG_E_SHAPE;
 * a moment not 16-byte aligned or stats not 8-byte aligned -> MSIG_E_ALIGN; then msig_batch's own checks as msig_backward makes
 * them (shape, NULL buffers — grads is required —, alignment, workspace size: the TRAINING layout, kernel forms).
 * _multi: learning rate and step count per fold (m->lr, m->step), the backward GRU kernel form by m->form_folds / b->bwd_form as
 * in msig_train_step_multi. */
int msig_tt_step(const msig_batch* b, const msig_tt* t, float lr, int64_t step, void* stream);
int msig_tt_step_multi(const msig_batch* b, const msig_multi* m, const msig_tt* t, int64_t step, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSIG_TT_H */
