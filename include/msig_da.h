/* msig_da.h — subject-adversarial training (a domain discriminator with gradient reversal) inside the fused and fold-batched
 * train steps of libmsig_hip.so.
 *
 * msig_train_step[_multi] goes from the forward to Adam in one call: MSIG_WS_DFEAT, the gradient of the loss on the 128-d feature the
 * classifier sees, is written by the head's launch and consumed by the GRU backward inside that call, so a term can be added to it
 * only from inside.  The calls below are msig_st.h's train steps plus ONE launch between the head and the GRU backward, where
 * MSIG_WS_FEAT and MSIG_WS_DFEAT are both complete.  That launch trains a subject discriminator D on the feature and adds the
 * REVERSED gradient of its loss to MSIG_WS_DFEAT (Ganin & Lempitsky, "Unsupervised domain adaptation by backpropagation").  It stands
 * beside msig.h, msig_cw.h, msig_cg.h, msig_ft.h, msig_gc.h, msig_aug.h, msig_st.h, msig_ab.h, msig_at.h and msig_mc.h, which are
 * unchanged; libmsig_hip.so exports all of them.
 *
 * Discriminator.  D = Linear(128, 64) -> ReLU -> Linear(64, S), 2 <= S <= MSIG_MAX_K, no dropout.  Its
 * parameters and both Adam moments are flat buffers of msig_da_param_floats(S) floats laid out like the classifier's four tensors:
 * W0 (64,128) 8192 floats, b0 64, W3 (S,64) padded to a multiple of 4, b3 S padded to a multiple of 4.  They are the caller's: no
 * part of the model's flat parameter buffer.
 *
 * One step of one fold.  Row b < B has the feature f_b (MSIG_WS_FEAT) and a domain label d_b in [-1, S); -1 = the row has none
 * (a value outside [-1, S) is read as -1).  d_b = dom[idx[b]] when idx is non-NULL (the int64 store positions the batch was gathered
 * from), else dom[b].  With msig_st.h's partner rule d'_b = d_{B-1-b}, lam the fold's mixup weight (1 = none), mu = 1.f - lam,
 * a_b = lam [d_b >= 0], a'_b = mu [d'_b >= 0]:
 *     h = relu(f W0^T + b0),  z = h W3^T + b3,  p = softmax(z),  l_b(c) = -log p_b[c]
 *     n      = sum_b ( a_b + a'_b )
 *     L_dom  = sum_b ( a_b l_b(d_b) + a'_b l_b(d'_b) ) / n
 *     dz[b][c] = ( a_b (p_c - [c = d_b]) + a'_b (p_c - [c = d'_b]) ) / n
 * then the gradients of L_dom on W0, b0, W3, b3 and torch.optim.Adam on them (L2-in-gradient weight decay, bias corrections from the
 * fold's own step count, the fold's own learning rate), and g_b = dL_dom/df_b taken through D's parameters BEFORE their update.  If
 * the fold's lambda != 0:  dfeat_b = fadd(dfeat_b, fmul(-lambda, g_b)), two fp32 roundings, never an FMA.  If lambda == 0, dfeat is
 * not touched: D trains as a probe of how subject-identifiable the feature is and the model's bits are the plain step's.  If n == 0
 * nothing at all is written.  stats (optional, double[3], accumulated like msig_batch.loss_acc):
 *     [0] += n L_dom      [1] += rows with argmax z == d_b >= 0      [2] += rows with d_b >= 0
 * The domain loss takes no class weights and no label smoothing.  n and the loss are fp64 sums in one fixed order; every sum depends
 * on the fold's own rows alone, so a fold of a fold batch has the bits of its single call.
 *
 * Fold batches.  Fold z of a launch reads its features in model arena msig_multi.slot[z] (msig_multi.stride_bytes apart) and its
 * adversary buffers — params, exp_avg, exp_avg_sq, stats and dom — at slot[z] * msig_da.stride_bytes from the given pointers.  idx
 * is shared: fold z reads idx + z * idx_row_stride, as the gather does.  lambda, lr and step are per fold of the launch.
 *
 * Checks, all before any launch (in a fold batch msig_multi's own checks come first): NULL msig_da where one is required, NULL
 * dom / params / exp_avg / exp_avg_sq / feat / dfeat -> MSIG_E_NULL; S outside 2..MSIG_MAX_K, B outside 1..MSIG_DA_MAX_BATCH, a
 * step < 1, a lambda or lr that is NaN or negative, lam NaN or outside [0, 1], idx_row_stride < B in a fold batch with idx
 * -> MSIG_E_SHAPE; params / exp_avg / exp_avg_sq / feat / dfeat not 16-byte aligned, stats / idx not 8, dom not 4, or (fold batch)
 * a stride_bytes that is not a positive multiple of 256 -> MSIG_E_ALIGN.  In the train-step calls a NULL msig_da is accepted: the
 * call is then msig_st_train_step[_multi] itself, the same launches.  The clip norm of msig_st.clip covers the model's gradient
 * only; the reversed term is part of it (it flows through MSIG_WS_DFEAT).
 */
#ifndef MSIG_DA_H
#define MSIG_DA_H
#include "msig.h"
#include "msig_st.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSIG_DA_ABI_VERSION 1
#define MSIG_DA_MAX_BATCH 256

typedef struct msig_da {
  int32_t S;                            /* domains (training subjects of the fold), 2..MSIG_MAX_K */
  float weight_decay, beta1, beta2, eps;      /* D's Adam */
  const int32_t* dom;                   /* device: domain label per store position (idx given) or per batch row (idx NULL) */
  const int64_t* idx;                   /* device: the batch's store positions, or NULL */
  int64_t idx_row_stride;               /* fold batch: elements between the folds' rows of idx */
  float* params;                        /* device: msig_da_param_floats(S) floats */
  float* exp_avg;
  float* exp_avg_sq;
  double* stats;                        /* device: double[3], or NULL */
  int64_t stride_bytes;                 /* fold batch: bytes between the folds' adversary buffers (positive multiple of 256) */
  float lambda[MSIG_MAX_FOLDS];         /* per fold of the launch ([0] for a single model): weight of the reversed gradient, >= 0 */
  float lr[MSIG_MAX_FOLDS];             /* D's learning rate, >= 0 */
  int64_t step[MSIG_MAX_FOLDS];         /* D's optimiser step count, >= 1 */
} msig_da;

int msig_da_abi_version(void);
int64_t msig_da_struct_bytes(void);     /* sizeof(msig_da) of the build */
int64_t msig_da_param_floats(int32_t S);      /* floats of D's parameter buffer (and of each moment buffer); MSIG_E_SHAPE for a bad S */

/* The discriminator's step alone on caller-owned feat / dfeat ((B, 128) fp32 each).  lam: the mixup weight, host value(s). */
int msig_da_step(const msig_da* a, const float* feat, float* dfeat, int32_t B, float lam, void* stream);
int msig_da_step_multi(const msig_da* a, const msig_multi* m, const float* feat, float* dfeat, int32_t B, const float* lam, void* stream);

/* msig_st_train_step[_multi] with the step above between the head's launch and the GRU backward (its lam: msig_st.lam). */
int msig_da_train_step(const msig_batch* b, const msig_st* s, const msig_da* a, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                       float beta2, float eps, float weight_decay, int64_t step, void* stream);
int msig_da_train_step_multi(const msig_batch* b, const msig_multi* m, const msig_st* s, const msig_da* a, float* exp_avg,
                             float* exp_avg_sq, float beta1, float beta2, float eps, float weight_decay, int64_t step, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSIG_DA_H */
