/* msig_cw.h — class-weighted CrossEntropy in the forward and train-step calls of libmsig_hip.so.
 *
 * The reference declares a class-weighted loss: with config['trainer']['use_class_weights'] its Trainer computes
 * compute_class_weight('balanced', ...) and builds CrossEntropyLoss(weight=...) (trainer.py:65,80-97), the criterion of the train
 * step (trainer.py:147) and of validation / test (trainer.py:218).  The calls below are the msig.h calls with that criterion.  They
 * stand beside msig.h as msig_prep.h does: msig_batch, msig_multi, the workspace layout and every msig.h call are unchanged, and
 * libmsig_hip.so exports both sets.
 *
 * Semantics (torch's CrossEntropyLoss(weight=w), reduction 'mean'), for a batch of B windows with labels y and class weights w
 * (K floats, non-negative and finite):
 *     W               = sum_b w[y_b]                           (fp64, in one fixed order)
 *     WS_LOSS[0]      = sum_b w[y_b] nll_b / W                 (the weighted mean)
 *     WS_LOSS[1]      = B * WS_LOSS[0], and msig_batch.loss_acc[0] += the same (loss.item() * B, trainer.py:152,221)
 *     WS_DLOGITS[b][c] = w[y_b] (p[b][c] - [c == y_b]) / W
 * Probabilities, argmax and the count of correct windows (WS_LOSS[2], loss_acc[1]) are those of msig.h.  W = 0 (every label of
 * the batch has weight 0) gives NaN, as in torch.  A weighted mean depends on how a pass is cut into batches — in torch too.
 * All-ones weights give the unweighted calls' results bit for bit.
 *
 * Conventions are msig.h's.  class_weight is a DEVICE pointer to K floats, 4-byte aligned; NULL makes every call here exactly
 * its msig.h counterpart.  The argument checks, MSIG_E_* codes and "nothing launched on error" are the counterpart's, plus
 * MSIG_E_ALIGN for a misaligned class_weight (checked first).  The library cannot see the values before its kernels read them:
 * a binding checks them on the host (multimodalsignal_amd/_lib.py check_class_weight).  In a fold batch, fold z reads its own
 * vector at class_weight + m->slot[z] * m->stride_bytes — in its own arena, like every other buffer — because 'balanced'
 * weights differ between the folds' training sets.
 */
#ifndef MSIG_CW_H
#define MSIG_CW_H
#include "msig.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSIG_CW_ABI_VERSION 1

int msig_cw_abi_version(void);

/* msig_forward with the weighted criterion whenever b->labels != NULL: model(inputs) + CrossEntropyLoss(weight=w)
 * (trainer.py:146-147 in training, :217-218 in evaluation).  In training, or with keep_for_backward, WS_DLOGITS holds the
 * weighted gradient, so a following msig_backward(b, NULL, ...) is loss.backward() of the weighted loss (trainer.py:148),
 * the input gradient msig_batch.dx included. */
int msig_cw_forward(const msig_batch* b, const float* class_weight, void* stream);

/* msig_train_step with the weighted criterion: optimizer.zero_grad(); forward; weighted CE; backward; Adam (trainer.py:144-149). */
int msig_cw_train_step(const msig_batch* b, const float* class_weight, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                       float beta2, float eps, float weight_decay, int64_t step, void* stream);

/* msig_forward_multi / msig_train_step_multi with the weighted criterion; each fold's vector lives in its own arena. */
int msig_cw_forward_multi(const msig_batch* b, const msig_multi* m, const float* class_weight, void* stream);
int msig_cw_train_step_multi(const msig_batch* b, const msig_multi* m, const float* class_weight, float* exp_avg, float* exp_avg_sq,
                             float beta1, float beta2, float eps, float weight_decay, int64_t step, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSIG_CW_H */
