/* msig_cg.h — CnnGruModel, the cnn_gru baseline, in libmsig_hip.so.
 *
 * The reference's README compares CnnGruAttentionModel with a 'cnn_gru' baseline (MODEL_TO_USE = 'cnn_gru', README.md:13,81) that
 * its models.py never defines.  This project reads it as CnnGruAttentionModel with channel_attention removed:
 *     cnn_encoder -> permute -> GRU -> outputs[:, -1, :] -> classifier      (models.py:73-81 without line 75)
 * with the same layers, the same two configurations and the same reference quirks.  The calls below are the msig.h / msig_cw.h calls
 * of that model.  They stand beside msig.h and msig_cw.h, which are unchanged; libmsig_hip.so exports all three sets.
 *
 * Parameters: msig_cg_param_layout is msig_param_layout with the gate's two tensors (MSIG_P_GATE_W1, MSIG_P_GATE_W2) of size zero:
 * every other tensor keeps its enumerator and shape, and its offset moves down by the gate's padded size.  For C < 4, where the
 * attention model's gate has no hidden unit, both layouts are identical.  Gradients and both Adam moments use the same layout.
 *
 * Everything else is msig.h's: msig_shape, msig_batch, msig_multi, msig_workspace_layout / msig_workspace_bytes (the same regions
 * and sizes), the kernel forms, the MSIG_E_* codes, and "nothing launched on error".  The baseline leaves these workspace regions
 * unused: MSIG_WS_GATE_MEAN, MSIG_WS_GATE_PRE, MSIG_WS_GATE_S and MSIG_WS_DS.  MSIG_WS_GATE_EO still holds the even / odd sample sums
 * conv1's backward needs; an eval forward without keep_for_backward does not form them.
 *
 * class_weight: msig_cw.h's semantics — a DEVICE pointer to K floats, 4-byte aligned (MSIG_E_ALIGN, checked first); NULL = the
 * unweighted criterion; in a fold batch fold z reads its vector at class_weight + m->slot[z] * m->stride_bytes.  The backward has no
 * weight argument, as msig_backward serves msig_cw_forward: with dlogits = NULL it consumes the WS_DLOGITS of the forward, which the
 * weight of msig_cg_forward already scaled.
 */
#ifndef MSIG_CG_H
#define MSIG_CG_H
#include "msig.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSIG_CG_ABI_VERSION 1

int msig_cg_abi_version(void);

/* Offsets (floats) of the baseline's tensors in the flat parameter buffer; offsets[MSIG_NPARAM] is the padded total. */
int msig_cg_param_layout(int C, int K, int64_t* offsets /* host, [MSIG_NPARAM+1] */);

/* model(inputs) [+ CrossEntropyLoss(weight=class_weight) when b->labels != NULL]: msig_forward / msig_cw_forward of the baseline. */
int msig_cg_forward(const msig_batch* b, const float* class_weight, void* stream);

/* loss.backward() of a msig_cg_forward that kept for a backward (training, or keep_for_backward): msig_backward of the baseline,
 * the input gradient msig_batch.dx included (dx = the convolution's transposed taps applied to dL/d(conv1 output); no gate term). */
int msig_cg_backward(const msig_batch* b, const float* dlogits, void* stream);

/* optimizer.zero_grad(); forward; CE; backward; Adam — msig_train_step / msig_cw_train_step of the baseline. */
int msig_cg_train_step(const msig_batch* b, const float* class_weight, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                       float beta2, float eps, float weight_decay, int64_t step, void* stream);

/* Fold batches of baselines (msig_forward_multi / msig_train_step_multi).  Every fold of a launch is a baseline: msig_multi has no
 * per-slot model kind. */
int msig_cg_forward_multi(const msig_batch* b, const msig_multi* m, const float* class_weight, void* stream);
int msig_cg_train_step_multi(const msig_batch* b, const msig_multi* m, const float* class_weight, float* exp_avg, float* exp_avg_sq,
                             float beta1, float beta2, float eps, float weight_decay, int64_t step, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSIG_CG_H */
