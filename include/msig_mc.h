/* msig_mc.h — Monte-Carlo dropout: S stochastic passes of a trained model for the price of one trunk, in libmsig_hip.so.
 *
 * The model has two dropout sites (between the GRU layers, models.py:62, and in the classifier, models.py:69) and everything before
 * the first of them — ChannelAttention, cnn_encoder and GRU layer 0 — is deterministic in eval mode.  Monte-Carlo dropout wants S
 * passes with the masks ON and BatchNorm in its EVAL form, which msig_batch.training cannot express (1 = masks and batch statistics,
 * 0 = neither).  The calls of this header split an eval forward at the first dropout site:
 *
 *   msig_mc_trunk   x -> WS_H0 (gru_layers 0 or 2) or WS_FEAT (gru_layers 1): the eval front end and GRU layer 0, once per window;
 *   msig_mc_expand  every row of that region S times into the region of an S-times wider batch's workspace;
 *   msig_mc_tail    on the wide batch: GRU layer 1 and the classifier with the dropout masks on, BatchNorm not involved at all;
 *   msig_mc_reduce  the (N * S, K) logits -> per window: mean probability, its spread, prediction, predictive entropy, expected
 *                   entropy, mutual information and the vote split.
 *
 * The calls stand beside msig.h and its companions, which are unchanged, and launch no kernel of the model that an eval forward
 * does not launch: the same forms, the same arithmetic.
 *
 * Conventions are msig.h's: device pointers, asynchronous on `stream`, no allocation, no state; 0 = ok, > 0 a hipError_t of a
 * launch, < 0 an MSIG_E_* argument error found BEFORE anything is launched.
 */
#ifndef MSIG_MC_H
#define MSIG_MC_H
#include "msig.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSIG_MC_ABI_VERSION 1
#define MSIG_MC_MAX_SAMPLES 256

/* the model kind of a call: which parameter layout msig_batch.params has */
#define MSIG_MC_KIND_ATTENTION 0   /* CnnGruAttentionModel: msig_param_layout    */
#define MSIG_MC_KIND_CNN_GRU   1   /* CnnGruModel:          msig_cg_param_layout */

int msig_mc_abi_version(void);

/* The deterministic part of an eval forward: front end and GRU layer 0, nothing after them.  `b` is the descriptor msig_forward
 * takes, with training = 0, keep_for_backward = 0 and dx = NULL (else MSIG_E_SHAPE).  Leaves WS_H0 (B, TP, 128) — for
 * gru_layers = 1 also WS_FEAT (B, 128), the one-layer model's outputs[:, -1, :] — with the bits msig_forward (msig_cg_forward)
 * leaves there.  BatchNorm state and bn_count are not written. */
int msig_mc_trunk(const msig_batch* b, int32_t kind, void* stream);

/* dst[(n * S + s) * row_floats + i] = src[n * row_floats + i] for n < N, s < S, i < row_floats: src is read once, dst written S
 * times.  With row_floats % 4 == 0 and both pointers 16-byte aligned every access is 16 bytes wide; otherwise (pointers 4-byte
 * aligned, else MSIG_E_ALIGN) the element-wise form runs, with the same bits.  Indexing is 64-bit: N * S * row_floats may exceed
 * 2^31.  1 <= S <= MSIG_MC_MAX_SAMPLES, N >= 1, row_floats >= 1, N * S < 2^31.  src and dst must not overlap. */
int msig_mc_expand(const float* src, float* dst, int32_t N, int32_t S, int64_t row_floats, void* stream);

/* The stochastic part, on the stacked batch: `b` describes it — shape.B = rows (N * S), shape.C / T / K the model's, an ordinary
 * EVAL workspace of its own (msig_workspace_layout(shape, 0)) whose WS_H0 (gru_layers 0 or 2) or WS_FEAT (gru_layers 1) the caller
 * has filled (msig_mc_expand), the same params / bn_state / bn_count as the trunk's (the BatchNorm pointers are checked, never
 * dereferenced) and any non-NULL 16-byte aligned x (not read).  training = 0 is required (MSIG_E_SHAPE), keep_for_backward = 0 and
 * dx = NULL too.  Runs GRU layer 1 from WS_H0 and the classifier (one layer: the classifier from WS_FEAT) with dropout ON at
 * b->dropout_thr under b->key_gru / b->key_head, exactly as a training = 1 forward of a batch of `rows` rows masks them: GRU element
 * (row * TP + t) * 128 + u, head element row * 64 + v.  dropout_thr = 0 gives the eval forward's bits.  Writes WS_H1, WS_FEAT,
 * WS_HID and WS_LOGITS (and WS_GI, the projection scratch) of `b`'s workspace and nothing else: no softmax, no loss (labels are
 * ignored), no BatchNorm state.  MSIG_E_SHAPE if rows * TP * 128 > 2^31: the mask index is 32-bit. */
int msig_mc_tail(const msig_batch* b, int32_t kind, void* stream);

/* Per window n, over its S rows of logits (N * S, K), everything in fp64 and rounded to fp32 once on store:
 *   p_s     = softmax(logits[n * S + s]), max-subtracted
 *   mean_p  (N, K)  m = (sum_s p_s) / S, summed in increasing s
 *   std_p   (N, K)  sqrt((sum_s (p_s - m)^2) / S), the population standard deviation over s
 *   pred    (N)     first argmax of m
 *   entropy (N)     H(m) = -sum_k m_k ln m_k, 0 ln 0 = 0, in nats (predictive entropy)
 *   expected_entropy (N)  (sum_s H(p_s)) / S
 *   mutual_info (N) H(m) - expected entropy, not clamped (the two are computed separately: it may be a rounding below zero)
 *   votes   (N, K) int32: the number of s whose first maximal logit is k
 * Any output but mean_p may be NULL.  One thread owns a window: no atomics, one writer per output, and the bits depend on
 * neither N nor the grid.  2 <= K <= MSIG_MAX_K, 1 <= S <= MSIG_MC_MAX_SAMPLES, N >= 1, N * S < 2^31; every pointer 4-byte aligned. */
int msig_mc_reduce(const float* logits, int32_t N, int32_t S, int32_t K, float* mean_p, float* std_p, int32_t* pred, float* entropy,
                   float* expected_entropy, float* mutual_info, int32_t* votes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSIG_MC_H */
