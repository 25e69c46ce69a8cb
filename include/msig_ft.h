/* msig_ft.h — window embeddings and classifier-only training (few-shot subject calibration) in libmsig_hip.so.
 *
 * After a LOSO run the companion question is how much a model trained on the other subjects gains from a minute or two of
 * labelled data of the new wearer: freeze the feature extractor (CNN + GRU, in eval mode), re-fit the classifier on a handful of
 * the new subject's windows.  The reference has no such step; what it has is the classifier (models.py:66-71), its criterion
 * (trainer.py:147) and its optimiser (trainer.py:68), which the head epoch below applies to cached features.  The calls stand
 * beside msig.h, msig_cw.h and msig_cg.h, which are unchanged; libmsig_hip.so exports all four sets.
 *
 * Conventions are msig.h's: device pointers unless marked "host", asynchronous on `stream`, no allocation, no state; 0 = ok,
 * > 0 a hipError_t of a launch, < 0 an MSIG_E_* argument error found BEFORE anything is launched.
 */
#ifndef MSIG_FT_H
#define MSIG_FT_H
#include "msig.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSIG_FT_ABI_VERSION 1

int msig_ft_abi_version(void);
/* sizeof(msig_ft_head) (which = 0) / sizeof(msig_ft_multi) (which = 1) as the library was compiled; other values: -1. */
int64_t msig_ft_struct_bytes(int32_t which);

/* ---- features -------------------------------------------------------------------------------------------------------
 * The 128-dimensional vector the classifier sees, outputs[:, -1, :] (models.py:79): the front end and the GRU of an EVAL-mode
 * forward — running-statistics BatchNorm, no dropout, BatchNorm state untouched — with no head launch, then MSIG_WS_FEAT copied to
 * `out`, (B, 128) fp32, 16-byte aligned.  b->training must be 0 (MSIG_E_SHAPE otherwise); b->labels is not read.  The rows are the
 * very bits the eval-mode msig_forward (msig_cg_forward) of the same descriptor leaves in MSIG_WS_FEAT.  Both depths
 * (msig_batch.gru_layers 2 and the embedded 1, whose real features sit at columns 0..31 and 64..95).
 * kind: which model's front end and parameter layout — the head is the same for both, only these two calls need it. */
#define MSIG_FT_KIND_ATTENTION 0   /* CnnGruAttentionModel: msig.h, msig_param_layout    */
#define MSIG_FT_KIND_CNN_GRU   1   /* CnnGruModel:          msig_cg.h, msig_cg_param_layout */
int msig_ft_features(const msig_batch* b, int kind, float* out, void* stream);
/* The same for a fold batch: fold z of the launch (arena m->slot[z]) writes its rows at out + z * out_stride_bytes
 * (out_stride_bytes >= B * 512, a multiple of 16). */
int msig_ft_features_multi(const msig_batch* b, const msig_multi* m, int kind, float* out, int64_t out_stride_bytes, void* stream);

/* ---- head epoch: consecutive classifier-only train steps in ONE launch ---------------------------------------------------
 * With the extractor frozen and in eval mode a window's feature does not change from step to step, so calibration is a sequence
 * of small, strictly sequential steps on cached rows.  One call runs steps first_step .. first_step + n_steps - 1 of an epoch
 * whose visiting order the host made (`order`, the epoch's permutation): step s takes the rows
 *     idx = order[s * batch .. min((s + 1) * batch, n_order))          (a short last step, as DataLoader(drop_last=False))
 * and does
 *     hid    = dropout(relu(feat[idx] @ W0^T + b0));   logits = hid @ W3^T + b3                 (models.py:66-71)
 *     loss   = CrossEntropy(logits, labels[idx], weight = class_weight or none), mean reduction as torch   (trainer.py:147;
 *              weighted: msig_cw.h's semantics, sum_b w[y_b] nll_b / sum_b w[y_b])
 *     Adam (L2-in-gradient weight decay; bias correction by the step count step0 + (s - first_step)) on W0, b0, W3, b3 ONLY.
 * params / exp_avg / exp_avg_sq are flat buffers in the model's layout of which only the four classifier tensors are read or
 * written: cls_offset is offsets[MSIG_P_CLS0_W] of msig_param_layout (or msig_cg_param_layout) for the model's C and K, and
 * classifier.0.bias, classifier.3.weight and classifier.3.bias follow at their padded sizes (8192, 64, K * 64 floats on).  The
 * head is the same tensor sequence in both model kinds, so this call needs no kind.
 * Dropout: the mask of the step with count t is that of the classifier's dropout in msig_train_step at step t — key
 * msig_dropout_key(seed, t, 2), threshold as msig_batch.dropout_thr, element index = (row inside the step's mini-batch) * 64 +
 * hidden unit.  dropout_thr = 0 disables it.
 * loss_acc (optional, as msig_batch.loss_acc): [0] += the summed loss of every step (mean * rows of the step), [1] += correctly
 * classified rows, in step order.
 * For the embedded 32-unit model the head lives in the padded layout: the padded columns of W0 see zero features, receive
 * exactly zero gradient and stay exactly zero.
 * Every sum that decides bits (loss, class-weight total, weight gradients) runs in one fixed order that depends on the step's
 * rows alone: one call of S steps equals S calls of one step, and a fold of a batch equals its single call, bit for bit.
 *
 * Bounds: 2 <= K <= MSIG_MAX_K; 1 <= batch <= MSIG_FT_MAX_BATCH; 1 <= n_order <= N <= MSIG_FT_MAX_N; first_step >= 0, n_steps >= 1,
 * first_step + n_steps <= ceil(n_order / batch) (MSIG_E_SHAPE); step0 >= 1; 0 <= dropout_thr <= 256.  feat, params, exp_avg and
 * exp_avg_sq 16-byte aligned, labels and loss_acc 8-byte, order and class_weight 4-byte (MSIG_E_ALIGN).  The library cannot see
 * device values before its kernel reads them: entries of `order` outside [0, N) and labels outside [0, K) are the caller's
 * error; the kernel clamps them into range, so they never cause an access outside the buffers. */
#define MSIG_FT_MAX_BATCH 256
#define MSIG_FT_MAX_N     (1 << 24)
typedef struct msig_ft_head {
  int32_t K;                 /* classes                                                             */
  int32_t N;                 /* rows of feat / labels                                               */
  int32_t n_order;           /* entries of order = rows visited per epoch (<= N)                    */
  int32_t batch;             /* rows per step                                                       */
  int32_t first_step;        /* first step of this call inside the epoch, 0-based                   */
  int32_t n_steps;           /* steps of this call                                                  */
  int32_t dropout_thr;       /* round(p * 256); 0 disables                                          */
  int32_t reserved;          /* 0                                                                   */
  int64_t cls_offset;        /* floats: offsets[MSIG_P_CLS0_W] of the model's parameter layout       */
  int64_t step0;             /* 1-based optimiser step count of this call's first step              */
  uint64_t seed;             /* dropout seed (msig_dropout_key(seed, step count, 2))                */
  float lr, beta1, beta2, eps, weight_decay;
  float reserved_f;          /* 0                                                                   */
  const float*   feat;       /* (N, 128)                                                            */
  const int64_t* labels;     /* (N)                                                                 */
  const int32_t* order;      /* (n_order) row indices                                               */
  float* params;             /* flat, the model's layout                                            */
  float* exp_avg;            /* flat, same layout                                                   */
  float* exp_avg_sq;         /* flat, same layout                                                   */
  const float* class_weight; /* K floats or NULL                                                    */
  double* loss_acc;          /* [2] or NULL                                                         */
} msig_ft_head;

int msig_ft_head_epoch(const msig_ft_head* h, void* stream);

/* Fold batch: ONE launch runs the call for n folds (workgroup z = fold z).  `h` describes arena slot 0; every pointer of fold z
 * sits slot[z] * stride_bytes further on (class_weight and loss_acc too, when not NULL), as in msig_multi.  Shape, batch, step
 * range, betas, eps, weight decay and dropout threshold are shared; learning rate, first step count and dropout seed are per fold
 * (h->lr, h->step0 and h->seed are ignored).  Folds never interact. */
typedef struct msig_ft_multi {
  int32_t  n;                        /* folds in this launch, 1..MSIG_MAX_FOLDS                   */
  int32_t  slot[MSIG_MAX_FOLDS];     /* arena index of each (distinct, >= 0)                      */
  int32_t  reserved;                 /* 0                                                         */
  int64_t  stride_bytes;             /* bytes between consecutive arenas; positive multiple of 256 */
  float    lr[MSIG_MAX_FOLDS];
  int64_t  step0[MSIG_MAX_FOLDS];    /* >= 1                                                      */
  uint64_t seed[MSIG_MAX_FOLDS];
} msig_ft_multi;

int msig_ft_head_epoch_multi(const msig_ft_head* h, const msig_ft_multi* m, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSIG_FT_H */
