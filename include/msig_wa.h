/* msig_wa.h — weight averaging (an exponential moving average of the weights, or stochastic weight averaging) of the models that
 * libmsig_hip.so trains, single and in fold batches.
 *
 * The model a training run ends with is one iterate of a noisy trajectory.  An averaged model is a second copy of the parameters
 * and the BatchNorm statistics — the SHADOW — that is moved towards the model by one streaming launch after a train step (EMA) or
 * at the end of an epoch (SWA).  The calls below are that launch.  They stand beside msig.h, msig_cw.h, msig_cg.h, msig_ft.h,
 * msig_gc.h, msig_aug.h, msig_st.h, msig_ab.h, msig_at.h, msig_mc.h and msig_da.h, which are unchanged; libmsig_hip.so exports all
 * of them.  No train step and no forward is changed: the update is a launch of its own between two steps.
 *
 * One update of one fold, a = coef[z]:
 *     a == 0   nothing of that fold is read or written.
 *     a == 1   the shadow becomes a 32-bit copy of the model: parameters and BatchNorm statistics, bit for bit (NaN payloads and
 *              the sign of zero included).
 *     else     for every parameter float and every BatchNorm-state float   s = fadd(s, fmul(a, fsub(p, s)))
 *              — three fp32 roundings, never an FMA.
 *     a > 0    avg_bn_count becomes a copy of bn_count.
 * Which a a schedule gives — 1 - decay with a warm-up for EMA, 1 / (k + 1) for SWA — is the caller's business: the coefficients are
 * host values, one per fold of the launch.  tests/wa_reference.py restates the update and both schedules in numpy, bit for bit.
 *
 * There is NO forward of its own for the averaged model.  It is evaluated by the existing msig_st_forward[_multi] (or any other
 * forward of msig.h's family) with msig_batch.params / bn_state / bn_count pointing at the shadow.  In a fold batch every pointer
 * of a launch is fold slot 0's and slot s is s * msig_multi.stride_bytes further on, so the three shadow buffers must live INSIDE
 * the model arenas, at the same offset in each: that is the only layout the *_multi forward can read.  The update follows the same
 * rule: all six pointers of msig_wa are slot 0's.
 *
 * Fold independence.  A fold's result is a function of its own two buffers and its own a: a fold of a fold batch has the bits of
 * its single call, and arenas not named in msig_multi.slot are never touched.  One launch does all folds of a call (the fold is
 * the grid's third dimension); no atomics, no reductions.
 *
 * Checks, all before any launch (in a fold batch msig_multi's own checks come first): NULL msig_wa, params or avg_params, or the
 * four BatchNorm pointers (bn_state, bn_count, avg_bn_state, avg_bn_count) neither all NULL nor all non-NULL -> MSIG_E_NULL;
 * n_flat < 4 or not a multiple of 4, a coef of a participating fold that is NaN or outside [0, 1], avg_params == params or
 * avg_bn_state == bn_state -> MSIG_E_SHAPE; a float pointer not 16-byte aligned or a count pointer not 8-byte aligned
 * -> MSIG_E_ALIGN.  With the four BatchNorm pointers NULL only the parameters are averaged.
 */
#ifndef MSIG_WA_H
#define MSIG_WA_H
#include "msig.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSIG_WA_ABI_VERSION 1

typedef struct msig_wa {
  int64_t n_flat;                 /* floats of one model's flat parameter buffer: >= 4, a multiple of 4 (any such number, not only msig_param_layout's) */
  const float*   params;          /* the model (fold slot 0 in a fold batch) */
  const float*   bn_state;        /* MSIG_BN_STATE_FLOATS, or NULL together with bn_count / avg_bn_state / avg_bn_count: parameters only */
  const int64_t* bn_count;        /* [2] */
  float*   avg_params;            /* the shadow: n_flat floats */
  float*   avg_bn_state;          /* MSIG_BN_STATE_FLOATS */
  int64_t* avg_bn_count;          /* [2] */
  float    coef[MSIG_MAX_FOLDS];  /* a, per fold of the launch ([0] for a single model), 0 <= a <= 1 */
} msig_wa;

int msig_wa_abi_version(void);
int64_t msig_wa_struct_bytes(void);     /* sizeof(msig_wa) of the build */

int msig_wa_update(const msig_wa* w, void* stream);
int msig_wa_update_multi(const msig_wa* w, const msig_multi* m, void* stream);   /* all six pointers are slot 0's; slot s is s * m->stride_bytes on */

#ifdef __cplusplus
}
#endif
#endif /* MSIG_WA_H */
