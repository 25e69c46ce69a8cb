/* msig_ab.h — label-free BatchNorm adaptation to a new subject (AdaBN) in libmsig_hip.so.
 *
 * After a LOSO run the label-free companion of msig_ft.h: every weight stays as trained, and the running statistics of the two
 * BatchNorm layers are replaced by (or blended with) the statistics of the new subject's own, unlabelled windows — what the
 * per-subject z-score of the pipeline does to the input, one and two layers further in.  The reference has no such step.  The
 * calls stand beside msig.h, msig_cw.h, msig_cg.h and msig_ft.h, which are unchanged.
 *
 * Semantics.  With the model in eval mode, BatchNorm state src = rm1 rv1 rm2 rv2 (96 floats, msig_batch.bn_state),
 * the N windows X of one subject and a blend alpha in [0, 1]:
 *   stage 1   y1 = conv1(gate(x) * x) for all N windows; per channel m1 = the mean over all n1 = N * L1 positions, v1 = the UNBIASED
 *             variance (biased * n1 / (n1 - 1): what a training forward feeds into running_var);
 *             rm1' = (1 - alpha) * rm1 + alpha * m1,  rv1' = (1 - alpha) * rv1 + alpha * v1     (fp32, as written)
 *   stage 2   BatchNorm-1 in its EVAL form with rm1', rv1' — the statistics the model will be used with, not the batch's —
 *             p1 = pool(relu(bn1(y1))), y2 = conv2(p1); m2, v2 over n2 = N * L2 positions and the same blend.
 * The statistics are those of the WHOLE set, however it is cut into batches: an accumulator carries counts, sums and sums of
 * squares in fp64 from batch to batch, and a commit turns it into the new state.  The order of calls is
 *   zero the accumulator;  accumulate(stage 1) per batch;  commit(stage 1);  accumulate(stage 2) per batch with bn_state = the
 *   committed state;  commit(stage 2).
 * num_batches_tracked, every parameter and the source state are never written.
 *
 * Conventions are msig.h's: device pointers, asynchronous on `stream`, no allocation, no state; 0 = ok, > 0 a hipError_t of a
 * launch, < 0 an MSIG_E_* argument error found BEFORE anything is launched.
 */
#ifndef MSIG_AB_H
#define MSIG_AB_H
#include "msig.h"
#include "msig_ft.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSIG_AB_ABI_VERSION 1

int msig_ab_abi_version(void);

/* ---- accumulator ------------------------------------------------------------------------------------------------------------
 * MSIG_AB_ACC_DOUBLES fp64 values per model, caller-owned, 8-byte aligned; all-zero bytes = empty:
 *   [MSIG_AB_N1] positions seen by stage 1, [MSIG_AB_N2] by stage 2,
 *   [MSIG_AB_SUM1 .. +16) sums and [MSIG_AB_SQ1 .. +16) sums of squares of y1 per channel,
 *   [MSIG_AB_SUM2 .. +32) and [MSIG_AB_SQ2 .. +32) those of y2.
 * In a fold batch fold z's accumulator sits slot[z] * stride_bytes further on, like every other buffer. */
#define MSIG_AB_N1   0
#define MSIG_AB_N2   1
#define MSIG_AB_SUM1 2
#define MSIG_AB_SQ1  18
#define MSIG_AB_SUM2 34
#define MSIG_AB_SQ2  66
#define MSIG_AB_ACC_DOUBLES 98

/* Adds one batch of windows to stage `stage` (1 or 2) of `acc`.  b is an EVAL descriptor: b->training must be 0 (MSIG_E_SHAPE),
 * b->labels is not read, b->bn_state is READ ONLY (stage 2 normalises BatchNorm-1 with it, stage 1 does not read it) and
 * b->bn_count is not touched; the evaluation workspace layout suffices.  kind: MSIG_FT_KIND_* of msig_ft.h (which model's front
 * end and parameter layout).
 * Launches: stage 1 the gate (attention model) and conv1_fwd with its per-workgroup partial sums on, then the merge; stage 2 in
 * addition BatchNorm-1's eval-form constants and pool1_conv2_fwd with partial sums on, then the merge.  No stage-2 pooling, no
 * GRU, no head.  The merge reduces the batch's partial rows in fp64 in one fixed order and adds them, and the batch's position
 * count, to the accumulator: one writer per model, stream-ordered, no atomics. */
int msig_ab_accumulate(const msig_batch* b, int kind, int stage, double* acc, void* stream);
int msig_ab_accumulate_multi(const msig_batch* b, const msig_multi* m, int kind, int stage, double* acc, void* stream);

/* Finalises stage `stage` of `acc` — mean, variance clamped at 0, unbiased correction, blend, the formulas of a training forward's
 * running-statistic update — from bn_src into bn_dst (96 floats each, 4-byte aligned; bn_dst may equal bn_src).  Writes ONLY that
 * stage's slices of bn_dst: floats [0, 32) for stage 1, [32, 96) for stage 2.  alpha outside [0, 1] or not finite: MSIG_E_SHAPE.
 * alpha = 0 gives the source bits, alpha = 1 the target exactly.  With a count below 2 the stage's slices are copied from bn_src;
 * NaN is never written for finite sums.
 * _multi: acc, bn_src and bn_dst of fold z sit m->slot[z] * m->stride_bytes further on; alpha is shared. */
int msig_ab_commit(const double* acc, int stage, float alpha, const float* bn_src, float* bn_dst, void* stream);
int msig_ab_commit_multi(const double* acc, int stage, float alpha, const float* bn_src, float* bn_dst, const msig_multi* m, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSIG_AB_H */
