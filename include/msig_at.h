/* msig_at.h — integrated-gradients attribution: the two memory-bound ends of the path integral, in libmsig_hip.so.
 *
 * Since ABI 5 of msig.h the model has exact input gradients in eval mode (msig_batch.dx, keep_for_backward).  Integrated gradients
 * of a window x against a baseline x0 need, around the model's forward and backward, (1) the batch of path points between x0 and
 * x and (2) the weighted sum of the gradients at those points, times (x - x0), with its sums per time bin, per channel and per
 * window.  Both are pure streaming passes over (N * P, C, T) tensors; they are the two calls of this header.  The calls stand
 * beside msig.h and its companions, which are unchanged.
 *
 * Semantics.  F is the model in eval mode, v a vector over the K logits, f(x) = sum_k v[k] * logits(x)[k].
 *   path      xp[n * P + p][c][t] = fmaf(coef[p][c], x[n][c][t] - x0[n][c][t], x0[n][c][t])           (fp32, as written)
 *             except that coef == 1 gives x's own bits (x0 + (x - x0) rounds) as coef == 0 gives x0's: an occlusion row is the
 *             window with one channel replaced, bit for bit, for every baseline;
 *             integrated gradients fill coef[p][.] = alpha_p = (p + 1/2) / P (the midpoint rule, which never evaluates at the
 *             baseline itself); channel occlusion uses P = C + 1 rows, coef = 1 except coef[c][c] = 0 (row C is the window).
 *   reduce    G[n][c][t]   = sum_p w[p] * dx[n * P + p][c][t]      fp32, G = fmaf(w[p], dx_p, G) in the order p = 0 .. P-1 from G = 0
 *             map[n][c][t] = (x - x0) * G                           fp32: one subtraction, one product
 *             bins[n][c][j] = sum of map[n][c][t] over t in [j * bin, min(T, (j + 1) * bin)),  NB = ceil(T / bin) bins
 *             chan[n][c]   = sum_t map[n][c][t],   total[n] = sum_c chan[n][c]
 *             the three sums are carried in fp64 over the fp32 map values and rounded once on store.  No atomics: every output
 *             element has one writer and a summation order fixed by (T, bin) alone, so the bits do not depend on N, on the grid or
 *             on whether `map` is written.
 *   With w[p] = 1 / P and dx = df/dx at the path points, total ~ f(x) - f(x0); the residual is the quadrature error of P points.
 *
 * Conventions are msig.h's: device pointers, asynchronous on `stream`, no allocation, no state; 0 = ok, > 0 a hipError_t of a
 * launch, < 0 an MSIG_E_* argument error found BEFORE anything is launched.  Every buffer is contiguous; the (., C, T) tensors — x,
 * base (every kind), xp, dx, map — are 16-byte aligned, the small ones (coef, w, v, dlogits, bins, chan, total) 4-byte, scratch 8-byte.
 * Shape limits: 1 <= C <= MSIG_MAX_C, 2 <= K <= MSIG_MAX_K, T >= 16, 1 <= P <= MSIG_AT_MAX_POINTS, N >= 1.  Indexing is 64-bit:
 * N * P * C * T may exceed 2^31 elements; C * T, N * P and the number of workgroups (N * ceil(C * T / 1024), N * C) stay below 2^31.
 * With T % 4 != 0 the rows are not 16-byte aligned and both kernels take their element-wise form (same arithmetic, same bits as
 * the 16-byte form would give); with T % 4 == 0 every load and store of the (N * P, C, T) tensors is 16 bytes wide.
 */
#ifndef MSIG_AT_H
#define MSIG_AT_H
#include "msig.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSIG_AT_ABI_VERSION 1
#define MSIG_AT_MAX_POINTS 256

/* the baseline x0 of a call: what `base` points to */
#define MSIG_AT_BASE_ZERO    0   /* x0 = 0; `base` is not read (may be NULL) */
#define MSIG_AT_BASE_CHANNEL 1   /* (C): one value per channel */
#define MSIG_AT_BASE_SHARED  2   /* (C, T): one window for every input */
#define MSIG_AT_BASE_OWN     3   /* (N, C, T): one window per input */

int msig_at_abi_version(void);

/* Path points.  x (N, C, T); coef (P, C) on the DEVICE; xp (N * P, C, T) is written, row n * P + p.  v (N, K) is optional: when
 * given, dlogits (N * P, K) is required and each window's v is copied to its P rows (the upstream gradient of the path batch's
 * backward); when NULL, dlogits is not touched and K is not read.  x and x0 are read once per window, xp written P times. */
int msig_at_path(const float* x, const float* base, int32_t base_kind, const float* coef, const float* v,
                 int32_t N, int32_t P, int32_t C, int32_t T, int32_t K, float* xp, float* dlogits, void* stream);

/* Reduction of the path batch's input gradients dx (N * P, C, T) with the weights w (P) on the DEVICE, in ONE pass over dx.
 * map (N, C, T) may be NULL: then it is not written, and bins (N, C, NB), chan (N, C) and total (N) have the same bits.
 * scratch: N * C fp64 values, caller-owned, written and read by this call only (the channels' unrounded sums, from which the
 * second launch takes the windows' totals).  bin >= 1 samples per bin; a bin wider than T gives one bin.
 * Launches: at_reduce (one workgroup per (n, c) row) and at_total. */
int msig_at_reduce(const float* dx, const float* x, const float* base, int32_t base_kind, const float* w,
                   int32_t N, int32_t P, int32_t C, int32_t T, int32_t bin,
                   float* map, float* bins, float* chan, float* total, double* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSIG_AT_H */
