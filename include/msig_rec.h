/* msig_rec.h — windows of ONE continuous recording, normalised and transposed for the models, without materialising them: the input
 * side of multimodalsignal_amd/monitor.py, exported by libmsig_hip.so beside msig.h and its companions, none
 * of which changes.
 *
 * The recording.  sig is a device array (L, C_all) of float64, row-major — what msig_prep_resample writes.  Window n covers samples
 * [n * S, n * S + T); there are N = (L - T) / S + 1 of them by integer division (0 if L < T).  S >= 1 is free: smaller than, equal
 * to or larger than T.  Sizes and indices are 64-bit.  Per selected channel c (column cols[c]; cols is a HOST array):
 *     v = sig[i, cols[c]], or log1p of it where bit c of log1p_mask is set.
 *
 * msig_rec_stats: the statistics the reference windows [w0, w1) would have as materialised windows, from the recording itself.
 * Sample i has the integer weight m_i = the number of n in [w0, w1) with n * S <= i < n * S + T; with the pivot p = v at sample
 * w0 * S and W = (w1 - w0) * T:
 *     mean = p + sum m_i (v_i - p) / W        var = sum m_i (v_i - p)^2 / W - (mean - p)^2, clamped at 0
 * Every sample of the reference span [w0 * S, (w1 - 1) * S + T) is read once (not T / S times; samples no window covers, S > T, are
 * not read at all).  stats has msig_nr.h's layout (2 * MSIG_MAX_C + 1 doubles): [c] = mean, [MSIG_MAX_C + c] = 1 / (std + 1e-8),
 * [2 * MSIG_MAX_C] = w1 - w0.
 *
 * msig_rec_windows: windows n0 .. n0 + B - 1 straight into a (B, C, T) fp32 batch:
 *     out[b][c][t] = (float)((v - stats[c]) * stats[MSIG_MAX_C + c]),   v at sample (n0 + b) * S + t
 * — the expression, the log1p and the rounding sequence of msig_nr_normalise_subject, so with that call's stats the bits are its
 * output rows'.  Each sample of the batch's span is read and normalised once and stored into every window that covers it.
 * msig_rec_windows_multi: the same launch stores the batch into the x buffer of every arena slot of `m` (out_x is arena 0's, as for
 * msig_gather_windows_multi; slot z's is at (char*)out_x + m->slot[z] * m->stride_bytes): an M-member ensemble gets its input from
 * one read of the recording.  Only n, slot and stride_bytes of `m` are read beyond msig_multi's own checks.
 *
 * Conventions are msig_nr.h's: asynchronous on `stream`, no allocation, no state between calls, deterministic (fp64 partial sums
 * per workgroup, summed in one fixed order by one thread per channel; no float atomics).
 *
 * Checks, all before any launch: a NULL sig, cols, stats, scratch, out_x or m -> MSIG_E_NULL; L, T, S or C_all < 1, C outside
 * 1..MSIG_MAX_C, a column outside [0, C_all), w0 < 0, w0 >= w1, w1 > N, n0 < 0, B < 1 or n0 + B > N -> MSIG_E_SHAPE (then
 * msig_multi's own); sig, stats or scratch not 8-byte aligned, out_x not 16-byte aligned -> MSIG_E_ALIGN.
 */
#ifndef MSIG_REC_H
#define MSIG_REC_H
#include "msig.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSIG_REC_ABI_VERSION 1

int     msig_rec_abi_version(void);
int64_t msig_rec_scratch_bytes(void);      /* bytes of msig_rec_stats' `scratch` (device, 8-byte aligned) */

/* Host only.  The number of windows; 0 if L < T; MSIG_E_SHAPE if T < 1 or S < 1. */
int64_t msig_rec_count(int64_t L, int64_t T, int64_t S);

int msig_rec_stats(const double* sig, int64_t L, int32_t C_all, const int32_t* cols /* host */, int32_t C, uint32_t log1p_mask,
                   int64_t T, int64_t S, int64_t w0, int64_t w1, double* stats, void* scratch, void* stream);

int msig_rec_windows(const double* sig, int64_t L, int32_t C_all, const int32_t* cols /* host */, int32_t C, uint32_t log1p_mask,
                     int64_t T, int64_t S, int64_t n0, int32_t B, const double* stats, float* out_x, void* stream);

int msig_rec_windows_multi(const double* sig, int64_t L, int32_t C_all, const int32_t* cols /* host */, int32_t C, uint32_t log1p_mask,
                           int64_t T, int64_t S, int64_t n0, int32_t B, const double* stats, float* out_x, const msig_multi* m,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSIG_REC_H */
