/* msig_rs.h — causal polyphase FIR resampling by a rational ratio L / M, offline and in front of the live rings,
 * exported by libmsig_hip.so beside msig_lv.h and its companions, none of which changes.
 *
 * The definition.  `h` is a device table of 2 * half + 1 float64 taps (multimodalsignal_amd/resample.py builds scipy's resample_poly
 * filter: firwin(2 * half + 1, 1 / max(L, M), window = ("kaiser", beta)) * L).  Output m of the raw stream x, one row one sample of
 * C_all float64 columns, is
 *     y[m][c] = sum over j of h[half + m * M - j * L] * x[j][c],    j = max(0, ceil((m * M - half) / L)) .. floor((m * M + half) / L)
 * taken in ASCENDING j as acc = fma(h, x, acc) from acc = +0.0, in float64: raw samples before sample 0 count as zeros, and the
 * rounding sequence is fixed.  An output exists once its whole support has arrived:
 *     msig_rs_out_count(n_in, L, M, half) = 0 if n_in * L - half - 1 < 0, else (n_in * L - half - 1) / M + 1
 * so the outputs are a causal function of the stream, the first msig_rs_out_count rows of scipy.signal.resample_poly(x, L, M) and
 * none of its zero-padded tail.  Non-finite raw samples propagate by IEEE rules: an output whose support holds a NaN is NaN; there is
 * no special case.
 *
 * msig_rs_resample: the offline call, (n_in, C_all) -> (n_out, C_all), n_out = msig_rs_out_count(n_in, ...).
 *
 * msig_rs_lv_push: the live call, msig_lv_push with raw-rate chunks.  Chunk j = rows [sum of len[0..j), + len[j]) of the device buffer
 * `staging` holds the raw rows raw_written[j] .. raw_written[j] + len[j] - 1 of session sess[j].  Every output m in
 * [out_count(raw_written[j]), out_count(raw_written[j] + len[j])) is computed — by the device function the offline call uses: the
 * same bits — and stored into row m % R of the session's ring in the msig_lv.h pool, which msig_lv_windows_multi and its relatives
 * read unchanged.  Support rows older than the chunk come from the session's TAIL: `tails` is a caller-owned device block of
 * `sessions` rings, tail_bytes apart, of tail_rows raw rows each; raw row i lives in tail row i % tail_rows.  The call brings the tail
 * up to date with a second launch after the one that reads it (same stream: the order is the stream's).  tail_rows must be at least
 * (2 * half) / L + 1; the caller zeroes nothing — a row is never read before it was written.  staging == NULL: every row of every
 * chunk is missing (NaN), the resampled form of msig_gp_lv_skip.  sess, raw_written and len are HOST arrays of n entries, read before
 * the call returns.  One launch pair per MSIG_LV_GROUP sessions.  A chunk of 0 rows is allowed.
 *
 * Conventions are msig_lv.h's: asynchronous on `stream`, no allocation, no state between calls, no host synchronisation,
 * deterministic.
 *
 * Checks, all before any launch.  Both calls: a NULL h -> MSIG_E_NULL; L or M outside 1..MSIG_RS_MAX_RATIO, not coprime or equal,
 * half < max(L, M) or > MSIG_RS_MAX_HALF, C_all < 1 -> MSIG_E_SHAPE; h not 8-byte aligned -> MSIG_E_ALIGN.
 * msig_rs_resample: a NULL x with n_in > 0 or a NULL y with n_out > 0 -> MSIG_E_NULL; n_in < 0 or above MSIG_RS_MAX_ROWS, n_out other
 * than msig_rs_out_count -> MSIG_E_SHAPE; x or y not 8-byte aligned -> MSIG_E_ALIGN.
 * msig_rs_lv_push: a NULL pool, tails or host array -> MSIG_E_NULL; msig_lv_push's pool checks; tail_rows < (2 * half) / L + 1 or
 * above 2^31 - 1, tail_bytes < tail_rows * C_all * 8, n outside 1..sessions, a session outside [0, sessions), the same session twice,
 * raw_written < 0, len < 0 or above 2^31 - 1, raw_written + len above MSIG_RS_MAX_ROWS, a chunk that yields more than R outputs
 * -> MSIG_E_SHAPE; pool, tails or staging not 8-byte aligned, ring_bytes or tail_bytes not a multiple of 8 -> MSIG_E_ALIGN.
 * msig_rs_out_count returns MSIG_E_SHAPE for n_in < 0 or above MSIG_RS_MAX_ROWS or a refused L, M, half.
 */
#ifndef MSIG_RS_H
#define MSIG_RS_H
#include "msig.h"
#include "msig_lv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSIG_RS_ABI_VERSION 1
#define MSIG_RS_MAX_RATIO 4096                          /* L and M at most */
#define MSIG_RS_MAX_HALF (1 << 22)                      /* half at most: 1024 * MSIG_RS_MAX_RATIO */
#define MSIG_RS_MAX_ROWS ((int64_t)1 << 48)             /* raw rows of one stream at most: rows * L stays far inside int64 */

int msig_rs_abi_version(void);

int64_t msig_rs_out_count(int64_t n_in, int32_t L, int32_t M, int32_t half);

int msig_rs_resample(const double* x, int64_t n_in, int32_t C_all, const double* h, int32_t L, int32_t M, int32_t half, double* y,
                     int64_t n_out, void* stream);

int msig_rs_lv_push(double* pool, int32_t sessions, int64_t R, int64_t ring_bytes, int32_t C_all, double* tails, int64_t tail_rows,
                    int64_t tail_bytes, const double* h, int32_t L, int32_t M, int32_t half, const int32_t* sess /* host */,
                    const int64_t* raw_written /* host */, const int64_t* len /* host */, int32_t n, const double* staging, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSIG_RS_H */
