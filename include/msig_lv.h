/* msig_lv.h — live monitoring of many wearers: a pool of sample rings and window batches whose rows come from different sessions, the
 * input side of multimodalsignal_amd/live.py, exported by libmsig_hip.so beside msig_rec.h and its companions,
 * none of which changes.
 *
 * The pool.  One caller-owned device block of `sessions` rings, `ring_bytes` apart; a ring is R rows of C_all float64, one row one
 * sample, as in a recording.  Sample i of a session, counted from the session's start, lives in row i % R of its ring.  The caller
 * keeps every session's count of samples written so far (`written`) on the host and passes it in; the library keeps nothing.
 *
 * msig_lv_push: appends chunk j = rows [sum of len[0..j), + len[j]) of the device buffer `staging` (C_all float64 per row, the chunks
 * back to back) to session sess[j], whose ring holds written[j] samples so far: row r of the chunk goes to ring row
 * (written[j] + r) % R — the ring's end is wrapped inside the kernel.  sess, written and len are HOST arrays of n entries, read before
 * the call returns.  One launch per MSIG_LV_GROUP sessions (the table travels as kernel arguments).  A chunk of 0 rows is allowed.
 *
 * msig_lv_windows_multi: the counterpart of msig_rec_windows_multi for a batch whose rows come from different sessions.  Row b is
 * window win[b] of session sess[b], samples [win[b] * S, win[b] * S + T) of that session, read from its ring with wrap-around:
 *     out[b][c][t] = (float)((v - stats[s_b][c]) * stats[s_b][MSIG_MAX_C + c])
 * with cols, log1p_mask, the statement and the rounding sequence of msig_rec_windows: with the same statistics the bits are that
 * call's on the session's linear recording.  `stats` is a device table of one msig_nr.h record (MSIG_LV_STATS_DOUBLES doubles) per
 * session of the pool.  sess, win and written (the samples written to row b's session) are HOST arrays of B entries.  The batch goes
 * into the x buffer of every arena slot of `m`, as msig_rec_windows_multi's does.  Rows b, b + 1, ... that are consecutive windows of
 * one session form a run: a sample of a run is read and normalised once and stored into every window of the run that covers it.
 * One launch per MSIG_LV_GROUP runs.
 *
 * A session's "head:K" statistics need no call of their own: msig_rec_stats on the ring's first (K - 1) * S + T rows, while they
 * still lie unwrapped at the ring's start, is the offline call.
 *
 * Conventions are msig_rec.h's: asynchronous on `stream`, no allocation, no state between calls, no host synchronisation,
 * deterministic.
 *
 * Checks, all before any launch.  Both calls: a NULL pool or host array -> MSIG_E_NULL; sessions outside 1..MSIG_LV_MAX_SESSIONS,
 * R outside 1..2^31 - 1, C_all < 1, ring_bytes < R * C_all * 8 -> MSIG_E_SHAPE; pool not 8-byte aligned or ring_bytes not a multiple
 * of 8 -> MSIG_E_ALIGN (after the call's own shape checks).
 * msig_lv_push: a NULL staging -> MSIG_E_NULL; n outside 1..sessions, a session outside [0, sessions), the same session twice,
 * written < 0, a chunk of fewer than 0 or more than R rows -> MSIG_E_SHAPE; staging not 8-byte aligned -> MSIG_E_ALIGN.
 * msig_lv_windows_multi: a NULL cols, stats, out_x or m -> MSIG_E_NULL; T or S < 1, C outside 1..MSIG_MAX_C, a column outside
 * [0, C_all), B < 1, a session outside [0, sessions), win < 0, a window not yet complete (win * S + T > written) or already
 * overwritten (win * S < written - R) -> MSIG_E_SHAPE; stats not 8-byte aligned, out_x not 16-byte aligned -> MSIG_E_ALIGN; then
 * msig_multi's own checks, and MSIG_E_SHAPE where a slot's batch would reach into the next arena.
 */
#ifndef MSIG_LV_H
#define MSIG_LV_H
#include "msig.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSIG_LV_ABI_VERSION 1
#define MSIG_LV_MAX_SESSIONS 4096                       /* rings of one pool at most */
#define MSIG_LV_GROUP 128                               /* sessions (push) or runs (windows) one launch takes */
#define MSIG_LV_STATS_DOUBLES (2 * MSIG_MAX_C + 1)      /* one msig_nr.h statistics record */

int msig_lv_abi_version(void);

int msig_lv_push(double* pool, int32_t sessions, int64_t R, int64_t ring_bytes, int32_t C_all, const int32_t* sess /* host */,
                 const int64_t* written /* host */, const int64_t* len /* host */, int32_t n, const double* staging, void* stream);

int msig_lv_windows_multi(const double* pool, int32_t sessions, int64_t R, int64_t ring_bytes, int32_t C_all,
                          const int32_t* cols /* host */, int32_t C, uint32_t log1p_mask, int64_t T, int64_t S,
                          const int32_t* sess /* host */, const int64_t* win /* host */, const int64_t* written /* host */, int32_t B,
                          const double* stats, float* out_x, const msig_multi* m, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSIG_LV_H */
