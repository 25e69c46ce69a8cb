/* msig_rd.h — the exponentially decayed running reference: statistics that are a function of the window index and forget smoothly,
 * for one continuous recording and for the live sessions of a ring pool.  The input side of "decayed:H" in monitor.py, live.py and
 * the training store, exported by libmsig_hip.so beside msig_rn.h, which does not change.
 *
 * Notation, the pivot p[c] (v at sample 0) and the window-sum records W[k] (MSIG_RN_SUM_DOUBLES doubles, msig_rn_sums' reduction) are
 * msig_rn.h's.  `decay` is a double lambda in [0, 1] that the caller passes; the Python side uses lambda = exp2(-1 / H) for a
 * half-life of H windows.
 * Reference of window n: A_0 = W_0, c_0 = 1; for n >= 1, per column j of a record, A_n[j] = fma(lambda, A_{n-1}[j], W_n[j]) — one
 * lane owns column j, as in msig_rn_stats' expanding scan — and c_n = fma(lambda, c_{n-1}, 1.0): the effective number of windows,
 * a real number.
 * Statistics of window n: msig_rn.h's last lines with n_ref = c_n, i.e. count = c_n * T:
 *     dm = A1 / count, var = max(0, fma(-dm, dm, A2 / count)), [c] = p + dm, [MSIG_MAX_C + c] = 1 / (sqrt(var) + 1e-8),
 *     [2 * MSIG_MAX_C] = c_n.  Only the selected channels' entries are written.
 * Two anchors follow: lambda = 1 is msig_rn_stats(K = 0)'s table bit for bit (fma(1, a, w) = a + w, c_n = n + 1), lambda = 0 is
 * msig_rn_stats(K = 1)'s (fma(0, a, w) = w, c_n = 1).
 * Rows: msig_rn_windows[_multi] and msig_rn_lv_windows_multi take one record per row whatever wrote it; they serve here unchanged.
 *
 * msig_rd_stats: from the records of windows 0 .. N - 1 (`sums`, written by msig_rn_sums) the N statistics records (`table`).  One
 * wave scans the N windows, one lane per column of a record, the records loaded ahead of the recurrence.
 *
 * Live.  Every session of an msig_lv.h pool owns msig_rn_state_bytes(0) bytes of caller-owned device state, `state_bytes` apart; it
 * needs no initialisation.  In doubles, msig_rn.h's head: [0, MAX_C) the pivot, [MAX_C, 3 MAX_C) the carry A, [3 MAX_C] the next
 * expected window, [3 MAX_C + 1] = 0 (there is no ring of records), and of the head's reserved doubles [3 MAX_C + 2] =
 * MSIG_RD_STATE_C holds c and [3 MAX_C + 3] the lambda of the last step.
 * msig_rd_lv_step: msig_rn_lv_step with `decay` in place of K — for B rows (sess[b], win[b], written[b], next[b]: HOST arrays) it
 * reads the pivot from window 0 where a session starts (win == 0), forms each row's window sums from the ring with wrap-around
 * (msig_rn_sums' reduction: the same bits), advances the session's carry and c in row order and writes row b's statistics record to
 * table + b * MSIG_LV_STATS_DOUBLES.  The rows of one session are adjacent, consecutive windows in ascending order, beginning at
 * next[b].  One workgroup per session, one launch per MSIG_LV_GROUP sessions.  Every record equals msig_rd_stats' for the same
 * samples as one recording, bit for bit.
 *
 * Conventions are msig_rn.h's: asynchronous on `stream`, no allocation, no library state, no host synchronisation, deterministic
 * (no float atomics).
 *
 * Checks, all before any launch.  msig_rd_stats: msig_rn_stats', item for item (NULL -> MSIG_E_NULL; L, T, S or C_all < 1, C outside
 * 1..MSIG_MAX_C, a column outside [0, C_all), N < 1 or N > the window count -> MSIG_E_SHAPE; sig, sums or table not 8-byte aligned
 * -> MSIG_E_ALIGN), and `decay` outside [0, 1] or NaN -> MSIG_E_SHAPE where msig_rn_stats checks K (-0.0 and 1.0 are inside).
 * msig_rd_lv_step: msig_rn_lv_step's, item for item, with `decay` outside [0, 1] or NaN, or state_bytes < msig_rn_state_bytes(0),
 * -> MSIG_E_SHAPE where that call checks K.
 */
#ifndef MSIG_RD_H
#define MSIG_RD_H
#include "msig_rn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSIG_RD_ABI_VERSION 1
#define MSIG_RD_STATE_C (3 * MSIG_MAX_C + 2)            /* the double of a session's state that holds c, the effective window count */

int msig_rd_abi_version(void);

int msig_rd_stats(const double* sig, int64_t L, int32_t C_all, const int32_t* cols /* host */, int32_t C, uint32_t log1p_mask,
                  int64_t T, int64_t S, const double* sums, int64_t N, double decay, double* table, void* stream);

int msig_rd_lv_step(const double* pool, int32_t sessions, int64_t R, int64_t ring_bytes, int32_t C_all, const int32_t* cols /* host */,
                    int32_t C, uint32_t log1p_mask, int64_t T, int64_t S, double decay, double* state, int64_t state_bytes,
                    const int32_t* sess /* host */, const int64_t* win /* host */, const int64_t* written /* host */,
                    const int64_t* next /* host */, int32_t B, double* table, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSIG_RD_H */
