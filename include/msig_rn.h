/* msig_rn.h — causal running references: statistics that are a function of the window index, for one continuous recording and for
 * the live sessions of a ring pool.  The input side of monitor.py's and live.py's "expanding" and "trailing:K" references (DESIGN.md
 * section 36), exported by libmsig_hip.so beside msig_rec.h, msig_lv.h and their companions, none of which changes.
 *
 * Notation is msig_rec.h's: window n covers samples [n * S, n * S + T) of a (L, C_all) float64 recording, or of a session of an
 * msig_lv.h pool (sample i in ring row i % R); v is the sample of selected channel c, after log1p where bit c of log1p_mask is set.
 *
 * The pivot p[c] is v at sample 0 of the recording or session, fixed for its life.
 * Window sums.  Window k has one record of MSIG_RN_SUM_DOUBLES = 2 * MSIG_MAX_C doubles: [c] = W1[k][c] = sum over its own T samples
 * of (v - p[c]), [MSIG_MAX_C + c] = W2[k][c] = the sum of (v - p[c])^2, in fp64.  One workgroup of 256 threads takes one window:
 * thread j accumulates samples j, j + 256, ... in that order, the 64 lanes of a wave are added by xor-butterfly, the four waves in
 * index order.  The order is a function of T alone — not of where the samples lie (recording or wrapped ring), of the batch or of
 * the grid — so a window's record has the same bits wherever it is formed.
 * Reference of window n: the windows [a_n, n]; mode K = 0 ("expanding"): a_n = 0; K >= 1 ("trailing:K"): a_n = max(0, n - K + 1).
 * A = W[a_n] + W[a_n + 1] + ... + W[n], added left to right, per column; count = (n - a_n + 1) * T.  Expanding carries the sum from
 * window to window, which is the same sequence of additions, so trailing:K with K > n has expanding's bits for window n.  Trailing
 * is never a difference of prefix sums.
 * Statistics of window n, one msig_nr.h record (MSIG_LV_STATS_DOUBLES doubles) per window, with msig_rec_stats' last lines:
 *     dm = A1 / count, var = max(0, fma(-dm, dm, A2 / count)), [c] = p + dm, [MSIG_MAX_C + c] = 1 / (sqrt(var) + 1e-8),
 *     [2 * MSIG_MAX_C] = n - a_n + 1.  Only the selected channels' entries are written.
 * Rows: out[b][c][t] = (float)((v - rec_b[c]) * rec_b[MSIG_MAX_C + c]) with row b's own record — msig_rec_windows' statement and
 * rounding sequence: with the same record in every row the bits are that call's.
 *
 * msig_rn_sums: the records of windows [n0, n0 + B) of a recording into the device table `sums` (B records).
 * msig_rn_stats: from the records of windows 0 .. N - 1 (`sums`) and a mode K the N statistics records (`table`).  Trailing: one
 * wave per window adds its <= K terms.  Expanding: one wave scans the N windows, one lane per column of a record.
 * msig_rn_windows[_multi]: msig_rec_windows[_multi] with `table` = one record per ROW (row b's at table + b *
 * MSIG_LV_STATS_DOUBLES) in place of `stats`.  A thread owns one (row, t): it reads its sample once and stores the C values, in
 * every arena slot of `m`; consecutive lanes are consecutive t.
 *
 * Live.  Every session of an msig_lv.h pool owns msig_rn_state_bytes(K) bytes of caller-owned device state, `state_bytes` apart
 * (session s's at (char*)state + s * state_bytes); it needs no initialisation.  In doubles: [0, MAX_C) the pivot, [MAX_C, 3 MAX_C)
 * the expanding carry, [3 MAX_C] the next expected window, [3 MAX_C + 1] K, up to MSIG_RN_STATE_HEAD reserved; then, K >= 1, a ring
 * of K window-sum records, window k's in slot k % K.
 * msig_rn_lv_step: for B rows (sess[b], win[b], written[b]: HOST arrays as in msig_lv_windows_multi, and next[b]: the window the
 * caller expects session sess[b] to take next) it reads the pivot from window 0 where a session starts (win == 0), forms each
 * row's window sums from the ring with wrap-around (msig_rn_sums' reduction: the same bits), advances the session's carry or sum
 * ring in row order and writes row b's statistics record to table + b * MSIG_LV_STATS_DOUBLES.  The rows of one session are
 * adjacent in the batch, consecutive windows in ascending order, beginning at next[b]: the state continues where it stands.  One
 * workgroup per session, one launch per MSIG_LV_GROUP sessions.
 * msig_rn_lv_windows_multi: msig_lv_windows_multi with `table` = one record per ROW in place of the per-session `stats`.
 *
 * Conventions are msig_rec.h's: asynchronous on `stream`, no allocation, no library state, no host synchronisation, deterministic
 * (no float atomics).
 *
 * Checks, all before any launch.  The recording calls: msig_rec.h's, item for item (`sums` and `table` in the place of `stats`; NULL
 * -> MSIG_E_NULL; L, T, S or C_all < 1, C outside 1..MSIG_MAX_C, a column outside [0, C_all), n0 < 0, B < 1, n0 + B > the window
 * count -> MSIG_E_SHAPE; sig, sums or table not 8-byte aligned, out_x not 16-byte aligned -> MSIG_E_ALIGN; then msig_multi's own);
 * msig_rn_stats: N < 1 or N > the window count, K outside 0..MSIG_RN_MAX_K -> MSIG_E_SHAPE.
 * The live calls: msig_lv_windows_multi's, item for item (`table` in the place of `stats`).  msig_rn_lv_step in addition: a NULL
 * state or next -> MSIG_E_NULL; K outside 0..MSIG_RN_MAX_K, state_bytes < msig_rn_state_bytes(K), a session in two separate
 * places of the batch, a row that is not its session's next window (win != next for the session's first row, not the previous + 1
 * after it) -> MSIG_E_SHAPE; state not 8-byte aligned or state_bytes not a multiple of 8 -> MSIG_E_ALIGN.
 */
#ifndef MSIG_RN_H
#define MSIG_RN_H
#include "msig.h"
#include "msig_lv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSIG_RN_ABI_VERSION 1
#define MSIG_RN_MAX_K 4096                              /* windows of a trailing reference at most */
#define MSIG_RN_SUM_DOUBLES (2 * MSIG_MAX_C)            /* one window-sum record */
#define MSIG_RN_STATE_HEAD (4 * MSIG_MAX_C)             /* doubles of a session's state before its ring of records */

int     msig_rn_abi_version(void);
int64_t msig_rn_state_bytes(int32_t K);    /* one session's state for mode K (0 = expanding); MSIG_E_SHAPE if K is out of range */

int msig_rn_sums(const double* sig, int64_t L, int32_t C_all, const int32_t* cols /* host */, int32_t C, uint32_t log1p_mask,
                 int64_t T, int64_t S, int64_t n0, int64_t B, double* sums, void* stream);

int msig_rn_stats(const double* sig, int64_t L, int32_t C_all, const int32_t* cols /* host */, int32_t C, uint32_t log1p_mask,
                  int64_t T, int64_t S, const double* sums, int64_t N, int32_t K, double* table, void* stream);

int msig_rn_windows(const double* sig, int64_t L, int32_t C_all, const int32_t* cols /* host */, int32_t C, uint32_t log1p_mask,
                    int64_t T, int64_t S, int64_t n0, int32_t B, const double* table, float* out_x, void* stream);

int msig_rn_windows_multi(const double* sig, int64_t L, int32_t C_all, const int32_t* cols /* host */, int32_t C, uint32_t log1p_mask,
                          int64_t T, int64_t S, int64_t n0, int32_t B, const double* table, float* out_x, const msig_multi* m,
                          void* stream);

int msig_rn_lv_step(const double* pool, int32_t sessions, int64_t R, int64_t ring_bytes, int32_t C_all, const int32_t* cols /* host */,
                    int32_t C, uint32_t log1p_mask, int64_t T, int64_t S, int32_t K, double* state, int64_t state_bytes,
                    const int32_t* sess /* host */, const int64_t* win /* host */, const int64_t* written /* host */,
                    const int64_t* next /* host */, int32_t B, double* table, void* stream);

int msig_rn_lv_windows_multi(const double* pool, int32_t sessions, int64_t R, int64_t ring_bytes, int32_t C_all,
                             const int32_t* cols /* host */, int32_t C, uint32_t log1p_mask, int64_t T, int64_t S,
                             const int32_t* sess /* host */, const int64_t* win /* host */, const int64_t* written /* host */, int32_t B,
                             const double* table, float* out_x, const msig_multi* m, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSIG_RN_H */
