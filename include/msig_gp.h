/* msig_gp.h — gap-tolerant running references: msig_rn.h's and msig_rd.h's statistics per window for a recording or a live session
 * in which samples are MISSING, and rows in which a missing sample is the reference mean.  The input side of `gaps=Gaps(...)` in
 * monitor.py and live.py, exported by libmsig_hip.so beside msig_rn.h, msig_rd.h and msig_lv.h, none of
 * which changes.  Nobody who does not call these entry points runs a line of them.
 *
 * Notation is msig_rn.h's: window n covers samples [n * S, n * S + T) of a (L, C_all) float64 recording, or of a session of an
 * msig_lv.h pool (sample i in ring row i % R); v is the sample of selected channel c, after log1p where bit c of log1p_mask is set.
 *
 * Missing.  A selected sample is missing when the float64 v — after log1p — has an all-ones exponent field, (bits & 0x7ff0000000000000)
 * == 0x7ff0000000000000: NaN, +Inf, -Inf, and a log1p argument <= -1, which log1p turns into one of them.  The bit pattern is tested,
 * not a library predicate, so no compiler flag changes the answer.  Every other sample is valid.
 * Pivot.  p[c] is the first valid v of channel c in window order: the lowest-index sample of the lowest-index window that holds
 * one; fixed from then on.  One pivot record is MSIG_GP_PIVOT_DOUBLES = 2 * MSIG_MAX_C doubles: [c] = p[c] (0 while not found),
 * [MSIG_MAX_C + c] = 1.0 where found, 0.0 where not.  Windows before the pivot's have no valid sample of c, so nothing depended on it:
 * the definition is causal and the same offline and live.  With sample 0 valid it is msig_rn.h's pivot.
 * Window record.  MSIG_GP_SUM_DOUBLES = 3 * MSIG_MAX_C doubles: [c] = W1 = the sum over the window's VALID samples of (v - p[c]),
 * [MSIG_MAX_C + c] = W2 = the sum of (v - p[c])^2, [2 * MSIG_MAX_C + c] = N[c] = the number of valid samples, an exact integer.  The
 * reduction is msig_rn_sums': thread j of 256 takes samples j, j + 256, ... in that order, the 64 lanes of a wave by xor-butterfly, the
 * four waves in index order; a missing sample contributes the terms 0, 0 and 0, which change no partial sum's bits.  The order is a
 * function of T alone.  A window without a missing sample has msig_rn_sums' W1 and W2 bit for bit, and N = T.
 * Reference of window n.  The mode is one struct, msig_gp_mode {kind, K, decay}: MSIG_GP_EXPANDING (K and decay ignored),
 * MSIG_GP_TRAILING (1 <= K <= MSIG_RN_MAX_K) or MSIG_GP_DECAYED (decay = lambda in [0, 1]).  A record's 48 columns — W1, W2 and the
 * quotient q = N / T of every channel — combine by one rule, one lane per column: expanding carries A_n = A_{n-1} + X_n; trailing adds
 * the terms of windows max(0, n - K + 1) .. n left to right, never a difference; decayed A_n = fma(lambda, A_{n-1}, X_n); A_0 = X_0.
 * The combined quotient e[c] is channel c's effective window count and count = e[c] * T.  Without a missing sample every q is 1.0, e is
 * msig_rn.h's n - a_n + 1 or msig_rd.h's c_n exactly, and count and every later rounding are theirs; lambda = 1 is expanding and
 * lambda = 0 is trailing with K = 1, bit for bit.
 * Statistics of window n, one msig_nr.h record (MSIG_LV_STATS_DOUBLES doubles), msig_rn.h's last lines per selected channel:
 *     dm = A1 / count, var = max(0, fma(-dm, dm, A2 / count)), [c] = p + dm, [MSIG_MAX_C + c] = 1 / (sqrt(var) + 1e-8),
 *     [2 * MSIG_MAX_C] = the number of windows as msig_rn.h / msig_rd.h count them (n - a_n + 1, or c_n = fma(lambda, c_{n-1}, 1)).
 * A channel with count == 0 has no reference yet: [c] = 0 and [MSIG_MAX_C + c] = 0, so its rows are zeros.  So has a channel whose
 * mean or scale would not be finite (valid samples whose squares about the pivot overflow float64: |v - p| above about 1e154).
 * Coverage of window n: MSIG_GP_COV_DOUBLES = MSIG_MAX_C doubles, [c] = N_n[c] / T, the window's own.  Only the selected channels'
 * entries of a statistics or coverage record are written.
 * Rows: out[b][c][t] = (float)((v - rec_b[c]) * rec_b[MSIG_MAX_C + c]) for a valid sample — msig_rn_windows' statement, so with equal
 * records its bits — and +0.0f for a missing one (the reference mean after z-scoring) or where that float would not be finite.
 * Statistics records, coverage records and rows are finite for every input.
 *
 * msig_gp_pivot: the pivot record of the recording's first N windows.  One workgroup walks the windows in order; the 256 samples
 * at hand are tested at once, the first valid one per channel is picked by ballot and wave order.  No atomics.
 * msig_gp_sums: the records of windows [n0, n0 + B) into `sums`, about `pivot`.
 * msig_gp_stats: from `pivot` and the records of windows 0 .. N - 1 the N statistics records (`table`) and the N coverage records
 * (`coverage`).  Expanding and decayed: one wave scans the N windows.  Trailing: one wave per window adds its <= K terms.
 * msig_gp_windows[_multi]: msig_rn_windows[_multi] with the rule for missing samples.
 *
 * Live.  Every session of an msig_lv.h pool owns msig_gp_state_bytes(K) bytes of caller-owned device state, `state_bytes` apart; it
 * needs no initialisation (K = 0 for expanding and decayed).  In doubles: [0, MAX_C) the pivot, [MAX_C, 2 MAX_C) its found flags,
 * [2 MAX_C, 5 MAX_C) the three carries (W1, W2, e), [5 MAX_C] = MSIG_GP_STATE_NEXT the next expected window, then the window count
 * c_n, kind, K and decay of the last step, up to MSIG_GP_STATE_HEAD reserved; then, for trailing, a ring of K window records,
 * window k's in slot k % K.
 * msig_gp_lv_step: msig_rn_lv_step for the three modes.  For B rows (sess[b], win[b], written[b], next[b]: HOST arrays) it looks for
 * the pivot of every channel that has none yet in the window at hand, forms the window's record from the ring with wrap-around
 * (msig_gp_sums' reduction: the same bits), advances the session's state in row order and writes row b's statistics record to table
 * + b * MSIG_LV_STATS_DOUBLES and its coverage record to coverage + b * MSIG_GP_COV_DOUBLES.  A session starts where win == 0.  The
 * rows of one session are adjacent, consecutive windows in ascending order, beginning at next[b].  One workgroup per session, one
 * launch per MSIG_LV_GROUP sessions.  Every record equals msig_gp_stats' for the same samples as one recording, bit for bit.
 * msig_gp_lv_windows_multi: msig_rn_lv_windows_multi with the rule for missing samples.
 * msig_gp_lv_skip: appends len[j] missing rows — a quiet NaN (0x7ff8000000000000) in every column — to session sess[j], whose ring
 * holds written[j] samples: msig_lv_push without a staging buffer, with its wrap rule.
 *
 * Conventions are msig_rn.h's: asynchronous on `stream`, no allocation, no library state, no host synchronisation, deterministic
 * (no float atomics).
 *
 * Checks, all before any launch.  The recording calls: msig_rn.h's, item for item (`pivot`, `sums`, `table` and `coverage` 8-byte
 * aligned and not NULL; msig_gp_pivot and msig_gp_stats: N < 1 or N > the window count -> MSIG_E_SHAPE); a NULL mode -> MSIG_E_NULL;
 * a kind outside the three, K outside 1..MSIG_RN_MAX_K for trailing, decay outside [0, 1] or NaN for decayed -> MSIG_E_SHAPE where
 * msig_rn_stats checks K.  The live calls: msig_rn_lv_step's and msig_rn_lv_windows_multi's, item for item, with the mode in K's
 * place, state_bytes < msig_gp_state_bytes(K of a trailing mode, else 0) -> MSIG_E_SHAPE and a NULL coverage -> MSIG_E_NULL, coverage
 * not 8-byte aligned -> MSIG_E_ALIGN.  msig_gp_lv_skip: msig_lv_push's, item for item, without `staging`.
 */
#ifndef MSIG_GP_H
#define MSIG_GP_H
#include "msig.h"
#include "msig_lv.h"
#include "msig_rn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSIG_GP_ABI_VERSION 1
#define MSIG_GP_SUM_DOUBLES (3 * MSIG_MAX_C)            /* one window record: W1, W2, N */
#define MSIG_GP_PIVOT_DOUBLES (2 * MSIG_MAX_C)          /* one pivot record: the pivots, their found flags */
#define MSIG_GP_COV_DOUBLES MSIG_MAX_C                  /* one coverage record */
#define MSIG_GP_STATE_NEXT (5 * MSIG_MAX_C)             /* the double of a session's state that holds the next expected window */
#define MSIG_GP_STATE_HEAD (6 * MSIG_MAX_C)             /* doubles of a session's state before its ring of records */

#define MSIG_GP_EXPANDING 0
#define MSIG_GP_TRAILING 1
#define MSIG_GP_DECAYED 2

typedef struct msig_gp_mode {
  int32_t kind;         /* MSIG_GP_EXPANDING, MSIG_GP_TRAILING or MSIG_GP_DECAYED */
  int32_t K;            /* trailing: the windows of the reference */
  double  decay;        /* decayed: lambda */
} msig_gp_mode;

int     msig_gp_abi_version(void);
int64_t msig_gp_struct_bytes(void);        /* sizeof(msig_gp_mode) */
int64_t msig_gp_state_bytes(int32_t K);    /* one session's state (K = 0: expanding, decayed); MSIG_E_SHAPE if K is out of range */

int msig_gp_pivot(const double* sig, int64_t L, int32_t C_all, const int32_t* cols /* host */, int32_t C, uint32_t log1p_mask,
                  int64_t T, int64_t S, int64_t N, double* pivot, void* stream);

int msig_gp_sums(const double* sig, int64_t L, int32_t C_all, const int32_t* cols /* host */, int32_t C, uint32_t log1p_mask,
                 int64_t T, int64_t S, const double* pivot, int64_t n0, int64_t B, double* sums, void* stream);

int msig_gp_stats(const double* sig, int64_t L, int32_t C_all, const int32_t* cols /* host */, int32_t C, uint32_t log1p_mask,
                  int64_t T, int64_t S, const double* pivot, const double* sums, int64_t N, const msig_gp_mode* mode, double* table,
                  double* coverage, void* stream);

int msig_gp_windows(const double* sig, int64_t L, int32_t C_all, const int32_t* cols /* host */, int32_t C, uint32_t log1p_mask,
                    int64_t T, int64_t S, int64_t n0, int32_t B, const double* table, float* out_x, void* stream);

int msig_gp_windows_multi(const double* sig, int64_t L, int32_t C_all, const int32_t* cols /* host */, int32_t C, uint32_t log1p_mask,
                          int64_t T, int64_t S, int64_t n0, int32_t B, const double* table, float* out_x, const msig_multi* m,
                          void* stream);

int msig_gp_lv_step(const double* pool, int32_t sessions, int64_t R, int64_t ring_bytes, int32_t C_all, const int32_t* cols /* host */,
                    int32_t C, uint32_t log1p_mask, int64_t T, int64_t S, const msig_gp_mode* mode, double* state, int64_t state_bytes,
                    const int32_t* sess /* host */, const int64_t* win /* host */, const int64_t* written /* host */,
                    const int64_t* next /* host */, int32_t B, double* table, double* coverage, void* stream);

int msig_gp_lv_windows_multi(const double* pool, int32_t sessions, int64_t R, int64_t ring_bytes, int32_t C_all,
                             const int32_t* cols /* host */, int32_t C, uint32_t log1p_mask, int64_t T, int64_t S,
                             const int32_t* sess /* host */, const int64_t* win /* host */, const int64_t* written /* host */, int32_t B,
                             const double* table, float* out_x, const msig_multi* m, void* stream);

int msig_gp_lv_skip(double* pool, int32_t sessions, int64_t R, int64_t ring_bytes, int32_t C_all, const int32_t* sess /* host */,
                    const int64_t* written /* host */, const int64_t* len /* host */, int32_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSIG_GP_H */
