/* msig_mx.h — mixed-rate streams: a sample rate per column group in front of the live rings and offline,
 * exported by libmsig_hip.so beside msig_rs.h, which does not change.
 *
 * The definition.  The C_all columns of a session are split into G groups ("streams"); group g owns the contiguous columns
 * [col0, col0 + ncols) of every ring row and delivers raw rows of ncols float64 values at its own rate.  A group with L != M is
 * resampled by msig_rs.h's definition with the ratio (L, M, half) and the 2 * half + 1 taps at h + h_off: output m of column c is
 *     y[m][col0 + c] = sum over j of h[h_off + half + m * M - j * L] * x[j][c],   j ascending, acc = fma(h, x, acc) from +0.0
 * and exists once msig_rs_out_count(n_in, L, M, half) > m — the same device function as msig_rs_resample and msig_rs_lv_push, so a
 * column's bits do not depend on which of the calls formed it.  A group with L == M == 1 is the IDENTITY: half = 0, tail_rows = 0,
 * output m is raw row m COPIED (no fma: -0.0 and every NaN keep their bits), and n raw rows are n outputs.  All groups start at the
 * same instant: raw row 0 of every group is t = 0.
 *
 * msig_mx_resample: the offline call for ONE group: x is (n_in, ncols), y is (n_out, C_all); outputs 0 .. n_out - 1 go into columns
 * [col0, col0 + ncols) of y and no other value of y is touched.  Any 0 <= n_out <= out_count(n_in) is allowed (a recording is cut at
 * its slowest group).  g is a HOST pointer, read before the call returns; tail_rows and tail_off are not used.
 *
 * msig_mx_lv_push: msig_rs_lv_push with a chunk per (session, group).  Chunk j is len[j] raw rows of ncols(group[j]) doubles, the raw
 * rows raw_written[j] .. raw_written[j] + len[j] - 1 of group group[j] of session sess[j]; the chunks lie back to back in the device
 * buffer `staging` (chunks of different groups have different row widths).  The outputs [count_g(raw_written), count_g(raw_written + len))
 * are stored into columns [col0, col0 + ncols) of rows m % R of the session's ring in the msig_lv.h pool; the other columns of those
 * rows are not touched.  Support rows older than the chunk come from the group's own TAIL: `tails` holds `sessions` blocks, tail_bytes
 * apart; inside a session's block group g keeps tail_rows rows of ncols doubles at tail_off (in doubles), raw row i in tail row
 * i % tail_rows.  A second launch on the same stream brings the tails up to date.  staging == NULL: every row of every chunk is
 * missing (NaN).  sess, group, raw_written and len are HOST arrays of n entries and `groups` a HOST array of G entries, all read
 * before the call returns: the chunk table and the group table travel as kernel arguments, MSIG_MX_CHUNKS chunks a launch pair.
 * A chunk of 0 rows is allowed.  The rings' rows are complete only up to the slowest group's count; that is the caller's `written`.
 *
 * Conventions are msig_lv.h's: asynchronous on `stream`, no allocation, no upload, no state between calls, no host synchronisation,
 * deterministic.
 *
 * Checks, all before any launch.  A group (both calls): L == M == 1 with half != 0 or tail_rows != 0, any other (L, M, half) that
 * msig_rs.h refuses, h_off < 0, ncols < 1, col0 < 0 or col0 + ncols > C_all -> MSIG_E_SHAPE.
 * msig_mx_resample: a NULL g, a NULL h for a group that is not the identity, a NULL x with n_in > 0 or a NULL y with n_out > 0
 * -> MSIG_E_NULL; C_all < 1, n_in < 0 or above MSIG_RS_MAX_ROWS, n_out < 0 or above out_count(n_in) -> MSIG_E_SHAPE; x, y or h not
 * 8-byte aligned -> MSIG_E_ALIGN.
 * msig_mx_lv_push: a NULL pool, tails, groups or host array, a NULL h where a group is not the identity -> MSIG_E_NULL; msig_lv_push's
 * pool checks; G outside 1..MSIG_MX_MAX_GROUPS; two groups whose column ranges overlap; for a group that is not the identity
 * tail_rows < (2 * half) / L + 1 or above 2^31 - 1, tail_off < 0, a tail range that ends beyond tail_bytes, two tail ranges that
 * overlap; n outside 1..sessions * G, a session outside [0, sessions), group[j] outside [0, G), a (session, group) pair twice,
 * raw_written < 0, len < 0 or above 2^31 - 1, raw_written + len above MSIG_RS_MAX_ROWS, a chunk that yields more than R outputs
 * -> MSIG_E_SHAPE; pool, tails, h or staging not 8-byte aligned, ring_bytes or tail_bytes not a multiple of 8 -> MSIG_E_ALIGN.
 */
#ifndef MSIG_MX_H
#define MSIG_MX_H
#include "msig.h"
#include "msig_lv.h"
#include "msig_rs.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSIG_MX_ABI_VERSION 1
#define MSIG_MX_MAX_GROUPS 8                            /* column groups of a session at most */
#define MSIG_MX_CHUNKS 96                               /* (session, group) chunks one launch pair takes */

typedef struct {
  int32_t L, M, half;                                   /* the group's ratio; 1, 1, 0: the identity */
  int32_t col0, ncols;                                  /* its columns of a ring row */
  int32_t reserved;
  int64_t h_off;                                        /* its taps, in doubles into h */
  int64_t tail_rows;                                    /* raw rows a session keeps for it; 0 for the identity */
  int64_t tail_off;                                     /* its tail, in doubles into a session's tail block */
} msig_mx_group;

int msig_mx_abi_version(void);
int64_t msig_mx_struct_bytes(void);                     /* sizeof(msig_mx_group) of the build */

int msig_mx_resample(const double* x, int64_t n_in, const double* h, const msig_mx_group* g /* host */, double* y, int64_t n_out,
                     int32_t C_all, void* stream);

int msig_mx_lv_push(double* pool, int32_t sessions, int64_t R, int64_t ring_bytes, int32_t C_all, double* tails, int64_t tail_bytes,
                    const double* h, const msig_mx_group* groups /* host */, int32_t G, const int32_t* sess /* host */,
                    const int32_t* group /* host */, const int64_t* raw_written /* host */, const int64_t* len /* host */, int32_t n,
                    const double* staging, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSIG_MX_H */
