/* msig_aug.h — on-device window augmentation inside the training gather of libmsig_hip.so.
 *
 * A training batch is produced by one gather launch (msig_gather_windows; msig_gather_windows_multi writes a fold batch straight into
 * the arenas the next launch trains on), so a caller has no point at which it could transform x.  The calls below are those gathers
 * with the usual wearable-sensor augmentations applied to every gathered window on its way through the registers.  They stand beside
 * msig.h, msig_cw.h, msig_cg.h, msig_ft.h and msig_gc.h, which are unchanged; libmsig_hip.so exports all of them.
 *
 * Transforms, per gathered window, in this order.  A transform whose parameter is 0 is SKIPPED, not computed
 * with a neutral value (-0.0 * 1 + 0 is +0.0): with all four at 0 the calls leave exactly the plain gather's bits.
 *   1. magnitude scaling, scale_sigma > 0:   a = 1 + scale_sigma * g      one factor per (row, channel)     y = fmul(x, a)
 *   2. jitter, jitter_sigma > 0:             n = jitter_sigma * g         one draw per sample               y = fadd(y, n)
 *      (single fp32 roundings, never contracted into an FMA)
 *   3. time mask, mask_prob > 0:  with probability mask_prob per row one span [t0, t0 + len) is set to +0.0 in every channel,
 *      len uniform in 1..mask_max, t0 uniform in 0..T-len
 *   4. channel dropout, chan_drop_prob > 0:  each channel of a row is set to +0.0 over the whole window with that probability,
 *      independently; if every channel of a row was drawn, one channel chosen by the hash is kept.
 *
 * Randomness is counter-based and stateless: every draw is a pure function of (key, row in the batch, channel, sample), with
 * fmix32 the 32-bit murmur3 finaliser of the dropout streams and key = msig_dropout_key(seed, step, 3) (stream ids 1 and 2 are the
 * GRU and head dropout).  "row" is the row of the BATCH, not the store index: a window gathered twice is augmented twice.
 *     rk        = fmix32(key ^ (row * 0x9E3779B9))                                   row key
 *     ck        = fmix32(rk + (c + 1) * 0x7F4A7C15)                                  (row, channel) key
 *     scale     g(fmix32(ck ^ 0x80000001))
 *     jitter    g(fmix32(ck ^ t))                     t = sample index < 2^31: disjoint from the tagged words
 *     chan drop fmix32(ck ^ 0x80000002) <= thr(chan_drop_prob);   the kept one of an all-drawn row: mulhi(fmix32(rk ^ 0x80000006), C)
 *     mask      fmix32(rk ^ 0x80000003) <= thr(mask_prob);   len = 1 + mulhi(fmix32(rk ^ 0x80000004), mask_max);
 *               t0 = mulhi(fmix32(rk ^ 0x80000005), T - len + 1)
 *     g(w)      = (float)((b0 + b1 + b2 + b3) - 510) * MSIG_AUG_NOISE_K, b_i the bytes of w: a standardised 4-term sum (mean 0,
 *               variance 1, range +-510 k = +-3.45, kurtosis 2.7); integer arithmetic and ONE fp32 multiplication
 *     mulhi(w, n) = (uint32)(((uint64)w * n) >> 32)                                   uniform in 0..n-1
 *     thr(p)    = ceil(p * 2^32) - 1 in double precision (computed by the launcher): the event has probability ceil(p 2^32) / 2^32,
 *               exactly 1 for p = 1
 * All arithmetic is modulo 2^32.  tests/aug_reference.py restates this in numpy, bit for bit.
 *
 * Layout and conventions are the plain gathers': store (N, C, T) fp32, idx int64 store positions, out_x (B, C, T), labels optional
 * (store_labels / out_y NULL: not gathered).  In the multi call fold z reads idx + z * idx_row_stride, writes its own arena
 * (out + m->slot[z] * m->stride_bytes) and draws from a->key[z].
 *
 * Checks, all before any launch: NULL msig_aug, store, idx or out_x (multi: msig_multi) -> MSIG_E_NULL; in the multi call msig_multi's
 * own checks come next (msig.h); then MSIG_E_SHAPE for B outside 1..65535, C outside 1..MSIG_MAX_C, T < 4 or T % 4 != 0,
 * idx_row_stride < B, a negative or NaN sigma, mask_prob outside [0,1], chan_drop_prob outside [0,1), mask_prob > 0 with mask_max
 * outside 1..T; then store / out_x not 16-byte aligned -> MSIG_E_ALIGN.
 */
#ifndef MSIG_AUG_H
#define MSIG_AUG_H
#include "msig.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSIG_AUG_ABI_VERSION 1
#define MSIG_AUG_STREAM_ID 3                  /* msig_dropout_key's stream id of the augmentation keys */
#define MSIG_AUG_NOISE_K 0.006765875034f  /* fp32 nearest to 1 / sqrt(4 * (256^2 - 1) / 12) = 1 / sqrt(21845) */

typedef struct msig_aug {
  float scale_sigma, jitter_sigma, mask_prob, chan_drop_prob;
  int32_t mask_max, reserved;           /* reserved: write 0 (not read) */
  uint32_t key[MSIG_MAX_FOLDS];         /* per fold of the launch; [0] for a single model */
} msig_aug;

int msig_aug_abi_version(void);
int64_t msig_aug_struct_bytes(void);    /* sizeof(msig_aug) of the build */

/* msig_gather_windows with the augmentation (windows of C channels x T samples). */
int msig_aug_gather_windows(const float* store, const int64_t* store_labels, const int64_t* idx, int32_t B, int32_t C, int32_t T,
                            float* out_x, int64_t* out_y, const msig_aug* a, void* stream);

/* msig_gather_windows_multi with the augmentation; the parameters are the launch's, the keys per fold. */
int msig_aug_gather_windows_multi(const float* store, const int64_t* store_labels, const int64_t* idx, int64_t idx_row_stride, int32_t B,
                                  int32_t C, int32_t T, float* out_x, int64_t* out_y, const msig_multi* m, const msig_aug* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSIG_AUG_H */
