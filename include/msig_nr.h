/* msig_nr.h — per-subject normalisation of raw windows with the statistics of a REFERENCE subset of the subject's windows (the
 * baseline phase, or its first K windows), exported by libmsig_hip.so beside msig.h's msig_normalise_subject, which is unchanged
 * (as are msig_cw.h, msig_cg.h, msig_ft.h, msig_gc.h, msig_aug.h, msig_st.h, msig_ab.h, msig_at.h, msig_mc.h, msig_da.h, msig_wa.h
 * and msig_en.h).
 *
 * The rule.  ref[n] != 0 marks window n as a reference window.  Per selected channel c, over the
 * n_ref * T samples of the reference windows:
 *     v    = raw value, or log1p(raw) where bit c of log1p_mask is set
 *     m    = mean(v_ref),  s = population std(v_ref)  (one pass of float64 sums of v - p and its square, p the channel's value in
 *                                                      the subject's first row; the variance clamped at 0)
 *     out  = (float)((v - m) * (1 / (s + 1e-8)))      for EVERY window of the subject, transposed (N,T,C_all) -> (N,C,T)
 * A mask that selects no window, and a mask that selects every window, give the output of msig_normalise_subject on the same
 * input bit for bit: the statistics of all windows are accumulated beside the masked ones with that call's own row-to-thread
 * mapping and summation order, and the kernel — which counts the selected windows itself, the mask being device memory — takes
 * them in both cases.  Which windows a "baseline" or "baseline:K" reference selects is the caller's business: the library never
 * sees labels.
 *
 * Conventions are msig_normalise_subject's: asynchronous on `stream`, no allocation, no state between calls, deterministic
 * (fp64 partial sums per workgroup, summed in one fixed order by one thread per channel; no float atomics).
 *
 * stats (optional, device, 2 * MSIG_MAX_C + 1 doubles): [c] = m, [MSIG_MAX_C + c] = 1 / (s + 1e-8) of the statistics that were
 * applied, [2 * MSIG_MAX_C] = the number of windows the mask selects (0 = the all-window statistics were applied).
 *
 * Checks, all before any launch: NULL raw, cols, ref, out or scratch -> MSIG_E_NULL; N < 1, T < 1, C_all < 1, C outside
 * 1..MSIG_MAX_C or a column outside [0, C_all) -> MSIG_E_SHAPE; raw, scratch or stats not 8-byte aligned -> MSIG_E_ALIGN.
 */
#ifndef MSIG_NR_H
#define MSIG_NR_H
#include "msig.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSIG_NR_ABI_VERSION 1

int     msig_nr_abi_version(void);
int64_t msig_nr_scratch_bytes(void);      /* bytes of `scratch` (device, 8-byte aligned) */

/* raw: (N, T, C_all) float64, device.  cols: C host ints, the selected columns in output order.  ref: N device bytes.
 * out: (N, C, T) fp32, device. */
int msig_nr_normalise_subject(const double* raw, int64_t N, int32_t T, int32_t C_all, const int32_t* cols, int32_t C,
                              uint32_t log1p_mask, const uint8_t* ref, float* out, double* stats, void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSIG_NR_H */
