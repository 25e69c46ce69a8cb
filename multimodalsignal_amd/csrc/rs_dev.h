// The causal polyphase FIR resampler's shared device code (include/msig_rs.h, DESIGN.md sections 39 and 40): the ratio, the output
// count and rs_output, the ONE device function that forms an output sample.  resample.hip (one rate for every column) and mixed.hip
// (a rate per column group) both include it, so a column's bits do not depend on which call resampled it.
#ifndef MSIG_RS_DEV_H
#define MSIG_RS_DEV_H
#include "msig_dev.h"
#include "../../include/msig_rs.h"

struct RsRatio { int32_t L, M, half; };

// msig_rs_out_count without its checks
__host__ __device__ __forceinline__ int64_t rs_count(int64_t n_in, RsRatio r) {
  const int64_t v = n_in * r.L - r.half - 1;
  return v < 0 ? 0 : v / r.M + 1;
}

// Output m: x(j) is raw row j of the thread's column, asked for j = max(0, ceil((m M - half) / L)) .. floor((m M + half) / L) in
// ascending order.  The tap index half + m M - j L runs from at most 2 half down to at least 0.
template <class Fetch>
__device__ __forceinline__ double rs_output(int64_t m, RsRatio r, const double* __restrict__ h, Fetch x) {
  const int64_t c = m * r.M, lo = c - r.half;
  const int64_t j0 = lo <= 0 ? 0 : (lo + r.L - 1) / r.L, j1 = (c + r.half) / r.L;
  const double* tap = h + (r.half + c - j0 * r.L);
  double acc = 0.0;
  for (int64_t j = j0; j <= j1; ++j, tap -= r.L) acc = fma(*tap, x(j), acc);
  return acc;
}

static inline int rs_gcd(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

static inline int rs_ratio_check(int32_t L, int32_t M, int32_t half) {
  if (L < 1 || L > MSIG_RS_MAX_RATIO || M < 1 || M > MSIG_RS_MAX_RATIO || L == M || rs_gcd(L, M) != 1) return MSIG_E_SHAPE;
  if (half < (L > M ? L : M) || half > MSIG_RS_MAX_HALF) return MSIG_E_SHAPE;
  return 0;
}

#endif  // MSIG_RS_DEV_H
