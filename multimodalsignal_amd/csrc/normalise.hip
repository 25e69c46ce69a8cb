// Per-subject normalisation of raw windows (dataset.py:36-48) + the (N,T,C_all) -> (N,C,T) fp32 layout: msig_normalise_subject
// (include/msig.h), whose mean and std are the subject's own, and msig_nr_normalise_subject (include/msig_nr.h, DESIGN.md section
// 24), whose mean and std come from the subject's REFERENCE windows (ref[n] != 0) and are applied to all of its windows.  One kernel
// family, instantiated with and without a mask.  Three launches on one stream: one pass over the raw rows for the sums, one wave
// that reduces the partials in a fixed order and chooses the statistics, one pass that applies them and transposes.
//
// The all-window sums s1 / s2 are the same statements in both instantiations (row r of thread blockIdx.x * 256 + threadIdx.x,
// stride gridDim.x * 256, wave_sum_d, the four waves' sums added in wave order, the partials added in workgroup order), and the
// masked finalize takes them when the mask selects none or all of the windows: those two calls give msig_normalise_subject's bits.
// The unmasked instantiation reads no mask, forms no pivot and no masked sums, and touches only its own, smaller scratch.
//
// The masked sums are SHIFTED: they accumulate d = v - pivot[c] and d * d, the pivot being the channel's value in the subject's very
// first row (any value near the data serves; this one needs no pass of its own).  mean = pivot + sum(d) / n and
// var = sum(d * d) / n - (sum(d) / n)^2 then cancel nothing even for a channel such as a temperature of 33 +- 0.05, where the
// unshifted E[v^2] - E[v]^2 loses five to six of float64's sixteen digits — too many for statistics of a handful of windows that
// are then applied to a whole recording.  The all-window sums stay unshifted.
#include "msig_dev.h"
#include "../../include/msig_nr.h"

#define NR_WG 512                       // workgroups of the statistics pass at most: the sums depend on it
#define NR_PART (2 * MSIG_MAX_C)        // doubles of one workgroup's partial: sum[c], then sum of squares[c]
struct NrCols { int col[MSIG_MAX_C]; };

// scratch, in doubles —
//   msig_normalise_subject:     part_all[NR_WG][NR_PART], stats[2 * MSIG_MAX_C]
//   msig_nr_normalise_subject:  part_all[NR_WG][NR_PART], part_ref[NR_WG][NR_PART], pivot[MSIG_MAX_C], stats[2 * MSIG_MAX_C + 1]
// The plain call's buffer ends where its stats end: it has no part_ref, no pivot and no n_ref slot stats[2 * MSIG_MAX_C].
#define NORM_SCRATCH_DOUBLES ((int64_t)NR_WG * NR_PART + 2 * MSIG_MAX_C)
#define NR_SCRATCH_DOUBLES ((int64_t)NR_WG * NR_PART * 2 + MSIG_MAX_C + 2 * MSIG_MAX_C + 1)

template <bool MASKED>
__global__ __launch_bounds__(256) void nr_stats_kernel(const double* __restrict__ raw, int64_t rows, int T, int C_all, NrCols cols, int C,
                                                       uint32_t log1p_mask, const uint8_t* __restrict__ ref,
                                                       double* __restrict__ part_all, double* __restrict__ part_ref,
                                                       double* __restrict__ pivot) {
  constexpr int NSUM = MASKED ? 2 * NR_PART : NR_PART;
  __shared__ double red[4][NSUM];
  double s1[MSIG_MAX_C], s2[MSIG_MAX_C], m1[MSIG_MAX_C], m2[MSIG_MAX_C], pv[MSIG_MAX_C];
#pragma unroll
  for (int c = 0; c < MSIG_MAX_C; ++c) {
    s1[c] = s2[c] = m1[c] = m2[c] = pv[c] = 0.0;
    if (MASKED && c < C) {                                  // row 0 of the subject: the same value in every thread
      double v = raw[cols.col[c]];
      if ((log1p_mask >> c) & 1u) v = log1p(v);
      pv[c] = v;
      if (blockIdx.x == 0 && threadIdx.x == 0) pivot[c] = v;      // nr_finalize_kernel adds it back
    }
  }
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (int64_t)gridDim.x * 256) {
    const double* row = raw + r * C_all;
    bool sel = false;
    if constexpr (MASKED) sel = ref[r / T] != 0;
#pragma unroll
    for (int c = 0; c < MSIG_MAX_C; ++c)
      if (c < C) {
        double v = row[cols.col[c]];
        if ((log1p_mask >> c) & 1u) v = log1p(v);
        s1[c] += v; s2[c] = fma(v, v, s2[c]);          // one fused operation in both instantiations: it must not become v * v
        if (MASKED && sel) { const double d = v - pv[c]; m1[c] += d; m2[c] = fma(d, d, m2[c]); }      // and an addition
      }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < MSIG_MAX_C; ++c)
    if (c < C) {
      const double a = wave_sum_d(s1[c]), b = wave_sum_d(s2[c]);
      if (lane == 0) { red[w][c] = a; red[w][MSIG_MAX_C + c] = b; }
      if constexpr (MASKED) {
        const double ma = wave_sum_d(m1[c]), mb = wave_sum_d(m2[c]);
        if (lane == 0) { red[w][NR_PART + c] = ma; red[w][NR_PART + MSIG_MAX_C + c] = mb; }
      }
    }
  __syncthreads();
  if (threadIdx.x < NSUM) {
    const int j = threadIdx.x;              // columns >= C of a partial are never read (nr_finalize_kernel)
    const double sum = red[0][j] + red[1][j] + red[2][j] + red[3][j];
    if (j < NR_PART) part_all[(size_t)blockIdx.x * NR_PART + j] = sum;
    else part_ref[(size_t)blockIdx.x * NR_PART + (j - NR_PART)] = sum;
  }
}

// One wave.  MASKED: every lane counts its share of the mask (integers: the order is immaterial).  Lane l < NR_PART adds up column l
// of the partials — workgroup 0's first, then 1's, ... — with the loads of NR_BLOCK workgroups in flight at a time (a wave reads one
// partial as one 256-byte line; one load per addition, each waiting for the last, costs 0.12 ms for the same additions); then lane c
// takes channel c's two sums and finishes it.
#define NR_BLOCK 16
static_assert((MSIG_MAX_C & (MSIG_MAX_C - 1)) == 0 && NR_PART <= 64, "nr_finalize_kernel: one lane per column of a partial");
template <bool MASKED>
__global__ __launch_bounds__(64) void nr_finalize_kernel(const double* __restrict__ part_all, const double* __restrict__ part_ref,
                                                         const double* __restrict__ pivot, int nparts, int C, int64_t N, int T,
                                                         const uint8_t* __restrict__ ref,
                                                         double* __restrict__ stats, double* __restrict__ stats_out) {
  const int c = threadIdx.x;
  int64_t n_ref = 0;
  if constexpr (MASKED) {
    int mine = 0;
    for (int64_t n = threadIdx.x; n < N; n += 64) mine += ref[n] != 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    n_ref = mine;
    if (c == 0) {
      stats[2 * MSIG_MAX_C] = (double)n_ref;
      if (stats_out) stats_out[2 * MSIG_MAX_C] = (double)n_ref;
    }
  }
  const bool masked = MASKED && n_ref > 0 && n_ref < N;          // none or all selected: the all-window statistics
  const double* part = masked ? part_ref : part_all;
  double sum = 0.0;
  if (c < NR_PART && (c & (MSIG_MAX_C - 1)) < C) {     // columns of unselected channels were never written with sums
    int i = 0;
    for (; i + NR_BLOCK <= nparts; i += NR_BLOCK) {
      double t[NR_BLOCK];
#pragma unroll
      for (int j = 0; j < NR_BLOCK; ++j) t[j] = part[(size_t)(i + j) * NR_PART + c];
#pragma unroll
      for (int j = 0; j < NR_BLOCK; ++j) sum += t[j];
    }
    for (; i < nparts; ++i) sum += part[(size_t)i * NR_PART + c];
  }
  const double a = __shfl(sum, c & (MSIG_MAX_C - 1), 64), b = __shfl(sum, MSIG_MAX_C + (c & (MSIG_MAX_C - 1)), 64);
  if (c >= C) return;
  const double count = (double)((masked ? n_ref : N) * T);
  double mean = a / count;                            // masked: of d = v - pivot
  double var = fma(-mean, mean, b / count);           // b / count - mean * mean, the product fused: pinned
  if (var < 0.0) var = 0.0;
  if (masked) mean += pivot[c];
  const double inv = 1.0 / (sqrt(var) + 1e-8);
  stats[c] = mean;
  stats[MSIG_MAX_C + c] = inv;
  if (stats_out) { stats_out[c] = mean; stats_out[MSIG_MAX_C + c] = inv; }
}

__global__ __launch_bounds__(256) void nr_apply_kernel(const double* __restrict__ raw, int64_t N, int T, int C_all, NrCols cols, int C,
                                                       uint32_t log1p_mask, const double* __restrict__ stats, float* __restrict__ out) {
  const int64_t rows = N * T;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (int64_t)gridDim.x * 256) {
    const int64_t n = r / T;
    const int t = (int)(r - n * T);
    const double* row = raw + r * C_all;
#pragma unroll
    for (int c = 0; c < MSIG_MAX_C; ++c)
      if (c < C) {
        double v = row[cols.col[c]];
        if ((log1p_mask >> c) & 1u) v = log1p(v);
        out[((size_t)n * C + c) * T + t] = (float)((v - stats[c]) * stats[MSIG_MAX_C + c]);     // consecutive t: a wave's stores are contiguous
      }
  }
}

// ref NULL: the unmasked instantiations on the plain call's scratch (stats_out then has no reader and is NULL)
static int launch_normalise(const double* raw, int64_t N, int T, int C_all, const int32_t* cols, int C, uint32_t log1p_mask, const uint8_t* ref,
                            float* out, double* stats_out, void* scratch, hipStream_t st) {
  NrCols nc;
  for (int c = 0; c < MSIG_MAX_C; ++c) nc.col[c] = c < C ? cols[c] : 0;
  double* part_all = (double*)scratch;
  double* part_ref = ref ? part_all + (size_t)NR_WG * NR_PART : nullptr;
  double* pivot = ref ? part_ref + (size_t)NR_WG * NR_PART : nullptr;
  double* applied = ref ? pivot + MSIG_MAX_C : part_all + (size_t)NR_WG * NR_PART;
  const int64_t rows = N * T;
  const int grid = (int)((rows + 255) / 256 > NR_WG ? NR_WG : (rows + 255) / 256);
  {
    MSIG_K("nr_stats", st);
    if (ref) nr_stats_kernel<true><<<grid, 256, 0, st>>>(raw, rows, T, C_all, nc, C, log1p_mask, ref, part_all, part_ref, pivot);
    else nr_stats_kernel<false><<<grid, 256, 0, st>>>(raw, rows, T, C_all, nc, C, log1p_mask, nullptr, part_all, nullptr, nullptr);
  }
  MSIG_LAUNCH_CHECK();
  {
    MSIG_K("nr_finalize", st);
    if (ref) nr_finalize_kernel<true><<<1, 64, 0, st>>>(part_all, part_ref, pivot, grid, C, N, T, ref, applied, stats_out);
    else nr_finalize_kernel<false><<<1, 64, 0, st>>>(part_all, nullptr, nullptr, grid, C, N, T, nullptr, applied, nullptr);
  }
  MSIG_LAUNCH_CHECK();
  const int g2 = (int)((rows + 255) / 256 > 8192 ? 8192 : (rows + 255) / 256);
  { MSIG_K("nr_apply", st); nr_apply_kernel<<<g2, 256, 0, st>>>(raw, N, T, C_all, nc, C, log1p_mask, applied, out); }
  MSIG_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t msig_normalise_scratch_bytes(void) { return NORM_SCRATCH_DOUBLES * (int64_t)sizeof(double); }

extern "C" int msig_normalise_subject(const double* raw, int64_t N, int32_t T, int32_t C_all, const int32_t* cols, int32_t C,
                                      uint32_t log1p_mask, float* out, void* scratch, void* stream) {
  if (!raw || !cols || !out || !scratch) return MSIG_E_NULL;
  if (N < 1 || T < 1 || C_all < 1 || C < 1 || C > MSIG_MAX_C) return MSIG_E_SHAPE;
  for (int c = 0; c < C; ++c)
    if (cols[c] < 0 || cols[c] >= C_all) return MSIG_E_SHAPE;
  if (((uintptr_t)raw | (uintptr_t)scratch) & 7) return MSIG_E_ALIGN;
  return launch_normalise(raw, N, T, C_all, cols, C, log1p_mask, nullptr, out, nullptr, scratch, (hipStream_t)stream);
}

extern "C" int msig_nr_abi_version(void) { return MSIG_NR_ABI_VERSION; }
extern "C" int64_t msig_nr_scratch_bytes(void) { return NR_SCRATCH_DOUBLES * (int64_t)sizeof(double); }

extern "C" int msig_nr_normalise_subject(const double* raw, int64_t N, int32_t T, int32_t C_all, const int32_t* cols, int32_t C,
                                         uint32_t log1p_mask, const uint8_t* ref, float* out, double* stats, void* scratch, void* stream) {
  if (!raw || !cols || !ref || !out || !scratch) return MSIG_E_NULL;
  if (N < 1 || T < 1 || C_all < 1 || C < 1 || C > MSIG_MAX_C) return MSIG_E_SHAPE;
  for (int c = 0; c < C; ++c)
    if (cols[c] < 0 || cols[c] >= C_all) return MSIG_E_SHAPE;
  if (((uintptr_t)raw | (uintptr_t)scratch | (uintptr_t)stats) & 7) return MSIG_E_ALIGN;
  return launch_normalise(raw, N, T, C_all, cols, C, log1p_mask, ref, out, stats, scratch, (hipStream_t)stream);
}
