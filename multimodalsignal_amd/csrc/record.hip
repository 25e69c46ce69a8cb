// Windows of one continuous recording (include/msig_rec.h): the statistics of a range of reference windows
// and normalised, transposed (B, C, T) fp32 batches, both taken from the (L, C_all) float64 recording itself — the windows are never
// materialised.  A thread owns a SAMPLE, not a window element: it reads its row once, applies log1p and the z-score once, and then
// serves every window that covers the sample (rec_cover), in every arena slot of the launch.  Consecutive lanes hold consecutive
// samples, which are consecutive t of one channel of one window on the store side: a wave's stores are contiguous except where a
// window begins or ends inside it.
//
// The statistics are normalise.hip's masked sums with an integer weight per sample instead of a mask per window: the same shift by
// a pivot (here the first reference sample), the same fp64 accumulation per thread, wave_sum_d, the four waves added in wave order,
// the workgroups' partials added in workgroup order by one lane per column.  The normalisation is nr_apply_kernel's statement.
#include "msig_dev.h"
#include "../../include/msig_rec.h"

int msig_multi_fold_ctx(const msig_multi* m, FoldCtx& fc);                                  // api.hip: msig_multi's own checks

#define REC_WG 512                      // workgroups of the statistics pass at most: the sums depend on it
#define REC_PART (2 * MSIG_MAX_C)       // doubles of one workgroup's partial: sum[c], then sum of squares[c]
#define REC_SCRATCH_DOUBLES ((int64_t)REC_WG * REC_PART)
struct RecCols { int col[MSIG_MAX_C]; };
struct RecSlots { int n; int64_t off[MSIG_MAX_FOLDS]; };       // byte offset of every slot's batch from out_x

// The windows n in [a, b) that cover sample i, n * S <= i < n * S + T, as the inclusive range lo..hi (empty: lo > hi).
__device__ __forceinline__ void rec_cover(int64_t i, int64_t T, int64_t S, int64_t a, int64_t b, int64_t& lo, int64_t& hi) {
  const int64_t k = i - T + 1;                     // n * S >= k
  lo = k <= 0 ? 0 : (k + S - 1) / S;
  hi = i / S;
  if (lo < a) lo = a;
  if (hi > b - 1) hi = b - 1;
}

// samples [i0, i1): the span of the reference windows [w0, w1)
__global__ __launch_bounds__(256) void rec_stats_kernel(const double* __restrict__ sig, int C_all, RecCols cols, int C, uint32_t log1p_mask,
                                                        int64_t T, int64_t S, int64_t w0, int64_t w1, int64_t i0, int64_t i1,
                                                        double* __restrict__ part) {
  __shared__ double red[4][REC_PART];
  double m1[MSIG_MAX_C], m2[MSIG_MAX_C], pv[MSIG_MAX_C];
#pragma unroll
  for (int c = 0; c < MSIG_MAX_C; ++c) {
    m1[c] = m2[c] = pv[c] = 0.0;
    if (c < C) {                                            // the pivot: the first reference sample, the same value in every thread
      double v = sig[i0 * C_all + cols.col[c]];
      if ((log1p_mask >> c) & 1u) v = log1p(v);
      pv[c] = v;
    }
  }
  for (int64_t i = i0 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < i1; i += (int64_t)gridDim.x * 256) {
    int64_t lo, hi;
    rec_cover(i, T, S, w0, w1, lo, hi);
    if (lo > hi) continue;                                  // S > T: between two windows
    const double w = (double)(hi - lo + 1);                 // an integer <= ceil(T / S): exact
    const double* row = sig + i * C_all;
#pragma unroll
    for (int c = 0; c < MSIG_MAX_C; ++c)
      if (c < C) {
        double v = row[cols.col[c]];
        if ((log1p_mask >> c) & 1u) v = log1p(v);
        const double d = v - pv[c], wd = w * d;
        m1[c] += wd; m2[c] = fma(wd, d, m2[c]);
      }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < MSIG_MAX_C; ++c)
    if (c < C) {
      const double a = wave_sum_d(m1[c]), b = wave_sum_d(m2[c]);
      if (lane == 0) { red[wv][c] = a; red[wv][MSIG_MAX_C + c] = b; }
    }
  __syncthreads();
  if (threadIdx.x < REC_PART && (threadIdx.x & (MSIG_MAX_C - 1)) < C) {
    const int j = threadIdx.x;
    part[(size_t)blockIdx.x * REC_PART + j] = red[0][j] + red[1][j] + red[2][j] + red[3][j];
  }
}

#define REC_BLOCK 16
// One wave: lane l < REC_PART adds up column l of the partials, workgroup 0's first; then lane c finishes channel c.
static_assert((MSIG_MAX_C & (MSIG_MAX_C - 1)) == 0 && REC_PART <= 64, "rec_finalize_kernel: one lane per column of a partial");
__global__ __launch_bounds__(64) void rec_finalize_kernel(const double* __restrict__ sig, int C_all, RecCols cols, int C, uint32_t log1p_mask,
                                                          int64_t i0, const double* __restrict__ part, int nparts, double count,
                                                          double n_ref, double* __restrict__ stats) {
  const int c = threadIdx.x;
  double sum = 0.0;
  if (c < REC_PART && (c & (MSIG_MAX_C - 1)) < C) {      // REC_BLOCK loads in flight, added in workgroup order (nr_finalize_kernel's loop)
    int i = 0;
    for (; i + REC_BLOCK <= nparts; i += REC_BLOCK) {
      double t[REC_BLOCK];
#pragma unroll
      for (int j = 0; j < REC_BLOCK; ++j) t[j] = part[(size_t)(i + j) * REC_PART + c];
#pragma unroll
      for (int j = 0; j < REC_BLOCK; ++j) sum += t[j];
    }
    for (; i < nparts; ++i) sum += part[(size_t)i * REC_PART + c];
  }
  const double a = __shfl(sum, c & (MSIG_MAX_C - 1), 64), b = __shfl(sum, MSIG_MAX_C + (c & (MSIG_MAX_C - 1)), 64);
  if (c == 0) stats[2 * MSIG_MAX_C] = n_ref;
  if (c >= C) return;
  double p = sig[i0 * C_all + cols.col[c]];
  if ((log1p_mask >> c) & 1u) p = log1p(p);
  const double dm = a / count;                        // the mean of d = v - p
  double var = fma(-dm, dm, b / count);
  if (var < 0.0) var = 0.0;
  stats[c] = p + dm;
  stats[MSIG_MAX_C + c] = 1.0 / (sqrt(var) + 1e-8);
}

// samples [i0, i1): the span of the windows [n0, n0 + B)
__global__ __launch_bounds__(256) void rec_windows_kernel(const double* __restrict__ sig, int C_all, RecCols cols, int C, uint32_t log1p_mask,
                                                          int64_t T, int64_t S, int64_t n0, int64_t B, int64_t i0, int64_t i1,
                                                          const double* __restrict__ stats, float* __restrict__ out, RecSlots slots) {
  for (int64_t i = i0 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < i1; i += (int64_t)gridDim.x * 256) {
    int64_t lo, hi;
    rec_cover(i, T, S, n0, n0 + B, lo, hi);
    if (lo > hi) continue;
    const double* row = sig + i * C_all;
    float val[MSIG_MAX_C];
#pragma unroll
    for (int c = 0; c < MSIG_MAX_C; ++c) {
      val[c] = 0.f;
      if (c < C) {
        double v = row[cols.col[c]];
        if ((log1p_mask >> c) & 1u) v = log1p(v);
        val[c] = (float)((v - stats[c]) * stats[MSIG_MAX_C + c]);       // nr_apply_kernel's statement: the same bits
      }
    }
    for (int64_t n = lo; n <= hi; ++n) {
      const size_t at = (size_t)(n - n0) * C * T + (size_t)(i - n * S);      // [n - n0][0][t]
#pragma unroll
      for (int c = 0; c < MSIG_MAX_C; ++c)
        if (c < C)
          for (int z = 0; z < slots.n; ++z)
            *(float*)((char*)out + slots.off[z] + (at + (size_t)c * T) * sizeof(float)) = val[c];
    }
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------
static int64_t rec_count(int64_t L, int64_t T, int64_t S) { return L < T ? 0 : (L - T) / S + 1; }

// the checks the three calls share; fills nc and brings S into the recording's range (S > L: window 0 alone exists either way)
static int rec_check(const double* sig, int64_t L, int32_t C_all, const int32_t* cols, int32_t C, int64_t T, int64_t& S, const double* stats,
                     bool other_null, RecCols& nc) {
  if (!sig || !cols || !stats || other_null) return MSIG_E_NULL;
  if (L < 1 || T < 1 || S < 1 || C_all < 1 || C < 1 || C > MSIG_MAX_C) return MSIG_E_SHAPE;
  for (int c = 0; c < C; ++c)
    if (cols[c] < 0 || cols[c] >= C_all) return MSIG_E_SHAPE;
  for (int c = 0; c < MSIG_MAX_C; ++c) nc.col[c] = c < C ? cols[c] : 0;
  if (S > L) S = L;
  return 0;
}

extern "C" int msig_rec_abi_version(void) { return MSIG_REC_ABI_VERSION; }
extern "C" int64_t msig_rec_scratch_bytes(void) { return REC_SCRATCH_DOUBLES * (int64_t)sizeof(double); }
extern "C" int64_t msig_rec_count(int64_t L, int64_t T, int64_t S) { return T < 1 || S < 1 ? MSIG_E_SHAPE : rec_count(L, T, S); }

extern "C" int msig_rec_stats(const double* sig, int64_t L, int32_t C_all, const int32_t* cols, int32_t C, uint32_t log1p_mask, int64_t T,
                              int64_t S, int64_t w0, int64_t w1, double* stats, void* scratch, void* stream) {
  RecCols nc;
  int rc = rec_check(sig, L, C_all, cols, C, T, S, stats, !scratch, nc); if (rc) return rc;
  if (w0 < 0 || w0 >= w1 || w1 > rec_count(L, T, S)) return MSIG_E_SHAPE;
  if (((uintptr_t)sig | (uintptr_t)stats | (uintptr_t)scratch) & 7) return MSIG_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const int64_t i0 = w0 * S, i1 = (w1 - 1) * S + T, span = i1 - i0;       // i1 <= L: w1 <= N
  const int grid = (int)((span + 255) / 256 > REC_WG ? REC_WG : (span + 255) / 256);
  { MSIG_K("rec_stats", st); rec_stats_kernel<<<grid, 256, 0, st>>>(sig, C_all, nc, C, log1p_mask, T, S, w0, w1, i0, i1, (double*)scratch); }
  MSIG_LAUNCH_CHECK();
  {
    MSIG_K("rec_finalize", st);
    rec_finalize_kernel<<<1, 64, 0, st>>>(sig, C_all, nc, C, log1p_mask, i0, (const double*)scratch, grid, (double)(w1 - w0) * (double)T,
                                          (double)(w1 - w0), stats);
  }
  MSIG_LAUNCH_CHECK();
  return 0;
}

static int rec_windows(const double* sig, int64_t L, int32_t C_all, const int32_t* cols, int32_t C, uint32_t log1p_mask, int64_t T, int64_t S,
                       int64_t n0, int32_t B, const double* stats, float* out_x, const msig_multi* m, bool multi, void* stream) {
  RecCols nc;
  int rc = rec_check(sig, L, C_all, cols, C, T, S, stats, !out_x || (multi && !m), nc); if (rc) return rc;
  if (n0 < 0 || B < 1 || n0 + B > rec_count(L, T, S)) return MSIG_E_SHAPE;
  if ((((uintptr_t)sig | (uintptr_t)stats) & 7) || ((uintptr_t)out_x & 15)) return MSIG_E_ALIGN;
  RecSlots sl{};
  sl.n = 1;
  if (multi) {
    FoldCtx fc; rc = msig_multi_fold_ctx(m, fc); if (rc) return rc;
    if ((double)fc.stride < 4.0 * (double)B * (double)C * (double)T) return MSIG_E_SHAPE;       // a slot's batch would reach into the next arena
    sl.n = fc.n;
    for (int z = 0; z < fc.n; ++z) sl.off[z] = (int64_t)fc.slot[z] * fc.stride;
  }
  hipStream_t st = (hipStream_t)stream;
  const int64_t i0 = n0 * S, i1 = (n0 + B - 1) * S + T, span = i1 - i0;       // i1 <= L: n0 + B <= N
  const int grid = (int)((span + 255) / 256 > 4096 ? 4096 : (span + 255) / 256);
  {
    MSIG_K("rec_windows", st);
    rec_windows_kernel<<<grid, 256, 0, st>>>(sig, C_all, nc, C, log1p_mask, T, S, n0, (int64_t)B, i0, i1, stats, out_x, sl);
  }
  MSIG_LAUNCH_CHECK();
  return 0;
}

extern "C" int msig_rec_windows(const double* sig, int64_t L, int32_t C_all, const int32_t* cols, int32_t C, uint32_t log1p_mask, int64_t T,
                                int64_t S, int64_t n0, int32_t B, const double* stats, float* out_x, void* stream) {
  return rec_windows(sig, L, C_all, cols, C, log1p_mask, T, S, n0, B, stats, out_x, nullptr, false, stream);
}

extern "C" int msig_rec_windows_multi(const double* sig, int64_t L, int32_t C_all, const int32_t* cols, int32_t C, uint32_t log1p_mask,
                                      int64_t T, int64_t S, int64_t n0, int32_t B, const double* stats, float* out_x, const msig_multi* m,
                                      void* stream) {
  return rec_windows(sig, L, C_all, cols, C, log1p_mask, T, S, n0, B, stats, out_x, m, true, stream);
}
