// Causal running references (include/msig_rn.h): statistics per WINDOW — of windows 0..n ("expanding") or of
// the last K ("trailing:K") — for a continuous recording and for the sessions of a live ring pool, and the (B, C, T) batches whose
// every row is normalised with its own record.
//
// With a record per row, record.hip's "normalise a sample once, store it into every window that covers it" no longer applies: a
// sample has another value in every window.  So the unit of the statistics is the window's own pair of sums about a pivot that is
// fixed for the recording's life (rn_window_sums: one workgroup, one reduction order that depends on T alone, the samples reached
// through an addresser — linear recording or wrapped ring — so both give the same bits), and a window's reference is an ordered
// sum of such records: a carry for expanding, at most K terms added left to right for trailing (never a difference of prefix sums).
// rn_finalize is rec_finalize_kernel's last lines.  The row kernels are streaming kernels: a thread owns one (row, t), reads its
// sample's row once and stores the C values into every arena slot; consecutive lanes are consecutive t on the store side.
#include "msig_dev.h"
#include "../../include/msig_rn.h"
#include "../../include/msig_rd.h"

int msig_multi_fold_ctx(const msig_multi* m, FoldCtx& fc);                                  // api.hip: msig_multi's own checks

#define RN_PART MSIG_RN_SUM_DOUBLES     // doubles of one window-sum record: sum[c], then sum of squares[c]
#define RN_REC MSIG_LV_STATS_DOUBLES    // doubles of one statistics record
#define RN_BLOCK 16                     // loads in flight in the ordered sums (rec_finalize_kernel's REC_BLOCK)
#define RN_NEXT (3 * MSIG_MAX_C)        // a session's state: [0, MAX_C) pivot, [MAX_C, 3 MAX_C) carry, then next window, K
static_assert((MSIG_MAX_C & (MSIG_MAX_C - 1)) == 0 && RN_PART <= 64, "one lane per column of a record");
static_assert(RN_NEXT + 2 <= MSIG_RN_STATE_HEAD, "the state's head holds the pivot, the carry and two scalars");
struct RnCols { int col[MSIG_MAX_C]; };
struct RnSlots { int n; int64_t off[MSIG_MAX_FOLDS]; };        // byte offset of every slot's batch from out_x
struct RnRun { int64_t n0; int32_t session, count, b0, pad; };           // windows n0 .. n0 + count - 1 are rows b0 .. of the batch
struct RnRuns { RnRun e[MSIG_LV_GROUP]; };
static_assert(sizeof(RnRuns) + sizeof(RnSlots) + sizeof(RnCols) + 192 <= 4096, "the tables are kernel arguments");

// where sample i lives
struct RnLinear {
  const double* base; int64_t C_all;
  __device__ __forceinline__ const double* row(int64_t i) const { return base + i * C_all; }
};
struct RnRing {
  const double* base; int64_t C_all, R;
  __device__ __forceinline__ const double* row(int64_t i) const { return base + (i % R) * C_all; }
};

__device__ __forceinline__ double rn_value(const double* row, int col, bool lg) {
  double v = row[col];
  if (lg) v = log1p(v);
  return v;
}

// The sums of the T samples from i0 on about the pivots pv, by the whole workgroup of 256: w[c] = W1, w[MSIG_MAX_C + c] = W2 (shared).
// Thread-strided accumulation, wave_sum_d, the four waves in index order (rec_stats_kernel's end).  Ends synchronised.
template <class A>
__device__ __forceinline__ void rn_window_sums(const A& ad, int64_t i0, int64_t T, const RnCols& cols, int C, uint32_t log1p_mask,
                                               const double (&pv)[MSIG_MAX_C], double (*red)[RN_PART], double* w) {
  double m1[MSIG_MAX_C], m2[MSIG_MAX_C];
#pragma unroll
  for (int c = 0; c < MSIG_MAX_C; ++c) m1[c] = m2[c] = 0.0;
  for (int64_t t = threadIdx.x; t < T; t += 256) {
    const double* row = ad.row(i0 + t);
#pragma unroll
    for (int c = 0; c < MSIG_MAX_C; ++c)
      if (c < C) {
        const double d = rn_value(row, cols.col[c], (log1p_mask >> c) & 1u) - pv[c];
        m1[c] += d; m2[c] = fma(d, d, m2[c]);
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
  if (threadIdx.x < RN_PART && (threadIdx.x & (MSIG_MAX_C - 1)) < C) {
    const int j = threadIdx.x;
    w[j] = red[0][j] + red[1][j] + red[2][j] + red[3][j];
  }
  __syncthreads();
}

// rec[k] = record k's column (this lane's); the terms a .. n added left to right, RN_BLOCK loads in flight.
template <class F>
__device__ __forceinline__ double rn_span_sum(F rec, int64_t a, int64_t n) {
  double acc = *rec(a);
  int64_t k = a + 1;
  for (; k + RN_BLOCK <= n + 1; k += RN_BLOCK) {
    double t[RN_BLOCK];
#pragma unroll
    for (int q = 0; q < RN_BLOCK; ++q) t[q] = *rec(k + q);
#pragma unroll
    for (int q = 0; q < RN_BLOCK; ++q) acc += t[q];
  }
  for (; k <= n; ++k) acc += *rec(k);
  return acc;
}

// One wave, all 64 lanes: lane j < RN_PART holds column j of the reference's sums; lane c finishes channel c with its pivot p.
__device__ __forceinline__ void rn_finalize(double acc, double p, int C, double n_ref, double T, double* rec) {
  const int c = threadIdx.x & 63;
  const double a = __shfl(acc, c & (MSIG_MAX_C - 1), 64), b = __shfl(acc, MSIG_MAX_C + (c & (MSIG_MAX_C - 1)), 64);
  if (c == 0) rec[2 * MSIG_MAX_C] = n_ref;
  if (c >= C) return;
  const double count = n_ref * T;
  const double dm = a / count;                        // the mean of d = v - p
  double var = fma(-dm, dm, b / count);
  if (var < 0.0) var = 0.0;
  rec[c] = p + dm;
  rec[MSIG_MAX_C + c] = 1.0 / (sqrt(var) + 1e-8);
}

// window n0 + b per workgroup
__global__ __launch_bounds__(256) void rn_sums_kernel(const double* __restrict__ sig, int C_all, RnCols cols, int C, uint32_t log1p_mask,
                                                      int64_t T, int64_t S, int64_t n0, int64_t B, double* __restrict__ sums) {
  __shared__ double red[4][RN_PART];
  __shared__ double w[RN_PART];
  const RnLinear ad{sig, C_all};
  double pv[MSIG_MAX_C];
#pragma unroll
  for (int c = 0; c < MSIG_MAX_C; ++c) {
    pv[c] = 0.0;
    if (c < C) pv[c] = rn_value(sig, cols.col[c], (log1p_mask >> c) & 1u);      // sample 0 of the recording
  }
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    rn_window_sums(ad, (n0 + b) * S, T, cols, C, log1p_mask, pv, red, w);
    if (threadIdx.x < RN_PART && (threadIdx.x & (MSIG_MAX_C - 1)) < C) sums[b * RN_PART + threadIdx.x] = w[threadIdx.x];
  }
}

// K = 0: one wave scans the N windows.  K >= 1: a wave per window.
__global__ __launch_bounds__(64) void rn_stats_kernel(const double* __restrict__ sig, RnCols cols, int C, uint32_t log1p_mask, double T,
                                                      const double* __restrict__ sums, int64_t N, int K, double* __restrict__ table) {
  const int j = threadIdx.x;
  const bool on = j < RN_PART && (j & (MSIG_MAX_C - 1)) < C;
  double p = 0.0;
  if (j < C) p = rn_value(sig, cols.col[j], (log1p_mask >> j) & 1u);
  if (K == 0) {
    double acc = 0.0;
    for (int64_t n = 0; n < N; n += RN_BLOCK) {
      double t[RN_BLOCK];
#pragma unroll
      for (int q = 0; q < RN_BLOCK; ++q) t[q] = on && n + q < N ? sums[(n + q) * RN_PART + j] : 0.0;
#pragma unroll
      for (int q = 0; q < RN_BLOCK; ++q)
        if (n + q < N) {
          acc = n + q == 0 ? t[q] : acc + t[q];
          rn_finalize(acc, p, C, (double)(n + q + 1), T, table + (n + q) * RN_REC);
        }
    }
    return;
  }
  for (int64_t n = blockIdx.x; n < N; n += gridDim.x) {
    const int64_t a = n - K + 1 < 0 ? 0 : n - K + 1;
    double acc = 0.0;
    if (on) acc = rn_span_sum([&](int64_t k) { return sums + k * RN_PART + j; }, a, n);
    rn_finalize(acc, p, C, (double)(n - a + 1), T, table + n * RN_REC);
  }
}

// rows [0, count) are windows n0 .. of the addresser's samples: row q's record at rec0 + q * RN_REC, its output row at out row b0 + q
template <class A>
__device__ __forceinline__ void rn_rows(const A& ad, int64_t n0, int64_t count, int64_t b0, int64_t T, int64_t S, const RnCols& cols, int C,
                                        uint32_t log1p_mask, const double* __restrict__ rec0, float* __restrict__ out, const RnSlots& slots) {
  const int64_t total = count * T;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t q = e / T, t = e - q * T;
    const double* row = ad.row((n0 + q) * S + t);
    const double* rec = rec0 + q * RN_REC;
    const size_t at = (size_t)(b0 + q) * C * T + (size_t)t;                  // [b][0][t]
#pragma unroll
    for (int c = 0; c < MSIG_MAX_C; ++c)
      if (c < C) {
        const double v = rn_value(row, cols.col[c], (log1p_mask >> c) & 1u);
        const float val = (float)((v - rec[c]) * rec[MSIG_MAX_C + c]);       // nr_apply_kernel's statement: the same bits
        for (int z = 0; z < slots.n; ++z)
          *(float*)((char*)out + slots.off[z] + (at + (size_t)c * T) * sizeof(float)) = val;
      }
  }
}

__global__ __launch_bounds__(256) void rn_windows_kernel(const double* __restrict__ sig, int C_all, RnCols cols, int C, uint32_t log1p_mask,
                                                         int64_t T, int64_t S, int64_t n0, int64_t B, const double* __restrict__ table,
                                                         float* __restrict__ out, RnSlots slots) {
  rn_rows(RnLinear{sig, C_all}, n0, B, 0, T, S, cols, C, log1p_mask, table, out, slots);
}

// run blockIdx.y
__global__ __launch_bounds__(256) void rn_lv_windows_kernel(const double* __restrict__ pool, int64_t ring_doubles, int64_t R, int C_all, RnCols cols,
                                                            int C, uint32_t log1p_mask, int64_t T, int64_t S, const double* __restrict__ table,
                                                            float* __restrict__ out, RnSlots slots, RnRuns runs) {
  const RnRun r = runs.e[blockIdx.y];
  rn_rows(RnRing{pool + (int64_t)r.session * ring_doubles, C_all, R}, r.n0, r.count, r.b0, T, S, cols, C, log1p_mask,
          table + (int64_t)r.b0 * RN_REC, out, slots);
}

// run blockIdx.x: one session's rows in order — the window's sums by the workgroup, then wave 0 advances the session's state (lane j
// owns column j of the carry and of every record of the sum ring, so it reads back only what it wrote itself) and finishes the row
__global__ __launch_bounds__(256) void rn_lv_step_kernel(const double* __restrict__ pool, int64_t ring_doubles, int64_t R, int C_all, RnCols cols,
                                                         int C, uint32_t log1p_mask, int64_t T, int64_t S, int K, double* state_all,
                                                         int64_t state_doubles, double* __restrict__ table, RnRuns runs) {
  __shared__ double red[4][RN_PART];
  __shared__ double w[RN_PART];
  const RnRun r = runs.e[blockIdx.x];
  const RnRing ad{pool + (int64_t)r.session * ring_doubles, C_all, R};
  double* st = state_all + (int64_t)r.session * state_doubles;
  double* ring = st + MSIG_RN_STATE_HEAD;
  const bool first = r.n0 == 0;                       // the session starts here: sample 0 is in ring row 0 (window 0 is whole)
  double pv[MSIG_MAX_C];
#pragma unroll
  for (int c = 0; c < MSIG_MAX_C; ++c) {
    pv[c] = 0.0;
    if (c < C) pv[c] = first ? rn_value(ad.row(0), cols.col[c], (log1p_mask >> c) & 1u) : st[c];
  }
  const int j = threadIdx.x;
  const bool on = j < RN_PART && (j & (MSIG_MAX_C - 1)) < C;
  double p = 0.0, acc = 0.0;
  if (j < C) {
    p = first ? rn_value(ad.row(0), cols.col[j], (log1p_mask >> j) & 1u) : st[j];
    if (first) st[j] = p;                             // nobody reads st[0 .. C) in a launch that writes it
  }
  if (K == 0 && on && !first) acc = st[MSIG_MAX_C + j];
  for (int q = 0; q < r.count; ++q) {
    const int64_t n = r.n0 + q;
    rn_window_sums(ad, n * S, T, cols, C, log1p_mask, pv, red, w);
    if (j < 64) {
      int64_t a = 0;
      if (K == 0) {
        if (on) acc = n == 0 ? w[j] : acc + w[j];
      } else {
        a = n - K + 1 < 0 ? 0 : n - K + 1;
        if (on) {
          ring[(n % K) * RN_PART + j] = w[j];
          acc = rn_span_sum([&](int64_t k) { return ring + (k % K) * RN_PART + j; }, a, n);
        }
      }
      rn_finalize(acc, p, C, (double)(n - a + 1), (double)T, table + (int64_t)(r.b0 + q) * RN_REC);
    }
  }
  if (K == 0 && on) st[MSIG_MAX_C + j] = acc;
  if (j == 0) { st[RN_NEXT] = (double)(r.n0 + r.count); st[RN_NEXT + 1] = (double)K; }
}

// ---- the decayed reference (include/msig_rd.h) -------------------------------------------------
// A_n = fma(decay, A_{n-1}, W_n) per column, c_n = fma(decay, c_{n-1}, 1), A_0 = W_0, c_0 = 1; rn_finalize with n_ref = c_n.
#define RD_C MSIG_RD_STATE_C            // a session's state: the effective window count c, then the decay of the last step
static_assert(RD_C > RN_NEXT + 1 && RD_C + 2 <= MSIG_RN_STATE_HEAD, "c and the decay live in the head's reserved doubles");

// one wave scans the N windows: rn_stats_kernel's expanding branch with the decayed recurrence in place of the sum
__global__ __launch_bounds__(64) void rd_stats_kernel(const double* __restrict__ sig, RnCols cols, int C, uint32_t log1p_mask, double T,
                                                      const double* __restrict__ sums, int64_t N, double decay, double* __restrict__ table) {
  const int j = threadIdx.x;
  const bool on = j < RN_PART && (j & (MSIG_MAX_C - 1)) < C;
  double p = 0.0;
  if (j < C) p = rn_value(sig, cols.col[j], (log1p_mask >> j) & 1u);
  double acc = 0.0, cn = 0.0;
  for (int64_t n = 0; n < N; n += RN_BLOCK) {
    double t[RN_BLOCK];
#pragma unroll
    for (int q = 0; q < RN_BLOCK; ++q) t[q] = on && n + q < N ? sums[(n + q) * RN_PART + j] : 0.0;
#pragma unroll
    for (int q = 0; q < RN_BLOCK; ++q)
      if (n + q < N) {
        acc = n + q == 0 ? t[q] : fma(decay, acc, t[q]);
        cn = n + q == 0 ? 1.0 : fma(decay, cn, 1.0);
        rn_finalize(acc, p, C, cn, T, table + (n + q) * RN_REC);
      }
  }
}

// run blockIdx.x: rn_lv_step_kernel's expanding branch with the decayed recurrence; every lane of wave 0 carries c, lane 0 stores it
__global__ __launch_bounds__(256) void rd_lv_step_kernel(const double* __restrict__ pool, int64_t ring_doubles, int64_t R, int C_all, RnCols cols,
                                                         int C, uint32_t log1p_mask, int64_t T, int64_t S, double decay, double* state_all,
                                                         int64_t state_doubles, double* __restrict__ table, RnRuns runs) {
  __shared__ double red[4][RN_PART];
  __shared__ double w[RN_PART];
  const RnRun r = runs.e[blockIdx.x];
  const RnRing ad{pool + (int64_t)r.session * ring_doubles, C_all, R};
  double* st = state_all + (int64_t)r.session * state_doubles;
  const bool first = r.n0 == 0;                       // the session starts here: sample 0 is in ring row 0 (window 0 is whole)
  double pv[MSIG_MAX_C];
#pragma unroll
  for (int c = 0; c < MSIG_MAX_C; ++c) {
    pv[c] = 0.0;
    if (c < C) pv[c] = first ? rn_value(ad.row(0), cols.col[c], (log1p_mask >> c) & 1u) : st[c];
  }
  const int j = threadIdx.x;
  const bool on = j < RN_PART && (j & (MSIG_MAX_C - 1)) < C;
  double p = 0.0, acc = 0.0, cn = 0.0;
  if (j < C) {
    p = first ? rn_value(ad.row(0), cols.col[j], (log1p_mask >> j) & 1u) : st[j];
    if (first) st[j] = p;                             // nobody reads st[0 .. C) in a launch that writes it
  }
  if (on && !first) acc = st[MSIG_MAX_C + j];
  if (j < 64 && !first) cn = st[RD_C];                // wave 0 alone reads c, and its lane 0 alone stores it, at the end
  for (int q = 0; q < r.count; ++q) {
    const int64_t n = r.n0 + q;
    rn_window_sums(ad, n * S, T, cols, C, log1p_mask, pv, red, w);
    if (j < 64) {
      if (on) acc = n == 0 ? w[j] : fma(decay, acc, w[j]);
      cn = n == 0 ? 1.0 : fma(decay, cn, 1.0);
      rn_finalize(acc, p, C, cn, (double)T, table + (int64_t)(r.b0 + q) * RN_REC);
    }
  }
  if (on) st[MSIG_MAX_C + j] = acc;
  if (j == 0) { st[RN_NEXT] = (double)(r.n0 + r.count); st[RN_NEXT + 1] = 0.0; st[RD_C] = cn; st[RD_C + 1] = decay; }
}

// ---- host ----------------------------------------------------------------------------------------------------------
static int64_t rn_count(int64_t L, int64_t T, int64_t S) { return L < T ? 0 : (L - T) / S + 1; }

// msig_rec.h's shared checks (record.hip's rec_check); fills nc and brings S into the recording's range
static int rn_rec_check(const double* sig, int64_t L, int32_t C_all, const int32_t* cols, int32_t C, int64_t T, int64_t& S, const void* tab,
                        bool other_null, RnCols& nc) {
  if (!sig || !cols || !tab || other_null) return MSIG_E_NULL;
  if (L < 1 || T < 1 || S < 1 || C_all < 1 || C < 1 || C > MSIG_MAX_C) return MSIG_E_SHAPE;
  for (int c = 0; c < C; ++c)
    if (cols[c] < 0 || cols[c] >= C_all) return MSIG_E_SHAPE;
  for (int c = 0; c < MSIG_MAX_C; ++c) nc.col[c] = c < C ? cols[c] : 0;
  if (S > L) S = L;
  return 0;
}

extern "C" int msig_rn_abi_version(void) { return MSIG_RN_ABI_VERSION; }
extern "C" int64_t msig_rn_state_bytes(int32_t K) {
  if (K < 0 || K > MSIG_RN_MAX_K) return MSIG_E_SHAPE;
  return ((int64_t)MSIG_RN_STATE_HEAD + (int64_t)K * RN_PART) * (int64_t)sizeof(double);
}

extern "C" int msig_rn_sums(const double* sig, int64_t L, int32_t C_all, const int32_t* cols, int32_t C, uint32_t log1p_mask, int64_t T,
                            int64_t S, int64_t n0, int64_t B, double* sums, void* stream) {
  RnCols nc;
  int rc = rn_rec_check(sig, L, C_all, cols, C, T, S, sums, false, nc); if (rc) return rc;
  if (n0 < 0 || B < 1 || B > rn_count(L, T, S) || n0 > rn_count(L, T, S) - B) return MSIG_E_SHAPE;
  if (((uintptr_t)sig | (uintptr_t)sums) & 7) return MSIG_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  { MSIG_K("rn_sums", st); rn_sums_kernel<<<(unsigned)(B > 65536 ? 65536 : B), 256, 0, st>>>(sig, C_all, nc, C, log1p_mask, T, S, n0, B, sums); }
  MSIG_LAUNCH_CHECK();
  return 0;
}

// the reference's mode: K windows (0: expanding), or — decayed — a decay in [0, 1] (a NaN fails both comparisons)
struct RnMode { int32_t K; double decay; bool decayed; };
static bool rn_mode_ok(const RnMode& md) { return md.decayed ? md.decay >= 0.0 && md.decay <= 1.0 : md.K >= 0 && md.K <= MSIG_RN_MAX_K; }

static int rn_stats(const double* sig, int64_t L, int32_t C_all, const int32_t* cols, int32_t C, uint32_t log1p_mask, int64_t T, int64_t S,
                    const double* sums, int64_t N, const RnMode& md, double* table, void* stream) {
  RnCols nc;
  int rc = rn_rec_check(sig, L, C_all, cols, C, T, S, sums, !table, nc); if (rc) return rc;
  if (N < 1 || N > rn_count(L, T, S) || !rn_mode_ok(md)) return MSIG_E_SHAPE;
  if (((uintptr_t)sig | (uintptr_t)sums | (uintptr_t)table) & 7) return MSIG_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  if (md.decayed) {
    MSIG_K("rd_stats", st); rd_stats_kernel<<<1, 64, 0, st>>>(sig, nc, C, log1p_mask, (double)T, sums, N, md.decay, table);
  } else {
    const unsigned grid = md.K == 0 ? 1u : (unsigned)(N > 65536 ? 65536 : N);
    MSIG_K("rn_stats", st); rn_stats_kernel<<<grid, 64, 0, st>>>(sig, nc, C, log1p_mask, (double)T, sums, N, md.K, table);
  }
  MSIG_LAUNCH_CHECK();
  return 0;
}

extern "C" int msig_rn_stats(const double* sig, int64_t L, int32_t C_all, const int32_t* cols, int32_t C, uint32_t log1p_mask, int64_t T,
                             int64_t S, const double* sums, int64_t N, int32_t K, double* table, void* stream) {
  return rn_stats(sig, L, C_all, cols, C, log1p_mask, T, S, sums, N, RnMode{K, 0.0, false}, table, stream);
}

extern "C" int msig_rd_abi_version(void) { return MSIG_RD_ABI_VERSION; }
extern "C" int msig_rd_stats(const double* sig, int64_t L, int32_t C_all, const int32_t* cols, int32_t C, uint32_t log1p_mask, int64_t T,
                             int64_t S, const double* sums, int64_t N, double decay, double* table, void* stream) {
  return rn_stats(sig, L, C_all, cols, C, log1p_mask, T, S, sums, N, RnMode{0, decay, true}, table, stream);
}

static int rn_slots(const msig_multi* m, bool multi, int32_t B, int32_t C, int64_t T, RnSlots& sl) {
  sl = RnSlots{};
  sl.n = 1;
  if (!multi) return 0;
  FoldCtx fc; int rc = msig_multi_fold_ctx(m, fc); if (rc) return rc;
  if ((double)fc.stride < 4.0 * (double)B * (double)C * (double)T) return MSIG_E_SHAPE;       // a slot's batch would reach into the next arena
  sl.n = fc.n;
  for (int z = 0; z < fc.n; ++z) sl.off[z] = (int64_t)fc.slot[z] * fc.stride;
  return 0;
}

static int rn_windows(const double* sig, int64_t L, int32_t C_all, const int32_t* cols, int32_t C, uint32_t log1p_mask, int64_t T, int64_t S,
                      int64_t n0, int32_t B, const double* table, float* out_x, const msig_multi* m, bool multi, void* stream) {
  RnCols nc;
  int rc = rn_rec_check(sig, L, C_all, cols, C, T, S, table, !out_x || (multi && !m), nc); if (rc) return rc;
  if (n0 < 0 || B < 1 || n0 + B > rn_count(L, T, S)) return MSIG_E_SHAPE;
  if ((((uintptr_t)sig | (uintptr_t)table) & 7) || ((uintptr_t)out_x & 15)) return MSIG_E_ALIGN;
  RnSlots sl;
  rc = rn_slots(m, multi, B, C, T, sl); if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t blocks = ((int64_t)B * T + 255) / 256;
  {
    MSIG_K("rn_windows", st);
    rn_windows_kernel<<<(unsigned)(blocks > 65536 ? 65536 : blocks), 256, 0, st>>>(sig, C_all, nc, C, log1p_mask, T, S, n0, (int64_t)B, table, out_x, sl);
  }
  MSIG_LAUNCH_CHECK();
  return 0;
}

extern "C" int msig_rn_windows(const double* sig, int64_t L, int32_t C_all, const int32_t* cols, int32_t C, uint32_t log1p_mask, int64_t T,
                               int64_t S, int64_t n0, int32_t B, const double* table, float* out_x, void* stream) {
  return rn_windows(sig, L, C_all, cols, C, log1p_mask, T, S, n0, B, table, out_x, nullptr, false, stream);
}

extern "C" int msig_rn_windows_multi(const double* sig, int64_t L, int32_t C_all, const int32_t* cols, int32_t C, uint32_t log1p_mask,
                                     int64_t T, int64_t S, int64_t n0, int32_t B, const double* table, float* out_x, const msig_multi* m,
                                     void* stream) {
  return rn_windows(sig, L, C_all, cols, C, log1p_mask, T, S, n0, B, table, out_x, m, true, stream);
}

// msig_lv.h's pool checks (live.hip's)
static int rn_pool_shape(int32_t sessions, int64_t R, int64_t ring_bytes, int32_t C_all) {
  if (sessions < 1 || sessions > MSIG_LV_MAX_SESSIONS || R < 1 || R > INT32_MAX || C_all < 1) return MSIG_E_SHAPE;
  if (ring_bytes < R * (int64_t)C_all * (int64_t)sizeof(double)) return MSIG_E_SHAPE;
  return 0;
}
static bool rn_pool_misaligned(const void* pool, int64_t ring_bytes) { return ((uintptr_t)pool & 7) || (ring_bytes & 7); }

// msig_lv_windows_multi's shape checks of the batch's rows; fills nc
static int rn_lv_rows_check(int32_t sessions, int64_t R, int32_t C_all, const int32_t* cols, int32_t C, int64_t T, int64_t S, const int32_t* sess,
                            const int64_t* win, const int64_t* written, int32_t B, RnCols& nc) {
  if (T < 1 || S < 1 || C < 1 || C > MSIG_MAX_C || B < 1) return MSIG_E_SHAPE;
  for (int c = 0; c < C; ++c)
    if (cols[c] < 0 || cols[c] >= C_all) return MSIG_E_SHAPE;
  for (int c = 0; c < MSIG_MAX_C; ++c) nc.col[c] = c < C ? cols[c] : 0;
  for (int b = 0; b < B; ++b) {
    if (sess[b] < 0 || sess[b] >= sessions || win[b] < 0) return MSIG_E_SHAPE;
    if (written[b] < T || win[b] > (written[b] - T) / S) return MSIG_E_SHAPE;       // not yet complete: win * S + T > written
    if (win[b] * S < written[b] - R) return MSIG_E_SHAPE;                           // its first samples are already overwritten
  }
  return 0;
}

static int rn_lv_step(const double* pool, int32_t sessions, int64_t R, int64_t ring_bytes, int32_t C_all, const int32_t* cols, int32_t C,
                      uint32_t log1p_mask, int64_t T, int64_t S, const RnMode& md, double* state, int64_t state_bytes, const int32_t* sess,
                      const int64_t* win, const int64_t* written, const int64_t* next, int32_t B, double* table, void* stream) {
  if (!pool || !cols || !state || !sess || !win || !written || !next || !table) return MSIG_E_NULL;
  int rc = rn_pool_shape(sessions, R, ring_bytes, C_all); if (rc) return rc;
  RnCols nc;
  rc = rn_lv_rows_check(sessions, R, C_all, cols, C, T, S, sess, win, written, B, nc); if (rc) return rc;
  if (!rn_mode_ok(md) || state_bytes < msig_rn_state_bytes(md.K)) return MSIG_E_SHAPE;
  uint64_t seen[MSIG_LV_MAX_SESSIONS / 64] = {};
  for (int b = 0; b < B; ++b) {
    if (b > 0 && sess[b] == sess[b - 1]) {
      if (win[b] != win[b - 1] + 1) return MSIG_E_SHAPE;                 // not the session's next window
      continue;
    }
    uint64_t& word = seen[sess[b] >> 6];
    if (word >> (sess[b] & 63) & 1u) return MSIG_E_SHAPE;                // the session in two separate places
    word |= (uint64_t)1 << (sess[b] & 63);
    if (win[b] != next[b]) return MSIG_E_SHAPE;                          // the state stands elsewhere
  }
  if (rn_pool_misaligned(pool, ring_bytes) || (((uintptr_t)state | (uintptr_t)table) & 7) || (state_bytes & 7)) return MSIG_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  for (int b = 0; b < B;) {
    RnRuns runs{};
    int k = 0;
    for (; b < B && k < MSIG_LV_GROUP; ++k) {              // a run: the rows of one session
      int e = b + 1;
      while (e < B && sess[e] == sess[b]) ++e;
      runs.e[k] = RnRun{win[b], sess[b], e - b, b, 0};
      b = e;
    }
    if (md.decayed) {
      MSIG_K("rd_lv_step", st);
      rd_lv_step_kernel<<<(unsigned)k, 256, 0, st>>>(pool, ring_bytes / 8, R, C_all, nc, C, log1p_mask, T, S, md.decay, state, state_bytes / 8, table, runs);
    } else {
      MSIG_K("rn_lv_step", st);
      rn_lv_step_kernel<<<(unsigned)k, 256, 0, st>>>(pool, ring_bytes / 8, R, C_all, nc, C, log1p_mask, T, S, md.K, state, state_bytes / 8, table, runs);
    }
    MSIG_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int msig_rn_lv_step(const double* pool, int32_t sessions, int64_t R, int64_t ring_bytes, int32_t C_all, const int32_t* cols, int32_t C,
                               uint32_t log1p_mask, int64_t T, int64_t S, int32_t K, double* state, int64_t state_bytes, const int32_t* sess,
                               const int64_t* win, const int64_t* written, const int64_t* next, int32_t B, double* table, void* stream) {
  return rn_lv_step(pool, sessions, R, ring_bytes, C_all, cols, C, log1p_mask, T, S, RnMode{K, 0.0, false}, state, state_bytes, sess, win, written, next,
                    B, table, stream);
}

extern "C" int msig_rd_lv_step(const double* pool, int32_t sessions, int64_t R, int64_t ring_bytes, int32_t C_all, const int32_t* cols, int32_t C,
                               uint32_t log1p_mask, int64_t T, int64_t S, double decay, double* state, int64_t state_bytes, const int32_t* sess,
                               const int64_t* win, const int64_t* written, const int64_t* next, int32_t B, double* table, void* stream) {
  return rn_lv_step(pool, sessions, R, ring_bytes, C_all, cols, C, log1p_mask, T, S, RnMode{0, decay, true}, state, state_bytes, sess, win, written, next,
                    B, table, stream);
}

extern "C" int msig_rn_lv_windows_multi(const double* pool, int32_t sessions, int64_t R, int64_t ring_bytes, int32_t C_all, const int32_t* cols,
                                        int32_t C, uint32_t log1p_mask, int64_t T, int64_t S, const int32_t* sess, const int64_t* win,
                                        const int64_t* written, int32_t B, const double* table, float* out_x, const msig_multi* m, void* stream) {
  if (!pool || !cols || !sess || !win || !written || !table || !out_x || !m) return MSIG_E_NULL;
  int rc = rn_pool_shape(sessions, R, ring_bytes, C_all); if (rc) return rc;
  RnCols nc;
  rc = rn_lv_rows_check(sessions, R, C_all, cols, C, T, S, sess, win, written, B, nc); if (rc) return rc;
  if (rn_pool_misaligned(pool, ring_bytes) || ((uintptr_t)table & 7) || ((uintptr_t)out_x & 15)) return MSIG_E_ALIGN;
  RnSlots sl;
  rc = rn_slots(m, true, B, C, T, sl); if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  for (int b = 0; b < B;) {
    RnRuns runs{};
    int k = 0;
    int64_t most = 0;
    for (; b < B && k < MSIG_LV_GROUP; ++k) {              // a run: rows b .. that are consecutive windows of one session
      int e = b + 1;
      while (e < B && sess[e] == sess[b] && win[e] == win[e - 1] + 1) ++e;
      runs.e[k] = RnRun{win[b], sess[b], e - b, b, 0};
      if ((int64_t)(e - b) * T > most) most = (int64_t)(e - b) * T;
      b = e;
    }
    const int64_t blocks = (most + 255) / 256;
    {
      MSIG_K("rn_lv_windows", st);
      rn_lv_windows_kernel<<<dim3((unsigned)(blocks > 4096 ? 4096 : blocks), (unsigned)k), 256, 0, st>>>(pool, ring_bytes / 8, R, C_all, nc, C, log1p_mask,
                                                                                                     T, S, table, out_x, sl, runs);
    }
    MSIG_LAUNCH_CHECK();
  }
  return 0;
}
