// Gap-tolerant running references (include/msig_gp.h): running.hip's statistics per window and rows with a
// record per row, for recordings and live sessions in which samples are missing.  A sample is missing when its float64 value, after
// log1p, has an all-ones exponent field (gp_missing tests the bits).  Everything else is running.hip's shape: a window's record is
// taken by one workgroup in rn_window_sums' order with a third sum, the count of valid samples — a missing sample contributes three
// zeros through selects, no branch — a reference is an ordered combination of records (one lane per column of the 48: W1, W2 and the
// quotient N / T, whose combination is the channel's effective window count), and the row kernels are streaming kernels in which a
// thread owns one (row, t).  The pivot is no longer sample 0 but the first valid sample in window order: gp_window_pivot looks for
// it 256 samples at a time, by ballot and wave order.  Without a missing sample every value formed here has running.hip's bits.
#include "msig_dev.h"
#include "../../include/msig_gp.h"

int msig_multi_fold_ctx(const msig_multi* m, FoldCtx& fc);                                  // api.hip: msig_multi's own checks

#define GP_PART MSIG_GP_SUM_DOUBLES     // doubles of one window record: W1[c], W2[c], N[c]
#define GP_REC MSIG_LV_STATS_DOUBLES    // doubles of one statistics record
#define GP_COV MSIG_GP_COV_DOUBLES      // doubles of one coverage record
#define GP_BLOCK 16                     // loads in flight in the ordered sums (running.hip's RN_BLOCK)
#define GP_FOUND MSIG_MAX_C             // a pivot record and a session's state: [0, MAX_C) pivot, [MAX_C, 2 MAX_C) found flags
#define GP_CARRY (2 * MSIG_MAX_C)       // a session's state: the 48 carries
#define GP_NEXT MSIG_GP_STATE_NEXT      // then the next window, c_n, kind, K, decay
static_assert((MSIG_MAX_C & (MSIG_MAX_C - 1)) == 0 && GP_PART <= 64, "one lane per column of a record");
static_assert(GP_CARRY + GP_PART == GP_NEXT && GP_NEXT + 5 <= MSIG_GP_STATE_HEAD, "the state's head holds the pivot, the carries and five scalars");
static_assert(MSIG_GP_PIVOT_DOUBLES <= GP_PART, "a pivot record fits the shared record");
struct GpCols { int col[MSIG_MAX_C]; };
struct GpSlots { int n; int64_t off[MSIG_MAX_FOLDS]; };        // byte offset of every slot's batch from out_x
struct GpRun { int64_t n0; int32_t session, count, b0, pad; };           // windows n0 .. n0 + count - 1 are rows b0 .. of the batch
struct GpRuns { GpRun e[MSIG_LV_GROUP]; };
struct GpSkip { int32_t start, len, session, pad; };                     // len rows from ring row `start` on
struct GpSkips { GpSkip e[MSIG_LV_GROUP]; };
static_assert(sizeof(GpRuns) + sizeof(GpSlots) + sizeof(GpCols) + 192 <= 4096 && sizeof(GpSkips) + 64 <= 4096, "the tables are kernel arguments");

// where sample i lives
struct GpLinear {
  const double* base; int64_t C_all;
  __device__ __forceinline__ const double* row(int64_t i) const { return base + i * C_all; }
};
struct GpRing {
  const double* base; int64_t C_all, R;
  __device__ __forceinline__ const double* row(int64_t i) const { return base + (i % R) * C_all; }
};

__device__ __forceinline__ double gp_value(const double* row, int col, bool lg) {
  double v = row[col];
  if (lg) v = log1p(v);
  return v;
}

// NaN, +Inf, -Inf: an all-ones exponent field
__device__ __forceinline__ bool gp_missing(double v) {
  return (__double_as_longlong(v) & 0x7ff0000000000000LL) == 0x7ff0000000000000LL;
}
__device__ __forceinline__ bool gp_missing_f(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// The pivot record in w (shared: w[c] the pivot, w[GP_FOUND + c] 1.0 where found; set and synchronised on entry): every channel that
// has none yet takes the first valid sample of the T samples from i0 on.  256 samples at a time: the first valid lane of a wave by
// ballot, the four waves in index order; red is the scratch.  Leaves as soon as no channel is looking.  Ends synchronised.
template <class A>
__device__ __forceinline__ void gp_window_pivot(const A& ad, int64_t i0, int64_t T, const GpCols& cols, int C, uint32_t log1p_mask,
                                                double (*red)[GP_PART], double* w) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int64_t base = 0; base < T; base += 256) {
    bool need = false;
#pragma unroll
    for (int c = 0; c < MSIG_MAX_C; ++c)
      if (c < C) need |= w[GP_FOUND + c] == 0.0;
    if (!need) break;                                   // the same for every thread: w changes only between the two barriers below
    const int64_t t = base + threadIdx.x;
    const double* row = ad.row(i0 + (t < T ? t : 0));
#pragma unroll
    for (int c = 0; c < MSIG_MAX_C; ++c)
      if (c < C) {
        const double v = gp_value(row, cols.col[c], (log1p_mask >> c) & 1u);
        const unsigned long long b = __ballot(t < T && !gp_missing(v));
        if (b && lane == __ffsll((long long)b) - 1) red[wv][c] = v;
        if (lane == 0) red[wv][GP_FOUND + c] = b ? 1.0 : 0.0;
      }
    __syncthreads();
    if (threadIdx.x < C && w[GP_FOUND + threadIdx.x] == 0.0) {
      const int c = threadIdx.x;
      for (int k = 0; k < 4; ++k)
        if (red[k][GP_FOUND + c] != 0.0) { w[c] = red[k][c]; w[GP_FOUND + c] = 1.0; break; }
    }
    __syncthreads();
  }
}

// every selected channel of the pivot record in w has its pivot
__device__ __forceinline__ bool gp_all_found(const double* w, int C) {
  bool all = true;
#pragma unroll
  for (int c = 0; c < MSIG_MAX_C; ++c)
    if (c < C) all &= w[GP_FOUND + c] != 0.0;
  return all;
}

// The record of the T samples from i0 on about the pivots pv, by the whole workgroup of 256: w[c] = W1, w[MAX_C + c] = W2,
// w[2 MAX_C + c] = N (shared).  rn_window_sums with a validity select: a missing sample adds 0, 0 and 0.  Ends synchronised.
template <class A>
__device__ __forceinline__ void gp_window_sums(const A& ad, int64_t i0, int64_t T, const GpCols& cols, int C, uint32_t log1p_mask,
                                               const double (&pv)[MSIG_MAX_C], double (*red)[GP_PART], double* w) {
  double m1[MSIG_MAX_C], m2[MSIG_MAX_C], mn[MSIG_MAX_C];
#pragma unroll
  for (int c = 0; c < MSIG_MAX_C; ++c) m1[c] = m2[c] = mn[c] = 0.0;
  for (int64_t t = threadIdx.x; t < T; t += 256) {
    const double* row = ad.row(i0 + t);
#pragma unroll
    for (int c = 0; c < MSIG_MAX_C; ++c)
      if (c < C) {
        const double v = gp_value(row, cols.col[c], (log1p_mask >> c) & 1u);
        const bool ok = !gp_missing(v);
        const double d = ok ? v - pv[c] : 0.0;
        m1[c] += d; m2[c] = fma(d, d, m2[c]); mn[c] += ok ? 1.0 : 0.0;
      }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < MSIG_MAX_C; ++c)
    if (c < C) {
      const double a = wave_sum_d(m1[c]), b = wave_sum_d(m2[c]), n = wave_sum_d(mn[c]);
      if (lane == 0) { red[wv][c] = a; red[wv][MSIG_MAX_C + c] = b; red[wv][2 * MSIG_MAX_C + c] = n; }
    }
  __syncthreads();
  if (threadIdx.x < GP_PART && (threadIdx.x & (MSIG_MAX_C - 1)) < C) {
    const int j = threadIdx.x;
    w[j] = red[0][j] + red[1][j] + red[2][j] + red[3][j];
  }
  __syncthreads();
}

// column j of a record as a term of the reference: W1 and W2 as they are, N as the quotient N / T
__device__ __forceinline__ double gp_term(double x, int j, double T) { return j >= 2 * MSIG_MAX_C ? x / T : x; }

// term(k) = window k's term of this lane's column; the terms a .. n added left to right, GP_BLOCK loads in flight (rn_span_sum)
template <class F>
__device__ __forceinline__ double gp_span_sum(F term, int64_t a, int64_t n) {
  double acc = term(a);
  int64_t k = a + 1;
  for (; k + GP_BLOCK <= n + 1; k += GP_BLOCK) {
    double t[GP_BLOCK];
#pragma unroll
    for (int q = 0; q < GP_BLOCK; ++q) t[q] = term(k + q);
#pragma unroll
    for (int q = 0; q < GP_BLOCK; ++q) acc += t[q];
  }
  for (; k <= n; ++k) acc += term(k);
  return acc;
}

// One wave, all 64 lanes: lane j < GP_PART holds column j of the reference (acc) and of the window's own terms (own); lane c
// finishes channel c with its pivot p — rn_finalize with the channel's own count e * T, and the window's coverage.
__device__ __forceinline__ void gp_finalize(double acc, double own, double p, int C, double n_ref, double T, double* rec, double* cov) {
  const int c = threadIdx.x & 63, ci = c & (MSIG_MAX_C - 1);
  const double a = __shfl(acc, ci, 64), b = __shfl(acc, MSIG_MAX_C + ci, 64), e = __shfl(acc, 2 * MSIG_MAX_C + ci, 64);
  const double q = __shfl(own, 2 * MSIG_MAX_C + ci, 64);
  if (c == 0) rec[2 * MSIG_MAX_C] = n_ref;
  if (c >= C) return;
  cov[c] = q;
  const double count = e * T;
  const double dm = a / count;                        // the mean of d = v - p
  double var = fma(-dm, dm, b / count);
  if (var < 0.0) var = 0.0;
  const double mean = p + dm, inv = 1.0 / (sqrt(var) + 1e-8);
  const bool ok = count != 0.0 && !gp_missing(mean) && !gp_missing(inv);      // no reference yet, or one that float64 cannot hold
  rec[c] = ok ? mean : 0.0;
  rec[MSIG_MAX_C + c] = ok ? inv : 0.0;
}

// one workgroup: the windows in order until every channel has its pivot
__global__ __launch_bounds__(256) void gp_pivot_kernel(const double* __restrict__ sig, int C_all, GpCols cols, int C, uint32_t log1p_mask,
                                                       int64_t T, int64_t S, int64_t N, double* __restrict__ pivot) {
  __shared__ double red[4][GP_PART];
  __shared__ double w[GP_PART];
  const GpLinear ad{sig, C_all};
  if (threadIdx.x < GP_PART) w[threadIdx.x] = 0.0;
  __syncthreads();
  for (int64_t n = 0; n < N; ++n) {
    if (gp_all_found(w, C)) break;
    gp_window_pivot(ad, n * S, T, cols, C, log1p_mask, red, w);
  }
  if (threadIdx.x < MSIG_GP_PIVOT_DOUBLES && (threadIdx.x & (MSIG_MAX_C - 1)) < C) pivot[threadIdx.x] = w[threadIdx.x];
}

// window n0 + b per workgroup
__global__ __launch_bounds__(256) void gp_sums_kernel(const double* __restrict__ sig, int C_all, GpCols cols, int C, uint32_t log1p_mask,
                                                      int64_t T, int64_t S, const double* __restrict__ pivot, int64_t n0, int64_t B,
                                                      double* __restrict__ sums) {
  __shared__ double red[4][GP_PART];
  __shared__ double w[GP_PART];
  const GpLinear ad{sig, C_all};
  double pv[MSIG_MAX_C];
#pragma unroll
  for (int c = 0; c < MSIG_MAX_C; ++c) {
    pv[c] = 0.0;
    if (c < C) pv[c] = pivot[c];
  }
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    gp_window_sums(ad, (n0 + b) * S, T, cols, C, log1p_mask, pv, red, w);
    if (threadIdx.x < GP_PART && (threadIdx.x & (MSIG_MAX_C - 1)) < C) sums[b * GP_PART + threadIdx.x] = w[threadIdx.x];
  }
}

// expanding, decayed: one wave scans the N windows.  trailing: a wave per window.
__global__ __launch_bounds__(64) void gp_stats_kernel(const double* __restrict__ pivot, int C, double T, const double* __restrict__ sums, int64_t N,
                                                      int kind, int K, double decay, double* __restrict__ table, double* __restrict__ cov) {
  const int j = threadIdx.x;
  const bool on = j < GP_PART && (j & (MSIG_MAX_C - 1)) < C;
  double p = 0.0;
  if (j < C) p = pivot[j];
  if (kind != MSIG_GP_TRAILING) {
    const bool decayed = kind == MSIG_GP_DECAYED;
    double acc = 0.0, cn = 0.0;
    for (int64_t n = 0; n < N; n += GP_BLOCK) {
      double t[GP_BLOCK];
#pragma unroll
      for (int q = 0; q < GP_BLOCK; ++q) t[q] = on && n + q < N ? gp_term(sums[(n + q) * GP_PART + j], j, T) : 0.0;
#pragma unroll
      for (int q = 0; q < GP_BLOCK; ++q)
        if (n + q < N) {
          acc = n + q == 0 ? t[q] : (decayed ? fma(decay, acc, t[q]) : acc + t[q]);
          cn = !decayed ? (double)(n + q + 1) : (n + q == 0 ? 1.0 : fma(decay, cn, 1.0));
          gp_finalize(acc, t[q], p, C, cn, T, table + (n + q) * GP_REC, cov + (n + q) * GP_COV);
        }
    }
    return;
  }
  for (int64_t n = blockIdx.x; n < N; n += gridDim.x) {
    const int64_t a = n - K + 1 < 0 ? 0 : n - K + 1;
    double acc = 0.0, own = 0.0;
    if (on) {
      acc = gp_span_sum([&](int64_t k) { return gp_term(sums[k * GP_PART + j], j, T); }, a, n);
      own = gp_term(sums[n * GP_PART + j], j, T);
    }
    gp_finalize(acc, own, p, C, (double)(n - a + 1), T, table + n * GP_REC, cov + n * GP_COV);
  }
}

// rows [0, count) are windows n0 .. of the addresser's samples: row q's record at rec0 + q * GP_REC, its output row at out row b0 + q
template <class A>
__device__ __forceinline__ void gp_rows(const A& ad, int64_t n0, int64_t count, int64_t b0, int64_t T, int64_t S, const GpCols& cols, int C,
                                        uint32_t log1p_mask, const double* __restrict__ rec0, float* __restrict__ out, const GpSlots& slots) {
  const int64_t total = count * T;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t q = e / T, t = e - q * T;
    const double* row = ad.row((n0 + q) * S + t);
    const double* rec = rec0 + q * GP_REC;
    const size_t at = (size_t)(b0 + q) * C * T + (size_t)t;                  // [b][0][t]
#pragma unroll
    for (int c = 0; c < MSIG_MAX_C; ++c)
      if (c < C) {
        const double v = gp_value(row, cols.col[c], (log1p_mask >> c) & 1u);
        const float z = (float)((v - rec[c]) * rec[MSIG_MAX_C + c]);         // rn_rows' statement: the same bits
        const float val = gp_missing(v) || gp_missing_f(z) ? 0.f : z;        // a missing sample is the reference mean
        for (int s = 0; s < slots.n; ++s)
          *(float*)((char*)out + slots.off[s] + (at + (size_t)c * T) * sizeof(float)) = val;
      }
  }
}

__global__ __launch_bounds__(256) void gp_windows_kernel(const double* __restrict__ sig, int C_all, GpCols cols, int C, uint32_t log1p_mask,
                                                         int64_t T, int64_t S, int64_t n0, int64_t B, const double* __restrict__ table,
                                                         float* __restrict__ out, GpSlots slots) {
  gp_rows(GpLinear{sig, C_all}, n0, B, 0, T, S, cols, C, log1p_mask, table, out, slots);
}

// run blockIdx.y
__global__ __launch_bounds__(256) void gp_lv_windows_kernel(const double* __restrict__ pool, int64_t ring_doubles, int64_t R, int C_all, GpCols cols,
                                                            int C, uint32_t log1p_mask, int64_t T, int64_t S, const double* __restrict__ table,
                                                            float* __restrict__ out, GpSlots slots, GpRuns runs) {
  const GpRun r = runs.e[blockIdx.y];
  gp_rows(GpRing{pool + (int64_t)r.session * ring_doubles, C_all, R}, r.n0, r.count, r.b0, T, S, cols, C, log1p_mask,
          table + (int64_t)r.b0 * GP_REC, out, slots);
}

// run blockIdx.x: one session's rows in order — while a channel has no pivot the window at hand is searched and the pivot record
// goes to the state (thread j writes and later reads back its own double); then the window's record by the workgroup; then wave 0
// advances the session's state (lane j owns column j of the carries and of every record of the ring) and finishes the row
__global__ __launch_bounds__(256) void gp_lv_step_kernel(const double* __restrict__ pool, int64_t ring_doubles, int64_t R, int C_all, GpCols cols,
                                                         int C, uint32_t log1p_mask, int64_t T, int64_t S, int kind, int K, double decay,
                                                         double* state_all, int64_t state_doubles, double* __restrict__ table,
                                                         double* __restrict__ cov, GpRuns runs) {
  __shared__ double red[4][GP_PART];
  __shared__ double w[GP_PART];
  const GpRun r = runs.e[blockIdx.x];
  const GpRing ad{pool + (int64_t)r.session * ring_doubles, C_all, R};
  double* st = state_all + (int64_t)r.session * state_doubles;
  double* ring = st + MSIG_GP_STATE_HEAD;
  const bool first = r.n0 == 0;                       // the session starts here: nothing of the state is read
  const bool trailing = kind == MSIG_GP_TRAILING, decayed = kind == MSIG_GP_DECAYED;
  const int j = threadIdx.x;
  const bool on = j < GP_PART && (j & (MSIG_MAX_C - 1)) < C;
  const bool mine = j < MSIG_GP_PIVOT_DOUBLES && (j & (MSIG_MAX_C - 1)) < C;      // this thread keeps double j of the pivot record
  double pv[MSIG_MAX_C];
#pragma unroll
  for (int c = 0; c < MSIG_MAX_C; ++c) pv[c] = 0.0;
  double p = 0.0, acc = 0.0, cn = 0.0;
  if (!trailing && on && !first) acc = st[GP_CARRY + j];
  if (j < 64 && !first) cn = st[GP_NEXT + 1];         // wave 0 alone reads c_n, and its lane 0 alone stores it, at the end
  bool all = false;
  for (int q = 0; q < r.count; ++q) {
    const int64_t n = r.n0 + q;
    if (!all) {
      if (j < GP_PART) w[j] = mine && !(first && q == 0) ? st[j] : 0.0;
      __syncthreads();
      gp_window_pivot(ad, n * S, T, cols, C, log1p_mask, red, w);
      all = gp_all_found(w, C);
#pragma unroll
      for (int c = 0; c < MSIG_MAX_C; ++c) {
        if (c < C) pv[c] = w[c];
        if (j == c) p = pv[c];
      }
      if (mine) st[j] = w[j];                         // gp_window_sums overwrites w only behind its first barrier
    }
    gp_window_sums(ad, n * S, T, cols, C, log1p_mask, pv, red, w);
    if (j < 64) {
      const double x = on ? w[j] : 0.0, own = on ? gp_term(x, j, (double)T) : 0.0;
      int64_t a = 0;
      if (trailing) {
        a = n - K + 1 < 0 ? 0 : n - K + 1;
        if (on) {
          ring[(n % K) * GP_PART + j] = x;
          acc = gp_span_sum([&](int64_t k) { return gp_term(ring[(k % K) * GP_PART + j], j, (double)T); }, a, n);
        }
        cn = (double)(n - a + 1);
      } else {
        if (on) acc = n == 0 ? own : (decayed ? fma(decay, acc, own) : acc + own);
        cn = !decayed ? (double)(n + 1) : (n == 0 ? 1.0 : fma(decay, cn, 1.0));
      }
      gp_finalize(acc, own, p, C, cn, (double)T, table + (int64_t)(r.b0 + q) * GP_REC, cov + (int64_t)(r.b0 + q) * GP_COV);
    }
  }
  if (!trailing && on) st[GP_CARRY + j] = acc;
  if (j == 0) {
    st[GP_NEXT] = (double)(r.n0 + r.count); st[GP_NEXT + 1] = cn; st[GP_NEXT + 2] = (double)kind;
    st[GP_NEXT + 3] = (double)(trailing ? K : 0); st[GP_NEXT + 4] = decayed ? decay : 0.0;
  }
}

// entry blockIdx.y: len * C_all quiet NaNs into the ring, from ring row `start` on, wrapped once at most (lv_push_kernel's addresses)
__global__ __launch_bounds__(256) void gp_lv_skip_kernel(double* __restrict__ pool, int64_t ring_doubles, int64_t R, int C_all, GpSkips tab) {
  const GpSkip e = tab.e[blockIdx.y];
  const int64_t total = (int64_t)e.len * C_all, wrap = R * C_all, d0 = (int64_t)e.start * C_all;
  double* __restrict__ ring = pool + (int64_t)e.session * ring_doubles;
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < total; k += (int64_t)gridDim.x * 256) {
    int64_t d = d0 + k;
    if (d >= wrap) d -= wrap;
    ring[d] = __longlong_as_double(0x7ff8000000000000LL);
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------
static int64_t gp_count(int64_t L, int64_t T, int64_t S) { return L < T ? 0 : (L - T) / S + 1; }

// msig_rn.h's shared checks of a recording call (running.hip's rn_rec_check); fills nc and brings S into the recording's range
static int gp_rec_check(const double* sig, int64_t L, int32_t C_all, const int32_t* cols, int32_t C, int64_t T, int64_t& S, bool other_null,
                        GpCols& nc) {
  if (!sig || !cols || other_null) return MSIG_E_NULL;
  if (L < 1 || T < 1 || S < 1 || C_all < 1 || C < 1 || C > MSIG_MAX_C) return MSIG_E_SHAPE;
  for (int c = 0; c < C; ++c)
    if (cols[c] < 0 || cols[c] >= C_all) return MSIG_E_SHAPE;
  for (int c = 0; c < MSIG_MAX_C; ++c) nc.col[c] = c < C ? cols[c] : 0;
  if (S > L) S = L;
  return 0;
}

static bool gp_mode_ok(const msig_gp_mode& md) {
  if (md.kind == MSIG_GP_EXPANDING) return true;
  if (md.kind == MSIG_GP_TRAILING) return md.K >= 1 && md.K <= MSIG_RN_MAX_K;
  return md.kind == MSIG_GP_DECAYED && md.decay >= 0.0 && md.decay <= 1.0;          // a NaN fails both comparisons
}

extern "C" int msig_gp_abi_version(void) { return MSIG_GP_ABI_VERSION; }
extern "C" int64_t msig_gp_struct_bytes(void) { return (int64_t)sizeof(msig_gp_mode); }
extern "C" int64_t msig_gp_state_bytes(int32_t K) {
  if (K < 0 || K > MSIG_RN_MAX_K) return MSIG_E_SHAPE;
  return ((int64_t)MSIG_GP_STATE_HEAD + (int64_t)K * GP_PART) * (int64_t)sizeof(double);
}

extern "C" int msig_gp_pivot(const double* sig, int64_t L, int32_t C_all, const int32_t* cols, int32_t C, uint32_t log1p_mask, int64_t T,
                             int64_t S, int64_t N, double* pivot, void* stream) {
  GpCols nc;
  int rc = gp_rec_check(sig, L, C_all, cols, C, T, S, !pivot, nc); if (rc) return rc;
  if (N < 1 || N > gp_count(L, T, S)) return MSIG_E_SHAPE;
  if (((uintptr_t)sig | (uintptr_t)pivot) & 7) return MSIG_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  { MSIG_K("gp_pivot", st); gp_pivot_kernel<<<1, 256, 0, st>>>(sig, C_all, nc, C, log1p_mask, T, S, N, pivot); }
  MSIG_LAUNCH_CHECK();
  return 0;
}

extern "C" int msig_gp_sums(const double* sig, int64_t L, int32_t C_all, const int32_t* cols, int32_t C, uint32_t log1p_mask, int64_t T,
                            int64_t S, const double* pivot, int64_t n0, int64_t B, double* sums, void* stream) {
  GpCols nc;
  int rc = gp_rec_check(sig, L, C_all, cols, C, T, S, !pivot || !sums, nc); if (rc) return rc;
  if (n0 < 0 || B < 1 || B > gp_count(L, T, S) || n0 > gp_count(L, T, S) - B) return MSIG_E_SHAPE;
  if (((uintptr_t)sig | (uintptr_t)pivot | (uintptr_t)sums) & 7) return MSIG_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  {
    MSIG_K("gp_sums", st);
    gp_sums_kernel<<<(unsigned)(B > 65536 ? 65536 : B), 256, 0, st>>>(sig, C_all, nc, C, log1p_mask, T, S, pivot, n0, B, sums);
  }
  MSIG_LAUNCH_CHECK();
  return 0;
}

extern "C" int msig_gp_stats(const double* sig, int64_t L, int32_t C_all, const int32_t* cols, int32_t C, uint32_t log1p_mask, int64_t T,
                             int64_t S, const double* pivot, const double* sums, int64_t N, const msig_gp_mode* mode, double* table,
                             double* coverage, void* stream) {
  GpCols nc;
  int rc = gp_rec_check(sig, L, C_all, cols, C, T, S, !pivot || !sums || !mode || !table || !coverage, nc); if (rc) return rc;
  if (N < 1 || N > gp_count(L, T, S) || !gp_mode_ok(*mode)) return MSIG_E_SHAPE;
  if (((uintptr_t)sig | (uintptr_t)pivot | (uintptr_t)sums | (uintptr_t)table | (uintptr_t)coverage) & 7) return MSIG_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = mode->kind != MSIG_GP_TRAILING ? 1u : (unsigned)(N > 65536 ? 65536 : N);
  { MSIG_K("gp_stats", st); gp_stats_kernel<<<grid, 64, 0, st>>>(pivot, C, (double)T, sums, N, mode->kind, mode->K, mode->decay, table, coverage); }
  MSIG_LAUNCH_CHECK();
  return 0;
}

static int gp_slots(const msig_multi* m, bool multi, int32_t B, int32_t C, int64_t T, GpSlots& sl) {
  sl = GpSlots{};
  sl.n = 1;
  if (!multi) return 0;
  FoldCtx fc; int rc = msig_multi_fold_ctx(m, fc); if (rc) return rc;
  if ((double)fc.stride < 4.0 * (double)B * (double)C * (double)T) return MSIG_E_SHAPE;       // a slot's batch would reach into the next arena
  sl.n = fc.n;
  for (int z = 0; z < fc.n; ++z) sl.off[z] = (int64_t)fc.slot[z] * fc.stride;
  return 0;
}

static int gp_windows(const double* sig, int64_t L, int32_t C_all, const int32_t* cols, int32_t C, uint32_t log1p_mask, int64_t T, int64_t S,
                      int64_t n0, int32_t B, const double* table, float* out_x, const msig_multi* m, bool multi, void* stream) {
  GpCols nc;
  int rc = gp_rec_check(sig, L, C_all, cols, C, T, S, !table || !out_x || (multi && !m), nc); if (rc) return rc;
  if (n0 < 0 || B < 1 || n0 + B > gp_count(L, T, S)) return MSIG_E_SHAPE;
  if ((((uintptr_t)sig | (uintptr_t)table) & 7) || ((uintptr_t)out_x & 15)) return MSIG_E_ALIGN;
  GpSlots sl;
  rc = gp_slots(m, multi, B, C, T, sl); if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t blocks = ((int64_t)B * T + 255) / 256;
  {
    MSIG_K("gp_windows", st);
    gp_windows_kernel<<<(unsigned)(blocks > 65536 ? 65536 : blocks), 256, 0, st>>>(sig, C_all, nc, C, log1p_mask, T, S, n0, (int64_t)B, table, out_x, sl);
  }
  MSIG_LAUNCH_CHECK();
  return 0;
}

extern "C" int msig_gp_windows(const double* sig, int64_t L, int32_t C_all, const int32_t* cols, int32_t C, uint32_t log1p_mask, int64_t T,
                               int64_t S, int64_t n0, int32_t B, const double* table, float* out_x, void* stream) {
  return gp_windows(sig, L, C_all, cols, C, log1p_mask, T, S, n0, B, table, out_x, nullptr, false, stream);
}

extern "C" int msig_gp_windows_multi(const double* sig, int64_t L, int32_t C_all, const int32_t* cols, int32_t C, uint32_t log1p_mask,
                                     int64_t T, int64_t S, int64_t n0, int32_t B, const double* table, float* out_x, const msig_multi* m,
                                     void* stream) {
  return gp_windows(sig, L, C_all, cols, C, log1p_mask, T, S, n0, B, table, out_x, m, true, stream);
}

// msig_lv.h's pool checks (live.hip's)
static int gp_pool_shape(int32_t sessions, int64_t R, int64_t ring_bytes, int32_t C_all) {
  if (sessions < 1 || sessions > MSIG_LV_MAX_SESSIONS || R < 1 || R > INT32_MAX || C_all < 1) return MSIG_E_SHAPE;
  if (ring_bytes < R * (int64_t)C_all * (int64_t)sizeof(double)) return MSIG_E_SHAPE;
  return 0;
}
static bool gp_pool_misaligned(const void* pool, int64_t ring_bytes) { return ((uintptr_t)pool & 7) || (ring_bytes & 7); }

// msig_lv_windows_multi's shape checks of the batch's rows; fills nc
static int gp_lv_rows_check(int32_t sessions, int64_t R, int32_t C_all, const int32_t* cols, int32_t C, int64_t T, int64_t S, const int32_t* sess,
                            const int64_t* win, const int64_t* written, int32_t B, GpCols& nc) {
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

extern "C" int msig_gp_lv_step(const double* pool, int32_t sessions, int64_t R, int64_t ring_bytes, int32_t C_all, const int32_t* cols, int32_t C,
                               uint32_t log1p_mask, int64_t T, int64_t S, const msig_gp_mode* mode, double* state, int64_t state_bytes,
                               const int32_t* sess, const int64_t* win, const int64_t* written, const int64_t* next, int32_t B, double* table,
                               double* coverage, void* stream) {
  if (!pool || !cols || !mode || !state || !sess || !win || !written || !next || !table || !coverage) return MSIG_E_NULL;
  int rc = gp_pool_shape(sessions, R, ring_bytes, C_all); if (rc) return rc;
  GpCols nc;
  rc = gp_lv_rows_check(sessions, R, C_all, cols, C, T, S, sess, win, written, B, nc); if (rc) return rc;
  if (!gp_mode_ok(*mode)) return MSIG_E_SHAPE;
  const int32_t K = mode->kind == MSIG_GP_TRAILING ? mode->K : 0;
  if (state_bytes < msig_gp_state_bytes(K)) return MSIG_E_SHAPE;
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
  if (gp_pool_misaligned(pool, ring_bytes) || (((uintptr_t)state | (uintptr_t)table | (uintptr_t)coverage) & 7) || (state_bytes & 7)) return MSIG_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  for (int b = 0; b < B;) {
    GpRuns runs{};
    int k = 0;
    for (; b < B && k < MSIG_LV_GROUP; ++k) {              // a run: the rows of one session
      int e = b + 1;
      while (e < B && sess[e] == sess[b]) ++e;
      runs.e[k] = GpRun{win[b], sess[b], e - b, b, 0};
      b = e;
    }
    {
      MSIG_K("gp_lv_step", st);
      gp_lv_step_kernel<<<(unsigned)k, 256, 0, st>>>(pool, ring_bytes / 8, R, C_all, nc, C, log1p_mask, T, S, mode->kind, K, mode->decay, state,
                                                     state_bytes / 8, table, coverage, runs);
    }
    MSIG_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int msig_gp_lv_windows_multi(const double* pool, int32_t sessions, int64_t R, int64_t ring_bytes, int32_t C_all, const int32_t* cols,
                                        int32_t C, uint32_t log1p_mask, int64_t T, int64_t S, const int32_t* sess, const int64_t* win,
                                        const int64_t* written, int32_t B, const double* table, float* out_x, const msig_multi* m, void* stream) {
  if (!pool || !cols || !sess || !win || !written || !table || !out_x || !m) return MSIG_E_NULL;
  int rc = gp_pool_shape(sessions, R, ring_bytes, C_all); if (rc) return rc;
  GpCols nc;
  rc = gp_lv_rows_check(sessions, R, C_all, cols, C, T, S, sess, win, written, B, nc); if (rc) return rc;
  if (gp_pool_misaligned(pool, ring_bytes) || ((uintptr_t)table & 7) || ((uintptr_t)out_x & 15)) return MSIG_E_ALIGN;
  GpSlots sl;
  rc = gp_slots(m, true, B, C, T, sl); if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  for (int b = 0; b < B;) {
    GpRuns runs{};
    int k = 0;
    int64_t most = 0;
    for (; b < B && k < MSIG_LV_GROUP; ++k) {              // a run: rows b .. that are consecutive windows of one session
      int e = b + 1;
      while (e < B && sess[e] == sess[b] && win[e] == win[e - 1] + 1) ++e;
      runs.e[k] = GpRun{win[b], sess[b], e - b, b, 0};
      if ((int64_t)(e - b) * T > most) most = (int64_t)(e - b) * T;
      b = e;
    }
    const int64_t blocks = (most + 255) / 256;
    {
      MSIG_K("gp_lv_windows", st);
      gp_lv_windows_kernel<<<dim3((unsigned)(blocks > 4096 ? 4096 : blocks), (unsigned)k), 256, 0, st>>>(pool, ring_bytes / 8, R, C_all, nc, C, log1p_mask,
                                                                                                     T, S, table, out_x, sl, runs);
    }
    MSIG_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int msig_gp_lv_skip(double* pool, int32_t sessions, int64_t R, int64_t ring_bytes, int32_t C_all, const int32_t* sess,
                               const int64_t* written, const int64_t* len, int32_t n, void* stream) {
  if (!pool || !sess || !written || !len) return MSIG_E_NULL;
  int rc = gp_pool_shape(sessions, R, ring_bytes, C_all); if (rc) return rc;
  if (n < 1 || n > sessions) return MSIG_E_SHAPE;
  uint64_t seen[MSIG_LV_MAX_SESSIONS / 64] = {};
  for (int j = 0; j < n; ++j) {
    if (sess[j] < 0 || sess[j] >= sessions || written[j] < 0 || len[j] < 0 || len[j] > R) return MSIG_E_SHAPE;
    uint64_t& word = seen[sess[j] >> 6];
    if (word >> (sess[j] & 63) & 1u) return MSIG_E_SHAPE;              // the same session twice
    word |= (uint64_t)1 << (sess[j] & 63);
  }
  if (gp_pool_misaligned(pool, ring_bytes)) return MSIG_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  for (int j0 = 0; j0 < n; j0 += MSIG_LV_GROUP) {
    GpSkips tab{};
    int k = 0;
    int64_t most = 0;
    for (int j = j0; j < n && j < j0 + MSIG_LV_GROUP; ++j)
      if (len[j] > 0) {
        tab.e[k++] = GpSkip{(int32_t)(written[j] % R), (int32_t)len[j], sess[j], 0};
        if (len[j] > most) most = len[j];
      }
    if (!k) continue;
    const int64_t blocks = (most * C_all + 255) / 256;
    { MSIG_K("gp_lv_skip", st); gp_lv_skip_kernel<<<dim3((unsigned)(blocks > 1024 ? 1024 : blocks), (unsigned)k), 256, 0, st>>>(pool, ring_bytes / 8, R, C_all, tab); }
    MSIG_LAUNCH_CHECK();
  }
  return 0;
}
