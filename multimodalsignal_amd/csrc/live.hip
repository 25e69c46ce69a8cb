// Live monitoring of many wearers (include/msig_lv.h): a pool of sample rings, one per session, an append of
// chunks to many rings in one launch, and window batches whose rows come from different sessions.  Both kernels are streaming
// kernels in record.hip's shape.  lv_push_kernel: a thread owns one float64 of a chunk, consecutive lanes consecutive doubles of
// the staging buffer and of the ring (the ring's end excepted).  lv_windows_kernel is rec_windows_kernel with the sample's row taken
// modulo R from the session's ring and the statistics from the session's record: a thread owns a SAMPLE of a run of consecutive
// windows of one session, reads and normalises it once and serves every window of the run that covers it, in every arena slot —
// consecutive lanes are consecutive t of one channel of one window on the store side.  The per-session and per-run tables travel as
// kernel arguments, MSIG_LV_GROUP entries a launch: nothing is uploaded, allocated or kept.
#include "msig_dev.h"
#include "../../include/msig_lv.h"

int msig_multi_fold_ctx(const msig_multi* m, FoldCtx& fc);                                  // api.hip: msig_multi's own checks

struct LvCols { int col[MSIG_MAX_C]; };
struct LvSlots { int n; int64_t off[MSIG_MAX_FOLDS]; };        // byte offset of every slot's batch from out_x
struct LvChunk { int64_t src0; int32_t start, len, session, pad; };      // staging row of the chunk's first row; ring row it goes to
struct LvChunks { LvChunk e[MSIG_LV_GROUP]; };
struct LvRun { int64_t n0; int32_t session, count, b0, pad; };           // windows n0 .. n0 + count - 1 are rows b0 .. of the batch
struct LvRuns { LvRun e[MSIG_LV_GROUP]; };
static_assert(sizeof(LvChunks) + 64 <= 4096 && sizeof(LvRuns) + sizeof(LvSlots) + sizeof(LvCols) + 128 <= 4096, "the tables are kernel arguments");

// chunk blockIdx.y: its len * C_all doubles into the ring, from ring row `start` on, wrapped once at most (len <= R, start < R)
__global__ __launch_bounds__(256) void lv_push_kernel(double* __restrict__ pool, int64_t ring_doubles, int64_t R, int C_all,
                                                      const double* __restrict__ staging, LvChunks tab) {
  const LvChunk e = tab.e[blockIdx.y];
  const int64_t total = (int64_t)e.len * C_all, wrap = R * C_all, d0 = (int64_t)e.start * C_all;
  double* __restrict__ ring = pool + (int64_t)e.session * ring_doubles;
  const double* __restrict__ src = staging + e.src0 * C_all;
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < total; k += (int64_t)gridDim.x * 256) {
    int64_t d = d0 + k;
    if (d >= wrap) d -= wrap;
    ring[d] = src[k];
  }
}

// The windows n in [a, b) that cover sample i, n * S <= i < n * S + T, as the inclusive range lo..hi (record.hip's rec_cover).
__device__ __forceinline__ void lv_cover(int64_t i, int64_t T, int64_t S, int64_t a, int64_t b, int64_t& lo, int64_t& hi) {
  const int64_t k = i - T + 1;
  lo = k <= 0 ? 0 : (k + S - 1) / S;
  hi = i / S;
  if (lo < a) lo = a;
  if (hi > b - 1) hi = b - 1;
}

// run blockIdx.y: samples [n0 * S, (n0 + count - 1) * S + T) of its session
__global__ __launch_bounds__(256) void lv_windows_kernel(const double* __restrict__ pool, int64_t ring_doubles, int64_t R, int C_all, LvCols cols,
                                                         int C, uint32_t log1p_mask, int64_t T, int64_t S, const double* __restrict__ stats_all,
                                                         float* __restrict__ out, LvSlots slots, LvRuns runs) {
  const LvRun r = runs.e[blockIdx.y];
  const double* __restrict__ ring = pool + (int64_t)r.session * ring_doubles;
  const double* __restrict__ stats = stats_all + (int64_t)r.session * MSIG_LV_STATS_DOUBLES;
  const int64_t i0 = r.n0 * S, i1 = (r.n0 + r.count - 1) * S + T;
  for (int64_t i = i0 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < i1; i += (int64_t)gridDim.x * 256) {
    int64_t lo, hi;
    lv_cover(i, T, S, r.n0, r.n0 + r.count, lo, hi);
    if (lo > hi) continue;                                  // S > T: between two windows
    const double* row = ring + (i % R) * C_all;
    float val[MSIG_MAX_C];
#pragma unroll
    for (int c = 0; c < MSIG_MAX_C; ++c) {
      val[c] = 0.f;
      if (c < C) {
        double v = row[cols.col[c]];
        if ((log1p_mask >> c) & 1u) v = log1p(v);
        val[c] = (float)((v - stats[c]) * stats[MSIG_MAX_C + c]);       // rec_windows_kernel's statement: the same bits
      }
    }
    for (int64_t n = lo; n <= hi; ++n) {
      const size_t at = (size_t)(r.b0 + (n - r.n0)) * C * T + (size_t)(i - n * S);      // [b][0][t]
#pragma unroll
      for (int c = 0; c < MSIG_MAX_C; ++c)
        if (c < C)
          for (int z = 0; z < slots.n; ++z)
            *(float*)((char*)out + slots.off[z] + (at + (size_t)c * T) * sizeof(float)) = val[c];
    }
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------
// the pool's own shape checks; its alignment is checked by lv_pool_align after the call's other shape checks
static int lv_pool_shape(int32_t sessions, int64_t R, int64_t ring_bytes, int32_t C_all) {
  if (sessions < 1 || sessions > MSIG_LV_MAX_SESSIONS || R < 1 || R > INT32_MAX || C_all < 1) return MSIG_E_SHAPE;
  if (ring_bytes < R * (int64_t)C_all * (int64_t)sizeof(double)) return MSIG_E_SHAPE;
  return 0;
}
static bool lv_pool_misaligned(const void* pool, int64_t ring_bytes) { return ((uintptr_t)pool & 7) || (ring_bytes & 7); }

extern "C" int msig_lv_abi_version(void) { return MSIG_LV_ABI_VERSION; }

extern "C" int msig_lv_push(double* pool, int32_t sessions, int64_t R, int64_t ring_bytes, int32_t C_all, const int32_t* sess,
                            const int64_t* written, const int64_t* len, int32_t n, const double* staging, void* stream) {
  if (!pool || !sess || !written || !len || !staging) return MSIG_E_NULL;
  int rc = lv_pool_shape(sessions, R, ring_bytes, C_all); if (rc) return rc;
  if (n < 1 || n > sessions) return MSIG_E_SHAPE;
  uint64_t seen[MSIG_LV_MAX_SESSIONS / 64] = {};
  for (int j = 0; j < n; ++j) {
    if (sess[j] < 0 || sess[j] >= sessions || written[j] < 0 || len[j] < 0 || len[j] > R) return MSIG_E_SHAPE;
    uint64_t& word = seen[sess[j] >> 6];
    if (word >> (sess[j] & 63) & 1u) return MSIG_E_SHAPE;              // the same session twice
    word |= (uint64_t)1 << (sess[j] & 63);
  }
  if (lv_pool_misaligned(pool, ring_bytes) || ((uintptr_t)staging & 7)) return MSIG_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  int64_t src0 = 0;
  for (int j0 = 0; j0 < n; j0 += MSIG_LV_GROUP) {
    LvChunks tab{};
    int k = 0;
    int64_t most = 0;
    for (int j = j0; j < n && j < j0 + MSIG_LV_GROUP; ++j) {
      if (len[j] > 0) {
        tab.e[k++] = LvChunk{src0, (int32_t)(written[j] % R), (int32_t)len[j], sess[j], 0};
        if (len[j] > most) most = len[j];
      }
      src0 += len[j];
    }
    if (!k) continue;
    const int64_t blocks = (most * C_all + 255) / 256;
    {
      MSIG_K("lv_push", st);
      lv_push_kernel<<<dim3((unsigned)(blocks > 1024 ? 1024 : blocks), (unsigned)k), 256, 0, st>>>(pool, ring_bytes / 8, R, C_all, staging, tab);
    }
    MSIG_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int msig_lv_windows_multi(const double* pool, int32_t sessions, int64_t R, int64_t ring_bytes, int32_t C_all, const int32_t* cols,
                                     int32_t C, uint32_t log1p_mask, int64_t T, int64_t S, const int32_t* sess, const int64_t* win,
                                     const int64_t* written, int32_t B, const double* stats, float* out_x, const msig_multi* m, void* stream) {
  if (!pool || !cols || !sess || !win || !written || !stats || !out_x || !m) return MSIG_E_NULL;
  int rc = lv_pool_shape(sessions, R, ring_bytes, C_all); if (rc) return rc;
  if (T < 1 || S < 1 || C < 1 || C > MSIG_MAX_C || B < 1) return MSIG_E_SHAPE;
  LvCols nc;
  for (int c = 0; c < C; ++c)
    if (cols[c] < 0 || cols[c] >= C_all) return MSIG_E_SHAPE;
  for (int c = 0; c < MSIG_MAX_C; ++c) nc.col[c] = c < C ? cols[c] : 0;
  for (int b = 0; b < B; ++b) {
    if (sess[b] < 0 || sess[b] >= sessions || win[b] < 0) return MSIG_E_SHAPE;
    if (written[b] < T || win[b] > (written[b] - T) / S) return MSIG_E_SHAPE;       // not yet complete: win * S + T > written
    if (win[b] * S < written[b] - R) return MSIG_E_SHAPE;                           // its first samples are already overwritten
  }
  if (lv_pool_misaligned(pool, ring_bytes) || ((uintptr_t)stats & 7) || ((uintptr_t)out_x & 15)) return MSIG_E_ALIGN;
  FoldCtx fc; rc = msig_multi_fold_ctx(m, fc); if (rc) return rc;
  if ((double)fc.stride < 4.0 * (double)B * (double)C * (double)T) return MSIG_E_SHAPE;       // a slot's batch would reach into the next arena
  LvSlots sl{};
  sl.n = fc.n;
  for (int z = 0; z < fc.n; ++z) sl.off[z] = (int64_t)fc.slot[z] * fc.stride;
  hipStream_t st = (hipStream_t)stream;
  for (int b = 0; b < B;) {
    LvRuns runs{};
    int k = 0;
    int64_t most = 0;
    for (; b < B && k < MSIG_LV_GROUP; ++k) {              // a run: rows b .. that are consecutive windows of one session
      int e = b + 1;
      while (e < B && sess[e] == sess[b] && win[e] == win[e - 1] + 1) ++e;
      runs.e[k] = LvRun{win[b], sess[b], e - b, b, 0};
      const int64_t span = (int64_t)(e - b - 1) * S + T;
      if (span > most) most = span;
      b = e;
    }
    const int64_t blocks = (most + 255) / 256;
    {
      MSIG_K("lv_windows", st);
      lv_windows_kernel<<<dim3((unsigned)(blocks > 4096 ? 4096 : blocks), (unsigned)k), 256, 0, st>>>(pool, ring_bytes / 8, R, C_all, nc, C, log1p_mask,
                                                                                                  T, S, stats, out_x, sl, runs);
    }
    MSIG_LAUNCH_CHECK();
  }
  return 0;
}
