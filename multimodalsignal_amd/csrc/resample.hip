// Causal polyphase FIR resampling by L / M (include/msig_rs.h): the offline call over a whole recording and the
// live call that resamples raw-rate chunks straight into the msig_lv.h rings.  One device function, rs_output (rs_dev.h), forms an output
// sample for both: the taps in ascending raw row j, acc = fma(h, x, acc) in float64 — the two calls differ only in where x[j] comes
// from (the recording; or the chunk in the staging buffer and, for rows older than the chunk, the session's tail ring), so their bits
// are the same.  Both kernels are streaming kernels in live.hip's shape: a thread owns one output value, consecutive lanes are the
// C_all columns of one output and then the next output, so the loads of one raw row and the store of one ring row are contiguous, and
// the lanes of one output read the same tap (one broadcast load).  A raw row is read by about 2 * half / M outputs (20 at 10 zero
// crossings a side); those re-reads are served by the caches, nothing is staged in LDS: the tile of raw rows an output tile needs is
// tile * M / L + 2 * half / L rows, which has no bound that holds over the ratios the header admits.  The per-session table travels as
// kernel arguments, MSIG_LV_GROUP entries a launch: nothing is uploaded, allocated or kept.
#include "rs_dev.h"

struct RsChunk { int64_t src0, w; int32_t len, session; };      // staging row of the chunk's first row; raw rows the session had before it
struct RsChunks { RsChunk e[MSIG_LV_GROUP]; };
static_assert(sizeof(RsChunks) + 128 <= 4096, "the table is a kernel argument");

__global__ __launch_bounds__(256) void rs_resample_kernel(const double* __restrict__ x, int C_all, const double* __restrict__ h, RsRatio r,
                                                          double* __restrict__ y, int64_t n_out) {
  const int64_t total = n_out * C_all;
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < total; k += (int64_t)gridDim.x * 256) {
    const int64_t m = k / C_all;
    const double* col = x + (k - m * C_all);
    y[k] = rs_output(m, r, h, [&](int64_t j) { return col[j * C_all]; });
  }
}

// chunk blockIdx.y: outputs [count(w), count(w + len)) of its session into ring rows m % R.  Raw row j >= w is row j - w of the chunk
// (NaN where there is no staging buffer), an older one row j % tail_rows of the session's tail.
__global__ __launch_bounds__(256) void rs_lv_push_kernel(double* __restrict__ pool, int64_t ring_doubles, int64_t R, int C_all,
                                                         const double* __restrict__ tails, int64_t tail_rows, int64_t tail_doubles,
                                                         const double* __restrict__ h, RsRatio r, const double* __restrict__ staging, RsChunks tab) {
  const RsChunk e = tab.e[blockIdx.y];
  const int64_t m0 = rs_count(e.w, r), total = (rs_count(e.w + e.len, r) - m0) * C_all;
  double* __restrict__ ring = pool + (int64_t)e.session * ring_doubles;
  const double* __restrict__ tail = tails + (int64_t)e.session * tail_doubles;
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < total; k += (int64_t)gridDim.x * 256) {
    const int64_t q = k / C_all, m = m0 + q;
    const int c = (int)(k - q * C_all);
    ring[(m % R) * C_all + c] = rs_output(m, r, h, [&](int64_t j) {
      if (j >= e.w) return staging ? staging[(e.src0 + (j - e.w)) * C_all + c] : __longlong_as_double(0x7ff8000000000000LL);
      return tail[(j % tail_rows) * C_all + c];
    });
  }
}

// chunk blockIdx.y: its last min(len, tail_rows) raw rows into the session's tail, raw row j into tail row j % tail_rows — launched
// after rs_lv_push_kernel on the same stream, which has read the rows these replace
__global__ __launch_bounds__(256) void rs_lv_tail_kernel(double* __restrict__ tails, int64_t tail_rows, int64_t tail_doubles, int C_all,
                                                         const double* __restrict__ staging, RsChunks tab) {
  const RsChunk e = tab.e[blockIdx.y];
  const int64_t keep = e.len < tail_rows ? e.len : tail_rows, first = e.w + e.len - keep, total = keep * C_all;
  double* __restrict__ tail = tails + (int64_t)e.session * tail_doubles;
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < total; k += (int64_t)gridDim.x * 256) {
    const int64_t q = k / C_all, j = first + q;
    const int c = (int)(k - q * C_all);
    tail[(j % tail_rows) * C_all + c] = staging ? staging[(e.src0 + (j - e.w)) * C_all + c] : __longlong_as_double(0x7ff8000000000000LL);
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------
extern "C" int msig_rs_abi_version(void) { return MSIG_RS_ABI_VERSION; }

extern "C" int64_t msig_rs_out_count(int64_t n_in, int32_t L, int32_t M, int32_t half) {
  if (n_in < 0 || n_in > MSIG_RS_MAX_ROWS || rs_ratio_check(L, M, half)) return MSIG_E_SHAPE;
  return rs_count(n_in, RsRatio{L, M, half});
}

extern "C" int msig_rs_resample(const double* x, int64_t n_in, int32_t C_all, const double* h, int32_t L, int32_t M, int32_t half, double* y,
                                int64_t n_out, void* stream) {
  if (!h || (n_in > 0 && !x) || (n_out > 0 && !y)) return MSIG_E_NULL;
  int rc = rs_ratio_check(L, M, half); if (rc) return rc;
  if (C_all < 1 || n_in < 0 || n_in > MSIG_RS_MAX_ROWS) return MSIG_E_SHAPE;
  const RsRatio r{L, M, half};
  if (n_out != rs_count(n_in, r)) return MSIG_E_SHAPE;
  if (((uintptr_t)h & 7) || ((uintptr_t)x & 7) || ((uintptr_t)y & 7)) return MSIG_E_ALIGN;
  if (n_out == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int64_t blocks = (n_out * C_all + 255) / 256;
  {
    MSIG_K("rs_resample", st);
    rs_resample_kernel<<<dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), 256, 0, st>>>(x, C_all, h, r, y, n_out);
  }
  MSIG_LAUNCH_CHECK();
  return 0;
}

extern "C" int msig_rs_lv_push(double* pool, int32_t sessions, int64_t R, int64_t ring_bytes, int32_t C_all, double* tails, int64_t tail_rows,
                               int64_t tail_bytes, const double* h, int32_t L, int32_t M, int32_t half, const int32_t* sess,
                               const int64_t* raw_written, const int64_t* len, int32_t n, const double* staging, void* stream) {
  if (!pool || !tails || !h || !sess || !raw_written || !len) return MSIG_E_NULL;
  if (sessions < 1 || sessions > MSIG_LV_MAX_SESSIONS || R < 1 || R > INT32_MAX || C_all < 1) return MSIG_E_SHAPE;      // msig_lv_push's pool checks
  if (ring_bytes < R * (int64_t)C_all * (int64_t)sizeof(double)) return MSIG_E_SHAPE;
  int rc = rs_ratio_check(L, M, half); if (rc) return rc;
  if (tail_rows < (2 * (int64_t)half) / L + 1 || tail_rows > INT32_MAX) return MSIG_E_SHAPE;
  if (tail_bytes < tail_rows * (int64_t)C_all * (int64_t)sizeof(double)) return MSIG_E_SHAPE;
  if (n < 1 || n > sessions) return MSIG_E_SHAPE;
  const RsRatio r{L, M, half};
  uint64_t seen[MSIG_LV_MAX_SESSIONS / 64] = {};
  for (int j = 0; j < n; ++j) {
    if (sess[j] < 0 || sess[j] >= sessions || raw_written[j] < 0 || len[j] < 0 || len[j] > INT32_MAX) return MSIG_E_SHAPE;
    if (raw_written[j] > MSIG_RS_MAX_ROWS - len[j]) return MSIG_E_SHAPE;
    if (rs_count(raw_written[j] + len[j], r) - rs_count(raw_written[j], r) > R) return MSIG_E_SHAPE;      // an output would overwrite one of its own chunk
    uint64_t& word = seen[sess[j] >> 6];
    if (word >> (sess[j] & 63) & 1u) return MSIG_E_SHAPE;              // the same session twice
    word |= (uint64_t)1 << (sess[j] & 63);
  }
  if (((uintptr_t)pool & 7) || (ring_bytes & 7) || ((uintptr_t)tails & 7) || (tail_bytes & 7) || ((uintptr_t)h & 7) || ((uintptr_t)staging & 7))
    return MSIG_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  int64_t src0 = 0;
  for (int j0 = 0; j0 < n; j0 += MSIG_LV_GROUP) {
    RsChunks tab{};
    int k = 0;
    int64_t most_out = 0, most_keep = 0;
    for (int j = j0; j < n && j < j0 + MSIG_LV_GROUP; ++j) {
      if (len[j] > 0) {
        tab.e[k++] = RsChunk{src0, raw_written[j], (int32_t)len[j], sess[j]};
        const int64_t outs = rs_count(raw_written[j] + len[j], r) - rs_count(raw_written[j], r);
        const int64_t keep = len[j] < tail_rows ? len[j] : tail_rows;
        if (outs > most_out) most_out = outs;
        if (keep > most_keep) most_keep = keep;
      }
      src0 += len[j];
    }
    if (!k) continue;
    if (most_out > 0) {
      const int64_t blocks = (most_out * C_all + 255) / 256;
      {
        MSIG_K("rs_lv_push", st);
        rs_lv_push_kernel<<<dim3((unsigned)(blocks > 1024 ? 1024 : blocks), (unsigned)k), 256, 0, st>>>(pool, ring_bytes / 8, R, C_all, tails, tail_rows,
                                                                                                    tail_bytes / 8, h, r, staging, tab);
      }
      MSIG_LAUNCH_CHECK();
    }
    const int64_t blocks = (most_keep * C_all + 255) / 256;
    {
      MSIG_K("rs_lv_tail", st);
      rs_lv_tail_kernel<<<dim3((unsigned)(blocks > 1024 ? 1024 : blocks), (unsigned)k), 256, 0, st>>>(tails, tail_rows, tail_bytes / 8, C_all, staging, tab);
    }
    MSIG_LAUNCH_CHECK();
  }
  return 0;
}
