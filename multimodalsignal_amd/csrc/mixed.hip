// Mixed-rate streams (include/msig_mx.h): a sample rate per column group, offline and in front of the
// msig_lv.h rings.  Every output is formed by rs_output (rs_dev.h), the device function of resample.hip, so a column's bits are those
// of the single-rate calls; an identity group (L == M == 1) is copied.  The kernels keep resample.hip's shape: a thread owns one
// output value, consecutive lanes are the GROUP's columns of one output and then the next output, so the loads of a raw row are
// contiguous and the lanes of one output read the same tap; the store of an output row is a block of ncols doubles at a stride of
// C_all — strided where the group is narrower than the ring row, which is what a column group costs.  A chunk is a (session, group)
// pair; the chunk table and the group table travel as kernel arguments, MSIG_MX_CHUNKS chunks a launch: nothing is uploaded,
// allocated or kept.
#include "rs_dev.h"
#include "../../include/msig_mx.h"

struct MxChunk { int64_t src0, w; int32_t len, session, group, pad; };      // doubles into staging; raw rows the group had before the chunk
struct MxChunks { MxChunk e[MSIG_MX_CHUNKS]; };
struct MxGroups { msig_mx_group g[MSIG_MX_MAX_GROUPS]; };
static_assert(sizeof(msig_mx_group) == 48 && sizeof(MxChunk) == 32, "the layouts of msig_mx.h and of the chunk table");
static_assert(sizeof(MxChunks) + sizeof(MxGroups) + 128 <= 4096, "both tables are kernel arguments");

#define MX_NAN __longlong_as_double(0x7ff8000000000000LL)

__device__ __forceinline__ bool mx_identity(const msig_mx_group& g) { return g.L == 1 && g.M == 1; }

// one group of a recording: x (n_in, ncols) -> columns [col0, col0 + ncols) of y's first n_out rows
__global__ __launch_bounds__(256) void mx_resample_kernel(const double* __restrict__ x, const double* __restrict__ h, msig_mx_group g,
                                                          double* __restrict__ y, int64_t n_out, int C_all) {
  const RsRatio r{g.L, g.M, g.half};
  const int nc = g.ncols;
  const int64_t total = n_out * nc;
  const bool same = mx_identity(g);
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < total; k += (int64_t)gridDim.x * 256) {
    const int64_t m = k / nc;
    const int c = (int)(k - m * nc);
    const double* col = x + c;
    y[m * C_all + g.col0 + c] = same ? x[k] : rs_output(m, r, h + g.h_off, [&](int64_t j) { return col[j * nc]; });
  }
}

// chunk blockIdx.y: outputs [count(w), count(w + len)) of its group into its columns of ring rows m % R.  Raw row j >= w is row
// j - w of the chunk (NaN where there is no staging buffer), an older one row j % tail_rows of the group's tail in the session's block.
__global__ __launch_bounds__(256) void mx_lv_push_kernel(double* __restrict__ pool, int64_t ring_doubles, int64_t R, int C_all,
                                                         const double* __restrict__ tails, int64_t tail_doubles, const double* __restrict__ h,
                                                         const double* __restrict__ staging, MxGroups groups, MxChunks tab) {
  const MxChunk e = tab.e[blockIdx.y];
  const msig_mx_group g = groups.g[e.group];
  const RsRatio r{g.L, g.M, g.half};
  const int nc = g.ncols;
  const bool same = mx_identity(g);
  const int64_t m0 = rs_count(e.w, r), total = (rs_count(e.w + e.len, r) - m0) * nc;
  double* __restrict__ ring = pool + (int64_t)e.session * ring_doubles + g.col0;
  const double* __restrict__ tail = tails + (int64_t)e.session * tail_doubles + g.tail_off;
  const double* __restrict__ taps = h + g.h_off;
  const int64_t tail_rows = g.tail_rows;
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < total; k += (int64_t)gridDim.x * 256) {
    const int64_t q = k / nc, m = m0 + q;
    const int c = (int)(k - q * nc);
    double v;
    if (same) {
      v = staging ? staging[e.src0 + k] : MX_NAN;          // output m is raw row m = w + q: value k of the chunk
    } else {
      v = rs_output(m, r, taps, [&](int64_t j) {
        if (j >= e.w) return staging ? staging[e.src0 + (j - e.w) * nc + c] : MX_NAN;
#ifdef MSIG_NEGCTL_MIXED
        return tail[((j + 1) % tail_rows) * nc + c];        // negative control: the neighbouring tail row, in bounds by construction
#else
        return tail[(j % tail_rows) * nc + c];
#endif
      });
    }
    ring[(m % R) * C_all + c] = v;
  }
}

// chunk blockIdx.y: its last min(len, tail_rows) raw rows into the group's tail, raw row j into tail row j % tail_rows — launched
// after mx_lv_push_kernel on the same stream, which has read the rows these replace.  An identity group keeps no tail.
__global__ __launch_bounds__(256) void mx_lv_tail_kernel(double* __restrict__ tails, int64_t tail_doubles, const double* __restrict__ staging,
                                                         MxGroups groups, MxChunks tab) {
  const MxChunk e = tab.e[blockIdx.y];
  const msig_mx_group g = groups.g[e.group];
  const int nc = g.ncols;
  const int64_t tail_rows = g.tail_rows;
  const int64_t keep = e.len < tail_rows ? e.len : tail_rows, first = e.w + e.len - keep, total = keep * nc;
  double* __restrict__ tail = tails + (int64_t)e.session * tail_doubles + g.tail_off;
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < total; k += (int64_t)gridDim.x * 256) {
    const int64_t q = k / nc, j = first + q;
    const int c = (int)(k - q * nc);
    tail[(j % tail_rows) * nc + c] = staging ? staging[e.src0 + (j - e.w) * nc + c] : MX_NAN;
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------
static bool mx_same(const msig_mx_group& g) { return g.L == 1 && g.M == 1; }

// the checks of one group that both calls make
static int mx_group_check(const msig_mx_group& g, int32_t C_all) {
  if (mx_same(g)) {
    if (g.half != 0 || g.tail_rows != 0) return MSIG_E_SHAPE;
  } else {
    int rc = rs_ratio_check(g.L, g.M, g.half); if (rc) return rc;
    if (g.h_off < 0) return MSIG_E_SHAPE;
  }
  if (g.ncols < 1 || g.col0 < 0 || (int64_t)g.col0 + g.ncols > C_all) return MSIG_E_SHAPE;
  return 0;
}

extern "C" int msig_mx_abi_version(void) { return MSIG_MX_ABI_VERSION; }
extern "C" int64_t msig_mx_struct_bytes(void) { return (int64_t)sizeof(msig_mx_group); }

extern "C" int msig_mx_resample(const double* x, int64_t n_in, const double* h, const msig_mx_group* g, double* y, int64_t n_out, int32_t C_all,
                                void* stream) {
  if (!g || (n_in > 0 && !x) || (n_out > 0 && !y)) return MSIG_E_NULL;
  if (!mx_same(*g) && !h) return MSIG_E_NULL;
  if (C_all < 1) return MSIG_E_SHAPE;
  int rc = mx_group_check(*g, C_all); if (rc) return rc;
  if (n_in < 0 || n_in > MSIG_RS_MAX_ROWS) return MSIG_E_SHAPE;
  if (n_out < 0 || n_out > rs_count(n_in, RsRatio{g->L, g->M, g->half})) return MSIG_E_SHAPE;
  if (((uintptr_t)h & 7) || ((uintptr_t)x & 7) || ((uintptr_t)y & 7)) return MSIG_E_ALIGN;
  if (n_out == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int64_t blocks = (n_out * g->ncols + 255) / 256;
  {
    MSIG_K("mx_resample", st);
    mx_resample_kernel<<<dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), 256, 0, st>>>(x, h, *g, y, n_out, C_all);
  }
  MSIG_LAUNCH_CHECK();
  return 0;
}

extern "C" int msig_mx_lv_push(double* pool, int32_t sessions, int64_t R, int64_t ring_bytes, int32_t C_all, double* tails, int64_t tail_bytes,
                               const double* h, const msig_mx_group* groups, int32_t G, const int32_t* sess, const int32_t* group,
                               const int64_t* raw_written, const int64_t* len, int32_t n, const double* staging, void* stream) {
  if (!pool || !tails || !groups || !sess || !group || !raw_written || !len) return MSIG_E_NULL;
  if (sessions < 1 || sessions > MSIG_LV_MAX_SESSIONS || R < 1 || R > INT32_MAX || C_all < 1) return MSIG_E_SHAPE;      // msig_lv_push's pool checks
  if (ring_bytes < R * (int64_t)C_all * (int64_t)sizeof(double)) return MSIG_E_SHAPE;
  if (G < 1 || G > MSIG_MX_MAX_GROUPS) return MSIG_E_SHAPE;
  if (tail_bytes < 0) return MSIG_E_SHAPE;
  MxGroups gt{};
  for (int a = 0; a < G; ++a) {
    const msig_mx_group& g = groups[a];
    int rc = mx_group_check(g, C_all); if (rc) return rc;
    if (!mx_same(g)) {
      if (!h) return MSIG_E_NULL;
      if (g.tail_rows < (2 * (int64_t)g.half) / g.L + 1 || g.tail_rows > INT32_MAX || g.tail_off < 0) return MSIG_E_SHAPE;
      if (g.tail_off > tail_bytes / 8 || g.tail_rows * g.ncols > tail_bytes / 8 - g.tail_off) return MSIG_E_SHAPE;      // the tail ends beyond the block
    }
    for (int b = 0; b < a; ++b) {
      const msig_mx_group& o = groups[b];
      if (g.col0 < o.col0 + o.ncols && o.col0 < g.col0 + g.ncols) return MSIG_E_SHAPE;                               // columns owned twice
      if (!mx_same(g) && !mx_same(o) && g.tail_off < o.tail_off + o.tail_rows * o.ncols && o.tail_off < g.tail_off + g.tail_rows * g.ncols)
        return MSIG_E_SHAPE;                                                                                          // tail rows owned twice
    }
    gt.g[a] = g;
  }
  if (n < 1 || (int64_t)n > (int64_t)sessions * G) return MSIG_E_SHAPE;
  uint64_t seen[MSIG_LV_MAX_SESSIONS * MSIG_MX_MAX_GROUPS / 64] = {};
  for (int j = 0; j < n; ++j) {
    if (sess[j] < 0 || sess[j] >= sessions || group[j] < 0 || group[j] >= G) return MSIG_E_SHAPE;
    if (raw_written[j] < 0 || len[j] < 0 || len[j] > INT32_MAX) return MSIG_E_SHAPE;
    if (raw_written[j] > MSIG_RS_MAX_ROWS - len[j]) return MSIG_E_SHAPE;
    const msig_mx_group& g = groups[group[j]];
    const RsRatio r{g.L, g.M, g.half};
    if (rs_count(raw_written[j] + len[j], r) - rs_count(raw_written[j], r) > R) return MSIG_E_SHAPE;      // an output would overwrite one of its own chunk
    const int bit = sess[j] * MSIG_MX_MAX_GROUPS + group[j];
    uint64_t& word = seen[bit >> 6];
    if (word >> (bit & 63) & 1u) return MSIG_E_SHAPE;                  // the same (session, group) twice
    word |= (uint64_t)1 << (bit & 63);
  }
  if (((uintptr_t)pool & 7) || (ring_bytes & 7) || ((uintptr_t)tails & 7) || (tail_bytes & 7) || ((uintptr_t)h & 7) || ((uintptr_t)staging & 7))
    return MSIG_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  int64_t src0 = 0;
  for (int j0 = 0; j0 < n; j0 += MSIG_MX_CHUNKS) {
    MxChunks tab{};
    int k = 0;
    int64_t most_out = 0, most_keep = 0;          // in values: outputs or kept rows times the group's columns
    for (int j = j0; j < n && j < j0 + MSIG_MX_CHUNKS; ++j) {
      const msig_mx_group& g = groups[group[j]];
      if (len[j] > 0) {
        const RsRatio r{g.L, g.M, g.half};
        tab.e[k++] = MxChunk{src0, raw_written[j], (int32_t)len[j], sess[j], group[j], 0};
        const int64_t outs = (rs_count(raw_written[j] + len[j], r) - rs_count(raw_written[j], r)) * g.ncols;
        const int64_t keep = (len[j] < g.tail_rows ? len[j] : g.tail_rows) * g.ncols;
        if (outs > most_out) most_out = outs;
        if (keep > most_keep) most_keep = keep;
      }
      src0 += len[j] * g.ncols;
    }
    if (!k) continue;
    if (most_out > 0) {
      const int64_t blocks = (most_out + 255) / 256;
      {
        MSIG_K("mx_lv_push", st);
        mx_lv_push_kernel<<<dim3((unsigned)(blocks > 1024 ? 1024 : blocks), (unsigned)k), 256, 0, st>>>(pool, ring_bytes / 8, R, C_all, tails,
                                                                                                    tail_bytes / 8, h, staging, gt, tab);
      }
      MSIG_LAUNCH_CHECK();
    }
    if (most_keep > 0) {
      const int64_t blocks = (most_keep + 255) / 256;
      {
        MSIG_K("mx_lv_tail", st);
        mx_lv_tail_kernel<<<dim3((unsigned)(blocks > 1024 ? 1024 : blocks), (unsigned)k), 256, 0, st>>>(tails, tail_bytes / 8, staging, gt, tab);
      }
      MSIG_LAUNCH_CHECK();
    }
  }
  return 0;
}
