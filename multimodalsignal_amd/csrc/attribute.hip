// include/msig_at.h: the two memory-bound ends of integrated gradients — the path points between a baseline
// and a window, and the weighted sum of the path batch's input gradients with its per-bin, per-channel and per-window sums.  The
// model between them is msig.h's eval-mode forward kept for a backward and its backward with msig_batch.dx; nothing of it is here.
#include "msig_dev.h"
#include "../../include/msig_at.h"

#define AT_THREADS 256
#define AT_TILE 1024        // elements of a row (reduce) or of a window (path) per workgroup pass: 256 threads x 4
#define AT_PIECE 16         // fp32 values one thread adds up in a row before the partial sums of a bin are combined

__device__ __forceinline__ float at_base(const float* __restrict__ base, int kind, int64_t own, int c, int64_t i) {
  // own: offset of the window in an (N, C, T) baseline; i: offset of the element in the window
  if (kind == MSIG_AT_BASE_ZERO) return 0.0f;
  if (kind == MSIG_AT_BASE_CHANNEL) return base[c];
  if (kind == MSIG_AT_BASE_SHARED) return base[i];
  return base[own + i];
}
__device__ __forceinline__ float4 at_base4(const float* __restrict__ base, int kind, int64_t own, int c, int64_t i) {
  if (kind == MSIG_AT_BASE_ZERO) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (kind == MSIG_AT_BASE_CHANNEL) { const float s = base[c]; return make_float4(s, s, s, s); }
  if (kind == MSIG_AT_BASE_SHARED) return *(const float4*)(base + i);
  return *(const float4*)(base + own + i);
}

// ------------------------------------------------------------------------------------
// xp[n * P + p] = fmaf(coef[p][c], x[n] - x0, x0), and x[n] itself where coef is exactly 1 (x0 + (x - x0) rounds).  Workgroup (n, tile): AT_TILE consecutive elements of window n, read once (x and
// x0), written P times.  VEC (T % 4 == 0): a thread owns four consecutive elements — one channel, 16-byte loads and stores; else
// element e * 256 + tid of the tile, element-wise.  The first tile of a window also copies its v to the P rows of dlogits.
// ------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(AT_THREADS) void at_path_kernel(const float* __restrict__ x, const float* __restrict__ base, int kind,
                                                             const float* __restrict__ coef, const float* __restrict__ v, int P, int C, int T,
                                                             int K, int tiles, float* __restrict__ xp, float* __restrict__ dlogits) {
  const int n = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x % (unsigned)tiles);
  const int tid = threadIdx.x;
  const int CT = C * T;
  const int64_t own = (int64_t)n * CT;
  if (tile == 0 && v != nullptr) {
    for (int j = tid; j < P * K; j += AT_THREADS) dlogits[(int64_t)n * P * K + j] = v[(int64_t)n * K + j % K];
  }
  float* __restrict__ out = xp + (int64_t)n * P * CT;
  if (VEC) {
    const int i = tile * AT_TILE + 4 * tid;
    if (i >= CT) return;                                  // CT % 4 == 0: i + 3 < CT, and the four share a channel (T % 4 == 0)
    const int c = i / T;
    const float4 xv = *(const float4*)(x + own + i);
    const float4 b = at_base4(base, kind, own, c, i);
    const float4 d = make_float4(xv.x - b.x, xv.y - b.y, xv.z - b.z, xv.w - b.w);
    for (int p = 0; p < P; ++p) {
      const float a = coef[p * C + c];
      *(float4*)(out + (int64_t)p * CT + i) = a == 1.0f ? xv : make_float4(fmaf(a, d.x, b.x), fmaf(a, d.y, b.y), fmaf(a, d.z, b.z), fmaf(a, d.w, b.w));
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = tile * AT_TILE + e * AT_THREADS + tid;
      if (i >= CT) break;
      const int c = i / T;
      const float b = at_base(base, kind, own, c, i);
      const float xs = x[own + i], d = xs - b;
      for (int p = 0; p < P; ++p) {
        const float a = coef[p * C + c];
        out[(int64_t)p * CT + i] = a == 1.0f ? xs : fmaf(a, d, b);
      }
    }
  }
}

// ------------------------------------------------------------------------------------
// One workgroup per row (n, c), tile by tile of AT_TILE positions.
//   phase 1  G = sum_p w[p] * dx_p (fmaf chain in p order, eight 16-byte loads in flight per thread), map = (x - x0) * G into the
//            optional output and into LDS; every thread also keeps the fp64 sum of the values it made (the channel's sum).
//   phase 2  the tile is cut at the bin boundaries into segments and every segment into pieces of AT_PIECE values; one thread adds
//            up one piece in index order, in fp64.
//   phase 3  one thread per segment adds its pieces in order; a bin that ends in the tile is stored, one that goes on into the next
//            tile is carried there (at most one per tile: the last segment).
// The order of every sum is a function of (T, bin) alone.
// ------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(AT_THREADS) void at_reduce_kernel(const float* __restrict__ dx, const float* __restrict__ x,
                                                               const float* __restrict__ base, int kind, const float* __restrict__ w, int P, int C,
                                                               int T, int bin, int NB, float* __restrict__ map, float* __restrict__ bins,
                                                               float* __restrict__ chan, double* __restrict__ scratch) {
  __shared__ __attribute__((aligned(16))) float tv[AT_TILE];
  __shared__ double pp[AT_TILE];
  __shared__ double red[AT_THREADS];
  __shared__ double carry[2];
  __shared__ float ws[MSIG_AT_MAX_POINTS];
  const int row = blockIdx.x, n = row / C, c = row % C, tid = threadIdx.x;
  const int64_t CT = (int64_t)C * T;
  const int64_t ro = (int64_t)row * T;                                  // the row in x, map and an (N, C, T) baseline
  const int64_t own = (int64_t)n * CT, ci = (int64_t)c * T;             // at_base's window offset, the row's offset in its window
  const float* __restrict__ drow = dx + (int64_t)n * P * CT + ci;       // the row at p = 0; the P rows are CT floats apart
  for (int j = tid; j < P; j += AT_THREADS) ws[j] = w[j];
  if (tid < 2) carry[tid] = 0.0;
  double mine = 0.0;
  int par = 0;
  __syncthreads();
  for (int t0 = 0; t0 < T; t0 += AT_TILE, par ^= 1) {
    const int len = min(AT_TILE, T - t0);
    // ---- phase 1
    if (VEC) {
      const int t = t0 + 4 * tid;
      if (t < T) {                                                      // T % 4 == 0: t + 3 < T
        float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const float* __restrict__ src = drow + t;
        int p = 0;
        for (; p + 8 <= P; p += 8) {
          float4 q[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) q[u] = *(const float4*)(src + (int64_t)(p + u) * CT);
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const float a = ws[p + u];
            g.x = fmaf(a, q[u].x, g.x); g.y = fmaf(a, q[u].y, g.y); g.z = fmaf(a, q[u].z, g.z); g.w = fmaf(a, q[u].w, g.w);
          }
        }
        for (; p < P; ++p) {
          const float4 q = *(const float4*)(src + (int64_t)p * CT);
          const float a = ws[p];
          g.x = fmaf(a, q.x, g.x); g.y = fmaf(a, q.y, g.y); g.z = fmaf(a, q.z, g.z); g.w = fmaf(a, q.w, g.w);
        }
        const float4 xv = *(const float4*)(x + ro + t);
        const float4 b = at_base4(base, kind, own, c, ci + t);
        const float4 m = make_float4((xv.x - b.x) * g.x, (xv.y - b.y) * g.y, (xv.z - b.z) * g.z, (xv.w - b.w) * g.w);
        if (map != nullptr) *(float4*)(map + ro + t) = m;
        *(float4*)(tv + 4 * tid) = m;
        mine += (double)m.x; mine += (double)m.y; mine += (double)m.z; mine += (double)m.w;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int t = t0 + e * AT_THREADS + tid;
        if (t < T) {
          float g = 0.0f;
          for (int p = 0; p < P; ++p) g = fmaf(ws[p], drow[(int64_t)p * CT + t], g);
          const float m = (x[ro + t] - at_base(base, kind, own, c, ci + t)) * g;
          if (map != nullptr) map[ro + t] = m;
          tv[e * AT_THREADS + tid] = m;
          mine += (double)m;
        }
      }
    }
    __syncthreads();
    // ---- phase 2: segments s = 0 .. nseg-1 are the bins jb0 + s cut to the tile [0, len); segment 0 starts at 0
    const int jb0 = t0 / bin, nseg = (t0 + len - 1) / bin - jb0 + 1;
    const int len0 = (int)min((int64_t)len, ((int64_t)jb0 + 1) * bin - t0);            // of segment 0
    const int np0 = (len0 + AT_PIECE - 1) / AT_PIECE;
    const int npm = (int)(((int64_t)bin + AT_PIECE - 1) / AT_PIECE);                      // of a whole bin (used only when nseg > 1: bin < AT_TILE)
    const int lenl = nseg > 1 ? (int)(t0 + len - ((int64_t)jb0 + nseg - 1) * bin) : 0;  // of the last segment when it is not segment 0
    const int npl = (lenl + AT_PIECE - 1) / AT_PIECE;
    const int npc = nseg > 1 ? np0 + (nseg - 2) * npm + npl : np0;                        // <= AT_TILE: a piece holds at least one value
    for (int q = tid; q < npc; q += AT_THREADS) {
      int s = 0, k = q;
      if (q >= np0) { s = 1 + (q - np0) / npm; k = (q - np0) % npm; }
      const int a = s == 0 ? 0 : (int)(((int64_t)jb0 + s) * bin - t0);
      const int e = s == 0 ? len0 : (int)min((int64_t)len, ((int64_t)jb0 + s + 1) * bin - t0);
      const int lo = a + k * AT_PIECE, hi = min(e, lo + AT_PIECE);
      double acc = 0.0;
      for (int i = lo; i < hi; ++i) acc += (double)tv[i];
      pp[q] = acc;
    }
    __syncthreads();
    // ---- phase 3
    for (int s = tid; s < nseg; s += AT_THREADS) {
      const int q0 = s == 0 ? 0 : np0 + (s - 1) * npm;
      const int cnt = s == 0 ? np0 : (s == nseg - 1 ? npl : npm);
      double acc = s == 0 ? carry[par] : 0.0;
      for (int k = 0; k < cnt; ++k) acc += pp[q0 + k];
      const int64_t j = (int64_t)jb0 + s;
      const int64_t seg_end = s == 0 ? (int64_t)t0 + len0 : min((int64_t)t0 + len, (j + 1) * bin);
      const bool done = seg_end == min((int64_t)T, (j + 1) * bin);
      if (done) bins[(int64_t)row * NB + j] = (float)acc;
      if (s == nseg - 1) carry[par ^ 1] = done ? 0.0 : acc;
    }
    __syncthreads();
  }
  // ---- the channel's sum: the threads' fp64 partial sums in a fixed tree
  red[tid] = mine;
  __syncthreads();
  for (int s = AT_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) {
    chan[row] = (float)red[0];
    scratch[row] = red[0];
  }
}

// total[n] = the channels' unrounded sums in channel order, rounded once
__global__ __launch_bounds__(AT_THREADS) void at_total_kernel(const double* __restrict__ scratch, int N, int C, float* __restrict__ total) {
  const int n = blockIdx.x * AT_THREADS + threadIdx.x;
  if (n >= N) return;
  double acc = 0.0;
  for (int c = 0; c < C; ++c) acc += scratch[(int64_t)n * C + c];
  total[n] = (float)acc;
}

// ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
static inline bool at_mis16(const void* p) { return ((uintptr_t)p & 15) != 0; }
static inline bool at_mis4(const void* p) { return ((uintptr_t)p & 3) != 0; }

static int at_check_shape(int32_t base_kind, int32_t N, int32_t P, int32_t C, int32_t T) {
  if (base_kind < MSIG_AT_BASE_ZERO || base_kind > MSIG_AT_BASE_OWN) return MSIG_E_SHAPE;
  if (N < 1 || P < 1 || P > MSIG_AT_MAX_POINTS || C < 1 || C > MSIG_MAX_C || T < 16) return MSIG_E_SHAPE;
  if ((int64_t)C * T >= ((int64_t)1 << 31) || (int64_t)N * P >= ((int64_t)1 << 31)) return MSIG_E_SHAPE;
  return 0;
}

extern "C" int msig_at_abi_version(void) { return MSIG_AT_ABI_VERSION; }

extern "C" int msig_at_path(const float* x, const float* base, int32_t base_kind, const float* coef, const float* v,
                            int32_t N, int32_t P, int32_t C, int32_t T, int32_t K, float* xp, float* dlogits, void* stream) {
  if (!x || !coef || !xp) return MSIG_E_NULL;
  if (v && !dlogits) return MSIG_E_NULL;
  int rc = at_check_shape(base_kind, N, P, C, T);
  if (rc) return rc;
  if (base_kind != MSIG_AT_BASE_ZERO && !base) return MSIG_E_NULL;
  if (v && (K < 2 || K > MSIG_MAX_K)) return MSIG_E_SHAPE;
  const int64_t tiles = ((int64_t)C * T + AT_TILE - 1) / AT_TILE;
  if ((int64_t)N * tiles >= ((int64_t)1 << 31)) return MSIG_E_SHAPE;
  if (at_mis16(x) || at_mis16(xp) || (base_kind != MSIG_AT_BASE_ZERO && at_mis16(base)) || at_mis4(coef) || (v && (at_mis4(v) || at_mis4(dlogits))))
    return MSIG_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const float* b = base_kind == MSIG_AT_BASE_ZERO ? nullptr : base;
  MSIG_K("at_path", st);
  const dim3 grid((unsigned)((int64_t)N * tiles));
  if (T % 4 == 0) at_path_kernel<true><<<grid, AT_THREADS, 0, st>>>(x, b, base_kind, coef, v, P, C, T, K, (int)tiles, xp, dlogits);
  else at_path_kernel<false><<<grid, AT_THREADS, 0, st>>>(x, b, base_kind, coef, v, P, C, T, K, (int)tiles, xp, dlogits);
  MSIG_LAUNCH_CHECK();
  return 0;
}

extern "C" int msig_at_reduce(const float* dx, const float* x, const float* base, int32_t base_kind, const float* w,
                              int32_t N, int32_t P, int32_t C, int32_t T, int32_t bin,
                              float* map, float* bins, float* chan, float* total, double* scratch, void* stream) {
  if (!dx || !x || !w || !bins || !chan || !total || !scratch) return MSIG_E_NULL;
  int rc = at_check_shape(base_kind, N, P, C, T);
  if (rc) return rc;
  if (base_kind != MSIG_AT_BASE_ZERO && !base) return MSIG_E_NULL;
  if (bin < 1) return MSIG_E_SHAPE;
  if ((int64_t)N * C >= ((int64_t)1 << 31)) return MSIG_E_SHAPE;
  if (at_mis16(dx) || at_mis16(x) || at_mis16(map) || (base_kind != MSIG_AT_BASE_ZERO && at_mis16(base)) || at_mis4(w) || at_mis4(bins) ||
      at_mis4(chan) || at_mis4(total) || ((uintptr_t)scratch & 7))
    return MSIG_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const float* b = base_kind == MSIG_AT_BASE_ZERO ? nullptr : base;
  const int NB = (int)(((int64_t)T + bin - 1) / bin);
  {
    MSIG_K("at_reduce", st);
    const dim3 grid((unsigned)((int64_t)N * C));
    if (T % 4 == 0) at_reduce_kernel<true><<<grid, AT_THREADS, 0, st>>>(dx, x, b, base_kind, w, P, C, T, bin, NB, map, bins, chan, scratch);
    else at_reduce_kernel<false><<<grid, AT_THREADS, 0, st>>>(dx, x, b, base_kind, w, P, C, T, bin, NB, map, bins, chan, scratch);
    MSIG_LAUNCH_CHECK();
  }
  {
    MSIG_K("at_total", st);
    at_total_kernel<<<dim3((unsigned)((N + AT_THREADS - 1) / AT_THREADS)), AT_THREADS, 0, st>>>(scratch, N, C, total);
    MSIG_LAUNCH_CHECK();
  }
  return 0;
}
