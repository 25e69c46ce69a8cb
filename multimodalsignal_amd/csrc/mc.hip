// include/msig_mc.h: the two kernels of Monte-Carlo dropout that are not the model's — the S-fold replication of
// the trunk's output into the wide batch's workspace, and the reduction of the wide batch's logits to the per-window statistics.
// msig_mc_trunk and msig_mc_tail are launch orders of the model's own kernels: api.hip.
#include <math.h>
#include "msig_dev.h"
#include "../../include/msig_mc.h"

#define MC_THREADS 256
#define MC_TILE 1024        // floats of a row per workgroup: 256 threads x 4

// ------------------------------------------------------------------------------------
// dst[(n * S + s) * R + i] = src[n * R + i].  Workgroup (n, tile): MC_TILE consecutive floats of row n, read once, written S times.
// VEC (R % 4 == 0, both pointers 16-byte aligned): a thread owns four consecutive floats, 16-byte loads and stores; else float
// e * 256 + tid of the tile.  Every index is 64-bit; i < R is checked before any access, n < N by the grid.
// ------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(MC_THREADS) void mc_expand_kernel(const float* __restrict__ src, float* __restrict__ dst, int S, int64_t R,
                                                               int64_t tiles) {
  const int64_t n = (int64_t)blockIdx.x / tiles, tile = (int64_t)blockIdx.x % tiles;
  const int tid = threadIdx.x;
  const float* __restrict__ in = src + n * R;
  float* __restrict__ out = dst + n * S * R;
  if (VEC) {
    const int64_t i = tile * MC_TILE + 4 * tid;
    if (i >= R) return;                                     // R % 4 == 0: i + 3 < R
    const float4 v = *(const float4*)(in + i);
    for (int s = 0; s < S; ++s) *(float4*)(out + (int64_t)s * R + i) = v;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t i = tile * MC_TILE + e * MC_THREADS + tid;
      if (i >= R) break;
      const float v = in[i];
      for (int s = 0; s < S; ++s) out[(int64_t)s * R + i] = v;
    }
  }
}

// ------------------------------------------------------------------------------------
// One workgroup per window n, all of it in fp64.
//   phase 1  thread s < S: p_s = softmax of row n * S + s (max-subtracted) into LDS, H(p_s) and the row's first maximal logit;
//   phase 2  thread k < K: m_k = (sum_s p_s[k]) / S and the squared deviations, both in increasing s; the votes for class k;
//   phase 3  thread 0: the first argmax of m, H(m), the mean of H(p_s) in increasing s, their difference.
// Every sum has one owner and one order, fixed by (S, K): the bits of a window depend on nothing but its own S rows.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ double mc_plogp(double p) { return p > 0.0 ? p * log(p) : 0.0; }

__global__ __launch_bounds__(MC_THREADS) void mc_reduce_kernel(const float* __restrict__ logits, int S, int K, float* __restrict__ mean_p,
                                                               float* __restrict__ std_p, int* __restrict__ pred, float* __restrict__ entropy,
                                                               float* __restrict__ expected_entropy, float* __restrict__ mutual_info,
                                                               int* __restrict__ votes) {
  __shared__ double ps[MSIG_MC_MAX_SAMPLES * MSIG_MAX_K];
  __shared__ double hs[MSIG_MC_MAX_SAMPLES];
  __shared__ double ms[MSIG_MAX_K];
  __shared__ int vs[MSIG_MC_MAX_SAMPLES];
  const int64_t n = blockIdx.x;
  const int tid = threadIdx.x;
  if (tid < S) {
    const float* __restrict__ row = logits + (n * S + tid) * K;
    double e[MSIG_MAX_K];
    double mx = (double)row[0];
    int am = 0;
    for (int k = 1; k < K; ++k) {
      const double v = (double)row[k];
      if (v > mx) { mx = v; am = k; }
    }
    double sum = 0.0;
    for (int k = 0; k < K; ++k) { e[k] = exp((double)row[k] - mx); sum += e[k]; }
    double h = 0.0;
    for (int k = 0; k < K; ++k) {
      const double p = e[k] / sum;
      ps[tid * K + k] = p;
      h -= mc_plogp(p);
    }
    hs[tid] = h;
    vs[tid] = am;
  }
  __syncthreads();
  if (tid < K) {
    double acc = 0.0;
    int cnt = 0;
    for (int s = 0; s < S; ++s) { acc += ps[s * K + tid]; cnt += vs[s] == tid ? 1 : 0; }
    const double m = acc / (double)S;
    double sq = 0.0;
    for (int s = 0; s < S; ++s) { const double d = ps[s * K + tid] - m; sq += d * d; }
    ms[tid] = m;
    mean_p[n * K + tid] = (float)m;
    if (std_p) std_p[n * K + tid] = (float)sqrt(sq / (double)S);
    if (votes) votes[n * K + tid] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
    int am = 0;
    double h = 0.0;
    for (int k = 0; k < K; ++k) {
      if (ms[k] > ms[am]) am = k;
      h -= mc_plogp(ms[k]);
    }
    double eh = 0.0;
    for (int s = 0; s < S; ++s) eh += hs[s];
    eh /= (double)S;
    if (pred) pred[n] = am;
    if (entropy) entropy[n] = (float)h;
    if (expected_entropy) expected_entropy[n] = (float)eh;
    if (mutual_info) mutual_info[n] = (float)(h - eh);
  }
}

// ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
static inline bool mc_mis(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

extern "C" int msig_mc_abi_version(void) { return MSIG_MC_ABI_VERSION; }

extern "C" int msig_mc_expand(const float* src, float* dst, int32_t N, int32_t S, int64_t row_floats, void* stream) {
  if (!src || !dst) return MSIG_E_NULL;
  if (N < 1 || S < 1 || S > MSIG_MC_MAX_SAMPLES || row_floats < 1) return MSIG_E_SHAPE;
  if ((int64_t)N * S >= ((int64_t)1 << 31)) return MSIG_E_SHAPE;
  if (row_floats >= ((int64_t)1 << 40)) return MSIG_E_SHAPE;          // N * tiles and N * S * row_floats stay far inside 64 bits
  const int64_t tiles = (row_floats + MC_TILE - 1) / MC_TILE;
  if ((int64_t)N * tiles >= ((int64_t)1 << 31)) return MSIG_E_SHAPE;  // the grid
  if (mc_mis(src, 3) || mc_mis(dst, 3)) return MSIG_E_ALIGN;
  const bool vec = row_floats % 4 == 0 && !mc_mis(src, 15) && !mc_mis(dst, 15);
  hipStream_t st = (hipStream_t)stream;
  MSIG_K("mc_expand", st);
  const dim3 grid((unsigned)((int64_t)N * tiles));
  if (vec) mc_expand_kernel<true><<<grid, MC_THREADS, 0, st>>>(src, dst, S, row_floats, tiles);
  else mc_expand_kernel<false><<<grid, MC_THREADS, 0, st>>>(src, dst, S, row_floats, tiles);
  MSIG_LAUNCH_CHECK();
  return 0;
}

extern "C" int msig_mc_reduce(const float* logits, int32_t N, int32_t S, int32_t K, float* mean_p, float* std_p, int32_t* pred,
                              float* entropy, float* expected_entropy, float* mutual_info, int32_t* votes, void* stream) {
  if (!logits || !mean_p) return MSIG_E_NULL;
  if (N < 1 || S < 1 || S > MSIG_MC_MAX_SAMPLES || K < 2 || K > MSIG_MAX_K) return MSIG_E_SHAPE;
  if ((int64_t)N * S >= ((int64_t)1 << 31)) return MSIG_E_SHAPE;
  if (mc_mis(logits, 3) || mc_mis(mean_p, 3) || mc_mis(std_p, 3) || mc_mis(pred, 3) || mc_mis(entropy, 3) || mc_mis(expected_entropy, 3) ||
      mc_mis(mutual_info, 3) || mc_mis(votes, 3))
    return MSIG_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  MSIG_K("mc_reduce", st);
  mc_reduce_kernel<<<dim3((unsigned)N), MC_THREADS, 0, st>>>(logits, S, K, mean_p, std_p, pred, entropy, expected_entropy, mutual_info, votes);
  MSIG_LAUNCH_CHECK();
  return 0;
}
