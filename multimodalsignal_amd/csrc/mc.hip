// include/msig_mc.h: the two kernels of Monte-Carlo dropout that are not the model's — the S-fold replication of
// the trunk's output into the wide batch's workspace, and the reduction of the wide batch's logits to the per-window statistics.
// msig_mc_trunk and msig_mc_tail are launch orders of the model's own kernels: api.hip.
#include "member_stats.h"

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

// The reduction is member_stats (member_stats.h) over the S passes of a window, which lie window-major: pass s of window n at row
// n * S + s.  No slots, no member_pred, no disagreement.
__global__ __launch_bounds__(MEMBER_THREADS) void mc_reduce_kernel(const float* __restrict__ logits, int S, int K, float* __restrict__ mean_p,
                                                                   float* __restrict__ std_p, int* __restrict__ pred,
                                                                   float* __restrict__ entropy, float* __restrict__ expected_entropy,
                                                                   float* __restrict__ mutual_info, int* __restrict__ votes) {
  member_stats<false, MEMBER_FULL, true>(logits, MemberWhere{}, S, K, 1.0, mean_p, std_p, pred, entropy, expected_entropy, mutual_info, votes,
                                         nullptr, nullptr);
}

// ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
extern "C" int msig_mc_abi_version(void) { return MSIG_MC_ABI_VERSION; }

extern "C" int msig_mc_expand(const float* src, float* dst, int32_t N, int32_t S, int64_t row_floats, void* stream) {
  if (!src || !dst) return MSIG_E_NULL;
  if (N < 1 || S < 1 || S > MSIG_MC_MAX_SAMPLES || row_floats < 1) return MSIG_E_SHAPE;
  if ((int64_t)N * S >= ((int64_t)1 << 31)) return MSIG_E_SHAPE;
  if (row_floats >= ((int64_t)1 << 40)) return MSIG_E_SHAPE;          // N * tiles and N * S * row_floats stay far inside 64 bits
  const int64_t tiles = (row_floats + MC_TILE - 1) / MC_TILE;
  if ((int64_t)N * tiles >= ((int64_t)1 << 31)) return MSIG_E_SHAPE;  // the grid
  if (msig_misaligned(src, 3) || msig_misaligned(dst, 3)) return MSIG_E_ALIGN;
  const bool vec = row_floats % 4 == 0 && !msig_misaligned(src, 15) && !msig_misaligned(dst, 15);
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
  return member_launch("mc_reduce", logits, S, MSIG_MC_MAX_SAMPLES, N, K, false, {mean_p, std_p, pred, entropy, expected_entropy, mutual_info, votes},
                       (hipStream_t)stream, [&](dim3 grid, dim3 block, hipStream_t st) {
                         mc_reduce_kernel<<<grid, block, 0, st>>>(logits, S, K, mean_p, std_p, pred, entropy, expected_entropy, mutual_info, votes);
                       });
}
