// The window gathers.  gather_kernel is the plain copy (msig_gather_windows*, api.hip): by float4 when the window's float count is a
// multiple of 4, element by element otherwise (any window length: C * T need not be a multiple of 4).  On-device window augmentation inside
// the training gather (include/msig_aug.h) is that copy with per-channel magnitude scaling, additive jitter, a
// time mask and channel dropout applied in registers.  A streaming kernel: every input byte is read once and every output byte
// written once, as in the plain gather; the draws are counter-based hashes of (key, row, channel, sample), so there is no state and
// a fold's batch does not depend on the folds it shares the launch with.
#include <math.h>
#include "msig_dev.h"
#include "../../include/msig_aug.h"
#include "../../include/msig_st.h"

int msig_multi_fold_ctx(const msig_multi* m, FoldCtx& fc);                                  // api.hip: msig_multi's own checks

// blockIdx.z = fold (msig_gather_windows_multi): the store is shared, idx is (n, B) contiguous, the outputs are per-arena.
// V = float4: wv = window_floats / 4, rows 16-byte aligned (the caller checks); V = float: wv = window_floats, no alignment demand.
template <typename V>
__global__ __launch_bounds__(256) void gather_kernel(const float* __restrict__ store, const int64_t* __restrict__ store_y,
                                                     const int64_t* __restrict__ idx, int64_t idx_row_stride, int64_t wv,
                                                     float* __restrict__ ox, int64_t* __restrict__ oy, const FoldCtx fc) {
  FOLD_BEGIN; FS(ox); FS(oy);
  const int i = blockIdx.y;
  const int64_t src = idx[(int64_t)blockIdx.z * idx_row_stride + i];
  const V* sv = (const V*)(store) + src * wv;
  V* dv = (V*)(ox) + (int64_t)i * wv;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < wv; j += (int64_t)gridDim.x * 256) dv[j] = sv[j];
  if (oy && store_y && blockIdx.x == 0 && threadIdx.x == 0) oy[i] = store_y[src];
}

int launch_gather(const float* store, const int64_t* sy, const int64_t* idx, int64_t idx_row_stride, int B, int64_t wfloats, float* ox, int64_t* oy,
                  const FoldCtx& fc, hipStream_t st) {
  const bool vec = (wfloats & 3) == 0;
  const int64_t wv = vec ? wfloats / 4 : wfloats;
  int gx = (int)((wv + 255) / 256);
  if (gx > 64) gx = 64;
  {
    MSIG_K("gather", st);
    if (vec) gather_kernel<float4><<<dim3(gx, B, fc.n), 256, 0, st>>>(store, sy, idx, idx_row_stride, wv, ox, oy, fc);
    else gather_kernel<float><<<dim3(gx, B, fc.n), 256, 0, st>>>(store, sy, idx, idx_row_stride, wv, ox, oy, fc);
  }
  MSIG_LAUNCH_CHECK();
  return 0;
}

#define AUG_TAG_SCALE 0x80000001u
#define AUG_TAG_CDROP 0x80000002u
#define AUG_TAG_MASK  0x80000003u
#define AUG_TAG_MLEN  0x80000004u
#define AUG_TAG_MT0   0x80000005u
#define AUG_TAG_KEEP  0x80000006u

struct AugArgs {                          // the launch's parameters, thresholds already computed (host, double precision)
  float scale_sigma, jitter_sigma;
  uint32_t mask_thr, cdrop_thr;
  int32_t mask_on, cdrop_on, mask_max, T;
};
struct AugKeys { uint32_t key[MSIG_MAX_FOLDS]; };

// Every fp32 operation below is ONE rounding: no FMA may be formed, or the result is no longer the numpy restatement's.  The HIP
// headers' __fmul_rn / __fadd_rn do not give that on this toolchain — they are plain `*` / `+` (or library code that is) compiled
// contractable, and after inlining the pair becomes v_fma_f32 — so contraction is switched off for the rest of this file and the
// two operations are written out.
#pragma clang fp contract(off)
__device__ __forceinline__ float aug_fmul(float a, float b) { return a * b; }
__device__ __forceinline__ float aug_fadd(float a, float b) { return a + b; }

__host__ __device__ __forceinline__ uint32_t aug_row_key(uint32_t key, uint32_t row) { return fmix32(key ^ (row * 0x9E3779B9u)); }
__host__ __device__ __forceinline__ uint32_t aug_chan_key(uint32_t rk, uint32_t c) { return fmix32(rk + (c + 1u) * 0x7F4A7C15u); }
__host__ __device__ __forceinline__ uint32_t aug_mulhi(uint32_t w, uint32_t n) { return (uint32_t)(((uint64_t)w * n) >> 32); }
// standardised sum of the four bytes of a hash word: integer arithmetic and one fp32 multiplication
__device__ __forceinline__ float aug_noise(uint32_t w) {
  const int s = (int)((w & 0xFFu) + ((w >> 8) & 0xFFu) + ((w >> 16) & 0xFFu) + (w >> 24));
  return aug_fmul((float)(s - 510), MSIG_AUG_NOISE_K);
}

// grid: x = channel * chunks + chunk of the channel's T / 4 float4s, y = row of the batch, z = fold.  Everything a workgroup draws
// per row and per (row, channel) depends on blockIdx and kernel arguments alone: it is uniform, computed once on the scalar unit.
template <bool JITTER>
__global__ __launch_bounds__(256) void aug_gather_kernel(const float* __restrict__ store, const int64_t* __restrict__ store_y,
                                                         const int64_t* __restrict__ idx, int64_t idx_row_stride, int C, int chunks,
                                                         float* __restrict__ ox, int64_t* __restrict__ oy, const AugArgs a,
                                                         const AugKeys keys, const FoldCtx fc) {
  FOLD_BEGIN; FS(ox); FS(oy);
  const int row = blockIdx.y, c = blockIdx.x / chunks, chunk = blockIdx.x - c * chunks;
  const int T4 = a.T >> 2;
  const int64_t src = idx[(int64_t)blockIdx.z * idx_row_stride + row];
  const float4* s4 = (const float4*)(store) + (src * C + c) * T4;
  float4* d4 = (float4*)(ox) + ((int64_t)row * C + c) * T4;
  if (oy && store_y && blockIdx.x == 0 && threadIdx.x == 0) oy[row] = store_y[src];

  const uint32_t rk = aug_row_key(keys.key[blockIdx.z], (uint32_t)row);
  const uint32_t ck = aug_chan_key(rk, (uint32_t)c);
  const int stride = chunks * blockDim.x;

  // ---- channel dropout: the whole (row, channel) is +0.0, nothing is read ----
  if (a.cdrop_on && fmix32(ck ^ AUG_TAG_CDROP) <= a.cdrop_thr) {
    bool all = true;
    for (int cc = 0; cc < C; ++cc) all = all && fmix32(aug_chan_key(rk, (uint32_t)cc) ^ AUG_TAG_CDROP) <= a.cdrop_thr;
    if (!(all && (int)aug_mulhi(fmix32(rk ^ AUG_TAG_KEEP), (uint32_t)C) == c)) {
      for (int j = chunk * blockDim.x + threadIdx.x; j < T4; j += stride) d4[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      return;
    }
  }
  // ---- time mask: samples m0 <= t < m1 of every channel of the row (m0 = m1: none) ----
  int m0 = 0, m1 = 0;
  if (a.mask_on && fmix32(rk ^ AUG_TAG_MASK) <= a.mask_thr) {
    const int len = 1 + (int)aug_mulhi(fmix32(rk ^ AUG_TAG_MLEN), (uint32_t)a.mask_max);
    m0 = (int)aug_mulhi(fmix32(rk ^ AUG_TAG_MT0), (uint32_t)(a.T - len + 1));
    m1 = m0 + len;
  }
  const bool scale = a.scale_sigma != 0.f;
  const float gain = scale ? aug_fadd(1.f, aug_fmul(a.scale_sigma, aug_noise(fmix32(ck ^ AUG_TAG_SCALE)))) : 1.f;

  for (int j = chunk * blockDim.x + threadIdx.x; j < T4; j += stride) {
    const float4 v = s4[j];
    float y[4] = {v.x, v.y, v.z, v.w};
    const int t = 4 * j;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (scale) y[e] = aug_fmul(y[e], gain);
      if (JITTER) y[e] = aug_fadd(y[e], aug_fmul(a.jitter_sigma, aug_noise(fmix32(ck ^ (uint32_t)(t + e)))));
      if (t + e >= m0 && t + e < m1) y[e] = 0.f;
    }
    d4[j] = make_float4(y[0], y[1], y[2], y[3]);
  }
}

// ---- the gather with mixup (include/msig_st.h): out[b] = lam * A_b + mu * A_{B-1-b}, A_r the window of batch
// row r after that row's own transforms above ("augment the batch, then mix it"); with every transform off A_r is the plain window.
// AugRowChan is what aug_gather_kernel draws per (row, channel), aug_vec4 one float4 of A_r: the same statements in the same order,
// every fp32 operation one rounding (contraction is off), so A_r has aug_gather_kernel's bits.  A fold whose lam is 1 — uniform,
// blockIdx.z — stores A_b itself: the plain or augmented gather's bits, not a + 0 * b (which turns -0.0 into +0.0).
struct MixLam { float lam[MSIG_MAX_FOLDS]; };
struct AugRowChan { const float4* s4; uint32_t ck; int m0, m1; float gain; bool zero, scale; };

__device__ __forceinline__ AugRowChan aug_row_chan(const float* __restrict__ store, int64_t src, int row, int c, int C, int T4, const AugArgs& a,
                                                   uint32_t key) {
  AugRowChan r;
  r.s4 = (const float4*)(store) + (src * C + c) * T4;
  const uint32_t rk = aug_row_key(key, (uint32_t)row);
  r.ck = aug_chan_key(rk, (uint32_t)c);
  r.zero = false; r.m0 = 0; r.m1 = 0;
  if (a.cdrop_on && fmix32(r.ck ^ AUG_TAG_CDROP) <= a.cdrop_thr) {
    bool all = true;
    for (int cc = 0; cc < C; ++cc) all = all && fmix32(aug_chan_key(rk, (uint32_t)cc) ^ AUG_TAG_CDROP) <= a.cdrop_thr;
    r.zero = !(all && (int)aug_mulhi(fmix32(rk ^ AUG_TAG_KEEP), (uint32_t)C) == c);
  }
  if (a.mask_on && fmix32(rk ^ AUG_TAG_MASK) <= a.mask_thr) {
    const int len = 1 + (int)aug_mulhi(fmix32(rk ^ AUG_TAG_MLEN), (uint32_t)a.mask_max);
    r.m0 = (int)aug_mulhi(fmix32(rk ^ AUG_TAG_MT0), (uint32_t)(a.T - len + 1));
    r.m1 = r.m0 + len;
  }
  r.scale = a.scale_sigma != 0.f;
  r.gain = r.scale ? aug_fadd(1.f, aug_fmul(a.scale_sigma, aug_noise(fmix32(r.ck ^ AUG_TAG_SCALE)))) : 1.f;
  return r;
}
template <bool JITTER>
__device__ __forceinline__ void aug_vec4(const AugRowChan& r, int j, const AugArgs& a, float (&y)[4]) {
  if (r.zero) { y[0] = y[1] = y[2] = y[3] = 0.f; return; }       // channel dropout: +0.0, nothing is read
  const float4 v = r.s4[j];
  y[0] = v.x; y[1] = v.y; y[2] = v.z; y[3] = v.w;
  const int t = 4 * j;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (r.scale) y[e] = aug_fmul(y[e], r.gain);
    if (JITTER) y[e] = aug_fadd(y[e], aug_fmul(a.jitter_sigma, aug_noise(fmix32(r.ck ^ (uint32_t)(t + e)))));
    if (t + e >= r.m0 && t + e < r.m1) y[e] = 0.f;
  }
}

// aug_gather_kernel's grid: x = channel * chunks + chunk, y = row of the batch (B = gridDim.y), z = fold
template <bool JITTER>
__global__ __launch_bounds__(256) void mix_gather_kernel(const float* __restrict__ store, const int64_t* __restrict__ store_y,
                                                         const int64_t* __restrict__ idx, int64_t idx_row_stride, int C, int chunks,
                                                         float* __restrict__ ox, int64_t* __restrict__ oy, const AugArgs a,
                                                         const AugKeys keys, const MixLam ml, const FoldCtx fc) {
  FOLD_BEGIN; FS(ox); FS(oy);
  const int B = gridDim.y;
  const int row = blockIdx.y, prow = B - 1 - row, c = blockIdx.x / chunks, chunk = blockIdx.x - c * chunks;
  const int T4 = a.T >> 2;
  const int64_t* ix = idx + (int64_t)blockIdx.z * idx_row_stride;
  const int64_t src = ix[row];
  float4* d4 = (float4*)(ox) + ((int64_t)row * C + c) * T4;
  if (oy && store_y && blockIdx.x == 0 && threadIdx.x == 0) oy[row] = store_y[src];      // the row's own label
  const uint32_t key = keys.key[blockIdx.z];
  const float lam = ml.lam[blockIdx.z];
  const int stride = chunks * blockDim.x;
  const AugRowChan ra = aug_row_chan(store, src, row, c, C, T4, a, key);
  if (lam == 1.f) {
    for (int j = chunk * blockDim.x + threadIdx.x; j < T4; j += stride) {
      float y[4];
      aug_vec4<JITTER>(ra, j, a, y);
      d4[j] = make_float4(y[0], y[1], y[2], y[3]);
    }
    return;
  }
  const float mu = aug_fadd(1.f, -lam);
  const AugRowChan rb = aug_row_chan(store, ix[prow], prow, c, C, T4, a, key);
  for (int j = chunk * blockDim.x + threadIdx.x; j < T4; j += stride) {
    float y[4], p[4];
    aug_vec4<JITTER>(ra, j, a, y);
    aug_vec4<JITTER>(rb, j, a, p);
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = aug_fadd(aug_fmul(lam, y[e]), aug_fmul(mu, p[e]));
    d4[j] = make_float4(y[0], y[1], y[2], y[3]);
  }
}

// ceil(p * 2^32) - 1 for 0 < p <= 1: the event `word <= thr` has probability ceil(p 2^32) / 2^32
static uint32_t aug_threshold(float p) {
  const double v = ceil((double)p * 4294967296.0) - 1.0;
  return v <= 0.0 ? 0u : v >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)v;
}

static int aug_check(const msig_aug* a, int64_t B, int C, int T) {
  if (B < 1 || B > 65535 || C < 1 || C > MSIG_MAX_C || T < 4 || (T & 3)) return MSIG_E_SHAPE;
  if (!(a->scale_sigma >= 0.f) || !(a->jitter_sigma >= 0.f)) return MSIG_E_SHAPE;              // negative or NaN
  if (!(a->mask_prob >= 0.f && a->mask_prob <= 1.f) || !(a->chan_drop_prob >= 0.f && a->chan_drop_prob < 1.f)) return MSIG_E_SHAPE;
  if (a->mask_prob > 0.f && (a->mask_max < 1 || a->mask_max > T)) return MSIG_E_SHAPE;
  return 0;
}

// lam: NULL, or the folds' mixup weights (include/msig_st.h) of which at least one is not 1 — then mix_gather_kernel runs instead
static int launch_aug_gather(const float* store, const int64_t* sy, const int64_t* idx, int64_t idx_row_stride, int B, int C, int T, float* ox,
                             int64_t* oy, const msig_aug* a, const FoldCtx& fc, hipStream_t st, const float* lam = nullptr) {
  if (!lam && a->scale_sigma == 0.f && a->jitter_sigma == 0.f && a->mask_prob == 0.f && a->chan_drop_prob == 0.f)
    return launch_gather(store, sy, idx, idx_row_stride, B, (int64_t)C * T, ox, oy, fc, st);   // switched off: the plain gather itself
  AugArgs g{};
  g.scale_sigma = a->scale_sigma; g.jitter_sigma = a->jitter_sigma; g.T = T;
  g.mask_on = a->mask_prob > 0.f; g.mask_thr = g.mask_on ? aug_threshold(a->mask_prob) : 0u; g.mask_max = g.mask_on ? a->mask_max : 1;
  g.cdrop_on = a->chan_drop_prob > 0.f; g.cdrop_thr = g.cdrop_on ? aug_threshold(a->chan_drop_prob) : 0u;
  AugKeys keys{};
  for (int z = 0; z < fc.n; ++z) keys.key[z] = a->key[z];
  // a workgroup's elements share (row, channel): up to 256 threads of one float4 each over the channel's T / 4, at most 8
  // workgroups per (row, channel) — beyond that a thread takes several
  const int T4 = T / 4;
  const int threads = T4 >= 256 ? 256 : (T4 + 63) / 64 * 64;
  int chunks = (T4 + threads - 1) / threads;
  if (chunks > 8) chunks = 8;
  const dim3 grid((unsigned)(C * chunks), (unsigned)B, (unsigned)fc.n);
  if (lam) {
    MixLam ml{};
    for (int z = 0; z < fc.n; ++z) ml.lam[z] = lam[z];
    {
      MSIG_K("mix_gather", st);
      if (g.jitter_sigma != 0.f) mix_gather_kernel<true><<<grid, threads, 0, st>>>(store, sy, idx, idx_row_stride, C, chunks, ox, oy, g, keys, ml, fc);
      else mix_gather_kernel<false><<<grid, threads, 0, st>>>(store, sy, idx, idx_row_stride, C, chunks, ox, oy, g, keys, ml, fc);
    }
    MSIG_LAUNCH_CHECK();
    return 0;
  }
  {
    MSIG_K("aug_gather", st);
    if (g.jitter_sigma != 0.f) aug_gather_kernel<true><<<grid, threads, 0, st>>>(store, sy, idx, idx_row_stride, C, chunks, ox, oy, g, keys, fc);
    else aug_gather_kernel<false><<<grid, threads, 0, st>>>(store, sy, idx, idx_row_stride, C, chunks, ox, oy, g, keys, fc);
  }
  MSIG_LAUNCH_CHECK();
  return 0;
}

extern "C" int msig_aug_abi_version(void) { return MSIG_AUG_ABI_VERSION; }
extern "C" int64_t msig_aug_struct_bytes(void) { return (int64_t)sizeof(msig_aug); }

extern "C" int msig_aug_gather_windows(const float* store, const int64_t* store_labels, const int64_t* idx, int32_t B, int32_t C, int32_t T,
                                       float* out_x, int64_t* out_y, const msig_aug* a, void* stream) {
  if (!a || !store || !idx || !out_x) return MSIG_E_NULL;
  const int rc = aug_check(a, B, C, T); if (rc) return rc;
  if (((uintptr_t)store | (uintptr_t)out_x) & 15) return MSIG_E_ALIGN;
  return launch_aug_gather(store, store_labels, idx, B, B, C, T, out_x, out_y, a, single_fold(nullptr), (hipStream_t)stream);
}

extern "C" int msig_aug_gather_windows_multi(const float* store, const int64_t* store_labels, const int64_t* idx, int64_t idx_row_stride,
                                             int32_t B, int32_t C, int32_t T, float* out_x, int64_t* out_y, const msig_multi* m,
                                             const msig_aug* a, void* stream) {
  if (!a || !store || !idx || !out_x || !m) return MSIG_E_NULL;
  FoldCtx fc; int rc = msig_multi_fold_ctx(m, fc); if (rc) return rc;
  rc = aug_check(a, B, C, T); if (rc) return rc;
  if (idx_row_stride < B) return MSIG_E_SHAPE;
  if (((uintptr_t)store | (uintptr_t)out_x) & 15) return MSIG_E_ALIGN;
  return launch_aug_gather(store, store_labels, idx, idx_row_stride, B, C, T, out_x, out_y, a, fc, (hipStream_t)stream);
}

// ---- include/msig_st.h: the gathers with the mixup blend ------------------------------------------------------------------------
// the checks of the lam array (host values, n folds): 0 = every lam is 1 (no blend), 1 = blend, else MSIG_E_*
static int mix_check(const float* lam, int n) {
  int any = 0;
  for (int z = 0; z < n; ++z) {
    if (!(lam[z] >= 0.f && lam[z] <= 1.f)) return MSIG_E_SHAPE;          // NaN included
    if (lam[z] != 1.f) any = 1;
  }
  return any;
}
static const msig_aug kAugOff{};

extern "C" int msig_st_gather_windows(const float* store, const int64_t* store_labels, const int64_t* idx, int32_t B, int32_t C, int32_t T,
                                      float* out_x, int64_t* out_y, const msig_aug* a, const float* lam, void* stream) {
  if (!lam || !store || !idx || !out_x) return MSIG_E_NULL;
  if (!a) a = &kAugOff;
  const int mix = mix_check(lam, 1); if (mix < 0) return mix;
  const int rc = aug_check(a, B, C, T); if (rc) return rc;
  if (((uintptr_t)store | (uintptr_t)out_x) & 15) return MSIG_E_ALIGN;
  return launch_aug_gather(store, store_labels, idx, B, B, C, T, out_x, out_y, a, single_fold(nullptr), (hipStream_t)stream, mix ? lam : nullptr);
}

extern "C" int msig_st_gather_windows_multi(const float* store, const int64_t* store_labels, const int64_t* idx, int64_t idx_row_stride,
                                            int32_t B, int32_t C, int32_t T, float* out_x, int64_t* out_y, const msig_multi* m,
                                            const msig_aug* a, const float* lam, void* stream) {
  if (!lam || !store || !idx || !out_x || !m) return MSIG_E_NULL;
  if (!a) a = &kAugOff;
  FoldCtx fc; int rc = msig_multi_fold_ctx(m, fc); if (rc) return rc;
  const int mix = mix_check(lam, fc.n); if (mix < 0) return mix;
  rc = aug_check(a, B, C, T); if (rc) return rc;
  if (idx_row_stride < B) return MSIG_E_SHAPE;
  if (((uintptr_t)store | (uintptr_t)out_x) & 15) return MSIG_E_ALIGN;
  return launch_aug_gather(store, store_labels, idx, idx_row_stride, B, C, T, out_x, out_y, a, fc, (hipStream_t)stream, mix ? lam : nullptr);
}
