// include/msig_sam.h: the perturbation and the restore of a sharpness-aware step, and their stand-alone
// calls.  Streaming kernels over one model's ~124 k parameter floats: blockIdx.z = fold, SAM_WG workgroups per fold whatever the
// launch, 128-bit accesses on every whole quad of a tensor, no LDS beyond the four wave sums of the norm.
#include "msig_dev.h"
#include "../../include/msig_sam.h"

#define SAM_THREADS 256

int msig_param_table(int C, int K, int kind, int64_t* off, int64_t* len);                  // api.hip: offsets and TRUE lengths

// The state's regions, from fold z's base (include/msig_sam.h, "State"): statistics, partial sums, then the backups.
__device__ __forceinline__ double* sam_part(char* state) { return (double*)state + MSIG_SAM_NSTAT; }
__device__ __forceinline__ float* sam_backup(char* state) { return (float*)((double*)state + MSIG_SAM_NSTAT + SAM_WG); }

// The backup region is 16-byte aligned when the state is; a state that is only 8-byte aligned (all the header asks) takes two
// 64-bit accesses per quad instead.  a16 is uniform over the launch.
__device__ __forceinline__ void sam_store4(float* p, const float4 v, bool a16) {
  if (a16) *(float4*)p = v;
  else { ((float2*)p)[0] = make_float2(v.x, v.y); ((float2*)p)[1] = make_float2(v.z, v.w); }
}
__device__ __forceinline__ float4 sam_load4(const float* p, bool a16) {
  if (a16) return *(const float4*)p;
  const float2 lo = ((const float2*)p)[0], hi = ((const float2*)p)[1];
  return make_float4(lo.x, lo.y, hi.x, hi.y);
}

// u of one element and, for ASAM, its t = |p| + eta: one rounding per operation
template <bool ASAM>
__device__ __forceinline__ float sam_u(float p, float g, float eta, float& t) {
#pragma clang fp contract(off)
  if constexpr (!ASAM) { t = 1.f; return g; }
  t = fabsf(p) + eta;
  return t * g;
}

// ------------------------------------------------------------------------------------
// Sum of squares.  Thread T of the fold's SAM_WG * SAM_THREADS walks the tensors in table order, quads T, T + threads, ... of each
// (the elements of a quad in increasing order), and thread `tensor index` the tensor's last 1..3 elements one by one: the padding of
// `grads` is never read.  Lanes are reduced per wave, the four wave sums added in wave order: partial[blockIdx.x].  The walk
// and the grid depend on the table alone, i.e. on (C, K, kind).
// ------------------------------------------------------------------------------------
template <bool ASAM>
__global__ __launch_bounds__(SAM_THREADS) void sam_sq_kernel(const SamArgs a, const float* __restrict__ params, const float* __restrict__ grads,
                                                             const FoldCtx fc) {
#pragma clang fp contract(off)
  FOLD_BEGIN; FS(params); FS(grads);
  char* state = a.state + foff_;
  __shared__ double wsum[SAM_THREADS / 64];
  const int tid = threadIdx.x, gt = (int)blockIdx.x * SAM_THREADS + tid, nt = SAM_WG * SAM_THREADS;
  double acc = 0.0;
  for (int ti = 0; ti < MSIG_NPARAM; ++ti) {
    const int off = a.off[ti], len = a.len[ti], n4 = len >> 2, rem = len & 3;
    for (int q = gt; q < n4; q += nt) {
      const float4 g = *(const float4*)(grads + off + 4 * q);
      float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (ASAM) p = *(const float4*)(params + off + 4 * q);
      float t;
      const double u0 = (double)sam_u<ASAM>(p.x, g.x, a.eta, t), u1 = (double)sam_u<ASAM>(p.y, g.y, a.eta, t);
      const double u2 = (double)sam_u<ASAM>(p.z, g.z, a.eta, t), u3 = (double)sam_u<ASAM>(p.w, g.w, a.eta, t);
      acc += u0 * u0; acc += u1 * u1; acc += u2 * u2; acc += u3 * u3;
    }
    if (rem && gt == ti)
      for (int e = 0; e < rem; ++e) {
        const int i = off + 4 * n4 + e;
        float t;
        const double u = (double)sam_u<ASAM>(ASAM ? params[i] : 0.f, grads[i], a.eta, t);
        acc += u * u;
      }
  }
  acc = wave_sum_d(acc);
  if ((tid & 63) == 0) wsum[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) sam_part(state)[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// ------------------------------------------------------------------------------------
// The perturbation on the same walk: every thread adds the SAM_WG partials in index order (one order: N and coef are the same
// value in every workgroup), then backup = p, p = p + e.  A tensor's last partial quad is read and written whole in `params` and the
// backup — its padding is copied, not changed — and element by element in `grads`.  Workgroup 0 also copies the BatchNorm state,
// the counters and the loss triple into the state, and its thread 0 updates the norm statistics (one owner, stream order).
// ------------------------------------------------------------------------------------
template <bool ASAM>
__device__ __forceinline__ float sam_step(float p, float g, float eta, float coef) {
#pragma clang fp contract(off)
  float t;
  const float u = sam_u<ASAM>(p, g, eta, t);
  float e;
  if constexpr (ASAM) { const float tu = t * u; e = coef * tu; }
  else e = coef * u;
  return p + e;
}
template <bool ASAM>
__global__ __launch_bounds__(SAM_THREADS) void sam_perturb_kernel(const SamArgs a, float* __restrict__ params, const float* __restrict__ grads,
                                                                  const float* __restrict__ bn_state, const int64_t* __restrict__ bn_count,
                                                                  const float* __restrict__ ws_loss, const FoldCtx fc) {
#pragma clang fp contract(off)
  FOLD_BEGIN; FS(params); FS(grads); FS(bn_state); FS(bn_count); FS(ws_loss);
  char* state = a.state + foff_;
  const double* part = sam_part(state);
  float* bk = sam_backup(state);
  const bool a16 = a.a16 != 0;
  const int tid = threadIdx.x, gt = (int)blockIdx.x * SAM_THREADS + tid, nt = SAM_WG * SAM_THREADS;
  double s = 0.0;
  for (int i = 0; i < SAM_WG; ++i) s += part[i];
  const double N = sqrt(s);
  const float coef = (float)((double)a.rho / (N + 1e-12));
  for (int ti = 0; ti < MSIG_NPARAM; ++ti) {
    const int off = a.off[ti], len = a.len[ti], n4 = len >> 2, rem = len & 3;
    for (int q = gt; q < n4; q += nt) {
      const int i = off + 4 * q;
      const float4 g = *(const float4*)(grads + i);
      float4 p = *(const float4*)(params + i);
      sam_store4(bk + i, p, a16);
      p.x = sam_step<ASAM>(p.x, g.x, a.eta, coef); p.y = sam_step<ASAM>(p.y, g.y, a.eta, coef);
      p.z = sam_step<ASAM>(p.z, g.z, a.eta, coef); p.w = sam_step<ASAM>(p.w, g.w, a.eta, coef);
      *(float4*)(params + i) = p;
    }
    if (rem && gt == ti) {
      const int i = off + 4 * n4;
      const float4 p = *(const float4*)(params + i);             // the layout pads every tensor to whole quads: in bounds
      sam_store4(bk + i, p, a16);
      float v[4] = {p.x, p.y, p.z, p.w};
      for (int e = 0; e < rem; ++e) v[e] = sam_step<ASAM>(v[e], grads[i + e], a.eta, coef);
      *(float4*)(params + i) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
  if (blockIdx.x != 0) return;
  float* bnb = bk + a.n_flat;
  int64_t* cnt = (int64_t*)(bnb + 96);
  float* lossb = (float*)(cnt + 2);
  if (tid < 96) bnb[tid] = bn_state[tid];
  else if (tid < 98) cnt[tid - 96] = bn_count[tid - 96];
  else if (tid < 101) lossb[tid - 98] = ws_loss[tid - 98];
  if (tid == 0) {
    double* st = (double*)state;
    st[MSIG_SAM_NORM_SUM] += N;
    st[MSIG_SAM_NORM_MAX] = N > st[MSIG_SAM_NORM_MAX] ? N : st[MSIG_SAM_NORM_MAX];
    st[MSIG_SAM_NORM_LAST] = N;
  }
}

// ------------------------------------------------------------------------------------
// The restore: every quad of the padded layout from the backup; workgroup 0 the BatchNorm state and counters, and its thread 0
// the sharpness statistics and the loss triple.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(SAM_THREADS) void sam_restore_kernel(const SamArgs a, float* __restrict__ params, float* __restrict__ bn_state,
                                                                  int64_t* __restrict__ bn_count, float* __restrict__ ws_loss, int B, const FoldCtx fc) {
  FOLD_BEGIN; FS(params); FS(bn_state); FS(bn_count); FS(ws_loss);
  char* state = a.state + foff_;
  const float* bk = sam_backup(state);
  const bool a16 = a.a16 != 0;
  const int tid = threadIdx.x, gt = (int)blockIdx.x * SAM_THREADS + tid, nt = SAM_WG * SAM_THREADS;
  const int nq = (int)(a.n_flat >> 2);
  for (int q = gt; q < nq; q += nt) *(float4*)(params + 4 * q) = sam_load4(bk + 4 * q, a16);
  if (blockIdx.x != 0) return;
  const float* bnb = bk + a.n_flat;
  const int64_t* cnt = (const int64_t*)(bnb + 96);
  const float* lossb = (const float*)(cnt + 2);
  if (tid < 96) bn_state[tid] = bnb[tid];
  else if (tid < 98) bn_count[tid - 96] = cnt[tid - 96];
  if (tid == 0) {
    double* st = (double*)state;
    const double d = (double)ws_loss[1] / (double)B - (double)lossb[1] / (double)B;
    st[MSIG_SAM_SHARP_SUM] += d;
    st[MSIG_SAM_SHARP_LAST] = d;
    st[MSIG_SAM_STEPS] += 1.0;
    ws_loss[0] = lossb[0]; ws_loss[1] = lossb[1]; ws_loss[2] = lossb[2];
  }
}

int launch_sam_perturb(const SamArgs& a, float* params, const float* grads, const float* bn_state, const int64_t* bn_count,
                       const float* ws_loss, const FoldCtx& fc, hipStream_t st) {
  const dim3 grid(SAM_WG, 1, fc.n);
  {
    MSIG_K("sam_sq", st);
    if (a.adaptive) sam_sq_kernel<true><<<grid, SAM_THREADS, 0, st>>>(a, params, grads, fc);
    else sam_sq_kernel<false><<<grid, SAM_THREADS, 0, st>>>(a, params, grads, fc);
  }
  MSIG_LAUNCH_CHECK();
  {
    MSIG_K("sam_perturb", st);
    if (a.adaptive) sam_perturb_kernel<true><<<grid, SAM_THREADS, 0, st>>>(a, params, grads, bn_state, bn_count, ws_loss, fc);
    else sam_perturb_kernel<false><<<grid, SAM_THREADS, 0, st>>>(a, params, grads, bn_state, bn_count, ws_loss, fc);
  }
  MSIG_LAUNCH_CHECK();
  return 0;
}

int launch_sam_restore(const SamArgs& a, float* params, float* bn_state, int64_t* bn_count, float* ws_loss, int B, const FoldCtx& fc,
                       hipStream_t st) {
  { MSIG_K("sam_restore", st); sam_restore_kernel<<<dim3(SAM_WG, 1, fc.n), SAM_THREADS, 0, st>>>(a, params, bn_state, bn_count, ws_loss, B, fc); }
  MSIG_LAUNCH_CHECK();
  return 0;
}

// ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
extern "C" int msig_sam_abi_version(void) { return MSIG_SAM_ABI_VERSION; }
extern "C" int64_t msig_sam_struct_bytes(void) { return (int64_t)sizeof(msig_sam); }

static int64_t sam_state_bytes(int64_t n_flat) {
  return (MSIG_SAM_NSTAT + SAM_WG) * (int64_t)sizeof(double) + n_flat * 4 + 96 * 4 + 2 * 8 + 4 * 4;
}
extern "C" int64_t msig_sam_state_bytes(int C, int K, int kind) {
  if (kind != MSIG_GC_KIND_ATTENTION && kind != MSIG_GC_KIND_CNN_GRU) return MSIG_E_SHAPE;
  int64_t off[MSIG_NPARAM + 1], len[MSIG_NPARAM];
  const int rc = msig_param_table(C, K, kind, off, len);
  return rc ? (int64_t)rc : sam_state_bytes(off[MSIG_NPARAM]);
}

// every check of msig_sam.h's own arguments, before any launch
int msig_sam_make_args(const msig_sam* s, int C, int K, SamArgs& a) {
  if (!s) return MSIG_E_NULL;
  if (s->kind != MSIG_GC_KIND_ATTENTION && s->kind != MSIG_GC_KIND_CNN_GRU) return MSIG_E_SHAPE;
  if (s->adaptive != 0 && s->adaptive != 1) return MSIG_E_SHAPE;
  if (!(s->rho >= 0.f) || !(s->eta >= 0.f)) return MSIG_E_SHAPE;                       // NaN included
  if (!s->state) return MSIG_E_NULL;
  if ((uintptr_t)s->state & 7) return MSIG_E_ALIGN;
  int64_t off[MSIG_NPARAM + 1], len[MSIG_NPARAM];
  const int rc = msig_param_table(C, K, s->kind, off, len);
  if (rc) return rc;
  if (s->state_bytes < sam_state_bytes(off[MSIG_NPARAM])) return MSIG_E_WORKSPACE;
  a = SamArgs{};
  a.adaptive = s->adaptive; a.rho = s->rho; a.eta = s->eta;
  a.state = (char*)s->state;
  a.a16 = ((uintptr_t)s->state & 15) == 0;       // the arenas of a fold batch are 256 bytes apart: one answer for every fold
  a.n_flat = off[MSIG_NPARAM];
  for (int i = 0; i < MSIG_NPARAM; ++i) { a.off[i] = (int32_t)off[i]; a.len[i] = (int32_t)len[i]; }
  return 0;
}

extern "C" int msig_sam_perturb(float* params, const float* grads, float* bn_state, int64_t* bn_count, const float* ws_loss, int C, int K,
                                const msig_sam* s, void* stream) {
  SamArgs a; int rc = msig_sam_make_args(s, C, K, a); if (rc) return rc;
  if (!params || !grads || !bn_state || !bn_count || !ws_loss) return MSIG_E_NULL;
  if (((uintptr_t)params | (uintptr_t)grads) & 15) return MSIG_E_ALIGN;
  if (msig_misaligned(bn_state, 3) || msig_misaligned(ws_loss, 3) || msig_misaligned(bn_count, 7)) return MSIG_E_ALIGN;
  return launch_sam_perturb(a, params, grads, bn_state, bn_count, ws_loss, single_fold(nullptr), (hipStream_t)stream);
}

extern "C" int msig_sam_restore(float* params, float* bn_state, int64_t* bn_count, float* ws_loss, int32_t B, int C, int K, const msig_sam* s,
                                void* stream) {
  SamArgs a; int rc = msig_sam_make_args(s, C, K, a); if (rc) return rc;
  if (!params || !bn_state || !bn_count || !ws_loss) return MSIG_E_NULL;
  if (B < 1) return MSIG_E_SHAPE;
  if ((uintptr_t)params & 15) return MSIG_E_ALIGN;
  if (msig_misaligned(bn_state, 3) || msig_misaligned(ws_loss, 3) || msig_misaligned(bn_count, 7)) return MSIG_E_ALIGN;
  return launch_sam_restore(a, params, bn_state, bn_count, ws_loss, B, single_fold(nullptr), (hipStream_t)stream);
}
