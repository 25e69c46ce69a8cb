// Weight averaging (include/msig_wa.h): one streaming launch that moves a model's shadow — a second copy of
// its parameters and BatchNorm statistics — towards the model, s += a * (p - s), for every fold of a call.  Every byte of the model
// is read once, every byte of the shadow read and written once; a fold's elements depend on that fold's two buffers and its own
// coefficient alone, so there is nothing to reduce and nothing to order.
#include "msig_dev.h"
#include "../../include/msig_wa.h"

int msig_multi_fold_ctx(const msig_multi* m, FoldCtx& fc);                                  // api.hip: msig_multi's own checks

struct WaCoef { float a[MSIG_MAX_FOLDS]; };

// Every fp32 operation below is ONE rounding: no FMA may be formed, or the result is no longer the numpy restatement's.  As in
// augment.hip (whose comment says why __fmul_rn and friends do not give that here), contraction is switched off for the rest of
// this file and the three operations are written out.
#pragma clang fp contract(off)
__device__ __forceinline__ float wa_lerp(float s, float p, float a) {
  const float d = p - s;
  const float t = a * d;
  return s + t;
}

#define WA_THREADS 256
#define WA_MAX_WG 256            // workgroups per fold: beyond it a thread takes several float4s

// grid: x = workgroups over the fold's n4 parameter float4s followed by its bn4 BatchNorm-state float4s (bn4 = 0: parameters only),
// z = fold.  The coefficient is uniform per workgroup (blockIdx.z and a kernel argument): the three cases are scalar branches.
__global__ __launch_bounds__(WA_THREADS) void wa_update_kernel(const float* __restrict__ params, const float* __restrict__ bn_state,
                                                               const int64_t* __restrict__ bn_count, float* __restrict__ avg_params,
                                                               float* __restrict__ avg_bn_state, int64_t* __restrict__ avg_bn_count,
                                                               int64_t n4, int bn4, const WaCoef coef, const FoldCtx fc) {
  const float a = coef.a[blockIdx.z];
  if (a == 0.f) return;                                    // the fold sits this update out: nothing of it is read or written
  FOLD_BEGIN; FS(params); FS(bn_state); FS(bn_count); FS(avg_params); FS(avg_bn_state); FS(avg_bn_count);
  const int64_t total = n4 + bn4, stride = (int64_t)gridDim.x * WA_THREADS;
  const bool copy = a == 1.f;
  for (int64_t j = (int64_t)blockIdx.x * WA_THREADS + threadIdx.x; j < total; j += stride) {
    const bool bn = j >= n4;
    const float4* p4 = bn ? (const float4*)bn_state + (j - n4) : (const float4*)params + j;
    float4* s4 = bn ? (float4*)avg_bn_state + (j - n4) : (float4*)avg_params + j;
    const float4 p = *p4;
    if (copy) { *s4 = p; continue; }
    const float4 s = *s4;
    *s4 = make_float4(wa_lerp(s.x, p.x, a), wa_lerp(s.y, p.y, a), wa_lerp(s.z, p.z, a), wa_lerp(s.w, p.w, a));
  }
  if (bn4 && blockIdx.x == 0 && threadIdx.x < 2) avg_bn_count[threadIdx.x] = bn_count[threadIdx.x];
}

static int wa_update(const msig_wa* w, const FoldCtx& fc, hipStream_t st) {
  if (!w || !w->params || !w->avg_params) return MSIG_E_NULL;
  const int nbn = (w->bn_state != nullptr) + (w->bn_count != nullptr) + (w->avg_bn_state != nullptr) + (w->avg_bn_count != nullptr);
  if (nbn != 0 && nbn != 4) return MSIG_E_NULL;
  if (w->n_flat < 4 || (w->n_flat & 3)) return MSIG_E_SHAPE;
  for (int z = 0; z < fc.n; ++z)
    if (!(w->coef[z] >= 0.f && w->coef[z] <= 1.f)) return MSIG_E_SHAPE;                    // NaN included
  if (w->avg_params == w->params || (nbn && w->avg_bn_state == w->bn_state)) return MSIG_E_SHAPE;
  if (((uintptr_t)w->params | (uintptr_t)w->avg_params | (uintptr_t)w->bn_state | (uintptr_t)w->avg_bn_state) & 15) return MSIG_E_ALIGN;
  if (((uintptr_t)w->bn_count | (uintptr_t)w->avg_bn_count) & 7) return MSIG_E_ALIGN;
  WaCoef coef{};
  bool any = false;
  for (int z = 0; z < fc.n; ++z) { coef.a[z] = w->coef[z]; any = any || w->coef[z] != 0.f; }
  if (!any) return 0;                                      // every fold sits it out: no launch
  const int64_t n4 = w->n_flat / 4;
  const int bn4 = nbn ? MSIG_BN_STATE_FLOATS / 4 : 0;
  int64_t wg = (n4 + bn4 + WA_THREADS - 1) / WA_THREADS;
  if (wg > WA_MAX_WG) wg = WA_MAX_WG;
  const dim3 grid((unsigned)wg, 1u, (unsigned)fc.n);
  {
    MSIG_K("wa_update", st);
    wa_update_kernel<<<grid, WA_THREADS, 0, st>>>(w->params, w->bn_state, w->bn_count, w->avg_params, w->avg_bn_state, w->avg_bn_count, n4,
                                                 bn4, coef, fc);
  }
  MSIG_LAUNCH_CHECK();
  return 0;
}

extern "C" int msig_wa_abi_version(void) { return MSIG_WA_ABI_VERSION; }
extern "C" int64_t msig_wa_struct_bytes(void) { return (int64_t)sizeof(msig_wa); }

extern "C" int msig_wa_update(const msig_wa* w, void* stream) { return wa_update(w, single_fold(nullptr), (hipStream_t)stream); }

extern "C" int msig_wa_update_multi(const msig_wa* w, const msig_multi* m, void* stream) {
  if (!w || !m) return MSIG_E_NULL;
  FoldCtx fc; const int rc = msig_multi_fold_ctx(m, fc); if (rc) return rc;
  return wa_update(w, fc, (hipStream_t)stream);
}
