// include/msig_dro.h: group-DRO — one launch between ce_kernel and kd_apply_kernel / head_bwd_kernel that moves the fold's group
// weights q with the groups' losses and rescales every row of MSIG_WS_DLOGITS by q_g W / W_g.  A few hundred
// bytes per row, no MFMA, no atomics; the group sums run in row order out of LDS.
#include "msig_dev.h"
#include "../../include/msig_dro.h"

#define DRO_THREADS 256

int msig_multi_fold_ctx(const msig_multi* m, FoldCtx& fc);                                  // api.hip: msig_multi's own checks

// One workgroup per fold (blockIdx.z).
//   1  rows strided over the threads: t_b and m_b in fp64 and g_b into LDS (a row's K logits are read once)
//   2  thread g < G sums its group over the rows in increasing b (every lane reads the same LDS address: a broadcast); thread
//      MSIG_DRO_MAX_GROUPS, the first of the second wave, forms W the same way
//   3  thread 0: present groups, the update and normalisation of q in increasing g, the stats, the groups' fp32 factors
//   4  rows strided over the threads: dlogits *= r_b
// LDS: 2048 x (8 + 8 + 4) + 64 x (8 + 8 + 8 + 4 + 4) + 16 bytes = 43 024.
__global__ __launch_bounds__(DRO_THREADS) void dro_apply_kernel(const DroArgs a, const float* __restrict__ logits,
                                                                const int64_t* __restrict__ labels, const float* __restrict__ cw,
                                                                float* __restrict__ dlogits, const FoldCtx fc) {
#pragma clang fp contract(off)
  FOLD_BEGIN; FS(logits); FS(labels); FS(cw); FS(dlogits);
  const int z = blockIdx.z;
  const int64_t goff = (int64_t)fc.slot[z] * a.stride;
  const int32_t* __restrict__ grp = (const int32_t*)((const char*)a.grp + goff);
  float* q = (float*)((char*)a.q + goff);
  double* stats = a.stats ? (double*)((char*)a.stats + goff) : nullptr;
  const int64_t* __restrict__ idx = a.idx ? a.idx + (int64_t)z * a.idx_row_stride : nullptr;
  const int B = a.B, K = a.K, G = a.G;
  __shared__ double s_t[MSIG_DRO_MAX_BATCH], s_m[MSIG_DRO_MAX_BATCH];
  __shared__ int32_t s_g[MSIG_DRO_MAX_BATCH];
  __shared__ double s_T[MSIG_DRO_MAX_GROUPS], s_W[MSIG_DRO_MAX_GROUPS], s_Wall;
  __shared__ int32_t s_n[MSIG_DRO_MAX_GROUPS];
  __shared__ double s_q[MSIG_DRO_MAX_GROUPS];
  __shared__ float s_r[MSIG_DRO_MAX_GROUPS];
  __shared__ int32_t s_any;
  const int tid = threadIdx.x;
  const double eps = (double)a.eps, keep = 1.0 - eps, spread = eps / (double)K;

  // ---- 1: the rows' terms --------------------------------------------------------------------------------------------------------
  for (int row = tid; row < B; row += DRO_THREADS) {
    const int64_t y = labels[row];
    int32_t g = grp[idx ? idx[row] : (int64_t)row];
    double t = 0.0, m = 0.0;
    if (y < 0 || y >= K) g = -1;
    else {
      const float* __restrict__ lg = logits + (size_t)row * K;
      float zf[MSIG_MAX_K];                          // guarded full unrolls: the row stays in registers
#pragma unroll
      for (int c = 0; c < MSIG_MAX_K; ++c) zf[c] = c < K ? lg[c] : 0.f;
      float mx = zf[0];
#pragma unroll
      for (int c = 1; c < MSIG_MAX_K; ++c) if (c < K && zf[c] > mx) mx = zf[c];
      double S = 0.0;
#pragma unroll
      for (int c = 0; c < MSIG_MAX_K; ++c) if (c < K) S = S + exp((double)zf[c] - (double)mx);
      const double lnS = log(S);
      double all = 0.0, own = 0.0;
#pragma unroll
      for (int c = 0; c < MSIG_MAX_K; ++c) if (c < K) {
        const double l = -(((double)zf[c] - (double)mx) - lnS);
        const double wl = (cw ? (double)cw[c] : 1.0) * l;
        all = all + wl;
        if (c == (int)y) own = wl;
      }
      m = cw ? (double)cw[y] : 1.0;
      const double hard = keep * own, soft = spread * all;
      t = hard + soft;
    }
    if (g < 0 || g >= G) g = -1;
    s_t[row] = t; s_m[row] = m; s_g[row] = g;
  }
  __syncthreads();

  // ---- 2: the groups' sums, each by one thread in row order ---------------------------------------------------------------------
  if (tid < G) {
    double T = 0.0, W = 0.0; int n = 0;
#pragma unroll 4
    for (int row = 0; row < B; ++row) {
      const bool in = s_g[row] == tid;
      const double t = in ? s_t[row] : 0.0, m = in ? s_m[row] : 0.0;
      T = T + t; W = W + m; n += in ? 1 : 0;
    }
    s_T[tid] = T; s_W[tid] = W; s_n[tid] = n;
  } else if (tid == MSIG_DRO_MAX_GROUPS) {
    double W = 0.0;
#pragma unroll 4
    for (int row = 0; row < B; ++row) W = W + s_m[row];
    s_Wall = W;
  }
  __syncthreads();

  // ---- 3: q, the stats, the groups' factors ---------------------------------------------------------------------------------------
  if (tid == 0) {
    int any = 0;
    for (int g = 0; g < G; ++g) any |= (s_n[g] > 0 && s_W[g] > 0.0) ? 1 : 0;
    s_any = any;
    if (any) {
      const double W = s_Wall, eta = (double)a.eta;
      double Z = 0.0;
      if (!a.frozen) {
        for (int g = 0; g < G; ++g) {
          const bool present = s_n[g] > 0 && s_W[g] > 0.0;
          double v = (double)q[g];
          if (present) { const double L = s_T[g] / s_W[g]; const double up = exp(eta * L); v = v * up; }
          s_q[g] = v; Z = Z + v;
        }
      }
      double robust = 0.0;
      for (int g = 0; g < G; ++g) {
        const bool present = s_n[g] > 0 && s_W[g] > 0.0;
        float qf;
        if (a.frozen) qf = q[g];
        else { qf = (float)(s_q[g] / Z); q[g] = qf; }
        float r = 0.f;
        if (present) {
          const double num = (double)qf * W;
          r = (float)(num / s_W[g]);
          const double L = s_T[g] / s_W[g];
          const double term = (double)qf * L;
          robust = robust + term;
        }
        s_r[g] = r;
      }
      if (stats && !a.frozen) {
        for (int g = 0; g < G; ++g)
          if (s_n[g] > 0) {
            stats[g] += s_T[g]; stats[MSIG_DRO_MAX_GROUPS + g] += s_W[g]; stats[2 * MSIG_DRO_MAX_GROUPS + g] += (double)s_n[g];
          }
        stats[3 * MSIG_DRO_MAX_GROUPS] += robust; stats[3 * MSIG_DRO_MAX_GROUPS + 1] += 1.0;
      }
    }
  }
  __syncthreads();
  if (!s_any) return;

  // ---- 4: the rows' gradients ------------------------------------------------------------------------------------------------------
  for (int row = tid; row < B; row += DRO_THREADS) {
    const int g = s_g[row];
    const float r = g >= 0 ? s_r[g] : 0.f;
    float* __restrict__ dl = dlogits + (size_t)row * K;
    for (int c = 0; c < K; ++c) dl[c] = r * dl[c];
  }
}

int launch_dro_apply(const DroArgs& a, const float* logits, const int64_t* labels, const float* cw, float* dlogits, const FoldCtx& fc,
                     hipStream_t st) {
  { MSIG_K("dro_apply", st); dro_apply_kernel<<<dim3(1, 1, fc.n), DRO_THREADS, 0, st>>>(a, logits, labels, cw, dlogits, fc); }
  MSIG_LAUNCH_CHECK();
  return 0;
}

// ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
extern "C" int msig_dro_abi_version(void) { return MSIG_DRO_ABI_VERSION; }
extern "C" int64_t msig_dro_struct_bytes(void) { return (int64_t)sizeof(msig_dro); }

int msig_dro_make_args(const msig_dro* k, const FoldCtx& fc, int32_t B, int32_t K, float smoothing, DroArgs& a) {
  if (!k) return MSIG_E_NULL;
  if (!k->grp || !k->q) return MSIG_E_NULL;
  if (k->G < 1 || k->G > MSIG_DRO_MAX_GROUPS) return MSIG_E_SHAPE;
  if (!(k->eta >= 0.f)) return MSIG_E_SHAPE;                                                   // NaN included
  if (K < 2 || K > MSIG_MAX_K) return MSIG_E_SHAPE;
  if (B < 1 || B > MSIG_DRO_MAX_BATCH) return MSIG_E_SHAPE;
  if (!(smoothing >= 0.f && smoothing < 1.f)) return MSIG_E_SHAPE;
  const bool multi = fc.stride != 0;
  if (multi && k->idx && k->idx_row_stride < B) return MSIG_E_SHAPE;
  if (msig_misaligned(k->q, 3) || msig_misaligned(k->grp, 3)) return MSIG_E_ALIGN;
  if (msig_misaligned(k->stats, 7) || msig_misaligned(k->idx, 7)) return MSIG_E_ALIGN;
  if (multi && (k->stride_bytes <= 0 || (k->stride_bytes & 255))) return MSIG_E_ALIGN;
  a = DroArgs{};
  a.G = k->G; a.B = B; a.K = K; a.frozen = k->frozen != 0;
  a.eta = k->eta; a.eps = smoothing;
  a.grp = k->grp; a.idx = k->idx; a.idx_row_stride = multi ? k->idx_row_stride : 0;
  a.q = k->q; a.stats = k->stats;
  a.stride = multi ? k->stride_bytes : 0;
  return 0;
}

static int dro_apply(const msig_dro* k, const FoldCtx& fc, const float* logits, const int64_t* labels, const float* cw, float smoothing,
                     float* dlogits, int32_t B, int32_t K, hipStream_t st) {
  if (!k) return MSIG_E_NULL;
  if (!k->grp || !k->q || !logits || !labels || !dlogits) return MSIG_E_NULL;
  DroArgs a; int rc = msig_dro_make_args(k, fc, B, K, smoothing, a); if (rc) return rc;
  if (msig_misaligned(logits, 3) || msig_misaligned(dlogits, 3) || msig_misaligned(cw, 3) || msig_misaligned(labels, 7)) return MSIG_E_ALIGN;
  return launch_dro_apply(a, logits, labels, cw, dlogits, fc, st);
}
extern "C" int msig_dro_apply(const msig_dro* dro, const float* logits, const int64_t* labels, const float* class_weight, float smoothing,
                              float* dlogits, int32_t B, int32_t K, void* stream) {
  return dro_apply(dro, single_fold(nullptr), logits, labels, class_weight, smoothing, dlogits, B, K, (hipStream_t)stream);
}
extern "C" int msig_dro_apply_multi(const msig_dro* dro, const msig_multi* m, const float* logits, const int64_t* labels,
                                    const float* class_weight, float smoothing, float* dlogits, int32_t B, int32_t K, void* stream) {
  if (!dro || !m) return MSIG_E_NULL;
  FoldCtx fc; int rc = msig_multi_fold_ctx(m, fc); if (rc) return rc;
  return dro_apply(dro, fc, logits, labels, class_weight, smoothing, dlogits, B, K, (hipStream_t)stream);
}
