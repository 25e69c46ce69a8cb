// include/msig_kd.h: the teacher table of an ensemble's tempered probabilities and the distillation term of a train step — one
// launch between ce_kernel and head_bwd_kernel that blends the teacher's gradient into MSIG_WS_DLOGITS.
// Both kernels stream: a few hundred bytes per row, no MFMA, no LDS tiling.
#include "member_stats.h"

#define KD_THREADS 256

int msig_multi_fold_ctx(const msig_multi* m, FoldCtx& fc);                                  // api.hip: msig_multi's own checks

// Teacher: member_stats (member_stats.h) on the logits over T, its mean alone — q[n][k] rounded to fp32 on store
__global__ __launch_bounds__(MEMBER_THREADS) void kd_teacher_kernel(const float* __restrict__ logits, const MemberWhere wh, int M, int K,
                                                                    double T, float* __restrict__ q) {
  member_stats<true, MEMBER_MEAN, false>(logits, wh, M, K, T, q, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

// ------------------------------------------------------------------------------------
// The distillation term: one workgroup per fold (blockIdx.z), rows strided over the threads like ce_kernel.  Per row, fp32 with one
// rounding per operation (contraction off): the blended teacher row qm, s = softmax(z / T), dlogits = (1 - alpha) dlogits +
// kappa (s - qm) in place.  Then the row's fp64 KL term and whether the student's first argmax is the teacher's; per thread in
// increasing row order, per wave, and the four wave sums in wave order by thread 0.  Nothing depends on the folds beside this one.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(KD_THREADS) void kd_apply_kernel(const KdArgs a, const float* __restrict__ logits, float* __restrict__ dlogits,
                                                              const FoldCtx fc) {
#pragma clang fp contract(off)
  FOLD_BEGIN; FS(logits); FS(dlogits);
  const int z = blockIdx.z;
  const int64_t koff = (int64_t)fc.slot[z] * a.stride;
  const float* __restrict__ q = (const float*)((const char*)a.q + koff);
  double* stats = a.stats ? (double*)((char*)a.stats + koff) : nullptr;
  const int64_t* __restrict__ idx = a.idx ? a.idx + (int64_t)z * a.idx_row_stride : nullptr;
  const int B = a.B, K = a.K;
  const float lam = a.lam[z], mu = 1.f - lam;
  const float T = a.T, om = a.om, kappa = a.kappa;
  __shared__ double red[2][KD_THREADS / 64];
  const int tid = threadIdx.x;
  double lsum = 0.0, agree = 0.0;
  for (int row = tid; row < B; row += KD_THREADS) {
    const float* __restrict__ qa = q + (idx ? idx[row] : (int64_t)row) * K;
    float qm[MSIG_MAX_K], u[MSIG_MAX_K];
    if (lam == 1.f) {
      for (int c = 0; c < K; ++c) qm[c] = qa[c];
    } else {
      const float* __restrict__ qb = q + (idx ? idx[B - 1 - row] : (int64_t)(B - 1 - row)) * K;
      for (int c = 0; c < K; ++c) {
        const float own = lam * qa[c], par = mu * qb[c];
        qm[c] = own + par;
      }
    }
    const float* __restrict__ lg = logits + (size_t)row * K;
    float* __restrict__ dl = dlogits + (size_t)row * K;
    int az = 0, aq = 0;
    for (int c = 1; c < K; ++c) {
      if (lg[c] > lg[az]) az = c;
      if (qm[c] > qm[aq]) aq = c;
    }
    for (int c = 0; c < K; ++c) u[c] = lg[c] / T;
    float m = u[0];
    for (int c = 1; c < K; ++c) if (u[c] > m) m = u[c];
    float S = 0.f;
    for (int c = 0; c < K; ++c) { u[c] = u[c] - m; S = S + expf(u[c]); }
    const double lnS = log((double)S);
    double term = 0.0;
    for (int c = 0; c < K; ++c) {
      const float s = expf(u[c]) / S;
      const float keep = om * dl[c], add = kappa * (s - qm[c]);
      dl[c] = keep + add;
      if (qm[c] > 0.f) {
        const double qd = (double)qm[c];
        const double t = qd * (log(qd) - ((double)u[c] - lnS));
        term = term + t;
      }
    }
    lsum = lsum + term;
    agree += (az == aq) ? 1.0 : 0.0;
  }
  if (!stats) return;
  lsum = wave_sum_d(lsum); agree = wave_sum_d(agree);
  if ((tid & 63) == 0) { red[0][tid >> 6] = lsum; red[1][tid >> 6] = agree; }
  __syncthreads();
  if (tid == 0) {
    double ls = 0.0, cs = 0.0;
    for (int i = 0; i < KD_THREADS / 64; ++i) { ls = ls + red[0][i]; cs = cs + red[1][i]; }
    const double scaled = a.t2 * ls;
    stats[0] += scaled; stats[1] += cs; stats[2] += (double)B;
  }
}

int launch_kd_apply(const KdArgs& a, const float* logits, float* dlogits, const FoldCtx& fc, hipStream_t st) {
  { MSIG_K("kd_apply", st); kd_apply_kernel<<<dim3(1, 1, fc.n), KD_THREADS, 0, st>>>(a, logits, dlogits, fc); }
  MSIG_LAUNCH_CHECK();
  return 0;
}

// ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
static inline bool kd_bad_temperature(float T) { return !(T >= 1.f / 64.f && T <= 64.f); }      // NaN included

extern "C" int msig_kd_abi_version(void) { return MSIG_KD_ABI_VERSION; }
extern "C" int64_t msig_kd_struct_bytes(void) { return (int64_t)sizeof(msig_kd); }

int msig_kd_make_args(const msig_kd* k, const FoldCtx& fc, int32_t B, int32_t K, const float* lam, KdArgs& kd) {
  if (!k || !lam) return MSIG_E_NULL;
  if (!k->q) return MSIG_E_NULL;
  if (!(k->alpha >= 0.f && k->alpha <= 1.f)) return MSIG_E_SHAPE;                              // NaN included
  if (kd_bad_temperature(k->temperature)) return MSIG_E_SHAPE;
  if (K < 2 || K > MSIG_MAX_K || B < 1) return MSIG_E_SHAPE;
  const bool multi = fc.stride != 0;
  if (multi && k->idx && k->idx_row_stride < B) return MSIG_E_SHAPE;
  kd = KdArgs{};
  for (int i = 0; i < fc.n; ++i) {
    if (!(lam[i] >= 0.f && lam[i] <= 1.f)) return MSIG_E_SHAPE;
    kd.lam[i] = lam[i];
  }
  if (msig_misaligned(k->q, 3)) return MSIG_E_ALIGN;
  if (msig_misaligned(k->stats, 7) || msig_misaligned(k->idx, 7)) return MSIG_E_ALIGN;
  if (multi && (k->stride_bytes <= 0 || (k->stride_bytes & 255))) return MSIG_E_ALIGN;
  kd.B = B; kd.K = K;
  kd.q = k->q; kd.idx = k->idx; kd.idx_row_stride = multi ? k->idx_row_stride : 0;
  kd.stats = k->stats;
  kd.stride = multi ? k->stride_bytes : 0;
  kd.alpha = k->alpha; kd.T = k->temperature;
  kd.om = 1.f - k->alpha;
  kd.kappa = (float)((double)k->alpha * (double)k->temperature / (double)B);
  kd.t2 = (double)k->temperature * (double)k->temperature;
  return 0;
}

static int kd_apply(const msig_kd* k, const FoldCtx& fc, const float* logits, float* dlogits, int32_t B, int32_t K, const float* lam,
                    hipStream_t st) {
  if (!logits || !dlogits) return MSIG_E_NULL;
  KdArgs kd; int rc = msig_kd_make_args(k, fc, B, K, lam, kd); if (rc) return rc;
  if (msig_misaligned(logits, 3) || msig_misaligned(dlogits, 3)) return MSIG_E_ALIGN;
  return launch_kd_apply(kd, logits, dlogits, fc, st);
}
extern "C" int msig_kd_apply(const msig_kd* kd, const float* logits, float* dlogits, int32_t B, int32_t K, float lam, void* stream) {
  return kd_apply(kd, single_fold(nullptr), logits, dlogits, B, K, &lam, (hipStream_t)stream);
}
extern "C" int msig_kd_apply_multi(const msig_kd* kd, const msig_multi* m, const float* logits, float* dlogits, int32_t B, int32_t K,
                                   const float* lam, void* stream) {
  if (!kd || !m) return MSIG_E_NULL;
  FoldCtx fc; int rc = msig_multi_fold_ctx(m, fc); if (rc) return rc;
  return kd_apply(kd, fc, logits, dlogits, B, K, lam, (hipStream_t)stream);
}

static int kd_teacher(const float* logits, const MemberWhere& wh, int32_t M, int32_t max_members, int32_t N, int32_t K, float T, float* q,
                      void* stream) {
  return member_launch("kd_teacher", logits, M, max_members, N, K, wh.member_stride < (int64_t)N * K || kd_bad_temperature(T), {q},
                       (hipStream_t)stream, [&](dim3 grid, dim3 block, hipStream_t st) {
                         kd_teacher_kernel<<<grid, block, 0, st>>>(logits, wh, M, K, (double)T, q);
                       });
}
extern "C" int msig_kd_teacher(const float* logits, int64_t member_stride_floats, int32_t M, int32_t N, int32_t K, float T, float* q,
                               void* stream) {
  return kd_teacher(logits, member_where_stacked(member_stride_floats), M, MSIG_KD_MAX_MEMBERS, N, K, T, q, stream);
}
extern "C" int msig_kd_teacher_multi(const float* logits0, const msig_multi* m, int32_t N, int32_t K, float T, float* q, void* stream) {
  FoldCtx fc; const int rc = msig_multi_fold_ctx(m, fc); if (rc) return rc;
  return kd_teacher(logits0, member_where_from_multi(fc), fc.n, MSIG_MAX_FOLDS, N, K, T, q, stream);
}
