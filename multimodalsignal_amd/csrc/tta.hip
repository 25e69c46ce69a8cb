// include/msig_tt.h: the two launches an entropy-minimisation step adds to an eval forward and its backward —
// the objective's gradient on MSIG_WS_LOGITS, and an Adam update that touches only the selected parameter tensors.  Both stream a
// few kilobytes: no MFMA, no LDS tiling.
#include <math.h>
#include "msig_dev.h"
#include "../../include/msig_tt.h"

#define TT_THREADS 256
#define TT_WAVES (TT_THREADS / 64)

int msig_multi_fold_ctx(const msig_multi* m, FoldCtx& fc);                                  // api.hip: msig_multi's own checks
int msig_param_table(int C, int K, int kind, int64_t* off, int64_t* len);                   // api.hip: the layout of a kind

// Negative control of the objective (make negctl TENT=1; never defined in the product library): the gradient without H_b, that is
// -p lp alone — finite, plausible and wrong at every row, uniform rows included (the parity cases of tests/test_entropy_adapt_gpu.py
// must FAIL against it; tools/negative_controls.sh tent).
#ifdef MSIG_NEGCTL_TENT
constexpr int msig_negctl_tent = MSIG_NEGCTL_TENT;
#else
constexpr int msig_negctl_tent = 0;
#endif

// One row in fp64: lp[k] and p[k] for k < K, its entropy and its first argmax.  Fully unrolled over MSIG_MAX_K so that the two
// arrays stay in registers.
__device__ __forceinline__ void tt_row(const float* __restrict__ lg, int K, double (&lp)[MSIG_MAX_K], double (&p)[MSIG_MAX_K], double& H, int& am) {
#pragma clang fp contract(off)
  double z[MSIG_MAX_K];
#pragma unroll
  for (int c = 0; c < MSIG_MAX_K; ++c) z[c] = c < K ? (double)lg[c] : 0.0;
  double m = z[0];
  am = 0;
#pragma unroll
  for (int c = 1; c < MSIG_MAX_K; ++c)
    if (c < K && z[c] > m) { m = z[c]; am = c; }
  double S = 0.0;
#pragma unroll
  for (int c = 0; c < MSIG_MAX_K; ++c)
    if (c < K) { z[c] = z[c] - m; S = S + exp(z[c]); }
  const double lnS = log(S);
  double h = 0.0;
#pragma unroll
  for (int c = 0; c < MSIG_MAX_K; ++c) {
    lp[c] = 0.0; p[c] = 0.0;
    if (c < K) {
      lp[c] = z[c] - lnS;
      p[c] = exp(lp[c]);
      h = h + p[c] * lp[c];
    }
  }
  H = -h;
}

// ------------------------------------------------------------------------------------
// The objective's gradient: one workgroup per fold (blockIdx.z), rows strided over the threads.  Pass 1 forms every row's p and H and
// the column sums of p (per thread in increasing row order, per wave by wave_sum_d, the four wave sums in wave order); q, ln q and Hq
// follow; pass 2 forms the rows again — the same instructions on the same inputs — and writes dlogits.  Nothing depends on the folds
// beside this one.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(TT_THREADS) void tt_objective_kernel(const float* __restrict__ logits, float* __restrict__ dlogits, double* stats,
                                                                  int B, int K, double div, const FoldCtx fc) {
#pragma clang fp contract(off)
  FOLD_BEGIN; FS(logits); FS(dlogits); FS(stats);
  __shared__ double red[2 * MSIG_MAX_K + 1][TT_WAVES];
  __shared__ double sh_lq[MSIG_MAX_K], sh_sum[2 * MSIG_MAX_K + 1];
  const int tid = threadIdx.x;
  double psum[MSIG_MAX_K], cnt[MSIG_MAX_K], hsum = 0.0;
#pragma unroll
  for (int c = 0; c < MSIG_MAX_K; ++c) { psum[c] = 0.0; cnt[c] = 0.0; }
  if (tid < (2 * MSIG_MAX_K + 1) * TT_WAVES) (&red[0][0])[tid] = 0.0;      // the rows of the classes beyond K stay zero
  __syncthreads();
  for (int row = tid; row < B; row += TT_THREADS) {
    double lp[MSIG_MAX_K], p[MSIG_MAX_K], H; int am;
    tt_row(logits + (size_t)row * K, K, lp, p, H, am);
    hsum = hsum + H;
#pragma unroll
    for (int c = 0; c < MSIG_MAX_K; ++c) { psum[c] = psum[c] + p[c]; cnt[c] += (c == am) ? 1.0 : 0.0; }
  }
#pragma unroll
  for (int c = 0; c < MSIG_MAX_K; ++c) {
    if (c < K) {                                   // K is uniform over the workgroup: every lane takes part in the butterfly
      const double a = wave_sum_d(psum[c]), n = wave_sum_d(cnt[c]);
      if ((tid & 63) == 0) { red[c][tid >> 6] = a; red[MSIG_MAX_K + c][tid >> 6] = n; }
    }
  }
  hsum = wave_sum_d(hsum);
  if ((tid & 63) == 0) red[2 * MSIG_MAX_K][tid >> 6] = hsum;
  __syncthreads();
  if (tid < 2 * MSIG_MAX_K + 1) {
    double s = 0.0;
    for (int i = 0; i < TT_WAVES; ++i) s = s + red[tid][i];
    sh_sum[tid] = s;
    if (tid < MSIG_MAX_K) {
      const double q = s / (double)B;
      sh_lq[tid] = (tid >= K || q == 0.0) ? 0.0 : log(q);      // a NaN q is not 0: its logarithm is taken and propagates
    }
  }
  __syncthreads();
  double lq[MSIG_MAX_K];
#pragma unroll
  for (int c = 0; c < MSIG_MAX_K; ++c) lq[c] = sh_lq[c];
  const double dB = (double)B;
  for (int row = tid; row < B; row += TT_THREADS) {
    double lp[MSIG_MAX_K], p[MSIG_MAX_K], H; int am;
    tt_row(logits + (size_t)row * K, K, lp, p, H, am);
    double cb = 0.0;
#pragma unroll
    for (int c = 0; c < MSIG_MAX_K; ++c) cb = cb + p[c] * lq[c];
    float* __restrict__ dl = dlogits + (size_t)row * K;
#pragma unroll
    for (int c = 0; c < MSIG_MAX_K; ++c) {
      if (c < K) {
        const double ent = msig_negctl_tent == 1 ? -(p[c] * lp[c]) : -(p[c] * (lp[c] + H));
        const double dv = div * (p[c] * (lq[c] - cb));
        dl[c] = (float)((ent + dv) / dB);
      }
    }
  }
  if (stats && tid == 0) {
    double hq = 0.0;
    for (int c = 0; c < K; ++c) { const double q = sh_sum[c] / dB; hq = hq + q * sh_lq[c]; }
    stats[MSIG_TT_S_ENT] += sh_sum[2 * MSIG_MAX_K]; stats[MSIG_TT_S_ROWS] += dB;
    stats[MSIG_TT_S_HQ] += -hq; stats[MSIG_TT_S_STEPS] += 1.0;
    for (int c = 0; c < K; ++c) { stats[MSIG_TT_S_P + c] += sh_sum[c]; stats[MSIG_TT_S_PRED + c] += sh_sum[MSIG_MAX_K + c]; }
  }
}

int launch_tt_objective(const float* logits, float* dlogits, double* stats, int B, int K, float div, const FoldCtx& fc, hipStream_t st) {
  { MSIG_K("tt_objective", st); tt_objective_kernel<<<dim3(1, 1, fc.n), TT_THREADS, 0, st>>>(logits, dlogits, stats, B, K, (double)div, fc); }
  MSIG_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------
// The selective Adam: adam_kernel's statements (head.hip; msig_dev.h ADAM_FUSED_V), four elements per thread, over the float4s of the
// selected tensors' slots only.  sel lists the slots as (first float4, running count); a thread finds the slot of its i-th selected
// float4 by walking the at most MSIG_NPARAM entries.  Learning rate and bias correction per fold (blockIdx.z).
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tt_adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                      const TtSel sel, float b1, float b2, float eps, float wd, const FoldCtx fc) {
  FOLD_BEGIN; FS(p); FS(g); FS(m); FS(v);
  const float lr_over_bc1 = fc.lr_over_bc1[blockIdx.z], inv_sqrt_bc2 = fc.inv_sqrt_bc2[blockIdx.z];
  for (int s = blockIdx.x * 256 + threadIdx.x; s < sel.total4; s += gridDim.x * 256) {
    int r = 0;
    while (r < sel.n - 1 && s >= sel.cum4[r]) ++r;
    const int64_t i = (int64_t)sel.first4[r] + (s - (r ? sel.cum4[r - 1] : 0));
    float4 pp = ((float4*)p)[i], mm = ((float4*)m)[i], vv = ((float4*)v)[i];
    const float4 gg = ((const float4*)g)[i];
    float pa[4] = {pp.x, pp.y, pp.z, pp.w}, ma[4] = {mm.x, mm.y, mm.z, mm.w}, va[4] = {vv.x, vv.y, vv.z, vv.w};
    const float ga[4] = {gg.x, gg.y, gg.z, gg.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) pa[e] = adam_update<ADAM_FUSED_V>(pa[e], ga[e], ma[e], va[e], lr_over_bc1, inv_sqrt_bc2, b1, b2, eps, wd);
    ((float4*)p)[i] = make_float4(pa[0], pa[1], pa[2], pa[3]);
    ((float4*)m)[i] = make_float4(ma[0], ma[1], ma[2], ma[3]);
    ((float4*)v)[i] = make_float4(va[0], va[1], va[2], va[3]);
  }
}

// the selected tensors' slots of the layout of (C, K, kind); MSIG_E_SHAPE for a bad kind or selection
int msig_tt_make_sel(int C, int K, int kind, uint32_t select, TtSel& sel) {
  if (kind != MSIG_FT_KIND_ATTENTION && kind != MSIG_FT_KIND_CNN_GRU) return MSIG_E_SHAPE;
  if (select == 0 || (select >> MSIG_NPARAM) != 0) return MSIG_E_SHAPE;
  int64_t off[MSIG_NPARAM + 1], len[MSIG_NPARAM];
  const int rc = msig_param_table(C, K, kind, off, len);
  if (rc) return rc;
  sel = TtSel{};
  int total = 0;
  for (int t = 0; t < MSIG_NPARAM; ++t) {
    const int n4 = (int)((off[t + 1] - off[t]) / 4);       // offsets are multiples of 4: a slot is whole float4s
    if (!((select >> t) & 1u) || n4 == 0) continue;
    total += n4;
    sel.first4[sel.n] = (int32_t)(off[t] / 4); sel.cum4[sel.n] = total; ++sel.n;
  }
  sel.total4 = total;
  return 0;
}

// fc.lr_over_bc1 / inv_sqrt_bc2 are the folds' (filled by the caller: msig_tt_fill_adam)
int launch_tt_adam(float* p, const float* g, float* m, float* v, const TtSel& sel, float b1, float b2, float eps, float wd, const FoldCtx& fc,
                   hipStream_t st) {
  if (sel.total4 == 0) return 0;                       // the selection names only empty tensors (the gate of a cnn_gru model)
  int blocks = (sel.total4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  { MSIG_K("tt_adam", st); tt_adam_kernel<<<dim3(blocks, 1, fc.n), 256, 0, st>>>(p, g, m, v, sel, b1, b2, eps, wd, fc); }
  MSIG_LAUNCH_CHECK();
  return 0;
}

// Adam's bias corrections per fold, formed on the host as train_step_fc forms them (and launch_adam for one model)
void msig_tt_fill_adam(FoldCtx& fc, const float* lrs, const int64_t* steps, int64_t step, float beta1, float beta2) {
  for (int i = 0; i < fc.n; ++i) {
    const double s_i = (double)((steps && steps[i] > 0) ? steps[i] : step);
    const double bc1 = 1.0 - pow((double)beta1, s_i), bc2 = 1.0 - pow((double)beta2, s_i);
    fc.lr_over_bc1[i] = (float)((double)lrs[i] / bc1);
    fc.inv_sqrt_bc2[i] = (float)(1.0 / sqrt(bc2));
  }
}

// ---- the C ABI (the step itself is api.hip's: it runs the forward's and the backward's launchers) -----------------------------------
extern "C" int msig_tt_abi_version(void) { return MSIG_TT_ABI_VERSION; }
extern "C" int64_t msig_tt_struct_bytes(void) { return (int64_t)sizeof(msig_tt); }

bool msig_tt_bad_diversity(float div) { return !(div >= 0.f && div <= 3.0e38f); }      // NaN and infinity included

static int tt_objective(const float* logits, int32_t B, int32_t K, float div, float* dlogits, double* stats, const FoldCtx& fc, hipStream_t st) {
  if (!logits || !dlogits) return MSIG_E_NULL;
  if (B < 1 || B > MSIG_TT_MAX_BATCH || K < 2 || K > MSIG_MAX_K || msig_tt_bad_diversity(div)) return MSIG_E_SHAPE;
  if (msig_misaligned(logits, 3) || msig_misaligned(dlogits, 3) || msig_misaligned(stats, 7)) return MSIG_E_ALIGN;
  return launch_tt_objective(logits, dlogits, stats, B, K, div, fc, st);
}
extern "C" int msig_tt_objective(const float* logits, int32_t B, int32_t K, float diversity, float* dlogits, double* stats, void* stream) {
  return tt_objective(logits, B, K, diversity, dlogits, stats, single_fold(nullptr), (hipStream_t)stream);
}
extern "C" int msig_tt_objective_multi(const float* logits, int32_t B, int32_t K, float diversity, float* dlogits, double* stats,
                                       const msig_multi* m, void* stream) {
  if (!m) return MSIG_E_NULL;
  FoldCtx fc; const int rc = msig_multi_fold_ctx(m, fc); if (rc) return rc;
  return tt_objective(logits, B, K, diversity, dlogits, stats, fc, (hipStream_t)stream);
}

static int tt_adam(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int32_t C, int32_t K, int32_t kind, uint32_t select,
                   const float* lrs, const int64_t* steps, float beta1, float beta2, float eps, float wd, int64_t step, FoldCtx fc, hipStream_t st) {
  if (!params || !grads || !exp_avg || !exp_avg_sq) return MSIG_E_NULL;
  TtSel sel; const int rc = msig_tt_make_sel(C, K, kind, select, sel); if (rc) return rc;
  if (step < 1) return MSIG_E_SHAPE;
  if (steps)
    for (int i = 0; i < fc.n; ++i) if (steps[i] < 0) return MSIG_E_SHAPE;
  if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) return MSIG_E_ALIGN;
  msig_tt_fill_adam(fc, lrs, steps, step, beta1, beta2);
  return launch_tt_adam(params, grads, exp_avg, exp_avg_sq, sel, beta1, beta2, eps, wd, fc, st);
}
extern "C" int msig_tt_adam(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int32_t C, int32_t K, int32_t kind,
                            uint32_t select, float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, void* stream) {
  return tt_adam(params, grads, exp_avg, exp_avg_sq, C, K, kind, select, &lr, nullptr, beta1, beta2, eps, weight_decay, step, single_fold(nullptr),
                 (hipStream_t)stream);
}
extern "C" int msig_tt_adam_multi(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int32_t C, int32_t K, int32_t kind,
                                  uint32_t select, float beta1, float beta2, float eps, float weight_decay, int64_t step, const msig_multi* m,
                                  void* stream) {
  if (!m) return MSIG_E_NULL;
  FoldCtx fc; const int rc = msig_multi_fold_ctx(m, fc); if (rc) return rc;
  return tt_adam(params, grads, exp_avg, exp_avg_sq, C, K, kind, select, m->lr, m->step, beta1, beta2, eps, weight_decay, step, fc, (hipStream_t)stream);
}
