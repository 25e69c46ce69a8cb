// include/msig_da.h: the subject discriminator's step — forward, CrossEntropy against the rows' domain labels, backward, Adam on
// its own parameters and the REVERSED feature gradient added to MSIG_WS_DFEAT — in ONE launch between the head and the GRU backward
// of a fused train step.
#include "msig_dev.h"
#include "head_mlp.h"

// ------------------------------------------------------------------------------------
// One workgroup of 256 threads per fold (blockIdx.z), B <= MSIG_DA_MAX_BATCH rows, the thread map of head_epoch_kernel
// (finetune.hip) and the classifier's pieces (head_mlp.h): D's 9.3 k floats sit in LDS for the call, every element of W0 / b0 /
// W3 / b3 has ONE owner thread that accumulates its gradient over the rows in batch order and applies Adam,
//   W0 (64,128): thread (kcol = tid & 127, half = tid >> 7) owns rows half * 32 + j, j < 32, of column kcol; TRANSPOSED in LDS,
//                W0t[k * 65 + v]: the forward (lane = v), the owners and the feature gradient (lane = k, stride 65) all reach it
//                without a bank conflict;
//   W3 (S,64)  : thread tid owns elements tid + 256 * j, j < 4 (rows at stride 65 in LDS);   b0: tid < 64;   b3: tid < S;
// and rows run in chunks of 16, in batch order.  The feature gradient g[row][k] = sum_v W0[v][k] dpre[row][v] of a chunk is taken
// by thread (kcol, half) for rows half * 8 + r, r < 8, from the parameters as the launch found them (they are updated after the
// last chunk).  n and the loss are fp64 sums, lane = row, wave reduction, the four wave sums in wave order.  Nothing depends on the
// folds beside this one.  Plain fp32 FMA, no MFMA: 5 x 131 k multiply-adds per 16 rows are about a microsecond of arithmetic on four
// waves; the launch is bound by its seven barriers per chunk, the serial FMA chains between them and the global round trip of D and
// its moments — 81 us at B = 64, 58 us without the feature gradient — which the matrix pipes would not shorten.
// ------------------------------------------------------------------------------------
#define DA_W3S 65      // the logits' lanes are (row, class): classes of a row 65 floats apart sit in different banks

__global__ __launch_bounds__(256) void da_step_kernel(const DaArgs a, const float* __restrict__ feat, float* __restrict__ dfeat,
                                                      const FoldCtx fc) {
  FOLD_BEGIN; FS(feat); FS(dfeat);
  const int z = blockIdx.z;
  const int64_t doff = (int64_t)fc.slot[z] * a.stride;
  const int32_t* dom = (const int32_t*)((const char*)a.dom + doff);
  float* params = (float*)((char*)a.params + doff);
  float* ea = (float*)((char*)a.exp_avg + doff);
  float* eas = (float*)((char*)a.exp_avg_sq + doff);
  double* stats = a.stats ? (double*)((char*)a.stats + doff) : nullptr;
  const int64_t* idx = a.idx ? a.idx + (int64_t)z * a.idx_row_stride : nullptr;
  const int S = a.S, B = a.B;
  float* W0 = params;
  float* b0 = W0 + 64 * 128;
  float* W3 = b0 + 64;
  float* b3 = W3 + S * 64;

  __shared__ float W0t[128 * W0T_S];
  __shared__ float W3s[MSIG_MAX_K * DA_W3S];
  __shared__ float b0s[64];
  __shared__ float b3s[MSIG_MAX_K];
  __shared__ __attribute__((aligned(16))) float fs[HEAD_ROWS * 128];
  __shared__ float hs[HEAD_ROWS * 64];
  __shared__ float dps[HEAD_ROWS * 64];
  __shared__ float dls[HEAD_ROWS * MSIG_MAX_K];
  __shared__ float lgs[HEAD_ROWS * MSIG_MAX_K];
  __shared__ int ds[MSIG_DA_MAX_BATCH];
  __shared__ double rowloss[MSIG_DA_MAX_BATCH];
  __shared__ float rowok[MSIG_DA_MAX_BATCH];
  __shared__ double red[3][4];

  const int tid = threadIdx.x;
  const int v = tid & 63, rg = tid >> 6, kcol = tid & 127, half = tid >> 7;
  const float lam = a.lam[z], mu = 1.f - lam;

  // ---- the rows' domain labels; n = sum_b (a_b + a'_b) ----
  if (tid < B) {
    const int d = idx ? dom[idx[tid]] : dom[tid];
    ds[tid] = (d < 0 || d >= S) ? -1 : d;
  }
  __syncthreads();
  {
    double w = 0.0;
    if (tid < B) w = (double)(ds[tid] >= 0 ? lam : 0.f) + (double)(ds[B - 1 - tid] >= 0 ? mu : 0.f);
    w = wave_sum_d(w);
    if ((tid & 63) == 0) red[2][tid >> 6] = w;
  }
  __syncthreads();
  const double n = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
  if (n == 0.0) return;                  // no labelled row: nothing is written (the whole workgroup leaves)
  const float inv = 1.0f / (float)n;

  // ---- D: global -> LDS ----
#pragma unroll
  for (int j = 0; j < 32; ++j) W0t[kcol * W0T_S + half * 32 + j] = W0[(half * 32 + j) * 128 + kcol];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = tid + 256 * j;
    if (i < S * 64) W3s[(i >> 6) * DA_W3S + (i & 63)] = W3[i];
  }
  if (tid < 64) b0s[tid] = b0[tid];
  if (tid < S) b3s[tid] = b3[tid];

  HEAD_GRADS_ZERO
  const float lambda = a.lambda[z], nlambda = -lambda;
  __syncthreads();

#pragma unroll 1
  for (int r0 = 0; r0 < B; r0 += HEAD_ROWS) {
    HEAD_STAGE_ROWS4(feat + (size_t)row * 128, r0, B)
    __syncthreads();
    // ---- h = relu(f W0^T + b0) ----
    {
      const float bv = b0s[v];
      HEAD_HIDDEN_CHAIN(acc, W0t, bv)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = r0 + rg * 4 + r;
        hs[(rg * 4 + r) * 64 + v] = (row < B && acc[r] > 0.f) ? acc[r] : 0.f;
      }
    }
    __syncthreads();
    // ---- z = h W3^T + b3 ----
    for (int i = tid; i < HEAD_ROWS * S; i += 256) {
      const int rl = i / S, c = i - rl * S;
      HEAD_LOGIT(acc, W3s, DA_W3S, b3s, c, rl)
      lgs[rl * MSIG_MAX_K + c] = acc;
    }
    __syncthreads();
    // ---- CrossEntropy against the row's own and its partner's domain label ----
    if (tid < HEAD_ROWS) {
      const int row = r0 + tid;
      if (row < B) {
        const float* lg = &lgs[tid * MSIG_MAX_K];
        int am;
        const float lse = ce_row_lse(lg, S, am);
        const int d = ds[row], d2 = ds[B - 1 - row];
        const float a1 = d >= 0 ? lam : 0.f, a2 = d2 >= 0 ? mu : 0.f;
        double rl = 0.0;
        if (d >= 0) rl += (double)a1 * (double)(lse - lg[d]);
        if (d2 >= 0) rl += (double)a2 * (double)(lse - lg[d2]);
        rowloss[row] = rl;
        rowok[row] = (d >= 0 && am == d) ? 1.f : 0.f;
        for (int c = 0; c < S; ++c) {
          const float p = expf(lg[c] - lse);
          dls[tid * MSIG_MAX_K + c] = (a1 * (p - (c == d ? 1.f : 0.f)) + a2 * (p - (c == d2 ? 1.f : 0.f))) * inv;
        }
      } else {
        for (int c = 0; c < S; ++c) dls[tid * MSIG_MAX_K + c] = 0.f;
      }
    }
    __syncthreads();
    HEAD_DPRE(W3s, DA_W3S, S, a)                 // dpre = relu'(h) * (dz W3)
    __syncthreads();
    HEAD_GRADS_ADD(S)                            // the owners' gradient chains over the chunk's rows
    // ---- g = dpre W0 through the parameters as found; dfeat += -lambda g, two roundings ----
    if (lambda != 0.f) {
      float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int vv = 0; vv < 64; ++vv) {
        const float wv = W0t[kcol * W0T_S + vv];
#pragma unroll
        for (int r = 0; r < 8; ++r) g[r] += wv * dps[(half * 8 + r) * 64 + vv];
      }
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int row = r0 + half * 8 + r;
        if (row < B) {
#pragma clang fp contract(off)
          float* p = dfeat + (size_t)row * 128 + kcol;
          const float t = nlambda * g[r];
          *p = *p + t;
        }
      }
    }
    __syncthreads();                     // the next chunk overwrites fs / hs / dps / dls
  }

  // ---- statistics: n L_dom, rows whose argmax is their label, labelled rows ----
  {
    double ls = tid < B ? rowloss[tid] : 0.0, cs = tid < B ? (double)rowok[tid] : 0.0, cn = (tid < B && ds[tid] >= 0) ? 1.0 : 0.0;
    ls = wave_sum_d(ls); cs = wave_sum_d(cs); cn = wave_sum_d(cn);
    if ((tid & 63) == 0) { red[0][tid >> 6] = ls; red[1][tid >> 6] = cs; red[2][tid >> 6] = cn; }
  }
  // ---- Adam, every element by its owner, in the forms these sites have always been compiled to (msig_dev.h AdamForm): parameters
  // and moments written back ----
  const float lrb = a.lr_over_bc1[z], isb = a.inv_sqrt_bc2[z];
  // parameter DST, with its moments at element `at` of theirs, from its LDS value P and its gradient G, by its owner
#define DA_OWNER_ADAM(FORM, DST, at, P, G)                                                                                 \
  {                                                                                                                    \
    float m = ea[at], s = eas[at];                                                                                     \
    DST = adam_update<FORM>(P, G, m, s, lrb, isb, a.b1, a.b2, a.eps, a.wd);                                            \
    ea[at] = m; eas[at] = s;                                                                                           \
  }
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const int i = (half * 32 + j) * 128 + kcol;
    DA_OWNER_ADAM(ADAM_FUSED_V, W0[i], i, W0t[kcol * W0T_S + half * 32 + j], dW0acc[j])
  }
  const int64_t o3 = W3 - W0, ob0 = b0 - W0, ob3 = b3 - W0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = tid + 256 * j;
    if (i < S * 64) DA_OWNER_ADAM(ADAM_FUSED_G, W3[i], o3 + i, W3s[(i >> 6) * DA_W3S + (i & 63)], dW3acc[j])
  }
  if (tid < 64) DA_OWNER_ADAM(ADAM_FUSED_G, b0[tid], ob0 + tid, b0s[tid], db0acc)
  if (tid < S) DA_OWNER_ADAM(ADAM_FUSED_G, b3[tid], ob3 + tid, b3s[tid], db3acc)
#undef DA_OWNER_ADAM
  __syncthreads();
  if (tid == 0 && stats) {
    double ls = 0.0, cs = 0.0, cn = 0.0;
    for (int i = 0; i < 4; ++i) { ls += red[0][i]; cs += red[1][i]; cn += red[2][i]; }
    stats[0] += ls; stats[1] += cs; stats[2] += cn;
  }
}

int launch_da_step(const DaArgs& a, const float* feat, float* dfeat, const FoldCtx& fc, hipStream_t st) {
  { MSIG_K("da_step", st); da_step_kernel<<<dim3(1, 1, fc.n), 256, 0, st>>>(a, feat, dfeat, fc); }
  MSIG_LAUNCH_CHECK();
  return 0;
}
