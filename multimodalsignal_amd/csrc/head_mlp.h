// The 128 -> 64 -> K classifier  feat -> hid = dropout(relu(W0 feat + b0)) -> logits = W3 hid + b3, its CrossEntropy terms and its
// backward pass, each statement group ONCE, for the five kernels that hold it: head_fwd_kernel, head_bwd_kernel, head_step_kernel
// (head.hip), head_epoch_kernel (finetune.hip) and da_step_kernel (adversary.hip, the subject discriminator: the same network with
// S outputs).  The pieces are MACROS, not functions, as gru_frag.h's are and for its reason: as __forceinline__ functions they kept
// every bit but not the schedule — head_step_kernel 0.3 us, head_epoch_kernel 4 - 8 %, da_step_kernel 1 - 3 % slower (DESIGN.md
// section 29) — while one textual definition expanded at every site compiles to the instruction stream the written-out copies had.
// tests/test_head_mlp_golden_gpu.py holds all five to the bits of those copies.
// A piece works on a group of HEAD_ROWS rows in LDS and reads the names of its site: the arrays
//   fs[16][128] features, hs[16][64] hidden layer (0 in the rows past the batch), dps[16][64] d(pre-activation),
//   dls[16][MSIG_MAX_K] dlogits, the accumulators dW0acc[32], dW3acc[4], db0acc, db3acc (HEAD_GRADS_ZERO declares them)
// and the thread map tid = threadIdx.x of 256; v = tid & 63, rg = tid >> 6 (hidden unit v of rows rg * 4 .. + 4); kcol = tid & 127,
// half = tid >> 7 (column kcol of W0: its rows half * 32 .. + 32 as gradient accumulators, the group's rows half * 8 .. + 8 of the
// feature gradient); dW3 element tid + 256 * j, j < 4; db0: tid < 64; db3: tid < K.  What differs between the sites is an argument:
// the transposed weight W0t[k * W0T_S + v], W3s and its row stride (64; 65 in the discriminator), where the bias lives (global or
// LDS), the class count.  The site places the barriers: a piece reads what the previous one wrote.
#pragma once
#include "msig_dev.h"

#define HEAD_ROWS 16
#define W0T_S 65     // padded row stride of the transposed Linear(128,64) weight in LDS

// 32 KB of W0, transposed into LDS: eight loads in flight per thread (a plain loop is 32 round trips); and W3 as it lies
#define HEAD_STAGE_WEIGHTS(W0, W3, K, W0t, W3s)                                                                                     \
  for (int j0 = 0; j0 < 32; j0 += 8) {                                                                                              \
    float q[8];                                                                                                                     \
    _Pragma("unroll") for (int u = 0; u < 8; ++u) q[u] = W0[tid + 256 * (j0 + u)];                                                  \
    _Pragma("unroll") for (int u = 0; u < 8; ++u) { const int i = tid + 256 * (j0 + u), v = i >> 7, k = i & 127; W0t[k * W0T_S + v] = q[u]; }\
  }                                                                                                                                 \
  for (int i = tid; i < K * 64; i += 256) W3s[i] = W3[i];
// the group's feature rows r0 .. r0 + 16 of a batch of B (zeros past it), one float per access
#define HEAD_STAGE_ROWS(feat, r0, B)                                                                                                \
  for (int i = tid; i < HEAD_ROWS * 128; i += 256) {                                                                                \
    const int row = r0 + (i >> 7);                                                                                                  \
    fs[i] = row < B ? feat[(size_t)row * 128 + (i & 127)] : 0.f;                                                                    \
  }
// the same rows as two float4 per thread (fs 16-byte aligned); ROWPTR: the address of batch row `row`, an expression in `row`
#define HEAD_STAGE_ROWS4(ROWPTR, r0, B)                                                                                             \
  _Pragma("unroll") for (int q = 0; q < 2; ++q) {                                                                                   \
    const int i4 = tid + 256 * q, rl = i4 >> 5, c4 = i4 & 31, row = r0 + rl;                                                        \
    float4 val = make_float4(0.f, 0.f, 0.f, 0.f);                                                                                   \
    if (row < B) val = ((const float4*)(ROWPTR))[c4];                                                                               \
    ((float4*)fs)[i4] = val;                                                                                                        \
  }
// hidden layer, thread (v, rg): acc[4], the chain over k = 0..127 from the bias BIAS (an expression: b0[v], or a value read before)
#define HEAD_HIDDEN_CHAIN(acc, W0t, BIAS)                                                                                           \
  float acc[4] = {BIAS, BIAS, BIAS, BIAS};                                                                                          \
  for (int k = 0; k < 128; ++k) {                                                                                                   \
    const float wv = W0t[k * W0T_S + v];                                                                                            \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) acc[r] += wv * fs[(rg * 4 + r) * 128 + k];                                        \
  }
// hv = dropout(relu(a)) of hidden unit v of batch row `row` (element index row * 64 + v; thr = 0: no dropout)
#define HEAD_RELU_DROPOUT(hv, a, row, thr, key, dscale)                                                                             \
  float hv = a > 0.f ? a : 0.f;                                                                                                     \
  if (thr > 0) {                                                                                                                    \
    const uint32_t e = (uint32_t)row * 64u + (uint32_t)v;                                                                           \
    hv *= drop_mul(drop_word(e, key), e & 3, thr, dscale);                                                                          \
  }
// a = b3[c] + sum_vv W3[c][vv] hs[rl][vv], in that order (W3S: the row stride of W3s)
#define HEAD_LOGIT(a, W3s, W3S, b3, c, rl)                                                                                          \
  float a = b3[c];                                                                                                                  \
  for (int vv = 0; vv < 64; ++vv) a += W3s[c * W3S + vv] * hs[rl * 64 + vv];

// Soft targets (include/msig_st.h): label smoothing eps of the launch and the mixup weight lam of each fold, the
// partner of row b being row B-1-b.  A fold with eps = 0 and lam = 1 (`plain`, uniform per fold) runs the plain statements, so its
// bits are the plain kernel's whatever its companions use.  Every operation of the soft statements is one rounding (contraction off).
struct SoftCoef { bool plain; float a1, a2, ek, wsum; double d1, d2, dk; };
template <bool CW>
__device__ __forceinline__ SoftCoef soft_coef(float eps, float lam, const float* __restrict__ cw, int K) {
#pragma clang fp contract(off)
  SoftCoef s;
  s.plain = eps == 0.f && lam == 1.f;
  const float om = 1.f - eps;
  s.a1 = om * lam; s.a2 = om * (1.f - lam); s.ek = eps / (float)K;
  const double de = (double)eps, dl = (double)lam, dom = 1.0 - de;
  s.d1 = dom * dl; s.d2 = dom * (1.0 - dl); s.dk = de / (double)K;
  s.wsum = (float)K;
  if constexpr (CW) { float t = 0.f; for (int c = 0; c < K; ++c) t = t + cw[c]; s.wsum = t; }
  return s;
}
// one row's term of the loss sum, fp64: (1-eps)(lam w[y] l(y) + (1-lam) w[y'] l(y')) + (eps/K) sum_c w_c l(c), l(c) = lse - lg[c]
template <bool CW>
__device__ __forceinline__ double soft_row_loss(const SoftCoef& s, const float* lg, float lse, int y, int y2, const float* __restrict__ cw, int K) {
#pragma clang fp contract(off)
  const double wy = CW ? (double)cw[y] : 1.0, wy2 = CW ? (double)cw[y2] : 1.0;
  double all = 0.0;
  for (int c = 0; c < K; ++c) all = all + (CW ? (double)cw[c] : 1.0) * (double)(lse - lg[c]);
  const double own = (s.d1 * wy) * (double)(lse - lg[y]);
  const double par = (s.d2 * wy2) * (double)(lse - lg[y2]);
  return (own + par) + s.dk * all;
}
// dL/dz[b][c] of the same, fp32
__device__ __forceinline__ float soft_dlogit(const SoftCoef& s, float p, int c, int y, int y2, float wy, float wy2, float wc, float invW) {
#pragma clang fp contract(off)
  const float own = (s.a1 * wy) * (p - (c == y ? 1.f : 0.f));
  const float par = (s.a2 * wy2) * (p - (c == y2 ? 1.f : 0.f));
  const float sm = s.ek * (p * s.wsum - wc);
  return ((own + par) + sm) * invW;
}

// The plain and class-weighted CrossEntropy statements of one row (CW: the site's flag): dL/dlogit of class c from its softmax p,
// and the row's term of the loss sum in fp64 — ce_row_terms, head_step_kernel and head_epoch_kernel
#define HEAD_CE_DL(p, c, y, wy, inv) (CW ? (wy * (p - (c == y ? 1.f : 0.f))) * inv : (p - (c == y ? 1.f : 0.f)) * inv)
#define HEAD_CE_ROW_LOSS(lg, lse, y, wy) (CW ? (double)wy * (double)(lse - lg[y]) : (double)(lse - lg[y]))

// One row of CrossEntropy from its K logits lg in global memory, label y (partner's label y2, read when `soft`): am = the argmax,
// emit(c, p, dl) per class with the softmax p and dL/dlogit dl (the caller stores what it keeps), and, returned, the row's term of
// the loss sum (fp64): ce_kernel and loss_finalize.  inv = 1 / B, or 1 / W with class weights (cw: K weights, read when CW or soft).
template <bool CW, bool ST, typename F>
__device__ __forceinline__ double ce_row_terms(const float* lg, int K, int y, int y2, const float* cw, float inv, bool soft, const SoftCoef& sc,
                                               int& am, F&& emit) {
  const float lse = ce_row_lse(lg, K, am);
  const float wy = CW ? cw[y] : 1.f, wy2 = (CW && ST && soft) ? cw[y2] : 1.f;
  for (int c = 0; c < K; ++c) {
    const float p = expf(lg[c] - lse);
    emit(c, p, (ST && soft) ? soft_dlogit(sc, p, c, y, y2, wy, wy2, CW ? cw[c] : 1.f, inv) : HEAD_CE_DL(p, c, y, wy, inv));
  }
  if (ST && soft) return soft_row_loss<CW>(sc, lg, lse, y, y2, cw, K);
  return HEAD_CE_ROW_LOSS(lg, lse, y, wy);
}

// the owners' gradient accumulators of a workgroup, zero to begin with
#define HEAD_GRADS_ZERO                                                                                                             \
  float dW0acc[32];                                                                                                                 \
  _Pragma("unroll") for (int j = 0; j < 32; ++j) dW0acc[j] = 0.f;                                                                   \
  float dW3acc[4] = {0.f, 0.f, 0.f, 0.f};                                                                                           \
  float db0acc = 0.f, db3acc = 0.f;
// d(pre-activation of Linear(128,64)) = relu'(h) * SCALED, SCALED an expression in a = (dlogits W3)[rl][v]: a * dscale, or a
#define HEAD_DPRE(W3s, W3S, K, SCALED)                                                                                              \
  _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                                                   \
    const int rl = rg * 4 + r;                                                                                                      \
    float a = 0.f;                                                                                                                  \
    for (int c = 0; c < K; ++c) a += W3s[c * W3S + v] * dls[rl * MSIG_MAX_K + c];                                                   \
    dps[rl * 64 + v] = hs[rl * 64 + v] > 0.f ? SCALED : 0.f;                                                                        \
  }
// the group's 16 rows added to the owners' chains: dW3 / db3 / db0 as one sum over the rows, dW0 row by row
#define HEAD_GRADS_ADD(K)                                                                                                           \
  _Pragma("unroll") for (int j = 0; j < (msig_negctl_range == 3 ? 2 : 4); ++j) {                                                    \
    const int idx = tid + 256 * j;                                                                                                  \
    if (idx < K * 64) {                                                                                                             \
      const int c = idx >> 6, vv = idx & 63;                                                                                        \
      float a = 0.f;                                                                                                                \
      _Pragma("unroll 4") for (int rl = 0; rl < HEAD_ROWS; ++rl) a += dls[rl * MSIG_MAX_K + c] * hs[rl * 64 + vv];                  \
      dW3acc[j] += a;                                                                                                               \
    }                                                                                                                               \
  }                                                                                                                                 \
  if (tid < K) { float a = 0.f; for (int rl = 0; rl < HEAD_ROWS; ++rl) a += dls[rl * MSIG_MAX_K + tid]; db3acc += a; }              \
  if (tid < 64) { float a = 0.f; for (int rl = 0; rl < HEAD_ROWS; ++rl) a += dps[rl * 64 + tid]; db0acc += a; }                     \
  _Pragma("unroll 1") for (int rl = 0; rl < HEAD_ROWS; ++rl) {                                                                      \
    const float fv = fs[rl * 128 + kcol];                                                                                           \
    _Pragma("unroll") for (int j = 0; j < 32; ++j) dW0acc[j] += dps[rl * 64 + half * 32 + j] * fv;                                  \
  }
// dfeat[row][kcol] = sum_v W0[v][kcol] dpre[row][v], a chain over v = 0..63 from 0, thread (kcol, half): rows half * 8 .. + 8, one at
// a time (the discriminator keeps eight in flight and adds the result times -lambda: its own loop around the same chain)
#define HEAD_DFEAT(W0t, dfeat, r0, B)                                                                                               \
  _Pragma("unroll 1") for (int r = 0; r < 8; ++r) {                                                                                 \
    const int rl = half * 8 + r, row = r0 + rl;                                                                                     \
    float a = 0.f;                                                                                                                  \
    _Pragma("unroll 8") for (int vv = 0; vv < 64; ++vv) a += W0t[kcol * W0T_S + vv] * dps[rl * 64 + vv];                            \
    if (row < B) dfeat[(size_t)row * 128 + kcol] = a;                                                                               \
  }
// a workgroup's partial row [dW0 64*128][db0 64][dW3 K*64][db3 K]
#define HEAD_PART_STORE(P, K)                                                                                                       \
  _Pragma("unroll") for (int j = 0; j < 32; ++j) P[(half * 32 + j) * 128 + kcol] = dW0acc[j];                                       \
  if (tid < 64) P[64 * 128 + tid] = db0acc;                                                                                         \
  _Pragma("unroll") for (int j = 0; j < 4; ++j) { const int idx = tid + 256 * j; if (idx < K * 64) P[64 * 128 + 64 + idx] = dW3acc[j]; }\
  if (tid < K) P[64 * 128 + 64 + K * 64 + tid] = db3acc;
