// include/msig_ft.h: window embeddings (the copy of MSIG_WS_FEAT; the forward itself is api.hip's) and the head epoch —
// consecutive classifier-only train steps on cached features in ONE launch (few-shot subject calibration).
#include "msig_dev.h"
#include "finetune.h"
#include "head_mlp.h"

// ------------------------------------------------------------------------------------
// MSIG_WS_FEAT (B,128) of fold z -> out + z * out_stride
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ft_feat_copy_kernel(const float* __restrict__ feat, float* __restrict__ out, int64_t out_stride_bytes,
                                                           int n4, const FoldCtx fc) {
  FOLD_BEGIN; FS(feat);
  float4* o = (float4*)((char*)out + (int64_t)blockIdx.z * out_stride_bytes);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) o[i] = ((const float4*)feat)[i];
}

int launch_ft_feat_copy(const float* feat, float* out, int64_t out_stride_bytes, int B, const FoldCtx& fc, hipStream_t st) {
  const int n4 = B * 32;
  const int grid = (n4 + 255) / 256 < 256 ? (n4 + 255) / 256 : 256;
  { MSIG_K("ft_feat_copy", st); ft_feat_copy_kernel<<<dim3(grid, 1, fc.n), 256, 0, st>>>(feat, out, out_stride_bytes, n4, fc); }
  MSIG_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------
// Head epoch.  One workgroup of 256 threads per fold keeps the classifier (9.3 k floats) in LDS and both Adam moments in
// REGISTERS for the whole call — every element of W0 / b0 / W3 / b3 has ONE owner thread, which accumulates its gradient,
// applies Adam and writes the new value where the next step's forward reads it — so a step is barriers and LDS traffic, with no
// global round trip but the gather of its rows:
//   W0 (64,128): thread (kcol = tid & 127, half = tid >> 7) owns rows half * 32 + j, j < 32, of column kcol (head_bwd_kernel's
//                accumulator map); kept TRANSPOSED in LDS, W0t[k * 65 + v], which the forward (lane = v) and the owners
//                (lane = k, stride 65) both reach without a bank conflict;
//   W3 (K,64)  : thread tid owns elements tid + 256 * j, j < 4;   b0: tid < 64;   b3: tid < K.
// A step's rows run through head_mlp.h's pieces — the text head_fwd_kernel / ce_kernel / head_bwd_kernel expand — in chunks of 16
// rows, in batch order: a weight-gradient element is the chain  acc += dps[row] * feat[row]  over the step's rows 0, 1, 2, ... —
// one fixed order.  The loss and the class-weight total are fp64 sums in ce_kernel's / cw_total's order for a batch of <= 256 rows
// (lane = row, wave reduction, the four wave sums in wave order).  Nothing depends on the number of steps, on the position of a
// step inside the call or on the folds beside it.  Plain fp32 FMA, no MFMA: a step's contractions are 2 x 131 k multiply-adds per 16 rows — about
// a microsecond on four waves — beside six barriers; the matrix pipes would shorten only that microsecond, at the price of
// fragment shuffles through LDS for operands that are already there in the layout the VALU wants.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ double ft_powi(double b, int64_t e) {      // b^e by squaring: a function of (b, e) alone
  double r = 1.0;
  while (e > 0) { if (e & 1) r *= b; b *= b; e >>= 1; }
  return r;
}

template <bool CW>
__global__ __launch_bounds__(256) void head_epoch_kernel(const msig_ft_head h, const FtFolds ff) {
  const int fold = blockIdx.x;
  const int64_t foff_ = (int64_t)ff.slot[fold] * ff.stride;
  const float* feat = h.feat; const int64_t* labels = h.labels; const int32_t* order = h.order;
  float* params = h.params; float* ea = h.exp_avg; float* eas = h.exp_avg_sq;
  const float* cw = h.class_weight; double* lacc = h.loss_acc;
  FS(feat); FS(labels); FS(order); FS(params); FS(ea); FS(eas); FS(cw); FS(lacc);
  const int K = h.K;
  float* W0 = params + h.cls_offset;
  float* b0 = W0 + 64 * 128;
  float* W3 = b0 + 64;
  float* b3 = W3 + (K * 64 + 3) / 4 * 4;
  const int64_t om = W0 - params;      // the moments' tensors sit at the same offsets

  __shared__ float W0t[128 * W0T_S];
  __shared__ float W3s[MSIG_MAX_K * 64];
  __shared__ float b0s[64];
  __shared__ float b3s[MSIG_MAX_K];
  __shared__ float cws[MSIG_MAX_K];
  __shared__ __attribute__((aligned(16))) float fs[HEAD_ROWS * 128];
  __shared__ float hs[HEAD_ROWS * 64];
  __shared__ float dps[HEAD_ROWS * 64];
  __shared__ float dls[HEAD_ROWS * MSIG_MAX_K];
  __shared__ float lgs[HEAD_ROWS * MSIG_MAX_K];
  __shared__ int idxs[MSIG_FT_MAX_BATCH];
  __shared__ int ys[MSIG_FT_MAX_BATCH];
  __shared__ double rowloss[MSIG_FT_MAX_BATCH];
  __shared__ float rowok[MSIG_FT_MAX_BATCH];
  __shared__ double red[3][4];

  const int tid = threadIdx.x;
  const int v = tid & 63, rg = tid >> 6, kcol = tid & 127, half = tid >> 7;
  // ---- the head and its moments: global -> LDS / registers, once ----
  float m0[32], v0[32], m3[4], v3[4];
  float mb0 = 0.f, vb0 = 0.f, mb3 = 0.f, vb3 = 0.f;
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const int i = (half * 32 + j) * 128 + kcol;
    W0t[kcol * W0T_S + half * 32 + j] = W0[i];
    m0[j] = ea[om + i]; v0[j] = eas[om + i];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = tid + 256 * j;
    m3[j] = 0.f; v3[j] = 0.f;
    if (i < K * 64) { W3s[i] = W3[i]; m3[j] = (ea + om + (W3 - W0))[i]; v3[j] = (eas + om + (W3 - W0))[i]; }
  }
  if (tid < 64) { b0s[tid] = b0[tid]; mb0 = (ea + om + (b0 - W0))[tid]; vb0 = (eas + om + (b0 - W0))[tid]; }
  if (tid < K) { b3s[tid] = b3[tid]; mb3 = (ea + om + (b3 - W0))[tid]; vb3 = (eas + om + (b3 - W0))[tid]; }
  if (tid < MSIG_MAX_K) cws[tid] = (CW && tid < K) ? cw[tid] : 1.f;
  double acc_loss = 0.0, acc_ok = 0.0;          // thread 0: loss_acc, continued in step order
  if (tid == 0 && lacc) { acc_loss = lacc[0]; acc_ok = lacc[1]; }
  const int thr = h.dropout_thr;
  const float dscale = drop_scale(thr), dscale_bwd = thr > 0 ? drop_scale(thr) : 1.0f;
  const float lr = ff.lr[fold];
  __syncthreads();

#pragma unroll 1
  for (int s = 0; s < h.n_steps; ++s) {
    const int pos0 = (h.first_step + s) * h.batch;
    const int nb = min(h.batch, h.n_order - pos0);
    const int64_t t = ff.step0[fold] + s;
    const uint32_t key = dropout_key(ff.seed[fold], (uint64_t)t, 2);
    // ---- the step's rows and labels; W = sum_b w[y_b] in cw_total's order ----
    if (tid < nb) {
      const int r = min(max(order[pos0 + tid], 0), h.N - 1);
      idxs[tid] = r;
      const int64_t y = labels[r];
      ys[tid] = y < 0 ? 0 : (y > K - 1 ? K - 1 : (int)y);
    }
    float inv = 1.0f / (float)nb;
    double Wt = 0.0;
    if constexpr (CW) {
      double sw = tid < nb ? (double)cws[ys[tid]] : 0.0;
      sw = wave_sum_d(sw);
      if ((tid & 63) == 0) red[2][tid >> 6] = sw;
      __syncthreads();
      Wt = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
      inv = 1.0f / (float)Wt;
    }
    // Adam's bias corrections of step t, as train_step_fc forms them on the host
    const double bc1 = 1.0 - ft_powi((double)h.beta1, t), bc2 = 1.0 - ft_powi((double)h.beta2, t);
    const float lr_over_bc1 = (float)((double)lr / bc1), inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));

    HEAD_GRADS_ZERO
    __syncthreads();                     // idxs / ys are written; the previous step's parameter update is visible

#pragma unroll 1
    for (int r0 = 0; r0 < nb; r0 += HEAD_ROWS) {
      HEAD_STAGE_ROWS4(feat + (size_t)idxs[row] * 128, r0, nb)
      __syncthreads();
      // ---- head_fwd_kernel ----
      {
        const float bv = b0s[v];
        HEAD_HIDDEN_CHAIN(acc, W0t, bv)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = r0 + rg * 4 + r;
          HEAD_RELU_DROPOUT(hv, acc[r], row, thr, key, dscale)
          hs[(rg * 4 + r) * 64 + v] = row < nb ? hv : 0.f;       // the backward pieces read hid as 0 for the rows past the batch
        }
      }
      __syncthreads();
      for (int i = tid; i < HEAD_ROWS * K; i += 256) {
        const int rl = i / K, c = i - rl * K;
        HEAD_LOGIT(a, W3s, 64, b3s, c, rl)
        lgs[rl * MSIG_MAX_K + c] = a;
      }
      __syncthreads();
      // ---- ce_kernel, the rows of this chunk ----
      if (tid < HEAD_ROWS) {
        const int row = r0 + tid;
        if (row < nb) {
          const float* lg = &lgs[tid * MSIG_MAX_K];
          int am;
          const float lse = ce_row_lse(lg, K, am);
          const int y = ys[row];
          const float wy = cws[y];
          rowloss[row] = HEAD_CE_ROW_LOSS(lg, lse, y, wy);
          rowok[row] = (am == y) ? 1.f : 0.f;
          for (int c = 0; c < K; ++c) {
            const float p = expf(lg[c] - lse);
            dls[tid * MSIG_MAX_K + c] = HEAD_CE_DL(p, c, y, wy, inv);
          }
        } else {
          for (int c = 0; c < K; ++c) dls[tid * MSIG_MAX_K + c] = 0.f;
        }
      }
      __syncthreads();
      // ---- head_bwd_kernel, without dfeat (the extractor is frozen) ----
      HEAD_DPRE(W3s, 64, K, a * dscale_bwd)
      __syncthreads();
      HEAD_GRADS_ADD(K)
      __syncthreads();                   // the next chunk overwrites fs / hs / dps / dls
    }

    // ---- the step's loss and accuracy counter: ce_kernel's sums for a batch of <= 256 rows ----
    {
      double ls = tid < nb ? rowloss[tid] : 0.0, cs = tid < nb ? (double)rowok[tid] : 0.0;
      ls = wave_sum_d(ls); cs = wave_sum_d(cs);
      if ((tid & 63) == 0) { red[0][tid >> 6] = ls; red[1][tid >> 6] = cs; }
    }
    // ---- Adam, every element by its owner, in the forms these sites have always been compiled to (msig_dev.h AdamForm) ----
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      float* p = &W0t[kcol * W0T_S + half * 32 + j];
      *p = adam_update<ADAM_FUSED_V>(*p, dW0acc[j], m0[j], v0[j], lr_over_bc1, inv_sqrt_bc2, h.beta1, h.beta2, h.eps, h.weight_decay);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int idx = tid + 256 * j;
      if (idx < K * 64) W3s[idx] = adam_update<ADAM_PRODUCTS>(W3s[idx], dW3acc[j], m3[j], v3[j], lr_over_bc1, inv_sqrt_bc2, h.beta1, h.beta2, h.eps, h.weight_decay);
    }
    if (tid < 64) b0s[tid] = adam_update<ADAM_FUSED_V>(b0s[tid], db0acc, mb0, vb0, lr_over_bc1, inv_sqrt_bc2, h.beta1, h.beta2, h.eps, h.weight_decay);
    if (tid < K) b3s[tid] = adam_update<ADAM_FUSED_V>(b3s[tid], db3acc, mb3, vb3, lr_over_bc1, inv_sqrt_bc2, h.beta1, h.beta2, h.eps, h.weight_decay);
    __syncthreads();
    if (tid == 0) {
      double ls = 0.0, cs = 0.0;
      for (int i = 0; i < 4; ++i) { ls += red[0][i]; cs += red[1][i]; }
      if constexpr (CW) acc_loss += ls * ((double)nb / Wt);
      else acc_loss += ls;
      acc_ok += cs;
    }
  }

  // ---- write the head and its moments back, once ----
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const int i = (half * 32 + j) * 128 + kcol;
    W0[i] = W0t[kcol * W0T_S + half * 32 + j];
    ea[om + i] = m0[j]; eas[om + i] = v0[j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = tid + 256 * j;
    if (i < K * 64) { W3[i] = W3s[i]; (ea + om + (W3 - W0))[i] = m3[j]; (eas + om + (W3 - W0))[i] = v3[j]; }
  }
  if (tid < 64) { b0[tid] = b0s[tid]; (ea + om + (b0 - W0))[tid] = mb0; (eas + om + (b0 - W0))[tid] = vb0; }
  if (tid < K) { b3[tid] = b3s[tid]; (ea + om + (b3 - W0))[tid] = mb3; (eas + om + (b3 - W0))[tid] = vb3; }
  if (tid == 0 && lacc) { lacc[0] = acc_loss; lacc[1] = acc_ok; }
}

int launch_head_epoch(const msig_ft_head& h, const FtFolds& ff, hipStream_t st) {
  MSIG_K("head_epoch", st);
  if (h.class_weight) head_epoch_kernel<true><<<dim3(ff.n), 256, 0, st>>>(h, ff);
  else head_epoch_kernel<false><<<dim3(ff.n), 256, 0, st>>>(h, ff);
  MSIG_LAUNCH_CHECK();
  return 0;
}
