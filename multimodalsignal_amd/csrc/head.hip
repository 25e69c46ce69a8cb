// Classifier head (models.py:66-71,80), CrossEntropyLoss (trainer.py:69,147), the
// eval-time softmax/argmax (trainer.py:224-225), Adam (trainer.py:68,149) and the small
// utility kernels (partial-sum reduction, window gather).  These stages are <0.1 % of the
// FLOPs, so they are plain VALU kernels; what matters is that they stay on the stream and
// never force a host sync.  The classifier's statements themselves are head_mlp.h's.
#include "msig_dev.h"
#include "head_mlp.h"

#define HEAD_WG 128

// ------------------------------------------------------------------------------------
// feat (B,128) -> hid = dropout(relu(W0 feat + b0)) (B,64) -> logits = W3 hid + b3 (B,K)
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void head_fwd_kernel(const float* __restrict__ feat, const float* __restrict__ W0,
                                                       const float* __restrict__ b0, const float* __restrict__ W3,
                                                       const float* __restrict__ b3, float* __restrict__ hid,
                                                       float* __restrict__ logits, int B, int K, int drop_thr,
                                                       uint32_t drop_key, float dscale, const FoldCtx fc) {
  FOLD_BEGIN; FS(feat); FS(W0); FS(b0); FS(W3); FS(b3); FS(hid); FS(logits); drop_key = fc.key_head[blockIdx.z];
  __shared__ float W0t[128 * W0T_S];
  __shared__ float W3s[MSIG_MAX_K * 64];
  __shared__ float fs[HEAD_ROWS * 128];
  __shared__ float hs[HEAD_ROWS * 64];
  const int tid = threadIdx.x;
  HEAD_STAGE_WEIGHTS(W0, W3, K, W0t, W3s)
  const int ngroups = (B + HEAD_ROWS - 1) / HEAD_ROWS;
  const int v = tid & 63, rg = tid >> 6;
  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const int r0 = grp * HEAD_ROWS;
    __syncthreads();
    HEAD_STAGE_ROWS(feat, r0, B)
    __syncthreads();
    HEAD_HIDDEN_CHAIN(acc, W0t, b0[v])
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + rg * 4 + r;
      HEAD_RELU_DROPOUT(hv, acc[r], row, drop_thr, drop_key, dscale)
      hs[(rg * 4 + r) * 64 + v] = hv;
      if (row < B) hid[(size_t)row * 64 + v] = hv;
    }
    __syncthreads();
    for (int i = tid; i < HEAD_ROWS * K; i += 256) {
      const int rl = i / K, c = i - rl * K, row = r0 + rl;
      HEAD_LOGIT(a, W3s, 64, b3, c, rl)
      if (row < B) logits[(size_t)row * K + c] = a;
    }
  }
}

// Class-weighted CrossEntropy (include/msig_cw.h): W = sum_b w[y_b], the normaliser of the weighted mean, summed in fp64 in ONE
// fixed order whatever the workgroup's size — lane j of the first 256 threads adds rows j, j + 256, ... in turn, each wave reduces
// its lanes, the four wave sums are added in wave order — so that ce_kernel (1024 threads), every workgroup of head_step_kernel and
// the loss finalizer (256 each) hold the identical value.  Every thread of the workgroup must call it (it synchronises); red4 is
// shared memory of its own.
__device__ __forceinline__ double cw_total(const float* __restrict__ cw, const int64_t* __restrict__ labels, int B, double* red4) {
  const int tid = threadIdx.x;
  if (tid < 256) {
    double s = 0.0;
    for (int row = tid; row < B; row += 256) s += (double)cw[labels[row]];
    s = wave_sum_d(s);
    if ((tid & 63) == 0) red4[tid >> 6] = s;
  }
  __syncthreads();
  return (red4[0] + red4[1]) + (red4[2] + red4[3]);
}

// Soft targets (head_mlp.h): ST is one more flag beside CW on ce_kernel / head_step_kernel / loss_finalize (and on the two kernels
// the finalizer rides in); the ST = false instantiations take an empty SoftT and are what they were.  ce_kernel and
// head_step_kernel + loss_finalize agree in every bit because they share head_mlp.h's statements, not because the compiler happens to fuse alike.
template <bool ST> struct SoftT {};
template <> struct SoftT<true> { SoftArgs a; };
// what a launch's CrossEntropy rows share: W (class weights: cw_total's; else B, read when ST) and the fold's soft-target terms
template <bool CW, bool ST>
struct CeCtx { double W = 0.0; SoftCoef sc{}; bool soft = false; };
template <bool CW, bool ST>
__device__ __forceinline__ CeCtx<CW, ST> ce_ctx(const float* cw, const int64_t* labels, int B, int K, double* wred, const SoftT<ST>& sa, int fold) {
  CeCtx<CW, ST> x;
  if constexpr (CW) x.W = cw_total(cw, labels, B, wred);
  if constexpr (ST) {
    x.sc = soft_coef<CW>(sa.a.eps, sa.a.lam[fold], cw, K);
    x.soft = !x.sc.plain;
    if constexpr (!CW) x.W = (double)B;
  }
  return x;
}
// thread 0's tail of the loss: the sixteen wave sums in order, then lossbuf[0] = mean loss of this batch; lossbuf[1] = summed loss
// of this batch (loss.item() * B, trainer.py:152,221); lossbuf[2] = #correct of this batch — plain stores, no running sums: layouts
// of different batch sizes alias one pooled workspace, and the epoch sums live with the caller (lacc: msig_batch.loss_acc, the
// caller's running sums of a pass; one thread, stream order).
#define CE_THREADS 1024
template <bool WEIGHTED>
__device__ __forceinline__ void loss_tail(const double (*red)[CE_THREADS / 64], int B, double W, float* __restrict__ lossbuf, double* __restrict__ lacc) {
  double ls = 0.0, cs = 0.0;
  for (int i = 0; i < CE_THREADS / 64; ++i) { ls += red[0][i]; cs += red[1][i]; }
  const double sum = WEIGHTED ? ls * ((double)B / W) : ls;
  lossbuf[0] = (float)(ls / (WEIGHTED ? W : (double)B));
  lossbuf[1] = (float)sum;
  lossbuf[2] = (float)cs;
  if (lacc) { lacc[0] += sum; lacc[1] += cs; }
}

// ------------------------------------------------------------------------------------
// CrossEntropy (mean), dlogits, softmax probabilities, argmax, accuracy counter.
// Single workgroup (one deterministic sum) of CE_THREADS threads — with 256 the 32 rows per thread of a B = 8192 batch took 62 us,
// all of it exp / log latency.
// CW = class weights w (K floats, include/msig_cw.h; torch's CrossEntropyLoss(weight=w)): row b's terms carry w[y_b], the mean
// divides by W = sum_b w[y_b] (cw_total) instead of B, and lossbuf[1] / loss_acc[0] get B times that mean.  Arranged so that w = 1
// reproduces the unweighted instantiation's bits: W = B exactly, w_y * v = v, ls * (B / W) = ls.
// ------------------------------------------------------------------------------------
template <bool CW, bool ST = false>
__global__ __launch_bounds__(CE_THREADS) void ce_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                 float* __restrict__ probs, int* __restrict__ pred,
                                                 float* __restrict__ dlogits, float* __restrict__ lossbuf, double* __restrict__ lacc,
                                                 const float* __restrict__ cw, int B, int K, const FoldCtx fc, const SoftT<ST> sa) {
  FOLD_BEGIN; FS(logits); FS(labels); FS(probs); FS(pred); FS(dlogits); FS(lossbuf); FS(lacc);
  __shared__ double red[2][CE_THREADS / 64];
  __shared__ double wred[4];
  const int tid = threadIdx.x;
  double lsum = 0.0, correct = 0.0;
  if constexpr (CW) FS(cw);
  const CeCtx<CW, ST> x = ce_ctx<CW, ST>(cw, labels, B, K, wred, sa, blockIdx.z);
  const float inv = 1.0f / (CW ? (float)x.W : (float)B);
  for (int row = tid; row < B; row += CE_THREADS + (msig_negctl_batch == 2 && row < CE_THREADS ? 1 : 0)) {
    const int y = (int)labels[row], y2 = x.soft ? (int)labels[B - 1 - row] : y;
    int am;
    lsum += ce_row_terms<CW, ST>(logits + (size_t)row * K, K, y, y2, cw, inv, x.soft, x.sc, am, [&](int c, float p, float dl) {
      probs[(size_t)row * K + c] = p;
      if (dlogits) dlogits[(size_t)row * K + c] = dl;
    });
    pred[row] = am;
    correct += (am == y) ? 1.0 : 0.0;
  }
  lsum = wave_sum_d(lsum); correct = wave_sum_d(correct);
  if ((tid & 63) == 0) { red[0][tid >> 6] = lsum; red[1][tid >> 6] = correct; }
  __syncthreads();
  if (tid == 0) loss_tail<CW || ST>(red, B, x.W, lossbuf, lacc);
}

// The reduction half of ce_kernel for the fused head (head_step_kernel wrote pred / probs / dlogits; the loss and the accuracy
// counter are sums over the whole batch): one workgroup of 256 threads plays ce_kernel's 1024 — virtual thread q * 256 + tid sums
// the rows ce_kernel's thread of that index sums, each real wave reduces four virtual waves, thread 0 adds the sixteen wave sums in
// ce_kernel's order.  Same values (ce_row_terms' return), same order, same tail: the loss is ce_kernel's, bit for bit.
template <bool CW, bool ST = false>
__device__ __forceinline__ void loss_finalize(const LossFin& lf, double (*red)[CE_THREADS / 64], double* wred, const SoftT<ST>& sa, int fold) {
  const int tid = threadIdx.x;
  const CeCtx<CW, ST> x = ce_ctx<CW, ST>(lf.cw, lf.labels, lf.B, lf.K, wred, sa, fold);
#pragma unroll 1
  for (int q = 0; q < CE_THREADS / 256; ++q) {
    double lsum = 0.0, correct = 0.0;
    for (int row = q * 256 + tid; row < lf.B; row += CE_THREADS + (msig_negctl_batch == 2 && row < CE_THREADS ? 1 : 0)) {
      const float* lg = lf.logits + (size_t)row * lf.K;
      int am;
      const float lse = ce_row_lse(lg, lf.K, am);
      const int y = (int)lf.labels[row];
      if (ST && x.soft) lsum += soft_row_loss<CW>(x.sc, lg, lse, y, (int)lf.labels[lf.B - 1 - row], lf.cw, lf.K);
      else lsum += HEAD_CE_ROW_LOSS(lg, lse, y, lf.cw[y]);
      correct += (am == y) ? 1.0 : 0.0;
    }
    lsum = wave_sum_d(lsum); correct = wave_sum_d(correct);
    if ((tid & 63) == 0) { red[0][q * 4 + (tid >> 6)] = lsum; red[1][q * 4 + (tid >> 6)] = correct; }
  }
  __syncthreads();
  if (tid == 0) loss_tail<CW || ST>(red, lf.B, x.W, lf.lossbuf, lf.lacc);
}

// softmax + argmax only (no labels)
__global__ __launch_bounds__(256) void softmax_kernel(const float* __restrict__ logits, float* __restrict__ probs,
                                                      int* __restrict__ pred, int B, int K, const FoldCtx fc) {
  FOLD_BEGIN; FS(logits); FS(probs); FS(pred);
  for (int row = blockIdx.x * 256 + threadIdx.x; row < B; row += gridDim.x * 256) {
    const float* lg = logits + (size_t)row * K;
    float mx = lg[0]; int am = 0;
    for (int c = 1; c < K; ++c) if (lg[c] > mx) { mx = lg[c]; am = c; }
    float se = 0.f;
    for (int c = 0; c < K; ++c) se += expf(lg[c] - mx);
    for (int c = 0; c < K; ++c) probs[(size_t)row * K + c] = expf(lg[c] - mx) / se;
    pred[row] = am;
  }
}

// ------------------------------------------------------------------------------------
// head backward: dlogits -> dW3, db3, dW0, db0 (per-workgroup partials, HEAD_PART_STORE's layout) and dfeat
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void head_bwd_kernel(const float* __restrict__ dlogits, const float* __restrict__ feat,
                                                       const float* __restrict__ hid, const float* __restrict__ W0,
                                                       const float* __restrict__ W3, float* __restrict__ dfeat,
                                                       float* __restrict__ part, int B, int K, float dscale, const FoldCtx fc) {
  FOLD_BEGIN; FS(dlogits); FS(feat); FS(hid); FS(W0); FS(W3); FS(dfeat); FS(part);
  __shared__ float W0t[128 * W0T_S];
  __shared__ float W3s[MSIG_MAX_K * 64];
  __shared__ float fs[HEAD_ROWS * 128];
  __shared__ float hs[HEAD_ROWS * 64];
  __shared__ float dps[HEAD_ROWS * 64];
  __shared__ float dls[HEAD_ROWS * MSIG_MAX_K];
  const int tid = threadIdx.x;
  HEAD_STAGE_WEIGHTS(W0, W3, K, W0t, W3s)
  HEAD_GRADS_ZERO
  const int ngroups = (B + HEAD_ROWS - 1) / HEAD_ROWS;
  const int v = tid & 63, rg = tid >> 6, kcol = tid & 127, half = tid >> 7;
  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const int r0 = grp * HEAD_ROWS;
    if (msig_negctl_batch == 3 && grp >= (int)gridDim.x && r0 + 1 >= B) break;      // uniform over the workgroup
    __syncthreads();
    HEAD_STAGE_ROWS(feat, r0, B)
    for (int i = tid; i < HEAD_ROWS * 64; i += 256) { const int row = r0 + (i >> 6); hs[i] = row < B ? hid[(size_t)row * 64 + (i & 63)] : 0.f; }
    for (int i = tid; i < HEAD_ROWS * K; i += 256) { const int row = r0 + i / K; dls[(i / K) * MSIG_MAX_K + (i % K)] = row < B ? dlogits[(size_t)row * K + (i % K)] : 0.f; }
    __syncthreads();
    HEAD_DPRE(W3s, 64, K, a * dscale)
    __syncthreads();
    HEAD_GRADS_ADD(K)
    HEAD_DFEAT(W0t, dfeat, r0, B)
  }
  float* P = part + (size_t)blockIdx.x * (64 * 128 + 64 + K * 64 + K);
  HEAD_PART_STORE(P, K)
}

// ------------------------------------------------------------------------------------
// The head of a fused train step at few windows, one launch instead of three (head_fwd, ce, head_bwd): a workgroup takes ONE
// group of 16 rows through the classifier, its rows' CrossEntropy terms (dlogits need nothing but their own row) and the
// backward pass, with the weights, the features, the hidden layer and dlogits staying in LDS.  What needs the whole batch — the
// loss and the accuracy counter — is summed by loss_finalize in the step's last launch.  The pieces are the ones head_fwd_kernel /
// ce_kernel / head_bwd_kernel are made of (head_mlp.h, one text each): the step's bits are those of the three launches
// (tests/test_parity_gpu.py::test_fused_step_equals_separate_calls_bit_for_bit).  grid = (B + 15) / 16 <= HEAD_WG workgroups, each
// writing one partial row, as head_bwd_kernel does at that size.  CW: class-weighted CrossEntropy (ce_kernel<true>) — a row's dlogits
// need the whole batch's W, which every workgroup sums itself over all B <= 2048 labels in cw_total's one order (no extra launch).
// ------------------------------------------------------------------------------------
template <bool CW, bool ST = false>
__global__ __launch_bounds__(256) void head_step_kernel(const float* __restrict__ feat, const float* __restrict__ W0, const float* __restrict__ b0,
                                                        const float* __restrict__ W3, const float* __restrict__ b3, const int64_t* __restrict__ labels,
                                                        float* __restrict__ hid, float* __restrict__ logits, float* __restrict__ probs, int* __restrict__ pred,
                                                        float* __restrict__ dlogits, float* __restrict__ dfeat, float* __restrict__ part,
                                                        const float* __restrict__ cw,
                                                        int B, int K, int drop_thr, uint32_t drop_key, float dscale, float dscale_bwd, const FoldCtx fc,
                                                        const SoftT<ST> sa) {
  FOLD_BEGIN; FS(feat); FS(W0); FS(b0); FS(W3); FS(b3); FS(labels); FS(hid); FS(logits); FS(probs); FS(pred); FS(dlogits); FS(dfeat); FS(part);
  drop_key = fc.key_head[blockIdx.z];
  __shared__ float W0t[128 * W0T_S];
  __shared__ float W3s[MSIG_MAX_K * 64];
  __shared__ float fs[HEAD_ROWS * 128];
  __shared__ float hs[HEAD_ROWS * 64];
  __shared__ float dps[HEAD_ROWS * 64];
  __shared__ float dls[HEAD_ROWS * MSIG_MAX_K];
  __shared__ float lgs[HEAD_ROWS * MSIG_MAX_K];
  const int tid = threadIdx.x;
  HEAD_STAGE_WEIGHTS(W0, W3, K, W0t, W3s)
  const int v = tid & 63, rg = tid >> 6, kcol = tid & 127, half = tid >> 7;
  const int r0 = blockIdx.x * HEAD_ROWS;
  HEAD_STAGE_ROWS(feat, r0, B)
  float invW = 0.f;
  if constexpr (CW) {
    __shared__ double wred[4];
    FS(cw);
    invW = 1.0f / (float)cw_total(cw, labels, B, wred);
  }
  __syncthreads();
  // ---- head_fwd_kernel ----
  {
    HEAD_HIDDEN_CHAIN(acc, W0t, b0[v])
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + rg * 4 + r;
      HEAD_RELU_DROPOUT(hv, acc[r], row, drop_thr, drop_key, dscale)
      hs[(rg * 4 + r) * 64 + v] = hv;
      if (row < B) hid[(size_t)row * 64 + v] = hv;
    }
  }
  __syncthreads();
  for (int i = tid; i < HEAD_ROWS * K; i += 256) {
    const int rl = i / K, c = i - rl * K, row = r0 + rl;
    HEAD_LOGIT(a, W3s, 64, b3, c, rl)
    lgs[rl * MSIG_MAX_K + c] = a;
    if (row < B) logits[(size_t)row * K + c] = a;
  }
  __syncthreads();
  // ---- ce_kernel, the rows of this group (its sums: loss_finalize) ----
  if (tid < HEAD_ROWS) {
    const int row = r0 + tid;
    if (row < B) {
      const float* lg = &lgs[tid * MSIG_MAX_K];
      const float invB = 1.0f / (float)B;
      int am;
      const float lse = ce_row_lse(lg, K, am);
      const int y = (int)labels[row];
      pred[row] = am;
      const float wy = CW ? cw[y] : 1.f;
      SoftCoef sc{};
      bool soft = false;
      int y2 = y;
      float wy2 = wy;
      if constexpr (ST) {
        sc = soft_coef<CW>(sa.a.eps, sa.a.lam[blockIdx.z], cw, K);
        soft = !sc.plain;
        if (soft) { y2 = (int)labels[B - 1 - row]; wy2 = CW ? cw[y2] : 1.f; }
      }
      for (int c = 0; c < K; ++c) {
        const float p = expf(lg[c] - lse);
        probs[(size_t)row * K + c] = p;
        float dl;
        if (ST && soft) dl = soft_dlogit(sc, p, c, y, y2, wy, wy2, CW ? cw[c] : 1.f, CW ? invW : invB);
        else dl = HEAD_CE_DL(p, c, y, wy, (CW ? invW : invB));
        dlogits[(size_t)row * K + c] = dl;
        dls[tid * MSIG_MAX_K + c] = dl;
      }
    } else {
      for (int c = 0; c < K; ++c) dls[tid * MSIG_MAX_K + c] = 0.f;
    }
  }
  // the backward pieces read hid as 0 for the rows past the batch
  for (int i = tid; i < HEAD_ROWS * 64; i += 256) if (r0 + (i >> 6) >= B) hs[i] = 0.f;
  __syncthreads();
  // ---- head_bwd_kernel ----
  HEAD_GRADS_ZERO
  {
    HEAD_DPRE(W3s, 64, K, a * dscale_bwd)
    __syncthreads();
    HEAD_GRADS_ADD(K)
    HEAD_DFEAT(W0t, dfeat, r0, B)
  }
  float* P = part + (size_t)blockIdx.x * (64 * 128 + 64 + K * 64 + K);
  HEAD_PART_STORE(P, K)
}

// ------------------------------------------------------------------------------------
// out[c] = sum_r part[r*row_stride + c], fp64 accumulation in a fixed order
// ------------------------------------------------------------------------------------
// 32 columns x 8 row-lanes per workgroup; a lane sums every 8th row with 8 loads in flight into 8
// accumulators that are combined in a fixed order (deterministic for a given nrows)
#define CS_COLS 32
#define CS_LANES 8
__device__ __forceinline__ double colsum_lane(const float* __restrict__ p, int nrows, size_t stride, int ry) {
  double a[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = 0.0;
  int r = ry;
  for (; r + 7 * CS_LANES < nrows; r += 8 * CS_LANES) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = p[(size_t)(r + j * CS_LANES) * stride];
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] += (double)v[j];
  }
  for (; r < nrows; r += CS_LANES) a[0] += (double)p[(size_t)r * stride];
  return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}
__device__ __forceinline__ double colsum_fold(double (*red)[CS_COLS], int cx) {
  return ((red[0][cx] + red[1][cx]) + (red[2][cx] + red[3][cx])) + ((red[4][cx] + red[5][cx]) + (red[6][cx] + red[7][cx]));
}

// One launch reduces every job: blockIdx.x walks the 32-column blocks of ALL jobs back to back (blk0[j] = first block of job j),
// blockIdx.y = fold.  Round 4's grid was (blocks of the WIDEST job, jobs, folds): 768 x 32 x folds workgroups of which nine in ten
// found no columns and left — at 15 folds 370 000 workgroups, and the launch took what dispatching them takes (0.16 ms) whatever
// the bytes; now 4 000 per fold, every one with work.
struct ColsumJobs { ColsumJob j[MSIG_MAX_JOBS]; int blk0[MSIG_MAX_JOBS + 1]; int n; };
__device__ __forceinline__ int colsum_find_job(const ColsumJobs& jobs, int blk) {      // uniform: scalar loop over <= 40 entries
  int j = 0;
  while (j + 1 < jobs.n && blk >= jobs.blk0[j + 1]) ++j;
  return j;
}
static int colsum_fill(const ColsumPlan& plan, ColsumJobs& a) {
  int at = 0;
  for (int i = 0; i < plan.n; ++i) { a.j[i] = plan.job[i]; a.blk0[i] = at; at += (plan.job[i].ncols + CS_COLS - 1) / CS_COLS; }
  for (int i = plan.n; i < MSIG_MAX_JOBS; ++i) { a.j[i] = ColsumJob{nullptr, 0, 0, 0, 0, nullptr}; a.blk0[i] = at; }
  a.blk0[MSIG_MAX_JOBS] = at;
  a.n = plan.n;
  return at;
}

// What the three reduction kernels share: the workgroup's job and its fold's pointers, the lane sums of its 32 columns into red,
// the barrier, and — in the lane that owns a live column c (row-lane 0: `owner`) — the folded float sum stored to out[c], or read
// from it when the job is a gradient already in place (nrows == 0: nothing to add up, no barrier).  Every thread of the workgroup
// must call it.
struct ColsumCol { float* out; int c; bool owner; float gsum; };      // out: the job's, of this fold
__device__ __forceinline__ ColsumCol colsum_column(const ColsumJobs& jobs, const FoldCtx& fc, double (*red)[CS_COLS]) {
  const int ji = colsum_find_job(jobs, blockIdx.x);
  ColsumJob jb = jobs.j[ji];
  const int64_t foff_ = (int64_t)fc.slot[blockIdx.y] * fc.stride;
  FS(jb.part); FS(jb.out);
  const int cx = threadIdx.x & (CS_COLS - 1), ry = threadIdx.x / CS_COLS;
  const int c = ((int)blockIdx.x - jobs.blk0[ji]) * CS_COLS + cx;
  if (jb.nrows > 0) {
    red[ry][cx] = c < jb.ncols ? colsum_lane(jb.part + jb.col0 + c, jb.nrows, (size_t)jb.row_stride, ry) : 0.0;
    __syncthreads();
  }
  ColsumCol r{jb.out, c, ry == 0 && c < jb.ncols, 0.f};
  if (r.owner) {
    if (jb.nrows > 0) { r.gsum = (float)colsum_fold(red, cx); jb.out[c] = r.gsum; }
    else r.gsum = jb.out[c];
  }
  return r;
}

// The fused head's loss (launched only then): the one workgroup past the column blocks runs loss_finalize and answers true.
template <bool CW, bool ST>
__device__ __forceinline__ bool colsum_loss_workgroup(const ColsumJobs& jobs, const LossFin& loss_in, const FoldCtx& fc, const SoftT<ST>& sa) {
  if ((int)blockIdx.x != jobs.blk0[MSIG_MAX_JOBS]) return false;
  __shared__ double lred[2][CE_THREADS / 64];
  __shared__ double wred[4];
  LossFin lf = loss_in;
  const int64_t foff_ = (int64_t)fc.slot[blockIdx.y] * fc.stride;
  FS(lf.logits); FS(lf.labels); FS(lf.lossbuf); FS(lf.lacc);
  if constexpr (CW) FS(lf.cw);
  loss_finalize<CW, ST>(lf, lred, wred, sa, (int)blockIdx.y);
  return true;
}

// The <CW, ST> instantiation of a kernel family and its SoftT argument, picked in one place: f(CwSt<CW, ST>{}, SoftT<ST>) launches.
template <bool CW, bool ST> struct CwSt { static constexpr bool cw = CW, st = ST; };
template <typename F>
static void cw_st_dispatch(const float* cw, const SoftArgs* soft, F&& f) {
  if (soft) {
    const SoftT<true> sa{*soft};
    if (cw) f(CwSt<true, true>{}, sa); else f(CwSt<false, true>{}, sa);
  }
  else if (cw) f(CwSt<true, false>{}, SoftT<false>{});
  else f(CwSt<false, false>{}, SoftT<false>{});
}

__global__ __launch_bounds__(256) void colsum_plan_kernel(const ColsumJobs jobs, const FoldCtx fc) {
  __shared__ double red[CS_LANES][CS_COLS];
  colsum_column(jobs, fc, red);
}

template <bool CW, bool ST = false>
__global__ __launch_bounds__(256) void colsum_adam_kernel(const ColsumJobs jobs, const AdamArgs ad_in, const LossFin loss_in, const FoldCtx fc,
                                                          const SoftT<ST> sa) {
  __shared__ double red[CS_LANES][CS_COLS];
  if (colsum_loss_workgroup<CW, ST>(jobs, loss_in, fc, sa)) return;
  AdamArgs ad = ad_in;
  const int64_t foff_ = (int64_t)fc.slot[blockIdx.y] * fc.stride;
  FS(ad.p); FS(ad.g); FS(ad.m); FS(ad.v);
  const ColsumCol col = colsum_column(jobs, fc, red);
  if (col.owner) {
    const int64_t i = (col.out - ad.g) + col.c;
    float m = ad.m[i], v = ad.v[i];
    ad.p[i] = adam_update(ad.p[i], col.gsum, m, v, fc.lr_over_bc1[blockIdx.y], fc.inv_sqrt_bc2[blockIdx.y], ad.b1, ad.b2, ad.eps, ad.wd);
    ad.m[i] = m;
    ad.v[i] = v;
  }
}

int launch_colsum_adam_plan(const ColsumPlan& plan, const AdamArgs& ad, const FoldCtx& fc, hipStream_t st) {
  if (plan.n <= 0) return 0;
  ColsumJobs a;
  const int nblk = colsum_fill(plan, a);
  if (nblk <= 0) return 0;
  {
    MSIG_K("colsum_adam", st);
    const dim3 grid(nblk + (plan.loss.logits ? 1 : 0), fc.n);
    cw_st_dispatch(plan.loss.cw, plan.loss.logits ? plan.soft : nullptr, [&](auto k, const auto& sa) {
      colsum_adam_kernel<decltype(k)::cw, decltype(k)::st><<<grid, 256, 0, st>>>(a, ad, plan.loss, fc, sa);
    });
  }
  MSIG_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------
// Gradient-norm clipping (include/msig_gc.h): colsum_adam's launch as two.  The global norm has to be known between
// the reduction and the Adam update of every element, and a hand-over between workgroups inside one kernel costs a kernel boundary
// on this part — so the boundary is a launch.
//   colsum_sq_kernel  colsum_adam's reduction half on the same grid: writes g, and each workgroup the fp64 sum of its 32 columns'
//                     squares to partial[blockIdx.x] of its fold's clip state (in-place jobs only read and square).  Which
//                     columns a workgroup owns follows from the plan, i.e. from the model's shape: the partials and the order
//                     they are added in do not depend on the folds of the launch.  The fused head's loss workgroup rides along.
//   clip_adam_kernel  a few fat workgroups per fold (the ~4 000 partials are 32 KB: re-read by every workgroup of the launch, so
//                     there are at most a few hundred of those, not thousands): each sums the partials in ONE order (thread t adds
//                     t, t + 256, ..., each wave reduces its lanes, the four wave sums are added in wave order), forms coef, and
//                     walks its share of the column blocks: g' = g * coef stored, then colsum_adam_kernel's Adam statements.
// With coef = 1 the step's bits are the unclipped step's: see the note at the arithmetic of clip_adam_kernel.
// ------------------------------------------------------------------------------------
template <bool CW, bool ST = false>
__global__ __launch_bounds__(256) void colsum_sq_kernel(const ColsumJobs jobs, double* __restrict__ state, const LossFin loss_in, const FoldCtx fc,
                                                        const SoftT<ST> sa) {
  __shared__ double red[CS_LANES][CS_COLS];
  if (colsum_loss_workgroup<CW, ST>(jobs, loss_in, fc, sa)) return;
  const int64_t foff_ = (int64_t)fc.slot[blockIdx.y] * fc.stride;
  FS(state);
  const ColsumCol col = colsum_column(jobs, fc, red);
  if (threadIdx.x < 64) {                                     // wave 0: lanes 0..31 own the columns, lanes 32..63 add zeros
    double sq = col.owner ? (double)col.gsum * (double)col.gsum : 0.0;
    sq = wave_sum_d(sq);
    if (threadIdx.x == 0) state[MSIG_GC_NSTAT + blockIdx.x] = sq;
  }
}

#define CLIP_SUB (256 / CS_COLS)      // column blocks a workgroup covers at once
#define CLIP_U 4                      // of those per thread, their loads in flight together
#define CLIP_MIN_WG 16
__global__ __launch_bounds__(256) void clip_adam_kernel(const ColsumJobs jobs, const AdamArgs ad_in, const ClipArgs cl, const FoldCtx fc) {
  __shared__ double wsum[4];
  AdamArgs ad = ad_in;
  double* state = cl.state;
  const int64_t foff_ = (int64_t)fc.slot[blockIdx.y] * fc.stride;
  FS(state); FS(ad.p); FS(ad.g); FS(ad.m); FS(ad.v);
  ad.lr_over_bc1 = fc.lr_over_bc1[blockIdx.y];
  ad.inv_sqrt_bc2 = fc.inv_sqrt_bc2[blockIdx.y];
  const int nblk = jobs.blk0[MSIG_MAX_JOBS];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < nblk; i += 256) s += state[MSIG_GC_NSTAT + i];
  s = wave_sum_d(s);
  if ((tid & 63) == 0) wsum[tid >> 6] = s;
  __syncthreads();
  const double N = sqrt((wsum[0] + wsum[1]) + (wsum[2] + wsum[3]));
  const double max_norm = cl.max_norm[blockIdx.y];
  const double q = max_norm / (N + 1e-6);
  const float coef = (float)(q > 1.0 ? 1.0 : q);             // torch's clamp(max=1): a NaN quotient stays NaN
  if (blockIdx.x == 0 && tid == 0) {                          // the fold's running statistics: one thread, stream order
    state[MSIG_GC_SUM] += N;
    state[MSIG_GC_MAX] = N > state[MSIG_GC_MAX] ? N : state[MSIG_GC_MAX];
    state[MSIG_GC_CLIPPED] += N > max_norm ? 1.0 : 0.0;
    state[MSIG_GC_LAST] = N;
  }
  const int cx = tid & (CS_COLS - 1), sub = tid / CS_COLS;
  for (int b0 = (int)blockIdx.x * (CLIP_SUB * CLIP_U); b0 < nblk; b0 += (int)gridDim.x * (CLIP_SUB * CLIP_U)) {
    int64_t idx[CLIP_U];
    float g[CLIP_U], p[CLIP_U], m[CLIP_U], v[CLIP_U];
#pragma unroll
    for (int u = 0; u < CLIP_U; ++u) {
      const int blk = b0 + u * CLIP_SUB + sub;
      idx[u] = -1;
      g[u] = p[u] = m[u] = v[u] = 0.f;
      if (blk < nblk) {
        int ji = 0;
        for (int j = 1; j < jobs.n; ++j) ji += blk >= jobs.blk0[j] ? 1 : 0;      // colsum_find_job with a uniform trip count
        const int c = (blk - jobs.blk0[ji]) * CS_COLS + cx;
        if (c < jobs.j[ji].ncols) idx[u] = (jobs.j[ji].out - ad_in.g) + c;       // both are fold 0's pointers
      }
      if (idx[u] >= 0) { g[u] = ad.g[idx[u]]; p[u] = ad.p[idx[u]]; m[u] = ad.m[idx[u]]; v[u] = ad.v[idx[u]]; }
    }
#pragma unroll
    for (int u = 0; u < CLIP_U; ++u) {
      if (idx[u] < 0) continue;
      const int64_t i = idx[u];
      {
        // The clip is a multiplication of its own, one rounding; then the train step's Adam (msig_dev.h adam_update), the function
        // colsum_adam_kernel calls: with coef = 1 the step's bits are the unclipped step's.
#pragma clang fp contract(off)
        const float gsum = g[u] * coef;
        ad.g[i] = gsum;
        ad.p[i] = adam_update(p[u], gsum, m[u], v[u], ad.lr_over_bc1, ad.inv_sqrt_bc2, ad.b1, ad.b2, ad.eps, ad.wd);
        ad.m[i] = m[u];
        ad.v[i] = v[u];
      }
    }
  }
}

int launch_colsum_clip_adam_plan(const ColsumPlan& plan, const AdamArgs& ad, const FoldCtx& fc, const ClipArgs& cl, hipStream_t st) {
  if (plan.n <= 0) return 0;
  ColsumJobs a;
  const int nblk = colsum_fill(plan, a);
  if (nblk <= 0) return 0;
  if (nblk > cl.cap) return MSIG_E_WORKSPACE;      // msig_gc_state_bytes bounds the plan's column blocks: not reached
  {
    MSIG_K("colsum_sq", st);
    const dim3 grid(nblk + (plan.loss.logits ? 1 : 0), fc.n);
    cw_st_dispatch(plan.loss.cw, plan.loss.logits ? plan.soft : nullptr, [&](auto k, const auto& sa) {
      colsum_sq_kernel<decltype(k)::cw, decltype(k)::st><<<grid, 256, 0, st>>>(a, cl.state, plan.loss, fc, sa);
    });
  }
  MSIG_LAUNCH_CHECK();
  {
    MSIG_K("clip_adam", st);
    // about one workgroup per CU over the whole launch, never fewer than CLIP_MIN_WG per fold; the bits do not depend on the count
    const int per_pass = CLIP_SUB * CLIP_U;
    int wg = 256 / fc.n;
    if (wg < CLIP_MIN_WG) wg = CLIP_MIN_WG;
    if (wg > (nblk + per_pass - 1) / per_pass) wg = (nblk + per_pass - 1) / per_pass;
    clip_adam_kernel<<<dim3(wg, fc.n), 256, 0, st>>>(a, ad, cl, fc);
  }
  MSIG_LAUNCH_CHECK();
  return 0;
}

int launch_colsum_plan(const ColsumPlan& plan, const FoldCtx& fc, hipStream_t st) {
  if (plan.n <= 0) return 0;
  ColsumJobs a;
  const int nblk = colsum_fill(plan, a);
  if (nblk <= 0) return 0;
  { MSIG_K("colsum", st); colsum_plan_kernel<<<dim3(nblk, fc.n), 256, 0, st>>>(a, fc); }
  MSIG_LAUNCH_CHECK();
  return 0;
}

PartOffsets part_offsets(const StageDims& d) {
  PartOffsets o;
  const int64_t units = (int64_t)d.NT * d.TP;
  o.gru_rows = (int)(units < MSIG_DW_WG ? units : MSIG_DW_WG);
  int64_t at = 0;
  auto take = [&](int64_t n) { const int64_t r = at; at += (n + 63) / 64 * 64; return r; };
  o.head = take((int64_t)HEAD_WG * (64 * 128 + 64 + d.K * 64 + d.K));
  o.l1 = take(2 * (int64_t)o.gru_rows * (192 * 128 + 192 * 64 + 256));
  o.l0 = take(2 * (int64_t)o.gru_rows * (192 * 32 + 192 * 64 + 256));
  o.conv2 = take((int64_t)MSIG_CONV_DW_WG * 2560);
  o.conv1 = take((int64_t)MSIG_CONV_DW_WG * 16 * d.C * 7);
  o.total = at;
  return o;
}

// ------------------------------------------------------------------------------------
// msig_adam_step: Adam on a flat buffer, four elements per thread.  Its second moment is the fused form (msig_dev.h ADAM_FUSED_V),
// as this kernel has always been compiled: not the train step's, from the second step on.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, int64_t n4, float lr_over_bc1, float inv_sqrt_bc2,
                                                   float b1, float b2, float eps, float wd) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
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

// ------------------------------------------------------------------------------------
// Host launchers
// ------------------------------------------------------------------------------------
int launch_head_fwd(const msig_batch* b, const StageDims& d, const WsPtrs& w, const int64_t* po, const FoldCtx& fc, hipStream_t st,
                    const StepOpts& o, bool mc_tail) {
  const float* cw = o.cw;
  const SoftArgs* soft = o.soft;
  const float* P = b->params;
  const int thr = (b->training || mc_tail) ? b->dropout_thr : 0;
  const int ngroups = (d.B + HEAD_ROWS - 1) / HEAD_ROWS;
  const int grid = ngroups < 1024 ? ngroups : 1024;
  { MSIG_K("head_fwd", st); head_fwd_kernel<<<dim3(grid, 1, fc.n), 256, 0, st>>>(w.p<float>(MSIG_WS_FEAT), P + po[MSIG_P_CLS0_W], P + po[MSIG_P_CLS0_B], P + po[MSIG_P_CLS3_W],
                                         P + po[MSIG_P_CLS3_B], w.p<float>(MSIG_WS_HID), w.p<float>(MSIG_WS_LOGITS), d.B, d.K, thr,
                                         b->key_head, drop_scale(thr), fc); }
  MSIG_LAUNCH_CHECK();
  if (mc_tail) return 0;
  if (b->labels) {
    MSIG_K("ce", st);
    float* dl = msig_keeps(b) ? w.p<float>(MSIG_WS_DLOGITS) : nullptr;
    cw_st_dispatch(cw, soft, [&](auto k, const auto& sa) {
      ce_kernel<decltype(k)::cw, decltype(k)::st><<<dim3(1, 1, fc.n), CE_THREADS, 0, st>>>(
          w.p<float>(MSIG_WS_LOGITS), b->labels, w.p<float>(MSIG_WS_PROBS), w.p<int>(MSIG_WS_PRED), dl, w.p<float>(MSIG_WS_LOSS), b->loss_acc, cw, d.B,
          d.K, fc, sa);
    });
  } else {
    MSIG_K("softmax", st);
    softmax_kernel<<<dim3((d.B + 255) / 256, 1, fc.n), 256, 0, st>>>(w.p<float>(MSIG_WS_LOGITS), w.p<float>(MSIG_WS_PROBS), w.p<int>(MSIG_WS_PRED), d.B, d.K, fc);
  }
  MSIG_LAUNCH_CHECK();
  return 0;
}

int launch_head_bwd(const msig_batch* b, const float* dlogits, const StageDims& d, const WsPtrs& w, const int64_t* po, ColsumPlan& plan,
                    const FoldCtx& fc, hipStream_t st) {
  const float* P = b->params;
  float* G = b->grads;
  const int thr = b->training ? b->dropout_thr : 0;
  const int ngroups = (d.B + HEAD_ROWS - 1) / HEAD_ROWS;
  const int grid = ngroups < HEAD_WG ? ngroups : HEAD_WG;
  float* part = w.p<float>(MSIG_WS_GRAD_PART) + part_offsets(d).head;
  const int PS = 64 * 128 + 64 + d.K * 64 + d.K;
  { MSIG_K("head_bwd", st); head_bwd_kernel<<<dim3(grid, 1, fc.n), 256, 0, st>>>(dlogits ? dlogits : w.p<float>(MSIG_WS_DLOGITS), w.p<float>(MSIG_WS_FEAT), w.p<float>(MSIG_WS_HID),
                                         P + po[MSIG_P_CLS0_W], P + po[MSIG_P_CLS3_W], w.p<float>(MSIG_WS_DFEAT), part, d.B, d.K,
                                         thr > 0 ? drop_scale(thr) : 1.0f, fc); }
  MSIG_LAUNCH_CHECK();
  const bool ok = plan.add(part, grid, PS, 0, 64 * 128, G + po[MSIG_P_CLS0_W]) && plan.add(part, grid, PS, 64 * 128, 64, G + po[MSIG_P_CLS0_B]) &&
                  plan.add(part, grid, PS, 64 * 128 + 64, d.K * 64, G + po[MSIG_P_CLS3_W]) &&
                  plan.add(part, grid, PS, 64 * 128 + 64 + d.K * 64, d.K, G + po[MSIG_P_CLS3_B]);
  return ok ? 0 : MSIG_E_SHAPE;
}

// The fused head applies where a workgroup per group of 16 rows is also head_bwd_kernel's grid (one partial row per group).
bool head_step_applies(const msig_batch* b, const StageDims& d) {
  return b->training && b->labels && (d.B + HEAD_ROWS - 1) / HEAD_ROWS <= HEAD_WG;
}
int launch_head_step(const msig_batch* b, const StageDims& d, const WsPtrs& w, const int64_t* po, ColsumPlan& plan, const FoldCtx& fc, hipStream_t st,
                     const StepOpts& o) {
  const float* cw = o.cw;
  const SoftArgs* soft = o.soft;
  const float* P = b->params;
  float* G = b->grads;
  const int thr = b->dropout_thr;
  const int grid = (d.B + HEAD_ROWS - 1) / HEAD_ROWS;
  float* part = w.p<float>(MSIG_WS_GRAD_PART) + part_offsets(d).head;
  const int PS = 64 * 128 + 64 + d.K * 64 + d.K;
  {
    MSIG_K("head_step", st);
    cw_st_dispatch(cw, soft, [&](auto k, const auto& sa) {
      head_step_kernel<decltype(k)::cw, decltype(k)::st><<<dim3(grid, 1, fc.n), 256, 0, st>>>(
          w.p<float>(MSIG_WS_FEAT), P + po[MSIG_P_CLS0_W], P + po[MSIG_P_CLS0_B], P + po[MSIG_P_CLS3_W], P + po[MSIG_P_CLS3_B], b->labels,
          w.p<float>(MSIG_WS_HID), w.p<float>(MSIG_WS_LOGITS), w.p<float>(MSIG_WS_PROBS), w.p<int>(MSIG_WS_PRED), w.p<float>(MSIG_WS_DLOGITS),
          w.p<float>(MSIG_WS_DFEAT), part, cw, d.B, d.K, thr, b->key_head, drop_scale(thr), thr > 0 ? drop_scale(thr) : 1.0f, fc, sa);
    });
  }
  MSIG_LAUNCH_CHECK();
  plan.loss = LossFin{w.p<float>(MSIG_WS_LOGITS), b->labels, w.p<float>(MSIG_WS_LOSS), b->loss_acc, d.B, d.K, cw};
  plan.soft = soft;
  const bool ok = plan.add(part, grid, PS, 0, 64 * 128, G + po[MSIG_P_CLS0_W]) && plan.add(part, grid, PS, 64 * 128, 64, G + po[MSIG_P_CLS0_B]) &&
                  plan.add(part, grid, PS, 64 * 128 + 64, d.K * 64, G + po[MSIG_P_CLS3_W]) &&
                  plan.add(part, grid, PS, 64 * 128 + 64 + d.K * 64, d.K, G + po[MSIG_P_CLS3_B]);
  return ok ? 0 : MSIG_E_SHAPE;
}

int launch_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps, float wd,
                int64_t step, hipStream_t st) {
  const double bc1 = 1.0 - pow((double)b1, (double)step), bc2 = 1.0 - pow((double)b2, (double)step);
  const int64_t n4 = n / 4;
  int64_t blocks = (n4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  { MSIG_K("adam", st); adam_kernel<<<(int)blocks, 256, 0, st>>>(p, g, m, v, n4, (float)((double)lr / bc1), (float)(1.0 / sqrt(bc2)), b1, b2, eps, wd); }
  MSIG_LAUNCH_CHECK();
  return 0;
}
