// include/msig_ab.h: label-free BatchNorm adaptation (AdaBN).  The convolutions are frontend.hip's, launched with
// their per-workgroup partial sums on (api.hip); here are the two kernels that are new: the merge of a batch's partial rows into
// the caller's fp64 accumulator, and the commit of an accumulator into a BatchNorm state.
#include "msig_dev.h"
#include "../../include/msig_ab.h"

// ------------------------------------------------------------------------------------
// part[nrows][2 * CH] (sum[CH], sumsq[CH] per workgroup of the convolution) of fold z -> acc of fold z:
//   acc[sum0 + c] += colsum(c), acc[sq0 + c] += colsum(CH + c), acc[cnt] += count.
// One workgroup per fold reduces in fin_colsums' order — the order bn_finalize_kernel sums the same rows in, so one batch into an
// empty accumulator holds exactly the sums a training forward's finalize divides — and is the accumulator's only writer; launches
// on one stream are ordered, so the read-modify-write needs no atomic.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(FIN_THREADS) void ab_merge_kernel(const float* __restrict__ part, int nrows, int CH, int cnt, int sum0, int sq0,
                                                               double count, double* __restrict__ acc, const FoldCtx fc) {
  FOLD_BEGIN; FS(part); FS(acc);
  __shared__ double red[FIN_THREADS];
  const int tid = threadIdx.x;
  double s1, s2;
  bn_batch_sums(part, nrows, CH, count, red, s1, s2);      // the sums bn_finalize_kernel divides (msig_dev.h)
  if (tid < CH) {
    acc[sum0 + tid] += s1;
    acc[sq0 + tid] += s2;
  }
  if (tid == 0) acc[cnt] += count;
}

int launch_ab_merge(const float* part, int nrows, int stage, double count, double* acc, const FoldCtx& fc, hipStream_t st) {
  const bool s1 = stage == 1;
  MSIG_K("ab_merge", st);
  ab_merge_kernel<<<dim3(1, 1, fc.n), FIN_THREADS, 0, st>>>(part, nrows, s1 ? 16 : 32, s1 ? MSIG_AB_N1 : MSIG_AB_N2, s1 ? MSIG_AB_SUM1 : MSIG_AB_SUM2,
                                                          s1 ? MSIG_AB_SQ1 : MSIG_AB_SQ2, count, acc, fc);
  MSIG_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------
// The stage's running mean and variance from its accumulated sums: bn_finalize_kernel's statements (mean, variance clamped at 0,
// unbiased correction, bn_running_update with momentum = alpha), on the whole set's sums instead of one batch's.  src and dst
// may be the same buffer: a thread reads its own element before it writes it.  A count below 2 has no unbiased variance: the
// stage keeps the source's values.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void ab_commit_kernel(const double* acc, int CH, int cnt, int sum0, int sq0, int mean0, int var0, float momentum,
                                                       const float* bn_src, float* bn_dst, const FoldCtx fc) {
  FOLD_BEGIN; FS(acc); FS(bn_src); FS(bn_dst);
  const int tid = threadIdx.x;
  if (tid >= CH) return;
  const float* run_mean = bn_src + mean0;
  const float* run_var = bn_src + var0;
  const double count = acc[cnt];
  float new_mean = run_mean[tid], new_var = run_var[tid];
  if (count >= 2.0) {
    const double mean = acc[sum0 + tid] / count;
    double var = acc[sq0 + tid] / count - mean * mean;
    if (var < 0.0) var = 0.0;
    const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
    bn_running_update(momentum, (float)mean, (float)unbiased, run_mean[tid], run_var[tid], new_mean, new_var);
  }
  bn_dst[mean0 + tid] = new_mean;
  bn_dst[var0 + tid] = new_var;
}

int launch_ab_commit(const double* acc, int stage, float alpha, const float* bn_src, float* bn_dst, const FoldCtx& fc, hipStream_t st) {
  const bool s1 = stage == 1;
  MSIG_K("ab_commit", st);
  ab_commit_kernel<<<dim3(1, 1, fc.n), 64, 0, st>>>(acc, s1 ? 16 : 32, s1 ? MSIG_AB_N1 : MSIG_AB_N2, s1 ? MSIG_AB_SUM1 : MSIG_AB_SUM2,
                                                  s1 ? MSIG_AB_SQ1 : MSIG_AB_SQ2, s1 ? 0 : 32, s1 ? 16 : 64, alpha, bn_src, bn_dst, fc);
  MSIG_LAUNCH_CHECK();
  return 0;
}
