// include/msig_en.h: the reduction of M ensemble members' logits to the per-window statistics.  The arithmetic
// is the one mc.hip's mc_reduce_kernel instantiates (member_stats.h) — the same sums in the same order, so that the common outputs
// carry its bits — over logits that lie member-major: member m's (N, K) block where its own forward left it.
#include "member_stats.h"

int msig_multi_fold_ctx(const msig_multi* m, FoldCtx& fc);                                  // api.hip: msig_multi's own checks

// member_stats (member_stats.h) with every statistic, member_pred and disagreement included
__global__ __launch_bounds__(MEMBER_THREADS) void en_reduce_kernel(const float* __restrict__ logits, const MemberWhere wh, int M, int K,
                                                                   float* __restrict__ mean_p, float* __restrict__ std_p,
                                                                   int* __restrict__ pred, float* __restrict__ entropy,
                                                                   float* __restrict__ expected_entropy, float* __restrict__ mutual_info,
                                                                   int* __restrict__ votes, int* __restrict__ member_pred,
                                                                   float* __restrict__ disagreement) {
  member_stats<false, MEMBER_VOTERS, false>(logits, wh, M, K, 1.0, mean_p, std_p, pred, entropy, expected_entropy, mutual_info, votes, member_pred,
                                     disagreement);
}

// ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
extern "C" int msig_en_abi_version(void) { return MSIG_EN_ABI_VERSION; }

static int en_reduce(const float* logits, const MemberWhere& wh, int32_t M, int32_t max_members, int32_t N, int32_t K, float* mean_p,
                     float* std_p, int32_t* pred, float* entropy, float* expected_entropy, float* mutual_info, int32_t* votes,
                     int32_t* member_pred, float* disagreement, void* stream) {
  return member_launch("en_reduce", logits, M, max_members, N, K, wh.member_stride < (int64_t)N * K,
                       {mean_p, std_p, pred, entropy, expected_entropy, mutual_info, votes, member_pred, disagreement}, (hipStream_t)stream,
                       [&](dim3 grid, dim3 block, hipStream_t st) {
                         en_reduce_kernel<<<grid, block, 0, st>>>(logits, wh, M, K, mean_p, std_p, pred, entropy, expected_entropy, mutual_info,
                                                                  votes, member_pred, disagreement);
                       });
}

extern "C" int msig_en_reduce(const float* logits, int64_t member_stride_floats, int32_t M, int32_t N, int32_t K, float* mean_p,
                              float* std_p, int32_t* pred, float* entropy, float* expected_entropy, float* mutual_info, int32_t* votes,
                              int32_t* member_pred, float* disagreement, void* stream) {
  return en_reduce(logits, member_where_stacked(member_stride_floats), M, MSIG_EN_MAX_MEMBERS, N, K, mean_p, std_p, pred, entropy,
                   expected_entropy, mutual_info, votes, member_pred, disagreement, stream);
}

extern "C" int msig_en_reduce_multi(const float* logits0, const msig_multi* m, int32_t N, int32_t K, float* mean_p, float* std_p,
                                    int32_t* pred, float* entropy, float* expected_entropy, float* mutual_info, int32_t* votes,
                                    int32_t* member_pred, float* disagreement, void* stream) {
  FoldCtx fc; const int rc = msig_multi_fold_ctx(m, fc); if (rc) return rc;
  return en_reduce(logits0, member_where_from_multi(fc), fc.n, MSIG_MAX_FOLDS, N, K, mean_p, std_p, pred, entropy, expected_entropy,
                   mutual_info, votes, member_pred, disagreement, stream);
}
