// include/msig_en.h: the reduction of M ensemble members' logits to the per-window statistics.  The arithmetic
// is mc.hip's mc_reduce_kernel statement for statement — the same sums in the same order, so that the common outputs carry its bits —
// over logits that lie member-major: member m's (N, K) block where its own forward left it.
#include <math.h>
#include "msig_dev.h"
#include "../../include/msig_en.h"

#define EN_THREADS 256

int msig_multi_fold_ctx(const msig_multi* m, FoldCtx& fc);                                  // api.hip: msig_multi's own checks

// where member m's block starts, in floats from `logits`: (n_slots ? slot[m] : m) * stride
struct EnWhere {
  int64_t stride;
  int32_t n_slots;
  int32_t slot[MSIG_MAX_FOLDS];
};

// ------------------------------------------------------------------------------------
// One workgroup per window n, all of it in fp64.
//   phase 1  thread m < M: p_m = softmax of member m's row n (max-subtracted) into LDS, H(p_m) and the row's first maximal logit;
//   phase 2  thread k < K: mu_k = (sum_m p_m[k]) / M and the squared deviations, both in increasing m; the votes for class k;
//   phase 3  thread 0: the first argmax of mu, H(mu), the mean of H(p_m) in increasing m, their difference; the disagreement from
//            the integer votes.
// Every sum has one owner and one order, fixed by (M, K): the bits of a window depend on nothing but its own M rows.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ double en_plogp(double p) { return p > 0.0 ? p * log(p) : 0.0; }

__global__ __launch_bounds__(EN_THREADS) void en_reduce_kernel(const float* __restrict__ logits, const EnWhere wh, int M, int K,
                                                               float* __restrict__ mean_p, float* __restrict__ std_p, int* __restrict__ pred,
                                                               float* __restrict__ entropy, float* __restrict__ expected_entropy,
                                                               float* __restrict__ mutual_info, int* __restrict__ votes,
                                                               int* __restrict__ member_pred, float* __restrict__ disagreement) {
  __shared__ double ps[MSIG_EN_MAX_MEMBERS * MSIG_MAX_K];
  __shared__ double hs[MSIG_EN_MAX_MEMBERS];
  __shared__ double ms[MSIG_MAX_K];
  __shared__ int vs[MSIG_EN_MAX_MEMBERS];
  __shared__ int cs[MSIG_MAX_K];
  const int64_t n = blockIdx.x;
  const int tid = threadIdx.x;
  if (tid < M) {
    const int64_t blk = wh.n_slots ? (int64_t)wh.slot[tid] : (int64_t)tid;
    const float* __restrict__ row = logits + blk * wh.stride + n * K;
    double e[MSIG_MAX_K];
    double mx = (double)row[0];
    int am = 0;
    for (int k = 1; k < K; ++k) {
      const double v = (double)row[k];
      if (v > mx) { mx = v; am = k; }
    }
    double sum = 0.0;
    for (int k = 0; k < K; ++k) { e[k] = exp((double)row[k] - mx); sum += e[k]; }
    double h = 0.0;
    for (int k = 0; k < K; ++k) {
      const double p = e[k] / sum;
      ps[tid * K + k] = p;
      h -= en_plogp(p);
    }
    hs[tid] = h;
    vs[tid] = am;
    if (member_pred) member_pred[n * M + tid] = am;
  }
  __syncthreads();
  if (tid < K) {
    double acc = 0.0;
    int cnt = 0;
    for (int s = 0; s < M; ++s) { acc += ps[s * K + tid]; cnt += vs[s] == tid ? 1 : 0; }
    const double m = acc / (double)M;
    double sq = 0.0;
    for (int s = 0; s < M; ++s) { const double d = ps[s * K + tid] - m; sq += d * d; }
    ms[tid] = m;
    cs[tid] = cnt;
    mean_p[n * K + tid] = (float)m;
    if (std_p) std_p[n * K + tid] = (float)sqrt(sq / (double)M);
    if (votes) votes[n * K + tid] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
    int am = 0;
    double h = 0.0;
    for (int k = 0; k < K; ++k) {
      if (ms[k] > ms[am]) am = k;
      h -= en_plogp(ms[k]);
    }
    double eh = 0.0;
    for (int s = 0; s < M; ++s) eh += hs[s];
    eh /= (double)M;
    if (pred) pred[n] = am;
    if (entropy) entropy[n] = (float)h;
    if (expected_entropy) expected_entropy[n] = (float)eh;
    if (mutual_info) mutual_info[n] = (float)(h - eh);
    if (disagreement) {
      int same = 0;                                          // ordered pairs that agree: sum_k v_k (v_k - 1) <= 256 * 255
      for (int k = 0; k < K; ++k) same += cs[k] * (cs[k] - 1);
      disagreement[n] = M > 1 ? (float)(1.0 - (double)same / (double)(M * (M - 1))) : 0.0f;
    }
  }
}

// ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
static inline bool en_mis(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

extern "C" int msig_en_abi_version(void) { return MSIG_EN_ABI_VERSION; }

static int en_reduce(const float* logits, const EnWhere& wh, int32_t M, int32_t max_members, int32_t N, int32_t K, float* mean_p,
                     float* std_p, int32_t* pred, float* entropy, float* expected_entropy, float* mutual_info, int32_t* votes,
                     int32_t* member_pred, float* disagreement, hipStream_t st) {
  if (!logits || !mean_p) return MSIG_E_NULL;
  if (N < 1 || M < 1 || M > max_members || K < 2 || K > MSIG_MAX_K) return MSIG_E_SHAPE;
  if ((int64_t)M * N >= ((int64_t)1 << 31)) return MSIG_E_SHAPE;
  if (wh.stride < (int64_t)N * K) return MSIG_E_SHAPE;
  if (en_mis(logits, 3) || en_mis(mean_p, 3) || en_mis(std_p, 3) || en_mis(pred, 3) || en_mis(entropy, 3) || en_mis(expected_entropy, 3) ||
      en_mis(mutual_info, 3) || en_mis(votes, 3) || en_mis(member_pred, 3) || en_mis(disagreement, 3))
    return MSIG_E_ALIGN;
  MSIG_K("en_reduce", st);
  en_reduce_kernel<<<dim3((unsigned)N), EN_THREADS, 0, st>>>(logits, wh, M, K, mean_p, std_p, pred, entropy, expected_entropy, mutual_info,
                                                             votes, member_pred, disagreement);
  MSIG_LAUNCH_CHECK();
  return 0;
}

extern "C" int msig_en_reduce(const float* logits, int64_t member_stride_floats, int32_t M, int32_t N, int32_t K, float* mean_p,
                              float* std_p, int32_t* pred, float* entropy, float* expected_entropy, float* mutual_info, int32_t* votes,
                              int32_t* member_pred, float* disagreement, void* stream) {
  EnWhere wh{};
  wh.stride = member_stride_floats;
  return en_reduce(logits, wh, M, MSIG_EN_MAX_MEMBERS, N, K, mean_p, std_p, pred, entropy, expected_entropy, mutual_info, votes, member_pred,
                   disagreement, (hipStream_t)stream);
}

extern "C" int msig_en_reduce_multi(const float* logits0, const msig_multi* m, int32_t N, int32_t K, float* mean_p, float* std_p,
                                    int32_t* pred, float* entropy, float* expected_entropy, float* mutual_info, int32_t* votes,
                                    int32_t* member_pred, float* disagreement, void* stream) {
  FoldCtx fc; const int rc = msig_multi_fold_ctx(m, fc); if (rc) return rc;
  EnWhere wh{};
  wh.stride = fc.stride / 4;                                 // stride_bytes is a multiple of 256
  wh.n_slots = fc.n;
  for (int i = 0; i < fc.n; ++i) wh.slot[i] = fc.slot[i];
  return en_reduce(logits0, wh, fc.n, MSIG_MAX_FOLDS, N, K, mean_p, std_p, pred, entropy, expected_entropy, mutual_info, votes, member_pred,
                   disagreement, (hipStream_t)stream);
}
