// The fp64 reduction of M members' logit rows to per-window statistics, once: Monte-Carlo dropout's passes (mc.hip, include/
// msig_mc.h), a deep ensemble's members (ensemble.hip, include/msig_en.h) and a distillation teacher's members (distill.hip,
// include/msig_kd.h) are instantiations of member_stats below, which is why their common outputs carry the same bits.
#pragma once
#include <math.h>
#include <initializer_list>
#include "msig_dev.h"
#include "../../include/msig_mc.h"
#include "../../include/msig_en.h"
#include "../../include/msig_kd.h"

static_assert(MSIG_MC_MAX_SAMPLES == MSIG_EN_MAX_MEMBERS && MSIG_EN_MAX_MEMBERS == MSIG_KD_MAX_MEMBERS,
              "member_stats sizes its LDS arrays by one member count");
#define MEMBER_MAX MSIG_EN_MAX_MEMBERS
#define MEMBER_THREADS 256
static_assert(MEMBER_MAX <= MEMBER_THREADS && MSIG_MAX_K <= MEMBER_THREADS, "one thread per member, then one per class");

// The row of member m, window n starts at logits + member * member_stride + n * window_stride, in floats.  The window stride is a
// compile-time property of the layout, so that each kernel multiplies by the integers its predecessor multiplied by:
//   window-major (WINDOW_MAJOR: msig_mc_reduce)  member = m, member_stride = K, window_stride = M * K: row (n * M + m) of K floats;
//                                                no MemberWhere is read
//   stacked (msig_en_reduce, msig_kd_teacher)    member = m, member_stride = the caller's, window_stride = K
//   arena slots (the *_multi calls)              member = slot[m], member_stride = stride_bytes / 4, window_stride = K
struct MemberWhere {
  int64_t member_stride;
  int32_t n_slots;
  int32_t slot[MSIG_MAX_FOLDS];
};

// which statistics an instantiation produces
enum {
  MEMBER_MEAN = 0,       // mean_p alone (the teacher)
  MEMBER_FULL = 1,       // + std_p, pred, entropy, expected_entropy, mutual_info, votes
  MEMBER_VOTERS = 2      // + member_pred, disagreement
};

__device__ __forceinline__ double member_plogp(double p) { return p > 0.0 ? p * log(p) : 0.0; }

// ------------------------------------------------------------------------------------
// One workgroup of MEMBER_THREADS per window n = blockIdx.x, all of it in fp64.
//   phase 1  thread m < M: p_m = softmax of member m's row n (max-subtracted; TEMPERED: of the row over T) into LDS, H(p_m) and
//            the row's first maximal logit;
//   phase 2  thread k < K: mu_k = (sum_m p_m[k]) / M and the squared deviations, both in increasing m; the votes for class k;
//   phase 3  thread 0: the first argmax of mu, H(mu), the mean of H(p_m) in increasing m, their difference; the disagreement from
//            the integer votes.
// Every sum has one owner and one order, fixed by (M, K): the bits of a window depend on nothing but its own M rows.  Every output
// but mean_p may be NULL.  MEMBER_MEAN stops after phase 2's mean and keeps only the probabilities in LDS.  At T = 1 the division
// is exact, so a tempered mean_p is the untempered one bit for bit.  Votes are cast on the raw logits, so only MEMBER_MEAN is
// tempered.
// ------------------------------------------------------------------------------------
template <bool TEMPERED, int STATS, bool WINDOW_MAJOR>
__device__ __forceinline__ void member_stats(const float* __restrict__ logits, const MemberWhere& wh, int M, int K, double T,
                                             float* __restrict__ mean_p, float* __restrict__ std_p, int* __restrict__ pred,
                                             float* __restrict__ entropy, float* __restrict__ expected_entropy,
                                             float* __restrict__ mutual_info, int* __restrict__ votes, int* __restrict__ member_pred,
                                             float* __restrict__ disagreement) {
  static_assert(!TEMPERED || STATS == MEMBER_MEAN, "votes and entropies are those of the raw logits");
  constexpr bool FULL = STATS != MEMBER_MEAN, VOTERS = STATS == MEMBER_VOTERS;
  __shared__ double ps[MEMBER_MAX * MSIG_MAX_K];
  __shared__ double hs[MEMBER_MAX];          // the arrays below are touched by FULL alone: MEMBER_MEAN's LDS is ps
  __shared__ double ms[MSIG_MAX_K];
  __shared__ int vs[MEMBER_MAX];
  __shared__ int cs[MSIG_MAX_K];             // VOTERS alone
  const int64_t n = blockIdx.x;
  const int tid = threadIdx.x;
  if (tid < M) {
    const float* __restrict__ row;
    if constexpr (WINDOW_MAJOR) {
      row = logits + (n * M + tid) * K;
    } else {
      const int64_t blk = wh.n_slots ? (int64_t)wh.slot[tid] : (int64_t)tid;
      row = logits + blk * wh.member_stride + n * K;
    }
    double e[MSIG_MAX_K];
    double sum = 0.0;
    int am = 0;
    if constexpr (TEMPERED) {
      double u[MSIG_MAX_K];
      for (int k = 0; k < K; ++k) u[k] = (double)row[k] / T;
      double mx = u[0];
      for (int k = 1; k < K; ++k) if (u[k] > mx) mx = u[k];
      for (int k = 0; k < K; ++k) { e[k] = exp(u[k] - mx); sum += e[k]; }
    } else {
      double mx = (double)row[0];
      for (int k = 1; k < K; ++k) {
        const double v = (double)row[k];
        if (v > mx) { mx = v; am = k; }
      }
      for (int k = 0; k < K; ++k) { e[k] = exp((double)row[k] - mx); sum += e[k]; }
    }
    double h = 0.0;
    for (int k = 0; k < K; ++k) {
      const double p = e[k] / sum;
      ps[tid * K + k] = p;
      if constexpr (FULL) h -= member_plogp(p);
    }
    if constexpr (FULL) { hs[tid] = h; vs[tid] = am; }
    if constexpr (VOTERS) if (member_pred) member_pred[n * M + tid] = am;
  }
  __syncthreads();
  if (tid < K) {
    double acc = 0.0;
    int cnt = 0;
    for (int s = 0; s < M; ++s) {
      acc += ps[s * K + tid];
      if constexpr (FULL) cnt += vs[s] == tid ? 1 : 0;
    }
    const double m = acc / (double)M;
    double sq = 0.0;
    if constexpr (FULL) {
      for (int s = 0; s < M; ++s) { const double d = ps[s * K + tid] - m; sq += d * d; }
      ms[tid] = m;
      if constexpr (VOTERS) cs[tid] = cnt;
    }
    mean_p[n * K + tid] = (float)m;
    if constexpr (FULL) {
      if (std_p) std_p[n * K + tid] = (float)sqrt(sq / (double)M);
      if (votes) votes[n * K + tid] = cnt;
    }
  }
  if constexpr (FULL) {
    __syncthreads();
    if (tid == 0) {
      int am = 0;
      double h = 0.0;
      for (int k = 0; k < K; ++k) {
        if (ms[k] > ms[am]) am = k;
        h -= member_plogp(ms[k]);
      }
      double eh = 0.0;
      for (int s = 0; s < M; ++s) eh += hs[s];
      eh /= (double)M;
      if (pred) pred[n] = am;
      if (entropy) entropy[n] = (float)h;
      if (expected_entropy) expected_entropy[n] = (float)eh;
      if (mutual_info) mutual_info[n] = (float)(h - eh);
      if constexpr (VOTERS) if (disagreement) {
        int same = 0;                                          // ordered pairs that agree: sum_k v_k (v_k - 1) <= 256 * 255
        for (int k = 0; k < K; ++k) same += cs[k] * (cs[k] - 1);
        disagreement[n] = M > 1 ? (float)(1.0 - (double)same / (double)(M * (M - 1))) : 0.0f;
      }
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// the members of a *_multi call: msig_multi's arenas and its slots
inline MemberWhere member_where_from_multi(const FoldCtx& fc) {
  MemberWhere wh{};
  wh.member_stride = fc.stride / 4;                            // stride_bytes is a multiple of 256
  wh.n_slots = fc.n;
  for (int i = 0; i < fc.n; ++i) wh.slot[i] = fc.slot[i];
  return wh;
}
inline MemberWhere member_where_stacked(int64_t member_stride_floats) {
  MemberWhere wh{};
  wh.member_stride = member_stride_floats;
  return wh;
}

// The checks every reduction call makes, in the order the headers document, then ONE launch of `launch(grid, block, stream)` under
// the profile name `name`: NULL (logits, the first of `ptrs`), the shape, `bad_shape` (what the call checks beside: the member
// stride, the temperature), 4-byte alignment of logits and of every pointer in `ptrs` (NULL is aligned).
template <class Launch>
inline int member_launch(const char* name, const float* logits, int32_t M, int32_t max_members, int32_t N, int32_t K, bool bad_shape,
                         std::initializer_list<const void*> ptrs, hipStream_t st, Launch launch) {
  if (!logits || !*ptrs.begin()) return MSIG_E_NULL;
  if (N < 1 || M < 1 || M > max_members || K < 2 || K > MSIG_MAX_K) return MSIG_E_SHAPE;
  if ((int64_t)M * N >= ((int64_t)1 << 31)) return MSIG_E_SHAPE;
  if (bad_shape) return MSIG_E_SHAPE;
  if (msig_misaligned(logits, 3)) return MSIG_E_ALIGN;
  for (const void* p : ptrs) if (msig_misaligned(p, 3)) return MSIG_E_ALIGN;
  MSIG_K(name, st);
  launch(dim3((unsigned)N), dim3(MEMBER_THREADS), st);
  MSIG_LAUNCH_CHECK();
  return 0;
}
