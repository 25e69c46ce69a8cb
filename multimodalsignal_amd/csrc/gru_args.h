// Declarations shared by the GRU kernel files (gru.hip, gru_bwd4.hip, gru_bwd6.hip): argument blocks, fold-batching macros, the static
// for, diagnostic stamps and their report.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <type_traits>
#include <utility>
#include "msig_dev.h"

#define HS 68    // LDS row stride (floats) of the 16x64 state tile
#define DGS 196  // LDS row stride of the 16x192 dgh tile (backward recurrence)
#define RS 272   // LDS row stride of the 16x256 dg tile (bulk kernels)

// In-kernel phase stamps: compiled only into the diagnostic library (make stamps); never in the product .so.
#ifdef MSIG_STAMPS
#include <stdarg.h>
#include <initializer_list>
#include <vector>
#define STAMP_DECL unsigned long long ph_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tprev_ = stamp_now()
#define STAMP(i) do { const unsigned long long tn_ = stamp_now(); ph_[i] += tn_ - tprev_; tprev_ = tn_; } while (0)
__device__ __forceinline__ unsigned long long stamp_now() {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
// Host side: wait for the stream, read back n_rows rows of eight phase counters (one row per stamping workgroup), average every
// phase over the rows, divide by `divisor` (the step count, or 1) and print ONE line,
//   [stamps <tag>] <label> <cycles> | <label> <cycles> ...<tail>
// cols picks the phases and names them; the tag is printf-formatted from the trailing arguments.
struct StampCol { int ph; const char* label; };
__attribute__((format(printf, 7, 8)))
static void stamps_report(hipStream_t st, const unsigned long long* dbg, int n_rows, double divisor, std::initializer_list<StampCol> cols,
                          const char* tail, const char* tag_fmt, ...) {
  (void)hipStreamSynchronize(st);
  std::vector<unsigned long long> h((size_t)8 * n_rows);
  (void)hipMemcpy(h.data(), dbg, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost);
  double acc[8] = {0};
  for (int i = 0; i < n_rows; ++i) for (int j = 0; j < 8; ++j) acc[j] += (double)h[(size_t)i * 8 + j] / n_rows;
  char line[1024];
  int n = snprintf(line, sizeof line, "[stamps ");
  va_list ap;
  va_start(ap, tag_fmt);
  n += vsnprintf(line + n, sizeof line - n, tag_fmt, ap);
  va_end(ap);
  n += snprintf(line + n, sizeof line - n, "]");
  const char* sep = " ";
  for (const StampCol& c : cols) { n += snprintf(line + n, sizeof line - n, "%s%s %.0f", sep, c.label, acc[c.ph] / divisor); sep = " | "; }
  fprintf(stderr, "%s%s\n", line, tail);
}
// what the eight counters hold: gru_bwd_b3 (per tile); a chain wave (recurrence + gate math) and a bulk wave (dX / dW) of the
// pipelined kernels, whose second column is named by the kernel
#define B3_STAMP_COLS {{0, "top"}, {1, "dhMFMA"}, {2, "gates+ldsW"}, {3, "issue loads"}, {4, "dx"}, {5, "dW"}, {6, "barrier"}, {7, "vmcnt wait"}}
#define CHAIN_STAMP_COLS(reads) {{0, "loop top"}, {1, reads}, {2, "recurrence"}, {3, "dependent gate math + stores"}, {5, "barrier"}}
#define BULK_STAMP_COLS(reads) {{0, "loop top"}, {3, reads}, {4, "dW"}, {5, "barrier"}}
#else
#define STAMP_DECL
#define STAMP(i)
#endif

// compile-time unrolled loop: f(ic<0>{}) ... f(ic<N - 1>{})
template <int N> using ic = std::integral_constant<int, N>;
template <typename F, int... Is> __device__ __forceinline__ void sfor_impl(F&& f, std::integer_sequence<int, Is...>) { (f(ic<Is>{}), ...); }
template <int N, typename F> __device__ __forceinline__ void sfor(F&& f) { sfor_impl(f, std::make_integer_sequence<int, N>{}); }

// a run-time flag as a template argument: f(std::true_type{}) or f(std::false_type{})
template <typename F> static void with_flag(bool v, F&& f) { if (v) f(std::true_type{}); else f(std::false_type{}); }

struct GruDir {
  const float *Wih, *Whh, *bih, *bhh;
  int t_start, t_sign, n_steps;     // time index of step s: t = t_start + t_sign*s
  float* h;                         // h[b*h_bs + t*h_ts + h_col + u]
  int64_t h_bs, h_ts;
  int h_col;
  float* h_last;                    // optional copy of the final state: h_last[b*hl_bs + hl_col + u]
  int64_t hl_bs;
  int hl_col;
  float4* stash;                    // [(tile*n_steps + s)*4 + w][gate][lane] float4; NULL in eval
  // backward only
  const float* dh;                  // upstream gradient, see dh_mode
  int64_t dh_bs, dh_ts;
  int dh_col;
  int dh_mode;                      // 0: every step, dropout-masked (layer 0); 1: only the last step
  float* dx;                        // dx[b*dx_bs + t*dx_ts + k]
  int64_t dx_bs, dx_ts;
  int dx_accumulate;
  float* part;                      // dW partials [wg][192*I + 192*64 + 256]
};

struct GruArgs {
  GruDir dir[2];
  const float* x;                   // x[b*x_bs + t*x_ts + k]
  int64_t x_bs, x_ts;
  int B;
  int drop_thr;                     // dropout on x (layer-1 input) / on dh (layer-0 upstream grad)
  uint32_t drop_key;
  float drop_scale;
  float4* gi;                       // latency form only: input projections [(tile*n_steps + s)*4 + w][gate r,z,n][lane]
  size_t gi_dir_stride;             // float4 elements between the two directions' gi blocks
  unsigned long long* dbg;          // diagnostic stamps (MSIG_STAMPS builds only)
  int x_drop_thr;                   // fused backward only: dropout of the x tile (layer 1), independent of the dh mask
  uint32_t x_drop_key;
  float x_drop_scale;
  int stash_skip_hn;                // forward, layer 0: the backward form recomputes W_hn h + b_hn (gru_bwd_b6) — store r, z only
};

// Fold batching (msig_dev.h FoldCtx): the latency-form kernels run several independent models in one launch, blockIdx.z = fold.
// Every pointer of the argument block is fold 0's; the kernel shifts the ones it uses into this fold's arena (a by-value copy
// of ITS direction's GruDir — never of the whole argument block, whose dynamic indexing would land in scratch) and takes this
// fold's dropout key.
__device__ __forceinline__ void fold_dir(GruDir& g, const FoldCtx& fc) {
  FOLD_BEGIN;
  FS(g.Wih); FS(g.Whh); FS(g.bih); FS(g.bhh); FS(g.h); FS(g.h_last); FS(g.stash); FS(g.dh); FS(g.dx); FS(g.part);
}
#define FOLD_GRU_ARGS                                                         \
  GruDir D = a.dir[blockIdx.y];                                               \
  fold_dir(D, fc);                                                            \
  const float* ax_ = a.x; float4* agi_ = a.gi;                                \
  { FOLD_BEGIN; FS(ax_); FS(agi_); }                                          \
  [[maybe_unused]] const uint32_t akey_ = fc.key_gru[blockIdx.z]

// The throughput-form kernels come in two instantiations: FOLDS = false is the single-model kernel (arguments read straight from
// the kernarg segment); FOLDS = true shifts every pointer to the arena of fold blockIdx.z and takes that fold's dropout key —
// same arithmetic, so a fold's numbers are bit-identical in a fold batch and alone.
#define FOLD_GRU_ARGS_IF(FOLDS)                                                            \
  GruDir Dv_; const float* ax_ = a.x;                                                      \
  [[maybe_unused]] uint32_t akey_ = a.drop_key; [[maybe_unused]] uint32_t axkey_ = a.x_drop_key;  \
  if constexpr (FOLDS) {                                                                   \
    Dv_ = a.dir[blockIdx.y]; fold_dir(Dv_, fc);                                            \
    FOLD_BEGIN; FS(ax_);                                                                   \
    akey_ = axkey_ = fc.key_gru[blockIdx.z];                                               \
  }                                                                                        \
  const GruDir& D = FOLDS ? Dv_ : a.dir[blockIdx.y]

