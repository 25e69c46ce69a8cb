// Device-side helpers shared by every kernel file (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/msig.h"
#include "../../include/msig_gc.h"
#include "../../include/msig_da.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// D(16x16) += A(16x4) * B(4x16), exact fp32 (v_mfma_f32_16x16x4_f32).
// lane l: A[row l&15][k l>>4], B[k l>>4][col l&15]; D: col l&15, rows (l>>4)*4 + reg.
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// LDS-only barrier: does not drain outstanding global loads/stores (vmcnt).
// ---- split-bf16 ("bf16x3") contraction --------------------------------------------------------------------
// An fp32 value x is carried as three bf16 pieces x1 + x2 + x3 (x1 = top 16 bits of x, x2 = top 16 bits of x - x1, x3 likewise:
// 24 significant bits), and a product a*b as the six cross terms of order <= 2 accumulated in fp32 by
// v_mfma_f32_16x16x32_bf16, smallest first.  Measured on K = 64 dot products of the recurrence's value ranges
// (tools/mfma_bf16x3.hip, profiles/r01_bf16x3_microbench.log): rms error 3.0e-8 against fp64 vs 4.8e-8 for the
// v_mfma_f32_16x16x4_f32 chain — at least fp32 accuracy — at 16.5 instead of 3 x 32 cycles per 16x16x32 block.
// Lane map of the 16x16x32 instruction: A[i = lane&15][k = 8*(lane>>4) + j], B[k = 8*(lane>>4) + j][n = lane&15],
// j = 0..7; D as for 16x16x4 (col = lane&15, rows 4*(lane>>4) + e).
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
// The pieces are taken by TRUNCATION (the upper 16 bits of the fp32 pattern; the remainder x - piece is exact): bit
// masks and subtractions at full VALU rate instead of round-to-nearest conversions, and no less accurate in the sum
// (rms error 3.5e-8 on the same test).
__device__ __forceinline__ __bf16 top16(float x, float& rem) {
  const uint32_t u = __float_as_uint(x) & 0xFFFF0000u;
  rem = x - __uint_as_float(u);
  const unsigned short h = (unsigned short)(u >> 16);
  __bf16 r;
  __builtin_memcpy(&r, &h, 2);
  return r;
}
__device__ __forceinline__ void split3(float x, __bf16& a, __bf16& b, __bf16& c) {
  float r1, r2, r3;
  a = top16(x, r1); b = top16(r1, r2); c = top16(r2, r3);
}
// The same split for FOUR values at once, straight into the packed form the LDS planes take (bf16x4 per piece), in 7 instead of 11
// VALU instructions per pair of values: the packed pair of leading pieces P = (top16(a), top16(b)) is one v_perm_b32, and
// v_dot2c_f32_bf16 with the packed constant {-1, 0} resp. {0, -1} computes x - piece from it exactly (fp32 accumulate of an exact
// product: bit-identical to mask-and-subtract on 2^24 values incl. denormals, tools/split3_dot2_check.hip), so the mask and the
// separate subtraction go.  The constants must come from SGPRs: as a literal, {-1, 0} = 0x0000BF80 is folded to the inline
// constant -1.0, which this instruction reads as the fp32 pattern 0xBF800000 = {0, -1}.
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t top_pair(float a, float b) {            // (bits(b) & 0xffff0000) | (bits(a) >> 16)
  return __builtin_amdgcn_perm(__float_as_uint(b), __float_as_uint(a), 0x07060302u);
}
__device__ __forceinline__ void split3_pair(float a, float b, uint32_t& P0, uint32_t& P1, uint32_t& P2) {
  uint32_t klo, khi;
  asm("s_mov_b32 %0, 0xbf80\n\ts_mov_b32 %1, 0xbf800000" : "=s"(klo), "=s"(khi));
  const bf16x2 lo_m1 = __builtin_bit_cast(bf16x2, klo), hi_m1 = __builtin_bit_cast(bf16x2, khi);
  P0 = top_pair(a, b);
  a = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, P0), lo_m1, a, false);
  b = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, P0), hi_m1, b, false);
  P1 = top_pair(a, b);
  a = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, P1), lo_m1, a, false);
  b = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, P1), hi_m1, b, false);
  P2 = top_pair(a, b);
}
struct U2 { uint32_t x, y; };
__device__ __forceinline__ void split3_quad(const float (&v)[4], bf16x4 (&out)[3]) {
  U2 q[3];
  split3_pair(v[0], v[1], q[0].x, q[1].x, q[2].x);
  split3_pair(v[2], v[3], q[0].y, q[1].y, q[2].y);
#pragma unroll
  for (int pp = 0; pp < 3; ++pp) out[pp] = __builtin_bit_cast(bf16x4, q[pp]);
}
__device__ __forceinline__ void split3_quad(const f32x4& v, bf16x4 (&out)[3]) {
  const float t[4] = {v[0], v[1], v[2], v[3]};
  split3_quad(t, out);
}
// Negative controls of the parity tolerances (make negctl NEGCTL=k; never defined in the product library): the split-bf16 product
// WITHOUT its a1 * b1 cross term — a 2^-16 relative error per product — in ONE class of contractions, so that the parity gate is
// shown to catch a regression confined to it.  Every call site names its class: CT_BWD_REC the BPTT recurrence W_hh^T dgh, CT_DX the
// input gradient W_ih^T dgi, CT_DW the weight gradients, CT_FWD_REC the forward recurrence W_hh h (and gru_bwd_b6's recomputation of
// it), CT_FWD_PROJ the input projection W_ih x.  NEGCTL = 9 drops the term everywhere (round 3's control).
enum { CT_ANY = 0, CT_BWD_REC = 1, CT_DX = 2, CT_DW = 3, CT_FWD_REC = 4, CT_FWD_PROJ = 5 };
#ifdef MSIG_DROP_CROSS_TERM
template <int KIND> constexpr bool msig_drop_ct() { return MSIG_DROP_CROSS_TERM == 9 || MSIG_DROP_CROSS_TERM == KIND; }
#else
template <int KIND> constexpr bool msig_drop_ct() { return false; }
#endif
// Negative controls of the trained-like regimes (make negctl REGIME=k; never defined in the product library): one-line slips that
// no test near initialisation can see (tests/test_trained_regimes_gpu.py must FAIL against each; tools/negative_controls.sh regime).
//   1  gru_n_from_h and its inlined copies in gru_bwd4.hip / gru_bwd6.hip without the 1e-30 floor under 1 - z
//   2  the sigmoid of gru_gates and sigmoidf_fast as e^x / (1 + e^x): inf / inf from x = 88.7 on
//   3  bn_finalize_kernel's scale from |gamma|
//   4  the head's log-sum-exp (ce_row_lse) without subtracting the row maximum
#ifdef MSIG_NEGCTL_REGIME
constexpr int msig_negctl_regime = MSIG_NEGCTL_REGIME;
#else
constexpr int msig_negctl_regime = 0;
#endif
// Negative controls of the channel / class range (make negctl RANGE=k; never defined in the product library): one slip each, confined
// to code that only C = 9..15 or K > 8 reach and IN BOUNDS by construction — an omitted term or a changed value, never an index the
// product does not also form (tests/test_channel_class_range_gpu.py must FAIL against each; tools/negative_controls.sh range).
//   1  conv1_fwd_kernel<0>'s gated staging without the zero fill of the padded taps (they carry w1[o * K + 0] * gate instead)
//   2  conv1_bwd_kernel<0> with NB = K / 16 in its MFMA and record guards: the columns of the partial last block are never accumulated
//   3  HEAD_GRADS_ADD (head_mlp.h: head_bwd_kernel, head_step_kernel, head_epoch_kernel, da_step_kernel) accumulates dW3 in two of
//      the four register slots: rows c >= 8 of the gradient stay zero
#ifdef MSIG_NEGCTL_RANGE
constexpr int msig_negctl_range = MSIG_NEGCTL_RANGE;
#else
constexpr int msig_negctl_range = 0;
#endif
// Negative controls of the input regimes (make negctl INPUT=k; never defined in the product library): one slip each that no unit-scale,
// nearly centred input can see (tests/test_input_regimes_gpu.py must FAIL against each; tools/negative_controls.sh input).
//   1  bn_batch_sums always takes the unshifted fp32 sums: E[y^2] - mean^2 cancels in fp32 under a large channel mean
//   2  bn_finalize_kernel's training branch adds eps outside the square root: invstd = 1 / (sqrt(var) + eps)
#ifdef MSIG_NEGCTL_INPUT
constexpr int msig_negctl_input = MSIG_NEGCTL_INPUT;
#else
constexpr int msig_negctl_input = 0;
#endif
// Negative control of the stage-2 regimes (make negctl STAGE2=1; never defined in the product library): bn_batch_sums takes the unshifted
// fp32 sums for every channel of stage 2 (CH = 32) — the arithmetic stage 2 had before pool1_conv2_fwd_kernel carried shifted sums: exact
// enough on every channel near its centre, wrong where conv2's mean sits hundreds of spreads out (the conv2_offcentre cases of
// tests/test_stage2_regimes_gpu.py must FAIL against it; tools/negative_controls.sh stage2).
#ifdef MSIG_NEGCTL_STAGE2
constexpr int msig_negctl_stage2 = MSIG_NEGCTL_STAGE2;
#else
constexpr int msig_negctl_stage2 = 0;
#endif
// Negative controls of the window lengths (make negctl LENGTH=k; never defined in the product library): one slip each in a guard that
// only an unaligned window with more than one chunk reaches — a changed comparison, never an address the product does not also form
// (tests/test_window_lengths_gpu.py must FAIL against each; tools/negative_controls.sh length).
//   1  stage_x_chunk's scalar branch, item with t0 > 0: the padding test is g >= T - 1, so the window's last sample is read as padding
//   2  conv1_bwd_kernel<CT > 0>'s non-prefetch staging at T % 4 == 0 (i.e. T % 8 == 4): the zeroing guard is t >= L1 - 1
//   3  conv1_bwd_dx_kernel's position-wise staging, item with u0 > 0: the zeroing guard is t >= L1 - 1
#ifdef MSIG_NEGCTL_LENGTH
constexpr int msig_negctl_length = MSIG_NEGCTL_LENGTH;
#else
constexpr int msig_negctl_length = 0;
#endif
// Negative controls of the batch sizes (make negctl BATCH=k; never defined in the product library): one slip each in a guard on the
// batch size — a changed mask, stride, loop bound or unit count, never an address the product does not also form and never a
// condition that differs between the threads of a workgroup (tests/test_batch_sizes_gpu.py must FAIL against each;
// tools/negative_controls.sh batch).
//   1  bwd4_run (gru_bwd_seq4 / gru_bwd_seq4_dw1, the latency form's recurrence of both layers): in the SECOND half of a tile (rows
//      8 .. 15) a padding row takes its mask from its quad's first row, so the clamped copies of row B - 1 keep their gate
//      gradients and the dW / db contractions count that row up to four times: wrong at 9, 10, 11, 13, 14 and 15 rows
//   2  ce_kernel's and loss_finalize's row loops start their second pass one row late (stride 1025 once): row 1024 is never visited
//   3  head_bwd_kernel's group loop, in a workgroup's rounds after the first, asks for a SECOND live row (r0 + 1 < B for r0 < B): a
//      last group of one row beyond the 128-workgroup grid is skipped
//   4  dw2_role (gru_bwd_dxdw, gru_bwd_dw2, gru_bwd_seq4_dw1): a workgroup of the capped grid stops after its 8 units
#ifdef MSIG_NEGCTL_BATCH
constexpr int msig_negctl_batch = MSIG_NEGCTL_BATCH;
#else
constexpr int msig_negctl_batch = 0;
#endif
// Negative control of the supervised contrastive term (make negctl SUPCON=1; never defined in the product library): sc_grad_kernel
// without the transposed term C_ji of G_ij = C_ij + C_ji — a gradient that stays finite and plausible, and wrong (the `apply` parity
// cases of tests/test_supcon_gpu.py must FAIL against it; tools/negative_controls.sh supcon).
#ifdef MSIG_NEGCTL_SUPCON
constexpr int msig_negctl_supcon = MSIG_NEGCTL_SUPCON;
#else
constexpr int msig_negctl_supcon = 0;
#endif
// acc += A . B over one 32-wide k block, A and B given as their three pieces ([0] = leading piece)
template <int KIND = CT_ANY>
__device__ __forceinline__ f32x4 mfma_bf16x3(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[2], acc, 0, 0, 0);
  if constexpr (!msig_drop_ct<KIND>()) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], acc, 0, 0, 0);
  return acc;
}

// ---- two-piece fp16 contraction ("f16x2"), round 5: the FORWARD recurrences and the layer-1 input projection ---------------------
// x S = x0 + x1 with x0 = fp16(x S), x1 = fp16(x S - x0) (round to nearest; S a power of two that puts x S in the middle of fp16's
// range, so that the low piece is a NORMAL fp16 number: 2 x 11 significant bits + the sign of the remainder = fp32's 24), and
//     sum a b  =  [ sum a0 b0 + a0 b1 + a1 b0 ] / (S_a S_b)         (a1 b1: 2^-22 relative, dropped)
// — THREE v_mfma_f32_16x16x32_f16 per 16x16x32 block instead of split-bf16's six, one accumulator (both operands pre-scaled, the
// three terms share the scale), exact power-of-two post-scale.  Measured on the forward pass's three contraction shapes against
// fp64 (tools/mfma_f16x2.hip, profiles/r05_f16x2_microbench.log): rms error 2.97e-8 / 6.8e-8 / 1.07e-7 (K = 64 recurrence / K = 128
// layer-1 projection / K = 32) against 4.83e-8 / 9.7e-8 / 1.19e-7 for the v_mfma_f32_16x16x4_f32 chain and 3.46e-8 / 1.03e-7 / 8.4e-8
// for split-bf16; 304.6 instead of 592.6 cycles per wave-step of three K = 64 tiles.
// Range is what decides where it may be used: an operand must satisfy |x| S < 65504.  h is in [-1, 1] by construction (a convex
// combination of tanh values), the layer-1 input is h times the dropout scale, and the weights get their scale from their own
// maximum when a wave loads its fragment — so the forward recurrences and the layer-1 projection qualify.  The layer-0 input
// (BatchNorm output: unbounded outliers) and every backward contraction (gate gradients: no bound, and rows of very different
// magnitude in one tile) stay on split-bf16, whose pieces have fp32's exponent range.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4v __attribute__((ext_vector_type(4)));
#define F16X2_H_SCALE 4096.0f                 // |h| <= 1 -> |h S| <= 4096; the low piece is normal for |h| >= 2^-15
__device__ __forceinline__ void split2_quad(const f32x4& v, const float scale, f16x4& hi, f16x4& lo) {
  const f32x4 t = v * scale;
  hi = __builtin_convertvector(t, f16x4);
  const f32x4 back = __builtin_convertvector(hi, f32x4);
  lo = __builtin_convertvector(t - back, f16x4);
}
__device__ __forceinline__ void split2(const float x, const float scale, _Float16& hi, _Float16& lo) {
  const float t = x * scale;
  hi = (_Float16)t;
  lo = (_Float16)(t - (float)hi);
}
// power-of-two scale for a weight fragment whose largest magnitude over the WAVE is m: m S in [2^13, 2^14) (fp16's largest finite
// value is 65504); an all-zero fragment takes 2^12.  Exact: built from the exponent field.
__device__ __forceinline__ float f16x2_weight_scale(float m) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  const int e = (int)((__float_as_uint(m) >> 23) & 0xFF);            // biased exponent of the maximum: m in [2^(e-127), 2^(e-126))
  if (e == 0) return 4096.0f;
  const int se = 127 + 13 - (e - 127);                               // S = 2^(13 - (e - 127))
  return __uint_as_float((uint32_t)(se < 1 ? 1 : (se > 254 ? 254 : se)) << 23);
}
// acc += A . B over one 32-wide k block, A and B as their two pieces ([0] = leading piece); the result carries the factor S_a S_b.
// Negative control (MSIG_DROP_CROSS_TERM): without a1 * b0 — a 2^-11 relative error per product.
template <int KIND = CT_ANY>
__device__ __forceinline__ f32x4 mfma_f16x2(const f16x8 (&a)[2], const f16x8 (&b)[2], f32x4 acc) {
  if constexpr (!msig_drop_ct<KIND>()) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[1], b[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[0], b[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[0], b[0], acc, 0, 0, 0);
  return acc;
}

// LDS plane swizzle shared by the split-bf16 kernels: rows 16 * odd dwords apart, 8-element (16-byte) chunks of row r XORed with
// g(r >> 2), g = [0,3,2,1].  Row reads by ds_read_b128 (lane = (row li, chunk lq)), the producers' 8-byte stores and transposed
// reads of 32-column blocks are all conflict-free (derivation: gru_bwd4.hip; exact-integer check: tools/dw32_check.hip).
__device__ __forceinline__ int quad_swz(int row) { return ((4 - (row >> 2)) & 3) * 8; }

__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// v_exp_f32 / v_rcp_f32 based (1 ulp each): abs error ~1e-7, far inside the parity tolerance
__device__ __forceinline__ float sigmoidf_fast(float x) {
  if constexpr (msig_negctl_regime == 2) { const float ex = __expf(x); return ex * __builtin_amdgcn_rcpf(1.0f + ex); }
  return __builtin_amdgcn_rcpf(1.0f + __expf(-x));
}
__device__ __forceinline__ float tanhf_fast(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(__expf(2.0f * x) + 1.0f); }
// The GRU gate math of one lane (4 elements), written on 4-vectors so that the non-transcendental half compiles to
// packed fp32 instructions (v_pk_mul/add/fma_f32: two elements per issue slot) — VALU time adds to MFMA time on this
// part, so instruction count is what matters.  Same formulas as sigmoidf_fast / tanhf_fast:
//   r = sigmoid(a_r), z = sigmoid(a_z), n = tanh(a_in + r * a_hn), h' = n + z * (h - n)   [= (1-z) n + z h]
__device__ __forceinline__ void gru_gates(const f32x4& a_r, const f32x4& a_z, const f32x4& a_in, const f32x4& a_hn, const f32x4& h,
                                          f32x4& r, f32x4& z, f32x4& n, f32x4& hnew) {
  constexpr float L2E = 1.4426950408889634f;
  if constexpr (msig_negctl_regime == 2) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float pr = __builtin_amdgcn_exp2f(a_r[e] * L2E), pz = __builtin_amdgcn_exp2f(a_z[e] * L2E);
      r[e] = pr * __builtin_amdgcn_rcpf(pr + 1.0f); z[e] = pz * __builtin_amdgcn_rcpf(pz + 1.0f);
    }
  } else {
    f32x4 er = a_r * (-L2E), ez = a_z * (-L2E);
#pragma unroll
    for (int e = 0; e < 4; ++e) { er[e] = __builtin_amdgcn_exp2f(er[e]); ez[e] = __builtin_amdgcn_exp2f(ez[e]); }
    er = er + 1.0f; ez = ez + 1.0f;
#pragma unroll
    for (int e = 0; e < 4; ++e) { r[e] = __builtin_amdgcn_rcpf(er[e]); z[e] = __builtin_amdgcn_rcpf(ez[e]); }
  }
  f32x4 t = (a_in + r * a_hn) * (2.0f * L2E);
#pragma unroll
  for (int e = 0; e < 4; ++e) t[e] = __builtin_amdgcn_exp2f(t[e]);
  t = t + 1.0f;
#pragma unroll
  for (int e = 0; e < 4; ++e) t[e] = __builtin_amdgcn_rcpf(t[e]);
  n = 1.0f - 2.0f * t;
  hnew = n + z * (h - n);
}

// The backward pass does not read n_t from the stash (round 2: the forward kernels are bound by their stash writes — layer 0
// moves bytes at 4.3 TB/s whatever their number: 0.71 ms without, 0.82 ms with two, 1.28 ms with four stash vectors per step —
// so the stash holds r, z and W_hn h + b_hn only); it recovers n_t from the step's own output, h_t = n + z (h_{t-1} - n):
//     n = (h_t - z h_{t-1}) / (1 - z),   clamped to tanh's range.
// The quotient loses accuracy as z -> 1 (error ~ eps |h| / (1 - z)), but every use of n in the backward pass carries the factor
// (1 - z):  dn = dh (1-z)(1 - n^2),  dz = dh (h_{t-1} - n) z (1-z)  — so the error that reaches a gradient stays ~ eps |dh|,
// the clamp bounds it by (1 - z) |dh| where the quotient is noise, and z = 1 exactly (1 - z = 0) gives 0 * finite = 0, as it should.
__device__ __forceinline__ float gru_n_from_h(float h_new, float h_prev, float z, float one_minus_z) {
  const float num = __builtin_fmaf(-z, h_prev, h_new);
  if constexpr (msig_negctl_regime == 1) return __builtin_amdgcn_fmed3f(num * __builtin_amdgcn_rcpf(one_minus_z), -1.0f, 1.0f);
  return __builtin_amdgcn_fmed3f(num * __builtin_amdgcn_rcpf(__builtin_fmaxf(one_minus_z, 1e-30f)), -1.0f, 1.0f);
}

__host__ __device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}
// The dropout key of (seed, optimiser step, stream: 1 GRU, 2 head): msig_dropout_key (api.hip), and the head epoch's per step
__host__ __device__ __forceinline__ uint32_t dropout_key(uint64_t seed, uint64_t step, uint32_t stream_id) {
  const uint32_t lo = (uint32_t)(seed & 0xFFFFFFFFu), hi = (uint32_t)(seed >> 32);
  const uint32_t a = (uint32_t)((step * 0x9E3779B9ull) & 0xFFFFFFFFull);
  const uint32_t b = (uint32_t)(((uint64_t)stream_id * 0x7F4A7C15ull) & 0xFFFFFFFFull);
  return fmix32(lo ^ fmix32(a + b + hi));
}
// Dropout: element e is kept iff byte (e&3) of fmix32((e>>2) ^ key) >= thr.
__device__ __forceinline__ uint32_t drop_word(uint32_t elem_idx, uint32_t key) { return fmix32((elem_idx >> 2) ^ key); }
__device__ __forceinline__ float drop_mul(uint32_t word, int byte, int thr, float scale) {
  return (((word >> (8 * byte)) & 0xFFu) >= (uint32_t)thr) ? scale : 0.0f;
}
__host__ __device__ __forceinline__ float drop_scale(int thr) { return thr >= 256 ? 0.0f : 256.0f / (256.0f - (float)thr); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One row of CrossEntropy: argmax and log-sum-exp of its K logits (head_mlp.h ce_row_terms, and the discriminator's two-label form).
__device__ __forceinline__ float ce_row_lse(const float* lg, int K, int& am) {
  float mx = lg[0]; am = 0;
  for (int c = 1; c < K; ++c) if (lg[c] > mx) { mx = lg[c]; am = c; }
  float se = 0.f;
  if constexpr (msig_negctl_regime == 4) {
    for (int c = 0; c < K; ++c) se += expf(lg[c]);
    return logf(se);
  }
  for (int c = 0; c < K; ++c) se += expf(lg[c] - mx);
  return mx + logf(se);
}

// Column sums of part[nrows][ncol] (ncol <= 64; float or double rows) by one 1024-thread workgroup into red[0..ncol): 1024/ncol
// row-lanes, 8 loads in flight per lane, fixed combination order (deterministic for a given nrows).
#define FIN_THREADS 1024
template <typename PT>
__device__ __forceinline__ void fin_colsums(const PT* __restrict__ part, int nrows, int ncol, double* red) {
  const int tid = threadIdx.x;
  const int col = tid % ncol, grp = tid / ncol, ngrp = FIN_THREADS / ncol;
  double a[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = 0.0;
  if (grp < ngrp) {
    int r = grp;
    for (; r + 7 * ngrp < nrows; r += 8 * ngrp) {
      PT v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = part[(size_t)(r + j * ngrp) * ncol + col];
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] += (double)v[j];
    }
    for (; r < nrows; r += ngrp) a[0] += (double)part[(size_t)r * ncol + col];
  }
  red[tid] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  __syncthreads();
  double s = 0.0;
  if (tid < ncol)
    for (int g = 0; g < ngrp; ++g) s += red[g * ncol + tid];
  __syncthreads();
  if (tid < ncol) red[tid] = s;
  __syncthreads();
}

// BatchNorm's running-statistic update  new = (1 - momentum) * old + momentum * batch  with its roundings PINNED: the mean as two
// rounded products and their sum, the variance as one rounded product and a fused multiply-add.  That is what bn_finalize_kernel
// has always computed (the compiler's contraction of the plain expressions); written out so that adapt_bn.hip's commit, which
// must give the same bits from the same sums, does not depend on how another kernel's expressions happen to be contracted.
__device__ __forceinline__ void bn_running_update(float momentum, float mean, float unbiased, float old_mean, float old_var, float& new_mean,
                                                  float& new_var) {
#pragma clang fp contract(off)
  new_mean = (1.0f - momentum) * old_mean + momentum * mean;
  new_var = __builtin_fmaf(momentum, unbiased, (1.0f - momentum) * old_var);
}

// torch.optim.Adam with L2-in-gradient weight decay, one element, every rounding PINNED.  The library's
// Adam is the ADAM_STEP form:
//     gr    = fma(wd, p, g)
//     m'    = fma(b1, m, (1 - b1) * gr)
//     v'    = b2 * v + ((1 - b2) * gr) * gr            two rounded products and their sum
//     denom = fma(sqrt(v'), inv_sqrt_bc2, eps)
//     p'    = fma(-lr_over_bc1, m' / denom, p)
// Each of m' and v' is a sum of two products, of which contraction may fuse either or neither, and before this function existed
// the compiler chose per call site.  What it chose is kept, bit for bit, by the other three forms — they differ from ADAM_STEP in
// those two statements (ADAM_PRODUCTS: and in denom) only, and say so in their names' comments:
enum AdamForm {
  ADAM_STEP,       // the train steps: colsum_adam_kernel, clip_adam_kernel
  ADAM_FUSED_V,    // v' = fma(b2, v, ((1 - b2) * gr) * gr): adam_kernel; head_epoch_kernel's and da_step_kernel's W0 elements
                   // (32 per thread, compiled to packed instructions); head_epoch_kernel's b0 and b3
  ADAM_PRODUCTS,   // no sum of products fused but p': m' = b1 * m + (1 - b1) * gr as two rounded products and their sum, v' as
                   // ADAM_STEP, denom = sqrt(v') * inv_sqrt_bc2 + eps as a rounded product and a sum: head_epoch_kernel's W3
  ADAM_FUSED_G     // m' = fma(1 - b1, gr, b1 * m), v' as ADAM_STEP: da_step_kernel's W3, b0 and b3
};
template <AdamForm F = ADAM_STEP>
__device__ __forceinline__ float adam_update(float p, float g, float& m, float& v, float lr_over_bc1, float inv_sqrt_bc2, float b1, float b2,
                                             float eps, float wd) {
#pragma clang fp contract(off)
  const float gr = __builtin_fmaf(wd, p, g);
  const float g1 = (1.f - b1) * gr, g2 = ((1.f - b2) * gr) * gr;
  if constexpr (F == ADAM_PRODUCTS) m = b1 * m + g1;
  else if constexpr (F == ADAM_FUSED_G) m = __builtin_fmaf(1.f - b1, gr, b1 * m);
  else m = __builtin_fmaf(b1, m, g1);
  if constexpr (F == ADAM_FUSED_V) v = __builtin_fmaf(b2, v, g2);
  else v = b2 * v + g2;
  const float denom = F == ADAM_PRODUCTS ? sqrtf(v) * inv_sqrt_bc2 + eps : __builtin_fmaf(sqrtf(v), inv_sqrt_bc2, eps);
  return __builtin_fmaf(-lr_over_bc1, m / denom, p);
}

// ---- fold batching (msig_*_multi): one launch covers several independent models ("folds" of the LOSO loop) -------------
// Every buffer of fold f (parameters, gradients, Adam moments, BN state, workspace, input batch, labels) lives at the SAME
// offset inside a per-fold arena, arenas are `stride` bytes apart, and blockIdx.z selects the fold: every pointer a kernel
// receives is fold 0's and is shifted by slot[blockIdx.z] * stride at kernel entry (FOLD_BEGIN / FS).  The single-model entry
// points launch with n = 1, slot[0] = 0 (stride irrelevant).  Per-fold scalars (dropout keys, learning rate) are arrays
// indexed by blockIdx.z.
#define MSIG_FORM_AUTO (-1)      // internal: "no form named" (msig_batch.fwd_form / bwd_form == 0 and no environment default)
struct FoldCtx {
  int32_t n;
  int32_t slot[MSIG_MAX_FOLDS];
  int64_t stride;                         // bytes between consecutive arenas
  uint32_t key_gru[MSIG_MAX_FOLDS], key_head[MSIG_MAX_FOLDS];
  float lr_over_bc1[MSIG_MAX_FOLDS];      // Adam: lr / (1 - beta1^step) of each fold
  float inv_sqrt_bc2[MSIG_MAX_FOLDS];     //       1 / sqrt(1 - beta2^step) of each fold (folds may be at different step counts)
  int32_t form_folds;                     // fold count the GRU kernel forms are chosen for (msig_multi.form_folds; >= 1)
  int32_t fused_step;                     // host side: forward and backward of this step come from ONE descriptor (msig_train_step*)
};
__device__ __forceinline__ const void* msig_fold_addr(const void* p, int64_t off) { return p ? (const void*)((const char*)p + off) : p; }
#define FOLD_BEGIN const int64_t foff_ = (int64_t)fc.slot[blockIdx.z] * fc.stride
#define FS(p) p = (decltype(p))msig_fold_addr((const void*)(p), foff_)
// The forward keeps what a backward reads (pooling decisions, the gate's parity sums, GRU stashes, dL/dlogits of a call with labels):
// in training, and in an eval-mode forward that asked for it (msig_batch.keep_for_backward, ABI 5).  Batch statistics, the running-
// statistic update and dropout stay with `training` alone.
inline bool msig_keeps(const msig_batch* b) { return b->training || b->keep_for_backward; }

inline FoldCtx single_fold(const msig_batch* b) {
  FoldCtx fc{};
  fc.n = 1; fc.stride = 0; fc.form_folds = 1;
  fc.key_gru[0] = b ? b->key_gru : 0; fc.key_head[0] = b ? b->key_head : 0;
  return fc;
}

struct StageDims {
  int B, C, T, K, L1, P1, L2, TP, Cr, NT;  // NT = batch tiles of 16 rows
};
__host__ __device__ inline StageDims make_dims(const msig_shape& s) {
  StageDims d;
  d.B = s.B; d.C = s.C; d.T = s.T; d.K = s.K;
  d.L1 = (s.T + 6 - 7) / 2 + 1;
  d.P1 = (d.L1 + 2 - 3) / 2 + 1;
  d.L2 = (d.P1 + 4 - 5) / 2 + 1;
  d.TP = (d.L2 + 2 - 3) / 2 + 1;
  d.Cr = s.C / 4;
  d.NT = (s.B + 15) / 16;
  return d;
}

// a pointer argument that is not a multiple of mask + 1 bytes (NULL is aligned: optional pointers pass)
inline bool msig_misaligned(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

#define MSIG_LAUNCH_CHECK()                          \
  do {                                               \
    hipError_t e__ = hipGetLastError();              \
    if (e__ != hipSuccess) return (int)e__;          \
  } while (0)

// ---- optional per-kernel HIP-event timing (api.hip) -----------------------------
struct MsigProfScope {
  const char* name; hipStream_t st; void* rec;
  MsigProfScope(const char* name, hipStream_t st);
  ~MsigProfScope();
};
#define MSIG_K(name, st) MsigProfScope prof_scope__(name, st)

// ---- internal launchers (one per kernel file) ---------------------------------
struct WsPtrs {
  char* base;
  int64_t off[MSIG_NWS + 1];
  template <typename T> __host__ T* p(int region) const { return (T*)(base + off[region]); }
};

// gated = false: CnnGruModel's front end (include/msig_cg.h): conv1 on raw taps, no gate, no gate_bwd, no ds
// stats_stage 1 / 2 (include/msig_ab.h): stop after that stage's convolution, its partial sums on; *stats_rows = rows written
int launch_frontend_fwd(const msig_batch* b, const StageDims& d, const WsPtrs& w, const int64_t* po, const FoldCtx& fc, hipStream_t st,
                        bool gated = true, int stats_stage = 0, int* stats_rows = nullptr);
struct ColsumPlan;
int launch_frontend_bwd(const msig_batch* b, const StageDims& d, const WsPtrs& w, const int64_t* po, ColsumPlan& plan, const FoldCtx& fc, hipStream_t st,
                        bool gated = true);
// Monte-Carlo dropout (include/msig_mc.h) splits an eval forward at the first dropout site.  part: which layers
// launch_gru_fwd runs — all (every msig.h call), layer 0 alone (for gru_layers = 1 with its copy to WS_FEAT: the trunk) or layer 1
// alone from the WS_H0 it finds (the tail; nothing to run for gru_layers = 1).  force_drop: the dropout masks of b->dropout_thr
// although b->training = 0.  The defaults are every other call's launches, unchanged.
enum { GRU_PART_ALL = 0, GRU_PART_L0 = 1, GRU_PART_L1 = 2 };
int launch_gru_fwd(const msig_batch* b, const StageDims& d, const WsPtrs& w, const int64_t* po, const FoldCtx& fc, hipStream_t st,
                   int part = GRU_PART_ALL, bool force_drop = false);
// adapt_bn.hip (include/msig_ab.h): part[nrows][2 * CH] of every fold of the launch -> += into the stage's slots of its accumulator;
// the stage's slices of the BatchNorm state from the accumulator
int launch_ab_merge(const float* part, int nrows, int stage, double count, double* acc, const FoldCtx& fc, hipStream_t st);
int launch_ab_commit(const double* acc, int stage, float alpha, const float* bn_src, float* bn_dst, const FoldCtx& fc, hipStream_t st);
int launch_gru_bwd(const msig_batch* b, const StageDims& d, const WsPtrs& w, const int64_t* po, ColsumPlan& plan, const FoldCtx& fc, hipStream_t st);
// Soft targets (include/msig_st.h): the launch's label smoothing and every fold's mixup weight; NULL wherever it is
// taken = the plain criterion's kernels.
struct SoftArgs { float eps; float lam[MSIG_MAX_FOLDS]; };
struct ClipArgs;
struct DaArgs;
struct KdArgs;
struct SamArgs;
struct DroArgs;
struct ScArgs;
// What a forward or a train step does beyond the msig.h call (host side only; api.hip's entry points fill it after their own checks).
// Value-initialised = the plain call.  Each function that takes it reads only the fields named at its declaration.
struct StepOpts {
  const float* cw;          // class weights (include/msig_cw.h): K device floats of fold slot 0, shifted per fold like every buffer
  bool cg;                  // CnnGruModel (include/msig_cg.h): no gate, and a parameter layout without the gate tensors
  const ClipArgs* clip;     // gradient-norm clipping (include/msig_gc.h) between the reduction and the Adam update
  const SoftArgs* soft;     // soft targets (include/msig_st.h); NULL = the plain criterion's kernels
  const DaArgs* da;         // subject discriminator (include/msig_da.h): one more launch after the head's
  const KdArgs* kd;         // distillation (include/msig_kd.h): the unfused head with one more launch between ce and head_bwd
  const SamArgs* sam;       // sharpness-aware step (include/msig_sam.h): two passes with the unfused head, perturbation and restore between
  const DroArgs* dro;       // group-DRO (include/msig_dro.h): the unfused head with one more launch between ce and kd_apply / head_bwd
  const ScArgs* sc;         // supervised contrastive term (include/msig_sc.h): two more launches after the head's (and the adversary's)
};
// reads o.cw, o.soft.  mc_tail (include/msig_mc.h): the classifier's launch alone — no loss, no softmax — with the dropout mask of
// b->dropout_thr although b->training = 0
int launch_head_fwd(const msig_batch* b, const StageDims& d, const WsPtrs& w, const int64_t* po, const FoldCtx& fc, hipStream_t st,
                    const StepOpts& o, bool mc_tail = false);
int launch_head_bwd(const msig_batch* b, const float* dlogits, const StageDims& d, const WsPtrs& w, const int64_t* po, ColsumPlan& plan,
                    const FoldCtx& fc, hipStream_t st);
// head forward + CrossEntropy + head backward of a fused train step in one launch (few windows: see head.hip); false = not applicable
bool head_step_applies(const msig_batch* b, const StageDims& d);
// reads o.cw, o.soft
int launch_head_step(const msig_batch* b, const StageDims& d, const WsPtrs& w, const int64_t* po, ColsumPlan& plan, const FoldCtx& fc, hipStream_t st,
                     const StepOpts& o);
// Subject discriminator (include/msig_da.h, adversary.hip): msig_da after its checks, by value to the launch.  Pointers are fold
// slot 0's adversary buffers, `stride` bytes apart per slot; B rows; lam = the folds' mixup weights; Adam's bias corrections per
// fold, formed on the host as train_step_fc forms the model's.  One launch, between the head's and launch_gru_bwd.
struct DaArgs {
  int32_t S, B;
  const int32_t* dom; const int64_t* idx; int64_t idx_row_stride;
  float *params, *exp_avg, *exp_avg_sq; double* stats;
  int64_t stride;
  float b1, b2, eps, wd;
  float lambda[MSIG_MAX_FOLDS], lam[MSIG_MAX_FOLDS], lr_over_bc1[MSIG_MAX_FOLDS], inv_sqrt_bc2[MSIG_MAX_FOLDS];
};
int launch_da_step(const DaArgs& a, const float* feat, float* dfeat, const FoldCtx& fc, hipStream_t st);
// Distillation (include/msig_kd.h, distill.hip): msig_kd after its checks (msig_kd_make_args), by value to the launch.  q / stats are
// fold slot 0's, `stride` bytes apart per slot; B rows of K; om = 1.f - alpha, kappa = (float)((double)alpha * T / B), t2 = T * T in
// fp64; lam = the folds' mixup weights.  One launch, between ce_kernel and head_bwd_kernel, on WS_LOGITS / WS_DLOGITS.
struct msig_kd;
struct KdArgs {
  int32_t B, K;
  const float* q; const int64_t* idx; int64_t idx_row_stride;
  double* stats;
  int64_t stride;
  float alpha, T, om, kappa;
  double t2;
  float lam[MSIG_MAX_FOLDS];
};
// every check of msig_kd.h's own arguments, before any launch; fc: the folds of the launch (stride != 0: a fold batch); lam per fold
int msig_kd_make_args(const msig_kd* k, const FoldCtx& fc, int32_t B, int32_t K, const float* lam, KdArgs& kd);
int launch_kd_apply(const KdArgs& a, const float* logits, float* dlogits, const FoldCtx& fc, hipStream_t st);
// Sharpness-aware minimisation (include/msig_sam.h, sam.hip): msig_sam after its checks (msig_sam_make_args), by value to the launches.
// state: fold slot 0's, shifted per fold like every buffer; off / len: the parameter tensors' offsets and TRUE lengths in floats (the
// padding between tensors is len short of the next offset); n_flat: the padded total; a16: the state is 16-byte aligned.  pass2 is
// host side only: train_step_fc's second pass, which restores before its last launch.
#define SAM_WG 32                      // workgroups per fold of every sam.hip launch: the norm's partial sums are SAM_WG doubles
struct msig_sam;
struct SamArgs {
  int32_t adaptive, a16;
  float rho, eta;
  char* state;
  int64_t n_flat;
  int32_t off[MSIG_NPARAM], len[MSIG_NPARAM];
  bool pass2;
};
int msig_sam_make_args(const msig_sam* s, int C, int K, SamArgs& a);
// two launches: the per-workgroup sums of squares, then backup / perturbation / the copies of bn_state, bn_count, ws_loss[0..2]
int launch_sam_perturb(const SamArgs& a, float* params, const float* grads, const float* bn_state, const int64_t* bn_count,
                       const float* ws_loss, const FoldCtx& fc, hipStream_t st);
int launch_sam_restore(const SamArgs& a, float* params, float* bn_state, int64_t* bn_count, float* ws_loss, int B, const FoldCtx& fc,
                       hipStream_t st);
// Group-DRO (include/msig_dro.h, dro.hip): msig_dro after its checks (msig_dro_make_args), by value to the launch.  grp / q / stats are
// fold slot 0's, `stride` bytes apart per slot; B rows of K; eps: the launch's label smoothing.  One launch, between ce_kernel and
// kd_apply_kernel / head_bwd_kernel, on WS_LOGITS / WS_DLOGITS; labels and cw are the step's (fold slot 0's, shifted like every buffer).
struct msig_dro;
struct DroArgs {
  int32_t G, B, K, frozen;
  float eta, eps;
  const int32_t* grp; const int64_t* idx; int64_t idx_row_stride;
  float* q; double* stats;
  int64_t stride;
};
// every check of msig_dro.h's own arguments, before any launch; fc: the folds of the launch (stride != 0: a fold batch)
int msig_dro_make_args(const msig_dro* k, const FoldCtx& fc, int32_t B, int32_t K, float smoothing, DroArgs& a);
int launch_dro_apply(const DroArgs& a, const float* logits, const int64_t* labels, const float* cw, float* dlogits, const FoldCtx& fc,
                     hipStream_t st);
// Supervised contrastive term (include/msig_sc.h, supcon.hip): msig_sc after its checks (msig_sc_make_args), by value to the launches.
// grp / scratch / stats are fold slot 0's, `stride` bytes apart per slot; B rows of 128; weight per fold.  Two launches, between the
// head's launch (the adversary's when there is one) and launch_gru_bwd, on WS_FEAT / WS_DFEAT; labels are the step's.
struct msig_sc;
struct ScArgs {
  int32_t positives, B, K;
  float tau;
  const int32_t* grp; const int64_t* idx; int64_t idx_row_stride;
  char* scratch; double* stats;
  int64_t stride;
  float weight[MSIG_MAX_FOLDS];
};
// every check of msig_sc.h's own arguments, before any launch; fc: the folds of the launch (stride != 0: a fold batch)
int msig_sc_make_args(const msig_sc* k, const FoldCtx& fc, int32_t B, int32_t K, ScArgs& a);
int launch_sc_apply(const ScArgs& a, const float* feat, const int64_t* labels, float* dfeat, const FoldCtx& fc, hipStream_t st);
// Entropy-minimisation adaptation (include/msig_tt.h, tta.hip).  The objective: one launch on WS_LOGITS that writes WS_DLOGITS, between
// the forward's last launch and launch_head_bwd; logits / dlogits / stats are fold slot 0's, shifted per fold like every buffer.  The
// selective Adam: the selected tensors' slots of the flat layout as (first float4, running float4 count) pairs, by value to the launch;
// fc.lr_over_bc1 / inv_sqrt_bc2 per fold from msig_tt_fill_adam.
struct TtSel { int32_t n, total4; int32_t first4[MSIG_NPARAM], cum4[MSIG_NPARAM]; };
bool msig_tt_bad_diversity(float div);
int msig_tt_make_sel(int C, int K, int kind, uint32_t select, TtSel& sel);
void msig_tt_fill_adam(FoldCtx& fc, const float* lrs, const int64_t* steps, int64_t step, float beta1, float beta2);
int launch_tt_objective(const float* logits, float* dlogits, double* stats, int B, int K, float div, const FoldCtx& fc, hipStream_t st);
int launch_tt_adam(float* p, const float* g, float* m, float* v, const TtSel& sel, float b1, float b2, float eps, float wd, const FoldCtx& fc,
                   hipStream_t st);
// Weight-gradient reductions.  Every backward kernel leaves per-workgroup partials in its OWN sub-region of
// MSIG_WS_GRAD_PART (nothing aliases), and only records what has to be summed: out[c] = sum_r part[r*stride +
// col0 + c], fp64 accumulation in a fixed order.  The whole backward pass is then reduced by ONE launch
// (blockIdx.y = job) instead of one launch per stage — at the reference's batch size a step is bound by the
// number of launches, not by their work.
struct ColsumJob { const float* part; int nrows, row_stride, col0, ncols; float* out; };
#define MSIG_MAX_JOBS 40
// The loss of a fused train step whose head ran as ONE kernel (head.hip head_step_kernel): summed, in ce_kernel's order, by one
// extra workgroup of the step's last launch.  cw: class weights (include/msig_cw.h) or NULL.
struct LossFin { const float* logits; const int64_t* labels; float* lossbuf; double* lacc; int B, K; const float* cw; };
struct ColsumPlan {
  ColsumJob job[MSIG_MAX_JOBS];
  int n = 0;
  LossFin loss{nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr};
  const SoftArgs* soft = nullptr;      // of `loss` (host side; the launch passes it by value): soft targets, include/msig_st.h
  bool add(const float* part, int nrows, int row_stride, int col0, int ncols, float* out) {
    if (n >= MSIG_MAX_JOBS) return false;
    if (ncols > 0 && nrows > 0) job[n++] = ColsumJob{part, nrows, row_stride, col0, ncols, out};
    return true;
  }
  bool add_in_place(float* grad, int ncols) {          // gradient written directly by its kernel: nothing to sum
    if (n >= MSIG_MAX_JOBS) return false;
    if (ncols > 0) job[n++] = ColsumJob{nullptr, 0, 0, 0, ncols, grad};
    return true;
  }
};
int launch_colsum_plan(const ColsumPlan& plan, const FoldCtx& fc, hipStream_t st);
// The same reduction with the Adam update of every reduced element applied in the same launch (the train step's
// last two launches in one).  Jobs with nrows == 0 are "gradient already in place" ranges (BN affine, gate weights).
struct AdamArgs { float *p, *g, *m, *v; float lr_over_bc1, inv_sqrt_bc2, b1, b2, eps, wd; };
int launch_colsum_adam_plan(const ColsumPlan& plan, const AdamArgs& ad, const FoldCtx& fc, hipStream_t st);
// The same with gradient-norm clipping between the reduction and the update (include/msig_gc.h; head.hip colsum_sq_kernel +
// clip_adam_kernel).  state: fold slot 0's clip state (MSIG_GC_NSTAT doubles of statistics, then `cap` doubles for the
// per-workgroup sums of squares), shifted per fold like every buffer; max_norm per fold of the launch.
struct ClipArgs { double* state; int cap; double max_norm[MSIG_MAX_FOLDS]; };
int launch_colsum_clip_adam_plan(const ColsumPlan& plan, const AdamArgs& ad, const FoldCtx& fc, const ClipArgs& cl, hipStream_t st);
// sub-regions of MSIG_WS_GRAD_PART, in floats
struct PartOffsets { int64_t head, l1, l0, conv2, conv1, total; int gru_rows; };
PartOffsets part_offsets(const StageDims& d);

// Number of persistent workgroups used by reduction-style kernels; partial buffers are sized for it.
#define MSIG_PERSIST_WG 1024
#define MSIG_DW_WG 512

// ---- BatchNorm batch statistics (conv1_fwd_kernel, pool1_conv2_fwd_kernel) --------------------------------------------------------
// conv1 sees the raw input: a channel that sits many spreads from zero (a temperature column, a subject normalised against resting
// windows) gives conv1 outputs with mean^2 >> var.  conv2 sees BatchNorm-1's normalised, rectified output — centred enough near
// initialisation (mean^2 / var <= 7), but a trained BatchNorm-1 channel with a small gamma under a positive beta is "always on", and
// one-signed conv2 taps over such channels put conv2's mean a thousand spreads out (tests/regimes.py conv2_offcentre: mean^2 / var up
// to 1300; the one set of sums stage 2 used to keep failed the parity gate there at 1 .. 37 work items).  A workgroup of either kernel
// writes TWO rows of partial sums (WS_BN1_PART: [MSIG_PERSIST_WG][32] floats, then [MSIG_PERSIST_WG][32] doubles; WS_BN2_PART the
// same with 64 columns):
//   unshifted  sum y, sum y^2 per thread in fp32, reduced in fp32 — the sums this library has always formed.  Their variance
//              E[y^2] - mean^2 loses mean^2 / var of its relative precision: exact enough while the channel mean is a few spreads,
//              100 x worse at 10 spreads;
//   shifted    sum (y - p), sum (y - p)^2 per thread in fp32 with p = the thread's FIRST value of the channel, so what is squared is
//              of the size of the spread; bn_unshift turns (n, p, sums) into sum y, sum y^2 in double and the reductions stay double.
// bn_batch_sums picks per channel: the unshifted sums where they are well conditioned, mean^2 <= BN_SHIFT_RATIO x var (judged on the
// shifted sums) — every bit of every result on such inputs is what it was before the shifted sums existed, recorded training
// trajectories included —, the shifted sums beyond.  At the switch the unshifted variance carries 17 x the rounding of its sums, an
// order of magnitude inside what the parity gate allows.  bn_finalize_kernel and ab_merge_kernel both reduce through this function.
#define BN_SHIFT_RATIO 16.0
#define BN1_STAGE_CH 16
__device__ __forceinline__ void bn_unshift(int n, float p, float sd, float sq, double& s1, double& s2) {
  const double dn = (double)n, dp = (double)p, dsd = (double)sd;
  s1 = dn * dp + dsd;
  s2 = (double)sq + dp * (2.0 * dsd + dn * dp);
}
__device__ __forceinline__ const double* bn_shifted_part(const float* part, int CH) { return (const double*)(part + (size_t)MSIG_PERSIST_WG * 2 * CH); }
__device__ __forceinline__ double* bn_shifted_part(float* part, int CH) { return (double*)(part + (size_t)MSIG_PERSIST_WG * 2 * CH); }
// For tid < CH: the batch's sum y (s1) and sum y^2 (s2) of channel tid; returns whether they are the shifted ones.  Called by all
// FIN_THREADS threads; red: FIN_THREADS doubles.
__device__ __forceinline__ bool bn_batch_sums(const float* __restrict__ part, int nrows, int CH, double count, double* red, double& s1, double& s2) {
  const int tid = threadIdx.x;
  fin_colsums(part, nrows, 2 * CH, red);          // 2 * CH <= 64 columns
  s1 = 0.0; s2 = 0.0;
  if (tid < CH) { s1 = red[tid]; s2 = red[CH + tid]; }
  if (msig_negctl_input == 1 || (msig_negctl_stage2 == 1 && CH != BN1_STAGE_CH)) return false;
  __syncthreads();
  fin_colsums(bn_shifted_part(part, CH), nrows, 2 * CH, red);
  bool shifted = false;
  if (tid < CH) {
    const double t1 = red[tid], t2 = red[CH + tid], m = t1 / count;
    double v = t2 / count - m * m;
    if (v < 0.0) v = 0.0;
    shifted = m * m > BN_SHIFT_RATIO * v;
    if (shifted) { s1 = t1; s2 = t2; }
  }
  return shifted;
}
#define MSIG_CONV_DW_WG 1024      // conv weight-gradient kernels: 4 workgroups per CU hide their staging latency
