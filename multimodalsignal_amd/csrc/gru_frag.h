// Prologue pieces of the GRU kernels (gru.hip, gru_bwd4.hip, gru_bwd6.hip), each written once: the resident weight fragments (MFMA A
// operands, split once per launch), the bias terms, the dW tile tables of the pipelined layer-0 backward, the transposed LDS read.
// The fragment loaders are MACROS, not functions: a function boundary around a prologue — arguments by value or by reference, the
// fragment returned or filled in place — left the arithmetic alone but changed instruction order and register allocation far
// downstream (gru_fwd_ws: 2 - 9 % slower).  One textual definition expanded at every site compiles to the
// instruction stream the hand-written copies had.  The CT_* contraction tags stay at the MFMA call sites.
#pragma once
#include "gru_args.h"

#define LDS_AS __attribute__((address_space(3)))
__device__ __forceinline__ bf16x4 lds_tr_read(const __bf16* p) {      // ds_read_b64_tr_b16; EXEC must be all ones
  typedef __attribute__((__vector_size__(4 * sizeof(__bf16)))) __bf16 v4;
  const v4 r = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LDS_AS v4*)p);
  return __builtin_bit_cast(bf16x4, r);
}

// The resident operands are only ever read by MFMAs, which take A / B from either half of the unified register file; left to
// itself the allocator keeps part of them in arch VGPRs and parks the prefetched loads in AccVGPRs, from where every value the
// gate math needs has to be copied back first (58 / 90 v_accvgpr_read per wave-step in layer 0 / 1 of gru_bwd_b3, a quarter of the
// VALU work).  Passing them through an "a"-constrained asm pins them to AccVGPRs for the rest of the kernel.
#define PIN_ACC(v) asm volatile("" : "+a"(v))

// Row-major fragment: ROW = the lane's weight row (W[gate row][0]), LQ its k group; k block kb holds ROW[kb * 32 + LQ * 8 .. + 7].
// Two-piece fp16 (msig_dev.h f16x2): the values are loaded ONCE — the scale needs the fragment's largest magnitude before the
// split — and the pieces A[NKB][2] carry S_w = f16x2_weight_scale(max).  POST = 1 / (S_w S_OP), a power of two, undoes S_w and the
// scale S_OP of the other operand (F16X2_H_SCALE for the state, the dropout-derived one for layer 1's input).  LOAD8 is how the
// eight values of a k block arrive and join the maximum: FRAG_LOAD8_VEC4 (two 16-byte loads: the input weights' sites) or
// FRAG_LOAD8_INDEXED (the recurrent weights' sites).
#define FRAG_LOAD8_VEC4(wv, m, ptr)                                                                                                    \
  const float4* wi_ = (const float4*)(ptr);                                                                                           \
  const float4 a0 = wi_[0], a1 = wi_[1];                                                                                              \
  wv[0] = a0.x; wv[1] = a0.y; wv[2] = a0.z; wv[3] = a0.w; wv[4] = a1.x; wv[5] = a1.y; wv[6] = a1.z; wv[7] = a1.w;                     \
  _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) m = fmaxf(m, fabsf(wv[j_]));
#define FRAG_LOAD8_INDEXED(wv, m, ptr)                                                                                                 \
  const float* wr_ = (ptr);                                                                                                           \
  _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) { wv[j_] = wr_[j_]; m = fmaxf(m, fabsf(wv[j_])); }
#define LOAD_FRAG_F16X2(NKB, LOAD8, ROW, LQ, S_OP, A, POST)                                                                            \
  {                                                                                                                                   \
    float wv_[NKB][8], m_ = 0.f;                                                                                                      \
    _Pragma("unroll") for (int kb_ = 0; kb_ < NKB; ++kb_) { LOAD8(wv_[kb_], m_, ROW + kb_ * 32 + LQ * 8) }                                 \
    const float sw_ = f16x2_weight_scale(m_);                                                                                         \
    POST = 1.0f / (sw_ * S_OP);                                                                                                       \
    _Pragma("unroll") for (int kb_ = 0; kb_ < NKB; ++kb_)                                                                                \
      _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) { _Float16 p0, p1; split2(wv_[kb_][j_], sw_, p0, p1); A[kb_][0][j_] = p0; A[kb_][1][j_] = p1; } \
  }
// Split-bf16 (three pieces), same addressing: one k block (PTR = its eight values, A[3]), and a fragment of NKB of them (A[NKB][3]).
#define LOAD_FRAG_BF16X3_BLOCK(PTR, A)                                                                                                 \
  {                                                                                                                                   \
    const float* wr_ = PTR;                                                                                                           \
    _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) { __bf16 p0, p1, p2; split3(wr_[j_], p0, p1, p2); A[0][j_] = p0; A[1][j_] = p1; A[2][j_] = p2; } \
  }
#define LOAD_FRAG_BF16X3(NKB, ROW, LQ, A) \
  _Pragma("unroll") for (int kb_ = 0; kb_ < NKB; ++kb_) LOAD_FRAG_BF16X3_BLOCK(ROW + kb_ * 32 + LQ * 8, A[kb_])
// One element of a transposed split-bf16 fragment A[6][3] of the backward contractions: A[i = li][k] = W[k][CB * 16 + li] over the
// 192 gate rows [r|z|n] in six 32-wide k blocks (k = KB * 32 + lq * 8 + J), W row-major with leading dimension LD, CB the 16-wide
// column block; a wave that is not ACTIVE (dx2_role: fewer column blocks than waves) gets zeros and touches no memory.  The
// kernels keep their own loops around it — which fragments share a loop, and the order of their PIN_ACCs, decide the register
// allocation of the pipelined step bodies; li, lq and the scratch pieces p0, p1, p2 are the caller's.
#define FRAG_T_ELEM(A, W, LD, CB, KB, J, ACTIVE)                                                \
  split3(ACTIVE ? W[(size_t)(KB * 32 + lq * 8 + J) * LD + CB * 16 + li] : 0.f, p0, p1, p2);     \
  A[KB][0][J] = p0; A[KB][1][J] = p1; A[KB][2][J] = p2;

// One bias term of unit U as the gate math takes it: b_r = b_ir + b_hr, b_z = b_iz + b_hz, b_in, b_hn (D: the direction's GruDir).
#define GRU_BIAS_R(D, U) (D.bih[U] + D.bhh[U])
#define GRU_BIAS_Z(D, U) (D.bih[64 + U] + D.bhh[64 + U])
#define GRU_BIAS_IN(D, U) D.bih[128 + U]
#define GRU_BIAS_HN(D, U) D.bhh[128 + U]

// dW tile tables of the pipelined layer-0 backward (gru_bwd_b4 / b5 / b6): tile t = (A block: 32 consecutive columns of the
// gate-gradient planes [dr|dz|dhn|dn], B block: 32 columns of [x | h_prev]).
// n-gate role (wave w = 0, 1): 32 n-gate units: dW_ih <- dn . x, dW_hh <- dhn . h_prev
#define DW_TILES_N(w, aoff, boff)       \
  aoff[0] = 192 + 32 * w; boff[0] = 0;  \
  aoff[1] = 128 + 32 * w; boff[1] = 32; \
  aoff[2] = 128 + 32 * w; boff[2] = 64;
// r/z role (wave 2: the r gate, wave 3: the z gate): units lo / hi x columns x, h lo, h hi
#define DW_TILES_RZ(w, aoff, boff)                                                                              \
  const int gc_ = (w - 2) * 64;                                                                                 \
  _Pragma("unroll") for (int t = 0; t < 6; ++t) { aoff[t] = gc_ + 32 * (t / 3); boff[t] = 32 * (t % 3); }
