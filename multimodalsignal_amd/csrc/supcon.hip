// include/msig_sc.h: supervised contrastive loss on the 128-d feature — two launches between the head's launch and the GRU backward
// (DESIGN.md section 32).  B x B similarities over 128 dimensions and the gradient G . Z, both on the exact-fp32 matrix instruction;
// a workgroup owns 32 rows and walks the columns in tiles of 64 in increasing order, so every sum has one fixed order.
#include "msig_dev.h"
#include "../../include/msig_sc.h"

#define SC_THREADS 256
#define SC_ROWS 32               // rows a workgroup owns: two 16-row MFMA tiles
#define SC_COLS 64               // columns of a tile: one 16-column MFMA tile per wave
#define SC_D 128
#define SC_ZS 132                // floats between rows of Z in LDS: 16 lanes' ds_read_b128 of one k block fall into 64 distinct banks
#define SC_SS 68                 // floats between rows of the similarity tile in LDS: the D-layout stores are conflict-free

int msig_multi_fold_ctx(const msig_multi* m, FoldCtx& fc);                                  // api.hip: msig_multi's own checks

// What sc_rows_kernel leaves per row for sc_grad_kernel, after the B normalised rows of the scratch.
struct ScRow {
  double L;                      // lse_i - sum_p s_ip / |P(i)|  (0 for a row that is no anchor)
  float m, se;                   // row maximum over A(i) (-inf when A(i) is empty) and sum_a exp(s_ia - m)
  int32_t np, top;               // |P(i)|; 1 iff i is an anchor whose first maximum over A(i) is a positive
  float nrm;                     // max(||f_i||, 1e-12)
  int32_t pad;
};
static_assert(sizeof(ScRow) == 32, "ScRow");
static inline int64_t sc_scratch_bytes(int64_t B) { return (B * (SC_D * 4 + (int64_t)sizeof(ScRow)) + 255) / 256 * 256; }

struct ScFold {
  const int32_t* grp; const int64_t* idx;
  float* z; ScRow* rows; double* stats;
};
__device__ __forceinline__ ScFold sc_fold(const ScArgs& a, const FoldCtx& fc) {
  const int z = blockIdx.z;
  const int64_t goff = (int64_t)fc.slot[z] * a.stride;
  ScFold f;
  f.grp = a.grp ? (const int32_t*)((const char*)a.grp + goff) : nullptr;
  f.idx = a.idx ? a.idx + (int64_t)z * a.idx_row_stride : nullptr;
  char* scratch = a.scratch + goff;
  f.z = (float*)scratch;
  f.rows = (ScRow*)(scratch + (size_t)a.B * SC_D * 4);
  f.stats = a.stats ? (double*)((char*)a.stats + goff) : nullptr;
  return f;
}

// Rows r0 .. r0 + NR of feat, normalised, into LDS (rows >= B as zeros); a wave takes two rows per pass, 32 lanes x float4 each.
// The squares are summed in fp64 by an xor butterfly, whose result is the same in every lane and for every caller: a row has the
// same bits in the workgroup that owns it and in every workgroup that loads it as a column.
template <int NR>
__device__ __forceinline__ void sc_normalise_tile(const float* __restrict__ feat, int r0, int B, float* lds, float* zout, float* nrm_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int p = 0; p < NR / 8; ++p) {
    const int lr = p * 8 + wave * 2 + (lane >> 5), c4 = lane & 31;
    const int row = r0 + lr;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row < B) v = *(const f32x4*)(feat + (size_t)row * SC_D + c4 * 4);
    double ss = ((double)v[0] * (double)v[0] + (double)v[1] * (double)v[1]) + ((double)v[2] * (double)v[2] + (double)v[3] * (double)v[3]);
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    const float n = fmaxf((float)sqrt(ss), 1e-12f);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = v[e] / n;
    *(f32x4*)(lds + lr * SC_ZS + c4 * 4) = v;
    if (zout && row < B) *(f32x4*)(zout + (size_t)row * SC_D + c4 * 4) = v;
    if (nrm_out && c4 == 0) nrm_out[lr] = n;
  }
}
// The same rows as sc_rows_kernel left them in the scratch.
template <int NR>
__device__ __forceinline__ void sc_copy_tile(const float* __restrict__ z, int r0, int B, float* lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int p = 0; p < NR / 8; ++p) {
    const int lr = p * 8 + wave * 2 + (lane >> 5), c4 = lane & 31;
    const int row = r0 + lr;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row < B) v = *(const f32x4*)(z + (size_t)row * SC_D + c4 * 4);
    *(f32x4*)(lds + lr * SC_ZS + c4 * 4) = v;
  }
}
// Label and group of rows r0 .. r0 + n by the first n threads: y = -1 for a row that is not valid (or >= B), g = 0 in class mode.
__device__ __forceinline__ void sc_load_meta(const ScArgs& a, const ScFold& f, const int64_t* __restrict__ labels, int r0, int n, int* sy, int* sg) {
  const int tid = threadIdx.x;
  if (tid >= n) return;
  const int row = r0 + tid;
  int y = -1, g = 0;
  if (row < a.B) {
    const int64_t yy = labels[row];
    if (yy >= 0 && yy < a.K) y = (int)yy;
    if (a.positives) {
      g = f.grp[f.idx ? f.idx[row] : (int64_t)row];
      if (g < 0) y = -1;
    }
  }
  sy[tid] = y; sg[tid] = g;
}

// The workgroup's rows as A operands: lane (c = lane & 15, q = lane >> 4) holds k = 16 jj + 4 q + e of row 16 rt + c.  The k slots of
// one instruction are the four q; which k a slot carries is free as long as A and B agree.
__device__ __forceinline__ void sc_load_a(const float* zr, f32x4 (&a)[2][8]) {
  const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) a[rt][jj] = *(const f32x4*)(zr + (rt * 16 + c) * SC_ZS + 16 * jj + 4 * q);
}
// S (32 x 64) = Zr Zc^T / tau into LDS: wave w forms columns 16 w .. 16 w + 15 of both row tiles.  Both kernels call this one
// function: sc_grad_kernel sees the similarities sc_rows_kernel saw, bit for bit.
__device__ __forceinline__ void sc_sim_tile(const f32x4 (&a)[2][8], const float* zc, float tau, float* S) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) {
    const f32x4 b = *(const f32x4*)(zc + (wave * 16 + c) * SC_ZS + 16 * jj + 4 * q);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc0 = mfma16(a[0][jj][e], b[e], acc0);
      acc1 = mfma16(a[1][jj][e], b[e], acc1);
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    S[(q * 4 + e) * SC_SS + wave * 16 + c] = acc0[e] / tau;
    S[(16 + q * 4 + e) * SC_SS + wave * 16 + c] = acc1[e] / tau;
  }
}
// membership of column j (label yj, group gj; yj < 0: not valid) in A(i) and P(i)
__device__ __forceinline__ void sc_sets(bool cross, int i, int yi, int gi, int j, int yj, int gj, bool& inA, bool& inP) {
  const bool valid = yi >= 0 && yj >= 0 && i != j;
  const bool samey = yi == yj, sameg = cross && gi == gj;
  inA = valid && !(samey && sameg);
  inP = valid && samey && !sameg;
}

// ---- launch 1: the rows' statistics ---------------------------------------------------------------------------------------------------
//   1  the workgroup's 32 rows, normalised, into LDS and into the scratch
//   2  per tile of 64 columns: normalise on load (no prologue launch, no dependence on another workgroup), S on the matrix pipe, then
//      thread (row = tid >> 3, sub = tid & 7) folds columns 8 sub .. 8 sub + 7 into its running maximum, sum of exponentials (fp64),
//      positive count and sum (fp64) and first maximum
//   3  the eight threads of a row merge in increasing sub; one of them writes the row's record
// LDS: (32 + 64) x 132 x 4 + 32 x 68 x 4 + 896 = 60 288 bytes.
__global__ __launch_bounds__(SC_THREADS) void sc_rows_kernel(const ScArgs a, const float* __restrict__ feat, const int64_t* __restrict__ labels,
                                                             const FoldCtx fc) {
  FOLD_BEGIN; FS(feat); FS(labels);
  const ScFold f = sc_fold(a, fc);
  __shared__ __attribute__((aligned(16))) float s_zr[SC_ROWS * SC_ZS];
  __shared__ __attribute__((aligned(16))) float s_zc[SC_COLS * SC_ZS];
  __shared__ __attribute__((aligned(16))) float s_S[SC_ROWS * SC_SS];
  __shared__ float s_rn[SC_ROWS];
  __shared__ int s_ry[SC_ROWS], s_rg[SC_ROWS], s_cy[SC_COLS], s_cg[SC_COLS];
  const int tid = threadIdx.x, B = a.B;
  const int i0 = blockIdx.x * SC_ROWS;
  const bool cross = a.positives != 0;

  sc_normalise_tile<SC_ROWS>(feat, i0, B, s_zr, f.z, s_rn);
  sc_load_meta(a, f, labels, i0, SC_ROWS, s_ry, s_rg);
  __syncthreads();
  f32x4 af[2][8];
  sc_load_a(s_zr, af);
  const int r = tid >> 3, sub = tid & 7, gi = i0 + r;
  const int yi = s_ry[r], ggi = s_rg[r];
  float m = -INFINITY;
  double se = 0.0, sp = 0.0;
  int cnt = 0, arg = 0x7fffffff, pos = 0;

  for (int j0 = 0; j0 < B; j0 += SC_COLS) {
    sc_normalise_tile<SC_COLS>(feat, j0, B, s_zc, nullptr, nullptr);
    sc_load_meta(a, f, labels, j0, SC_COLS, s_cy, s_cg);
    __syncthreads();
    sc_sim_tile(af, s_zc, a.tau, s_S);
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int col = sub * 8 + e, j = j0 + col;
      bool inA, inP;
      sc_sets(cross, gi, yi, ggi, j, s_cy[col], s_cg[col], inA, inP);
      const float s = s_S[r * SC_SS + col];
      if (inA) {
        if (s > m) { se = se * (double)expf(m - s) + 1.0; m = s; arg = j; pos = inP ? 1 : 0; }
        else se += (double)expf(s - m);
      }
      if (inP) { sp += (double)s; cnt += 1; }
    }
    __syncthreads();          // the next tile overwrites s_zc, s_cy, s_cg and s_S
  }

  const int base = (tid & 63) & ~7;
  float M = -INFINITY;
  double SE = 0.0, SP = 0.0;
  int CNT = 0, ARG = 0x7fffffff, POS = 0;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const float mt = __shfl(m, base + t, 64);
    const double set = __shfl(se, base + t, 64), spt = __shfl(sp, base + t, 64);
    const int cntt = __shfl(cnt, base + t, 64), argt = __shfl(arg, base + t, 64), post = __shfl(pos, base + t, 64);
    if (mt != -INFINITY) {
      if (mt > M || (mt == M && argt < ARG)) { ARG = argt; POS = post; }
      if (mt > M) { SE = SE * (double)expf(M - mt) + set; M = mt; }
      else SE += set * (double)expf(mt - M);
    }
    SP += spt; CNT += cntt;
  }
  if (sub == 0 && gi < B) {
    ScRow rec;
    rec.L = CNT > 0 ? ((double)M + log(SE)) - SP / (double)CNT : 0.0;
    rec.m = M; rec.se = (float)SE;
    rec.np = CNT; rec.top = (CNT > 0 && POS) ? 1 : 0;
    rec.nrm = s_rn[r]; rec.pad = 0;
    f.rows[gi] = rec;
  }
}

// ---- launch 2: the statistics and the gradient ------------------------------------------------------------------------------------------
//   1  every workgroup counts the anchors from the rows' records; none: nothing is written
//   2  workgroup 0 of the fold adds the statistics: sum L_i in fp64 in increasing i by one thread out of LDS
//   3  per tile of 64 columns: the similarities again (sc_sim_tile), G_ij = C_ij + C_ji (without 1 / N_a) in place — S and the sets are
//      symmetric, so one s_ij serves both terms —, then dz (32 x 128) += G (32 x 64) . Z (64 x 128) with G read back as the A operand
//   4  the epilogue: dz through LDS, the normalisation's backward per row, dfeat += w * df in two roundings
// LDS: as sc_rows_kernel + 768 bytes of column statistics.
__global__ __launch_bounds__(SC_THREADS) void sc_grad_kernel(const ScArgs a, const int64_t* __restrict__ labels, float* __restrict__ dfeat,
                                                             const FoldCtx fc) {
#pragma clang fp contract(off)
  FOLD_BEGIN; FS(labels); FS(dfeat);
  const ScFold f = sc_fold(a, fc);
  __shared__ __attribute__((aligned(16))) float s_zr[SC_ROWS * SC_ZS];
  __shared__ __attribute__((aligned(16))) float s_zc[SC_COLS * SC_ZS];
  __shared__ __attribute__((aligned(16))) float s_S[SC_ROWS * SC_SS];
  __shared__ int s_ry[SC_ROWS], s_rg[SC_ROWS], s_cy[SC_COLS], s_cg[SC_COLS];
  __shared__ float s_cm[SC_COLS], s_crse[SC_COLS], s_cpinv[SC_COLS];
  const int tid = threadIdx.x, B = a.B;
  const int i0 = blockIdx.x * SC_ROWS;
  const bool cross = a.positives != 0;
  const float w = a.weight[blockIdx.z];

  int na = 0, ntop = 0;
  for (int b0 = 0; b0 < B; b0 += SC_THREADS) {
    const int row = b0 + tid;
    const bool anchor = row < B && f.rows[row].np > 0;
    na += __syncthreads_count(anchor ? 1 : 0);
    ntop += __syncthreads_count((anchor && f.rows[row].top) ? 1 : 0);
  }
  if (na == 0) return;
  if (blockIdx.x == 0 && f.stats) {
    double* sL = (double*)s_zc;                   // 2048 x 8 bytes of the column tile's 33 792, before its first use
    for (int row = tid; row < B; row += SC_THREADS) sL[row] = f.rows[row].np > 0 ? f.rows[row].L : 0.0;
    __syncthreads();
    if (tid == 0) {
      double sum = 0.0;
#pragma unroll 4
      for (int row = 0; row < B; ++row) sum = sum + sL[row];
      f.stats[0] += sum; f.stats[1] += (double)na; f.stats[2] += (double)ntop; f.stats[3] += 1.0;
    }
    __syncthreads();
  }
  if (w == 0.f) return;                           // a probe: the statistics alone

  sc_copy_tile<SC_ROWS>(f.z, i0, B, s_zr);
  sc_load_meta(a, f, labels, i0, SC_ROWS, s_ry, s_rg);
  __syncthreads();
  f32x4 af[2][8];
  sc_load_a(s_zr, af);
  const int r = tid >> 3, sub = tid & 7, gi = i0 + r;
  const int yi = s_ry[r], ggi = s_rg[r];
  // a row that is no anchor: m = +inf makes its exponentials 0, and its two factors are 0
  float mi = INFINITY, rsei = 0.f, pinvi = 0.f, nrmi = 1.f;
  if (gi < B) {
    const ScRow rec = f.rows[gi];
    nrmi = rec.nrm;
    if (rec.np > 0) { mi = rec.m; rsei = 1.0f / rec.se; pinvi = 1.0f / (float)rec.np; }
  }
  const int lane = tid & 63, wave = tid >> 6, c = lane & 15, q = lane >> 4;
  f32x4 dz[2][2];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int t = 0; t < 2; ++t) dz[rt][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int j0 = 0; j0 < B; j0 += SC_COLS) {
    sc_copy_tile<SC_COLS>(f.z, j0, B, s_zc);
    sc_load_meta(a, f, labels, j0, SC_COLS, s_cy, s_cg);
    if (tid < SC_COLS) {
      const int j = j0 + tid;
      float mj = INFINITY, rsej = 0.f, pinvj = 0.f;
      if (j < B) {
        const ScRow rec = f.rows[j];
        if (rec.np > 0) { mj = rec.m; rsej = 1.0f / rec.se; pinvj = 1.0f / (float)rec.np; }
      }
      s_cm[tid] = mj; s_crse[tid] = rsej; s_cpinv[tid] = pinvj;
    }
    __syncthreads();
    sc_sim_tile(af, s_zc, a.tau, s_S);
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int col = sub * 8 + e, j = j0 + col;
      bool inA, inP;
      sc_sets(cross, gi, yi, ggi, j, s_cy[col], s_cg[col], inA, inP);
      const float s = s_S[r * SC_SS + col];
      float ci = 0.f, cj = 0.f;
      if (inA) { ci = expf(s - mi) * rsei; cj = expf(s - s_cm[col]) * s_crse[col]; }
      if (inP) { ci = ci - pinvi; cj = cj - s_cpinv[col]; }
      if constexpr (msig_negctl_supcon == 1) cj = 0.f;
      s_S[r * SC_SS + col] = ci + cj;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < SC_COLS / 4; ++kk) {
      const float a0 = s_S[c * SC_SS + 4 * kk + q], a1 = s_S[(16 + c) * SC_SS + 4 * kk + q];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const float b = s_zc[(4 * kk + q) * SC_ZS + (2 * wave + t) * 16 + c];
        dz[0][t] = mfma16(a0, b, dz[0][t]);
        dz[1][t] = mfma16(a1, b, dz[1][t]);
      }
    }
    __syncthreads();          // the next tile overwrites s_zc, s_S and the column arrays
  }

  // dz (without its factor 1 / (tau N_a)) into LDS in row-major order: wave w holds columns 32 w .. 32 w + 31
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) s_zc[(rt * 16 + q * 4 + e) * SC_ZS + (2 * wave + t) * 16 + c] = dz[rt][t][e];
  __syncthreads();
  const float scale = (float)(1.0 / ((double)a.tau * (double)na));
  f32x4 zv[4], dv[4];
  float dot = 0.f;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    zv[v] = *(const f32x4*)(s_zr + r * SC_ZS + sub * 16 + v * 4);
    dv[v] = *(const f32x4*)(s_zc + r * SC_ZS + sub * 16 + v * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { dv[v][e] = dv[v][e] * scale; dot = dot + zv[v][e] * dv[v][e]; }
  }
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) dot = dot + __shfl_xor(dot, o, 64);
  if (gi < B) {
    float* __restrict__ out = dfeat + (size_t)gi * SC_D + sub * 16;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      f32x4 o = *(const f32x4*)(out + v * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float df = (dv[v][e] - zv[v][e] * dot) / nrmi;
        o[e] = o[e] + w * df;                     // contraction is off: a rounded product, then a rounded sum
      }
      *(f32x4*)(out + v * 4) = o;
    }
  }
}

int launch_sc_apply(const ScArgs& a, const float* feat, const int64_t* labels, float* dfeat, const FoldCtx& fc, hipStream_t st) {
  const dim3 grid((a.B + SC_ROWS - 1) / SC_ROWS, 1, fc.n);
  { MSIG_K("sc_rows", st); sc_rows_kernel<<<grid, SC_THREADS, 0, st>>>(a, feat, labels, fc); }
  MSIG_LAUNCH_CHECK();
  { MSIG_K("sc_grad", st); sc_grad_kernel<<<grid, SC_THREADS, 0, st>>>(a, labels, dfeat, fc); }
  MSIG_LAUNCH_CHECK();
  return 0;
}

// ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
extern "C" int msig_sc_abi_version(void) { return MSIG_SC_ABI_VERSION; }
extern "C" int64_t msig_sc_struct_bytes(void) { return (int64_t)sizeof(msig_sc); }
extern "C" int64_t msig_sc_scratch_bytes(int32_t B) {
  if (B < 1 || B > MSIG_SC_MAX_BATCH) return MSIG_E_SHAPE;
  return sc_scratch_bytes(B);
}

// the NULL and shape checks of msig_sc's own fields; the alignment checks follow in sc_check_align, after the caller's shape checks
int msig_sc_make_args(const msig_sc* k, const FoldCtx& fc, int32_t B, int32_t K, ScArgs& a) {
  if (!k) return MSIG_E_NULL;
  if (!k->scratch) return MSIG_E_NULL;
  if (k->positives == MSIG_SC_POS_CROSS_SUBJECT && !k->grp) return MSIG_E_NULL;
  if (k->positives != MSIG_SC_POS_CLASS && k->positives != MSIG_SC_POS_CROSS_SUBJECT) return MSIG_E_SHAPE;
  if (!(k->tau >= 1e-3f && k->tau <= 1e3f)) return MSIG_E_SHAPE;                              // NaN included
  for (int i = 0; i < fc.n; ++i)
    if (!(k->weight[i] >= 0.f)) return MSIG_E_SHAPE;
  if (B < 1 || B > MSIG_SC_MAX_BATCH) return MSIG_E_SHAPE;
  if (K < 2 || K > MSIG_MAX_K) return MSIG_E_SHAPE;
  const bool multi = fc.stride != 0;
  a = ScArgs{};
  a.positives = k->positives; a.B = B; a.K = K; a.tau = k->tau;
  a.grp = k->positives ? k->grp : nullptr; a.idx = k->positives ? k->idx : nullptr; a.idx_row_stride = multi ? k->idx_row_stride : 0;
  a.scratch = (char*)k->scratch; a.stats = k->stats;
  a.stride = multi ? k->stride_bytes : 0;
  for (int i = 0; i < fc.n; ++i) a.weight[i] = k->weight[i];
  return 0;
}
// what follows the caller's own shape checks (a train step's mixup weights): the last shape check and every alignment check
int msig_sc_check_align(const msig_sc* k, const FoldCtx& fc, int32_t B) {
  const bool multi = fc.stride != 0;
  if (multi && k->idx && k->idx_row_stride < B) return MSIG_E_SHAPE;
  if (msig_misaligned(k->scratch, 15)) return MSIG_E_ALIGN;
  if (msig_misaligned(k->stats, 7) || msig_misaligned(k->idx, 7)) return MSIG_E_ALIGN;
  if (msig_misaligned(k->grp, 3)) return MSIG_E_ALIGN;
  if (multi && (k->stride_bytes <= 0 || (k->stride_bytes & 255))) return MSIG_E_ALIGN;
  return 0;
}

static int sc_apply(const msig_sc* k, const FoldCtx& fc, const float* feat, const int64_t* labels, float* dfeat, int32_t B, int32_t K,
                    hipStream_t st) {
  if (!k) return MSIG_E_NULL;
  if (!k->scratch || !feat || !dfeat || !labels) return MSIG_E_NULL;
  ScArgs a; int rc = msig_sc_make_args(k, fc, B, K, a); if (rc) return rc;
  if ((rc = msig_sc_check_align(k, fc, B))) return rc;
  if (msig_misaligned(feat, 15) || msig_misaligned(dfeat, 15) || msig_misaligned(labels, 7)) return MSIG_E_ALIGN;
  return launch_sc_apply(a, feat, labels, dfeat, fc, st);
}
extern "C" int msig_sc_apply(const msig_sc* sc, const float* feat, const int64_t* labels, float* dfeat, int32_t B, int32_t K, void* stream) {
  return sc_apply(sc, single_fold(nullptr), feat, labels, dfeat, B, K, (hipStream_t)stream);
}
extern "C" int msig_sc_apply_multi(const msig_sc* sc, const msig_multi* m, const float* feat, const int64_t* labels, float* dfeat, int32_t B,
                                   int32_t K, void* stream) {
  if (!sc || !m) return MSIG_E_NULL;
  FoldCtx fc; int rc = msig_multi_fold_ctx(m, fc); if (rc) return rc;
  return sc_apply(sc, fc, feat, labels, dfeat, B, K, (hipStream_t)stream);
}
