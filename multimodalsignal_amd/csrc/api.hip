// extern "C" surface of libmsig_hip.so (declared in include/msig.h, msig_cw.h, msig_cg.h, msig_ft.h, msig_gc.h, msig_st.h, msig_da.h, msig_kd.h, msig_sam.h, msig_dro.h and msig_sc.h): argument checks,
// parameter / workspace layout, and the stage launch order.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include "msig_dev.h"
#include "../../include/msig_cw.h"
#include "../../include/msig_cg.h"
#include "../../include/msig_st.h"
#include "finetune.h"
#include "../../include/msig_ab.h"
#include "../../include/msig_mc.h"
#include "../../include/msig_kd.h"
#include "../../include/msig_sam.h"
#include "../../include/msig_dro.h"
#include "../../include/msig_sc.h"
#include "../../include/msig_tt.h"

// ---- profiling aid --------------------------------------------------------------
struct ProfRec { const char* name; hipEvent_t a, b; };
static bool g_prof_on = false;
static std::mutex g_prof_mu;          // several host threads may launch concurrently (one stream per fold)
static std::vector<ProfRec> g_recs;
static std::vector<hipEvent_t> g_pool;
static hipEvent_t prof_event() {
  if (!g_pool.empty()) { hipEvent_t e = g_pool.back(); g_pool.pop_back(); return e; }
  hipEvent_t e; (void)hipEventCreate(&e); return e;
}
MsigProfScope::MsigProfScope(const char* n, hipStream_t s) : name(n), st(s), rec(nullptr) {
  if (!g_prof_on) return;
  hipEvent_t ea;
  {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_recs.push_back(ProfRec{n, prof_event(), prof_event()});
    rec = (void*)(uintptr_t)g_recs.size();
    ea = g_recs.back().a;
  }
  (void)hipEventRecord(ea, st);
}
MsigProfScope::~MsigProfScope() {
  if (!rec) return;
  hipEvent_t eb;
  {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    eb = g_recs[(size_t)(uintptr_t)rec - 1].b;
  }
  (void)hipEventRecord(eb, st);
}
extern "C" int msig_profile_enable(int on) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (ProfRec& r : g_recs) { g_pool.push_back(r.a); g_pool.push_back(r.b); }
  g_recs.clear();
  g_prof_on = on != 0;
  return 0;
}
extern "C" int64_t msig_profile_report(char* buf, int64_t cap) {
  if (!buf || cap < 1) return MSIG_E_NULL;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  std::map<std::string, std::pair<int64_t, double>> agg;
  std::vector<std::string> order;
  for (ProfRec& r : g_recs) {
    if (hipEventSynchronize(r.b) != hipSuccess) return -5;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) return -5;
    if (!agg.count(r.name)) order.push_back(r.name);
    agg[r.name].first += 1; agg[r.name].second += (double)ms;
  }
  int64_t n = 0;
  for (const std::string& k : order) {
    char line[256];
    const int len = snprintf(line, sizeof line, "%s %lld %.6f\n", k.c_str(), (long long)agg[k].first, agg[k].second);
    if (n + len >= cap) break;
    memcpy(buf + n, line, (size_t)len); n += len;
  }
  buf[n] = 0;
  return n;
}

int launch_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps, float wd,
                int64_t step, hipStream_t st);
int launch_gather(const float* store, const int64_t* sy, const int64_t* idx, int64_t idx_row_stride, int B, int64_t wfloats, float* ox, int64_t* oy,
                  const FoldCtx& fc, hipStream_t st);

int msig_check_forms(const msig_batch* b);      // gru.hip
int msig_check_call_forms(const msig_batch* b, int n_tiles, const FoldCtx& fc);      // gru.hip: before the first launch of a call

static int check_shape(const msig_shape* s) {
  if (!s) return MSIG_E_NULL;
  if (s->B < 1 || s->C < 1 || s->C > MSIG_MAX_C || s->K < 2 || s->K > MSIG_MAX_K || s->T < 16) return MSIG_E_SHAPE;
  const StageDims d = make_dims(*s);
  if (d.TP < 1) return MSIG_E_SHAPE;
  // dropout masks and stash indices are 32-bit
  if ((int64_t)d.B * d.TP * 128 >= (int64_t)1 << 32) return MSIG_E_SHAPE;
  return 0;
}

extern "C" int msig_abi_version(void) { return MSIG_ABI_VERSION; }
extern "C" int64_t msig_struct_bytes(int32_t which) {
  return which == 0 ? (int64_t)sizeof(msig_batch) : which == 1 ? (int64_t)sizeof(msig_multi) : -1;
}

extern "C" int msig_stage_lengths(int T, int32_t* out) {
  if (!out) return MSIG_E_NULL;
  msig_shape s{1, 1, T, 2};
  const StageDims d = make_dims(s);
  out[0] = d.L1; out[1] = d.P1; out[2] = d.L2; out[3] = d.TP;
  return 0;
}

// gated = false: CnnGruModel's layout (include/msig_cg.h), the gate's two tensors with zero size.  len (optional): the tensors' true
// lengths — what lies between a tensor's end and the next offset is padding
static int param_layout(int C, int K, int64_t* off, bool gated, int64_t* len = nullptr) {
  if (!off) return MSIG_E_NULL;
  if (C < 1 || C > MSIG_MAX_C || K < 2 || K > MSIG_MAX_K) return MSIG_E_SHAPE;
  int64_t n[MSIG_NPARAM];
  const int Cr = gated ? C / 4 : 0;
  n[MSIG_P_GATE_W1] = (int64_t)Cr * C;
  n[MSIG_P_GATE_W2] = (int64_t)C * Cr;
  n[MSIG_P_CONV1_W] = 16 * C * 7;
  n[MSIG_P_BN1_G] = 16; n[MSIG_P_BN1_B] = 16;
  n[MSIG_P_CONV2_W] = 32 * 16 * 5;
  n[MSIG_P_BN2_G] = 32; n[MSIG_P_BN2_B] = 32;
  for (int layer = 0; layer < 2; ++layer)
    for (int dir = 0; dir < 2; ++dir) {
      n[MSIG_P_GRU_T(layer, dir, 0)] = 192 * (layer ? 128 : 32);
      n[MSIG_P_GRU_T(layer, dir, 1)] = 192 * 64;
      n[MSIG_P_GRU_T(layer, dir, 2)] = 192;
      n[MSIG_P_GRU_T(layer, dir, 3)] = 192;
    }
  n[MSIG_P_CLS0_W] = 64 * 128; n[MSIG_P_CLS0_B] = 64;
  n[MSIG_P_CLS3_W] = (int64_t)K * 64; n[MSIG_P_CLS3_B] = K;
  int64_t o = 0;
  for (int i = 0; i < MSIG_NPARAM; ++i) { off[i] = o; o += (n[i] + 3) / 4 * 4; if (len) len[i] = n[i]; }
  off[MSIG_NPARAM] = o;
  return 0;
}
// the layout of a MSIG_GC_KIND_* with the lengths (sam.hip walks the tensors, never the padding)
int msig_param_table(int C, int K, int kind, int64_t* off, int64_t* len) { return param_layout(C, K, off, kind == MSIG_GC_KIND_ATTENTION, len); }
extern "C" int msig_param_layout(int C, int K, int64_t* off) { return param_layout(C, K, off, true); }

static inline int64_t imin(int64_t a, int64_t b) { return a < b ? a : b; }
static inline int64_t imax(int64_t a, int64_t b) { return a > b ? a : b; }

extern "C" int msig_workspace_layout(const msig_shape* s, int training, int64_t* off) {
  int rc = check_shape(s);
  if (rc) return rc;
  if (!off) return MSIG_E_NULL;
  const StageDims d = make_dims(*s);
  const int64_t B = d.B, F = sizeof(float);
  int64_t sz[MSIG_NWS];
  for (int i = 0; i < MSIG_NWS; ++i) sz[i] = 0;
  sz[MSIG_WS_GATE_MEAN] = B * d.C * F;
  sz[MSIG_WS_GATE_PRE] = B * imax(d.Cr, 1) * F;
  sz[MSIG_WS_GATE_S] = B * d.C * F;
  sz[MSIG_WS_Y1] = B * d.L1 * 16 * F;
  sz[MSIG_WS_BN1_PART] = (int64_t)MSIG_PERSIST_WG * 32 * (F + (int64_t)sizeof(double));      // unshifted float rows, then shifted double rows (msig_dev.h)
  sz[MSIG_WS_BN1_STAT] = 80 * F;      // five rows: bn_finalize_kernel (frontend.hip)
  sz[MSIG_WS_P1] = B * d.P1 * 16 * F;
  sz[MSIG_WS_Y2] = B * d.L2 * 32 * F;
  sz[MSIG_WS_BN2_PART] = (int64_t)MSIG_PERSIST_WG * 64 * (F + (int64_t)sizeof(double));      // the same two sets of rows
  sz[MSIG_WS_BN2_STAT] = 160 * F;
  sz[MSIG_WS_P2] = B * d.TP * 32 * F;
  sz[MSIG_WS_H0] = B * d.TP * 128 * F;
  sz[MSIG_WS_H1] = B * d.TP * 64 * F;
  sz[MSIG_WS_FEAT] = B * 128 * F;
  sz[MSIG_WS_HID] = B * 64 * F;
  sz[MSIG_WS_LOGITS] = B * d.K * F;
  sz[MSIG_WS_PROBS] = B * d.K * F;
  sz[MSIG_WS_PRED] = B * (int64_t)sizeof(int32_t);
  sz[MSIG_WS_LOSS] = 4 * F;
  if (d.NT < 192) sz[MSIG_WS_GI] = 2 * (int64_t)d.NT * d.TP * 4 * 3 * 64 * 4 * F;   // latency form of the GRU forward (2 directions of layer 0)
  if (training) {
    const int64_t unit = 4096 * F;     // one (tile, step): 4 waves x 4 gates x 64 lanes x float4
    sz[MSIG_WS_STASH0] = 2 * (int64_t)d.NT * d.TP * unit;
    sz[MSIG_WS_STASH1] = (int64_t)d.NT * d.TP * unit;
    sz[MSIG_WS_STASH1R] = (int64_t)d.NT * unit;
    sz[MSIG_WS_DLOGITS] = B * d.K * F;
    sz[MSIG_WS_DFEAT] = B * 128 * F;
    sz[MSIG_WS_DH0] = B * d.TP * 128 * F;
    sz[MSIG_WS_DX0] = 2 * B * d.TP * 32 * F;
    sz[MSIG_WS_DY2] = B * d.L2 * 32 * F;
    sz[MSIG_WS_POOLC1] = B * d.P1 * 4;              // bytes
    sz[MSIG_WS_POOLC2] = B * d.TP * 8;
    sz[MSIG_WS_G1W] = B * (B >= 256 ? 1 : 8) * 32 * (int64_t)((d.C * 7 + 15) / 16 * 16) * F;      // small batches: up to 8 segment records per window (conv1_bwd_segs)
    sz[MSIG_WS_GATE_EO] = B * d.C * 2 * F;
    sz[MSIG_WS_DP1] = B * d.P1 * 16 * F;
    sz[MSIG_WS_DS] = B * d.C * F;
    sz[MSIG_WS_BNB_PART] = (int64_t)MSIG_PERSIST_WG * 64 * F;
    sz[MSIG_WS_BNB_STAT] = 64 * F;
    sz[MSIG_WS_GRAD_PART] = part_offsets(d).total * F;      // one sub-region per producer, see ColsumPlan
  }
  int64_t o = 0;
  for (int i = 0; i < MSIG_NWS; ++i) { off[i] = o; o += (sz[i] + 255) / 256 * 256; }
  off[MSIG_NWS] = o;
  return 0;
}

extern "C" int64_t msig_workspace_bytes(const msig_shape* s, int training) {
  int64_t off[MSIG_NWS + 1];
  const int rc = msig_workspace_layout(s, training, off);
  return rc ? (int64_t)rc : off[MSIG_NWS];
}

struct Ctx {
  StageDims d;
  WsPtrs w;
  int64_t po[MSIG_NPARAM + 1];
};

// cg: CnnGruModel (include/msig_cg.h), whose parameter layout has no gate tensors
static int make_ctx(const msig_batch* b, Ctx& c, bool need_grads, bool cg = false) {
  if (!b) return MSIG_E_NULL;
  int rc = check_shape(&b->shape);
  if (rc) return rc;
  if (!b->x || !b->params || !b->bn_state || !b->bn_count || !b->ws) return MSIG_E_NULL;
  if (need_grads && !b->grads) return MSIG_E_NULL;
  if (((uintptr_t)b->x | (uintptr_t)b->params | (uintptr_t)b->ws | (uintptr_t)b->grads | (uintptr_t)b->dx) & 15) return MSIG_E_ALIGN;
  if (b->dropout_thr < 0 || b->dropout_thr > 256) return MSIG_E_SHAPE;
  if ((uintptr_t)b->loss_acc & 7) return MSIG_E_ALIGN;
  if (b->dx && !msig_keeps(b)) return MSIG_E_SHAPE;         // an input gradient needs a forward that kept for a backward
  if (b->gru_layers < 0 || b->gru_layers > 2) return MSIG_E_SHAPE;
  if ((rc = msig_check_forms(b))) return rc;
  c.d = make_dims(b->shape);
  rc = msig_workspace_layout(&b->shape, msig_keeps(b), c.w.off);      // an eval forward kept for a backward has the training layout
  if (rc) return rc;
  if (b->ws_bytes < c.w.off[MSIG_NWS]) return MSIG_E_WORKSPACE;
  c.w.base = (char*)b->ws;
  return param_layout(b->shape.C, b->shape.K, c.po, !cg);
}

extern "C" int msig_frontend_fwd(const msig_batch* b, void* stream) {
  Ctx c; int rc = make_ctx(b, c, false); if (rc) return rc;
  return launch_frontend_fwd(b, c.d, c.w, c.po, single_fold(b), (hipStream_t)stream);
}
extern "C" int msig_gru_fwd(const msig_batch* b, void* stream) {
  Ctx c; int rc = make_ctx(b, c, false); if (rc) return rc;
  return launch_gru_fwd(b, c.d, c.w, c.po, single_fold(b), (hipStream_t)stream);
}
extern "C" int msig_head_ce_fwd(const msig_batch* b, void* stream) {
  Ctx c; int rc = make_ctx(b, c, false); if (rc) return rc;
  return launch_head_fwd(b, c.d, c.w, c.po, single_fold(b), (hipStream_t)stream, StepOpts{});
}
extern "C" int msig_head_ce_bwd(const msig_batch* b, const float* dlogits, void* stream) {
  Ctx c; int rc = make_ctx(b, c, true); if (rc) return rc;
  if (!msig_keeps(b)) return MSIG_E_SHAPE;
  ColsumPlan plan;
  if ((rc = launch_head_bwd(b, dlogits, c.d, c.w, c.po, plan, single_fold(b), (hipStream_t)stream))) return rc;
  return launch_colsum_plan(plan, single_fold(b), (hipStream_t)stream);
}
extern "C" int msig_gru_bwd(const msig_batch* b, void* stream) {
  Ctx c; int rc = make_ctx(b, c, true); if (rc) return rc;
  if (!msig_keeps(b)) return MSIG_E_SHAPE;
  ColsumPlan plan;
  if ((rc = launch_gru_bwd(b, c.d, c.w, c.po, plan, single_fold(b), (hipStream_t)stream))) return rc;
  return launch_colsum_plan(plan, single_fold(b), (hipStream_t)stream);
}
extern "C" int msig_frontend_bwd(const msig_batch* b, void* stream) {
  Ctx c; int rc = make_ctx(b, c, true); if (rc) return rc;
  if (!msig_keeps(b)) return MSIG_E_SHAPE;
  ColsumPlan plan;
  if ((rc = launch_frontend_bwd(b, c.d, c.w, c.po, plan, single_fold(b), (hipStream_t)stream))) return rc;
  return launch_colsum_plan(plan, single_fold(b), (hipStream_t)stream);
}

// Every msig_*_forward[_multi] ends here and every msig_*_train_step[_multi] in train_step_fc: an entry point checks its own
// arguments in its header's order, fills a StepOpts (msig_dev.h; StepOpts{} = the msig.h call) and calls.  Reads o.cw, o.cg, o.soft.
static int forward_fc(const msig_batch* b, const FoldCtx& fc, hipStream_t st, const StepOpts& o, bool with_head = true) {
  if (!b) return MSIG_E_NULL;
  if (b->dx && fc.stride != 0) return MSIG_E_SHAPE;          // no input gradients in fold batches
  Ctx c; int rc = make_ctx(b, c, false, o.cg); if (rc) return rc;
  if ((rc = msig_check_call_forms(b, c.d.NT, fc))) return rc;      // nothing has been launched: no model state has changed
  if ((rc = launch_frontend_fwd(b, c.d, c.w, c.po, fc, st, !o.cg))) return rc;
  if ((rc = launch_gru_fwd(b, c.d, c.w, c.po, fc, st))) return rc;
  return with_head ? launch_head_fwd(b, c.d, c.w, c.po, fc, st, o) : 0;
}
extern "C" int msig_forward(const msig_batch* b, void* stream) {
  return forward_fc(b, single_fold(b), (hipStream_t)stream, StepOpts{});
}

// reads o.cg
static int backward_fc(const msig_batch* b, const float* dlogits, const FoldCtx& fc, hipStream_t st, const StepOpts& o) {
  const bool cg = o.cg;
  Ctx c; int rc = make_ctx(b, c, true, cg); if (rc) return rc;
  if (!msig_keeps(b)) return MSIG_E_SHAPE;
  ColsumPlan plan;      // every weight-gradient reduction of the pass, done by one launch at the end
  if ((rc = launch_head_bwd(b, dlogits, c.d, c.w, c.po, plan, fc, st))) return rc;
  if ((rc = launch_gru_bwd(b, c.d, c.w, c.po, plan, fc, st))) return rc;
  if ((rc = launch_frontend_bwd(b, c.d, c.w, c.po, plan, fc, st, !cg))) return rc;
  return launch_colsum_plan(plan, fc, st);
}
extern "C" int msig_backward(const msig_batch* b, const float* dlogits, void* stream) {
  return backward_fc(b, dlogits, single_fold(b), (hipStream_t)stream, StepOpts{});
}

extern "C" int msig_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                              float beta1, float beta2, float eps, float weight_decay, int64_t step, void* stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq) return MSIG_E_NULL;
  if (n < 0 || (n & 3) || step < 1) return MSIG_E_SHAPE;
  if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) return MSIG_E_ALIGN;
  return launch_adam(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step, (hipStream_t)stream);
}

// One pass of a train step, forward through front-end backward, with every optional term at its place; the weight-gradient partials go to
// `plan`, which the caller reduces.  Both passes of a sharpness-aware step and every other step run THIS sequence: a term has one place.
// head_step: the head's forward, CrossEntropy and backward as one launch (train_step_fc decides).  Reads every field of o but clip and sam.
static int step_pass(const msig_batch* b, const Ctx& c, const FoldCtx& fc, hipStream_t st, const StepOpts& o, bool head_step, ColsumPlan& plan) {
  int rc;
  if ((rc = forward_fc(b, fc, st, o, !head_step))) return rc;
  if (o.dro && (rc = launch_dro_apply(*o.dro, c.w.p<float>(MSIG_WS_LOGITS), b->labels, o.cw, c.w.p<float>(MSIG_WS_DLOGITS), fc, st))) return rc;
  if (o.kd && (rc = launch_kd_apply(*o.kd, c.w.p<float>(MSIG_WS_LOGITS), c.w.p<float>(MSIG_WS_DLOGITS), fc, st))) return rc;
  if ((rc = head_step ? launch_head_step(b, c.d, c.w, c.po, plan, fc, st, o) : launch_head_bwd(b, nullptr, c.d, c.w, c.po, plan, fc, st))) return rc;
  // subject discriminator (include/msig_da.h): WS_FEAT and WS_DFEAT are complete here; its launch adds the reversed gradient to WS_DFEAT
  // (never under a sharpness-aware step: st_train_step refuses the pair)
  if (o.da && (rc = launch_da_step(*o.da, c.w.p<float>(MSIG_WS_FEAT), c.w.p<float>(MSIG_WS_DFEAT), fc, st))) return rc;
  // supervised contrastive term (include/msig_sc.h): two launches that add its gradient to WS_DFEAT; the head stays fused where it was
  if (o.sc && (rc = launch_sc_apply(*o.sc, c.w.p<float>(MSIG_WS_FEAT), b->labels, c.w.p<float>(MSIG_WS_DFEAT), fc, st))) return rc;
  if ((rc = launch_gru_bwd(b, c.d, c.w, c.po, plan, fc, st))) return rc;
  return launch_frontend_bwd(b, c.d, c.w, c.po, plan, fc, st, !o.cg);
}

// fc.lr_over_bc1 is filled in here from `lr` (single fold) or from m->lr (fold batch).  Reads every field of o.
static int train_step_fc(const msig_batch* b, FoldCtx fc, const float* lrs, const int64_t* steps, float* exp_avg, float* exp_avg_sq, float beta1,
                         float beta2, float eps, float weight_decay, int64_t step, hipStream_t st, const StepOpts& o) {
  const bool cg = o.cg;
  if (!b || !b->labels) return MSIG_E_NULL;
  if (!b->training) return MSIG_E_SHAPE;
  if (b->dx) return MSIG_E_SHAPE;                     // no input gradient in the fused step (ABI 5: msig_backward / msig_frontend_bwd only)
  if (!exp_avg || !exp_avg_sq) return MSIG_E_NULL;
  if (step < 1) return MSIG_E_SHAPE;
  if (steps)
    for (int i = 0; i < fc.n; ++i) if (steps[i] < 0) return MSIG_E_SHAPE;
  if (((uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) return MSIG_E_ALIGN;
  int rc;
  Ctx c;
  if ((rc = make_ctx(b, c, true, cg))) return rc;          // every argument check of the step before its first launch
  if ((rc = msig_check_call_forms(b, c.d.NT, fc))) return rc;
  fc.fused_step = 1;        // forward and backward forms resolve from this one descriptor: gru_fwd_ws may store the two-vector stash
  // sharpness-aware step (include/msig_sam.h): pass 1 here — the pass with the head unfused and a plan of its own, the reduction WITHOUT
  // Adam, the perturbation — then this function once more on copies of the descriptors that report nowhere (pass2), with the same keys
  if (o.sam && !o.sam->pass2) {
    ColsumPlan plan1;
    if ((rc = step_pass(b, c, fc, st, o, false, plan1))) return rc;
    if ((rc = launch_colsum_plan(plan1, fc, st))) return rc;
    if ((rc = launch_sam_perturb(*o.sam, (float*)b->params, b->grads, b->bn_state, b->bn_count, c.w.p<float>(MSIG_WS_LOSS), fc, st))) return rc;
    msig_batch b2 = *b;
    b2.loss_acc = nullptr;                  // epoch sums count a batch once, at w
    SamArgs sam2 = *o.sam;
    sam2.pass2 = true;
    KdArgs kd2;
    DroArgs dro2;
    ScArgs sc2;
    StepOpts o2 = o;
    o2.sam = &sam2;
    if (o.kd) { kd2 = *o.kd; kd2.stats = nullptr; o2.kd = &kd2; }
    if (o.dro) { dro2 = *o.dro; dro2.frozen = 1; dro2.stats = nullptr; o2.dro = &dro2; }      // q moved once, in pass 1
    if (o.sc) { sc2 = *o.sc; sc2.stats = nullptr; o2.sc = &sc2; }                              // the term is stateless: measured once, at w
    fc.fused_step = 0;                      // as this call received it: the second one sets it after its own checks
    return train_step_fc(&b2, fc, lrs, steps, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, step, st, o2);
  }
  // few windows: the head's forward, CrossEntropy and backward are one launch (head.hip head_step_kernel), its loss sums ride in the last one
  // distillation (include/msig_kd.h) needs WS_LOGITS and WS_DLOGITS complete between the criterion and the head's backward: unfused
  // a sharpness-aware step's second pass restores MSIG_WS_LOSS before the last launch, where head_step would finalise its sums: unfused
  // group-DRO (include/msig_dro.h) rescales WS_DLOGITS between the criterion and the distillation term: unfused
  const bool head_step = !o.kd && !o.sam && !o.dro && head_step_applies(b, c.d);
  // the pass, then ONE launch that reduces every weight-gradient partial and applies Adam to each reduced element
  // (plus the few gradients their kernels write in place): the arithmetic of msig_backward + msig_adam_step
  ColsumPlan plan;
  if ((rc = step_pass(b, c, fc, st, o, head_step, plan))) return rc;
  // second pass of a sharpness-aware step: back to w (and to pass 1's BatchNorm state and losses) before Adam reads the parameters
  if (o.sam && (rc = launch_sam_restore(*o.sam, (float*)b->params, b->bn_state, b->bn_count, c.w.p<float>(MSIG_WS_LOSS), c.d.B, fc, st))) return rc;
  const int in_place[6] = {MSIG_P_GATE_W1, MSIG_P_GATE_W2, MSIG_P_BN1_G, MSIG_P_BN1_B, MSIG_P_BN2_G, MSIG_P_BN2_B};
  for (int i = 0; i < 6; ++i) {
    const int t = in_place[i];
    if (!plan.add_in_place(b->grads + c.po[t], (int)(c.po[t + 1] - c.po[t]))) return MSIG_E_SHAPE;
  }
  for (int i = 0; i < fc.n; ++i) {         // bias corrections per fold: folds of a batch may be at different step counts (msig_multi.step)
    const double s_i = (double)((steps && steps[i] > 0) ? steps[i] : step);
    const double bc1 = 1.0 - pow((double)beta1, s_i), bc2 = 1.0 - pow((double)beta2, s_i);
    fc.lr_over_bc1[i] = (float)((double)lrs[i] / bc1);
    fc.inv_sqrt_bc2[i] = (float)(1.0 / sqrt(bc2));
  }
  const AdamArgs ad{(float*)b->params, b->grads, exp_avg, exp_avg_sq, fc.lr_over_bc1[0], fc.inv_sqrt_bc2[0], beta1, beta2, eps, weight_decay};
  // clip: the norm of the whole gradient has to be known between the reduction and the update — two launches (include/msig_gc.h)
  return o.clip ? launch_colsum_clip_adam_plan(plan, ad, fc, *o.clip, st) : launch_colsum_adam_plan(plan, ad, fc, st);
}

extern "C" int msig_train_step(const msig_batch* b, float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2,
                               float eps, float weight_decay, int64_t step, void* stream) {
  return train_step_fc(b, single_fold(b), &lr, nullptr, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, step, (hipStream_t)stream, StepOpts{});
}

// ---- fold batching -------------------------------------------------------------------------------------------------
static int make_fold_ctx(const msig_batch* b, const msig_multi* m, FoldCtx& fc) {
  if (!b || !m) return MSIG_E_NULL;
  if (m->n < 1 || m->n > MSIG_MAX_FOLDS) return MSIG_E_SHAPE;
  if (m->stride_bytes <= 0 || (m->stride_bytes & 255)) return MSIG_E_ALIGN;
  if (m->form_folds < 0 || m->form_folds > MSIG_MAX_FOLDS) return MSIG_E_SHAPE;
  fc = FoldCtx{};
  fc.n = m->n; fc.stride = m->stride_bytes; fc.form_folds = m->form_folds ? m->form_folds : m->n;
  for (int i = 0; i < m->n; ++i) {
    if (m->slot[i] < 0) return MSIG_E_SHAPE;
    for (int j = 0; j < i; ++j) if (m->slot[j] == m->slot[i]) return MSIG_E_SHAPE;        // two launches into one arena would race
    fc.slot[i] = m->slot[i]; fc.key_gru[i] = m->key_gru[i]; fc.key_head[i] = m->key_head[i];
  }
  return 0;
}
// msig_multi's own checks for a call that has no msig_batch (augment.hip)
int msig_multi_fold_ctx(const msig_multi* m, FoldCtx& fc) {
  msig_batch dummy{};
  return make_fold_ctx(&dummy, m, fc);
}
extern "C" int msig_forward_multi(const msig_batch* b, const msig_multi* m, void* stream) {
  FoldCtx fc; int rc = make_fold_ctx(b, m, fc); if (rc) return rc;
  return forward_fc(b, fc, (hipStream_t)stream, StepOpts{});
}
extern "C" int msig_train_step_multi(const msig_batch* b, const msig_multi* m, float* exp_avg, float* exp_avg_sq, float beta1, float beta2,
                                     float eps, float weight_decay, int64_t step, void* stream) {
  FoldCtx fc; int rc = make_fold_ctx(b, m, fc); if (rc) return rc;
  return train_step_fc(b, fc, m->lr, m->step, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, step, (hipStream_t)stream, StepOpts{});
}

// ---- class-weighted CrossEntropy (include/msig_cw.h): the same calls with the weight vector passed down to the loss kernels ----
extern "C" int msig_cw_abi_version(void) { return MSIG_CW_ABI_VERSION; }

extern "C" int msig_cw_forward(const msig_batch* b, const float* class_weight, void* stream) {
  if (msig_misaligned(class_weight, 3)) return MSIG_E_ALIGN;
  return forward_fc(b, single_fold(b), (hipStream_t)stream, StepOpts{class_weight});
}
extern "C" int msig_cw_train_step(const msig_batch* b, const float* class_weight, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                                  float beta2, float eps, float weight_decay, int64_t step, void* stream) {
  if (msig_misaligned(class_weight, 3)) return MSIG_E_ALIGN;
  return train_step_fc(b, single_fold(b), &lr, nullptr, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, step, (hipStream_t)stream,
                       StepOpts{class_weight});
}
extern "C" int msig_cw_forward_multi(const msig_batch* b, const msig_multi* m, const float* class_weight, void* stream) {
  if (msig_misaligned(class_weight, 3)) return MSIG_E_ALIGN;
  FoldCtx fc; int rc = make_fold_ctx(b, m, fc); if (rc) return rc;
  return forward_fc(b, fc, (hipStream_t)stream, StepOpts{class_weight});
}
extern "C" int msig_cw_train_step_multi(const msig_batch* b, const msig_multi* m, const float* class_weight, float* exp_avg, float* exp_avg_sq,
                                        float beta1, float beta2, float eps, float weight_decay, int64_t step, void* stream) {
  if (msig_misaligned(class_weight, 3)) return MSIG_E_ALIGN;
  FoldCtx fc; int rc = make_fold_ctx(b, m, fc); if (rc) return rc;
  return train_step_fc(b, fc, m->lr, m->step, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, step, (hipStream_t)stream, StepOpts{class_weight});
}

// ---- CnnGruModel, the baseline without ChannelAttention (include/msig_cg.h): the same steps on the gate-free front end ----------
extern "C" int msig_cg_abi_version(void) { return MSIG_CG_ABI_VERSION; }
extern "C" int msig_cg_param_layout(int C, int K, int64_t* off) { return param_layout(C, K, off, false); }

extern "C" int msig_cg_forward(const msig_batch* b, const float* class_weight, void* stream) {
  if (msig_misaligned(class_weight, 3)) return MSIG_E_ALIGN;
  return forward_fc(b, single_fold(b), (hipStream_t)stream, StepOpts{class_weight, true});
}
extern "C" int msig_cg_backward(const msig_batch* b, const float* dlogits, void* stream) {
  return backward_fc(b, dlogits, single_fold(b), (hipStream_t)stream, StepOpts{nullptr, true});
}
extern "C" int msig_cg_train_step(const msig_batch* b, const float* class_weight, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                                  float beta2, float eps, float weight_decay, int64_t step, void* stream) {
  if (msig_misaligned(class_weight, 3)) return MSIG_E_ALIGN;
  return train_step_fc(b, single_fold(b), &lr, nullptr, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, step, (hipStream_t)stream,
                       StepOpts{class_weight, true});
}
extern "C" int msig_cg_forward_multi(const msig_batch* b, const msig_multi* m, const float* class_weight, void* stream) {
  if (msig_misaligned(class_weight, 3)) return MSIG_E_ALIGN;
  FoldCtx fc; int rc = make_fold_ctx(b, m, fc); if (rc) return rc;
  return forward_fc(b, fc, (hipStream_t)stream, StepOpts{class_weight, true});
}
extern "C" int msig_cg_train_step_multi(const msig_batch* b, const msig_multi* m, const float* class_weight, float* exp_avg, float* exp_avg_sq,
                                        float beta1, float beta2, float eps, float weight_decay, int64_t step, void* stream) {
  if (msig_misaligned(class_weight, 3)) return MSIG_E_ALIGN;
  FoldCtx fc; int rc = make_fold_ctx(b, m, fc); if (rc) return rc;
  return train_step_fc(b, fc, m->lr, m->step, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, step, (hipStream_t)stream,
                       StepOpts{class_weight, true});
}

// ---- gradient-norm clipping (include/msig_gc.h): the train steps with the clip between the reduction and the Adam update ---------
extern "C" int msig_gc_abi_version(void) { return MSIG_GC_ABI_VERSION; }
extern "C" int64_t msig_gc_struct_bytes(void) { return (int64_t)sizeof(msig_gc_clip); }

// Column blocks of a train step's reduction plan, bounded from the layout alone: the plan's jobs cover every parameter element once,
// a job of n columns has ceil(n / 32) blocks, and there are at most MSIG_MAX_JOBS jobs.
static int64_t gc_partials(int C, int K, int kind) {
  int64_t po[MSIG_NPARAM + 1];
  const int rc = param_layout(C, K, po, kind == MSIG_GC_KIND_ATTENTION);
  if (rc) return rc;
  return po[MSIG_NPARAM] / 32 + MSIG_MAX_JOBS;
}
extern "C" int64_t msig_gc_state_bytes(int C, int K, int kind) {
  if (kind != MSIG_GC_KIND_ATTENTION && kind != MSIG_GC_KIND_CNN_GRU) return MSIG_E_SHAPE;
  const int64_t n = gc_partials(C, K, kind);
  return n < 0 ? n : (MSIG_GC_NSTAT + n) * (int64_t)sizeof(double);
}
// every check of msig_gc.h's own arguments, before the counterpart's and before any launch; n = folds of the launch
static int make_clip(const msig_batch* b, const msig_gc_clip* g, int n, ClipArgs& cl) {
  if (!g || !b) return MSIG_E_NULL;
  if (g->kind != MSIG_GC_KIND_ATTENTION && g->kind != MSIG_GC_KIND_CNN_GRU) return MSIG_E_SHAPE;
  for (int i = 0; i < n; ++i)
    if (!(g->max_norm[i] > 0.0)) return MSIG_E_SHAPE;                   // NaN included
  if (!g->state) return MSIG_E_NULL;
  if ((uintptr_t)g->state & 7) return MSIG_E_ALIGN;
  if (msig_misaligned(g->class_weight, 3)) return MSIG_E_ALIGN;
  const int64_t cap = gc_partials(b->shape.C, b->shape.K, g->kind);
  if (cap < 0) return (int)cap;
  if (g->state_bytes < (MSIG_GC_NSTAT + cap) * (int64_t)sizeof(double)) return MSIG_E_WORKSPACE;
  cl = ClipArgs{};
  cl.state = (double*)g->state;
  cl.cap = (int)cap;
  for (int i = 0; i < n; ++i) cl.max_norm[i] = g->max_norm[i];
  return 0;
}
extern "C" int msig_gc_train_step(const msig_batch* b, const msig_gc_clip* g, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                                  float beta2, float eps, float weight_decay, int64_t step, void* stream) {
  ClipArgs cl; int rc = make_clip(b, g, 1, cl); if (rc) return rc;
  return train_step_fc(b, single_fold(b), &lr, nullptr, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, step, (hipStream_t)stream,
                       StepOpts{g->class_weight, g->kind == MSIG_GC_KIND_CNN_GRU, &cl});
}
extern "C" int msig_gc_train_step_multi(const msig_batch* b, const msig_multi* m, const msig_gc_clip* g, float* exp_avg, float* exp_avg_sq,
                                        float beta1, float beta2, float eps, float weight_decay, int64_t step, void* stream) {
  FoldCtx fc; int rc = make_fold_ctx(b, m, fc); if (rc) return rc;
  ClipArgs cl; if ((rc = make_clip(b, g, fc.n, cl))) return rc;
  return train_step_fc(b, fc, m->lr, m->step, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, step, (hipStream_t)stream,
                       StepOpts{g->class_weight, g->kind == MSIG_GC_KIND_CNN_GRU, &cl});
}

// ---- soft targets (include/msig_st.h): label smoothing and mixup in the criterion of the same calls ------------------------------
extern "C" int msig_st_abi_version(void) { return MSIG_ST_ABI_VERSION; }
extern "C" int64_t msig_st_struct_bytes(void) { return (int64_t)sizeof(msig_st); }

// every check of msig_st.h's own arguments, before the counterpart's and before any launch; n = folds of the launch.  use = false:
// smoothing 0 and every lam 1 — the call is its counterpart (soft stays unused: the same launches).
static int make_soft(const msig_st* s, int n, SoftArgs& soft, bool& use) {
  if (!s) return MSIG_E_NULL;
  if (s->kind != MSIG_GC_KIND_ATTENTION && s->kind != MSIG_GC_KIND_CNN_GRU) return MSIG_E_SHAPE;
  if (!(s->smoothing >= 0.f && s->smoothing < 1.f)) return MSIG_E_SHAPE;                 // NaN included
  soft = SoftArgs{};
  soft.eps = s->smoothing;
  use = s->smoothing != 0.f;
  for (int i = 0; i < n; ++i) {
    if (!(s->lam[i] >= 0.f && s->lam[i] <= 1.f)) return MSIG_E_SHAPE;
    soft.lam[i] = s->lam[i];
    use = use || s->lam[i] != 1.f;
  }
  for (int i = n; i < MSIG_MAX_FOLDS; ++i) soft.lam[i] = 1.f;
  if (msig_misaligned(s->class_weight, 3)) return MSIG_E_ALIGN;
  return 0;
}
static int st_forward(const msig_batch* b, const FoldCtx& fc, const msig_st* s, hipStream_t st) {
  SoftArgs soft; bool use; int rc = make_soft(s, fc.n, soft, use); if (rc) return rc;
  return forward_fc(b, fc, st, StepOpts{s->class_weight, s->kind == MSIG_GC_KIND_CNN_GRU, nullptr, use ? &soft : nullptr});
}
static int make_da(const msig_da* a, const FoldCtx& fc, int32_t B, const float* lam, DaArgs& da);
int msig_sc_check_align(const msig_sc* k, const FoldCtx& fc, int32_t B);      // supcon.hip: what follows msig_sc_make_args and the lam check
// The optional terms of a train step as an entry point received them; a NULL member is the step without that term, StepTerms{} is
// msig_st_train_step[_multi] itself.  A narrower entry point leaves the members it has no parameter for NULL.
struct StepTerms {
  const msig_da* da;        // subject discriminator (include/msig_da.h)
  const msig_kd* kd;        // distillation (include/msig_kd.h); alpha == 0 after its checks = the step without it
  const msig_sam* sam;      // sharpness-aware step (include/msig_sam.h); rho == 0 after its checks = the step without it
  const msig_dro* dro;      // group-DRO (include/msig_dro.h)
  const msig_sc* sc;        // supervised contrastive term (include/msig_sc.h)
};
// Every msig_{st,da,kd,sam,dro,sc}_train_step[_multi] after its own first checks: the terms' checks in the headers' order, then train_step_fc.
static int st_train_step(const msig_batch* b, const FoldCtx& fc, const msig_st* s, const StepTerms& t, const float* lrs, const int64_t* steps,
                         float* exp_avg, float* exp_avg_sq, float beta1, float beta2, float eps, float weight_decay, int64_t step, hipStream_t st) {
  if (t.da && t.sam) return MSIG_E_SHAPE;      // two passes would advance the discriminator's own Adam twice
  const msig_da* a = t.da; const msig_kd* k = t.kd; const msig_sam* sm = t.sam; const msig_dro* dr = t.dro; const msig_sc* sk = t.sc;
  if ((sm || dr || sk) && (!s || !b)) return MSIG_E_NULL;
  SamArgs sam;                             // include/msig_sam.h: its own checks first; rho == 0 after them = the call without it
  int rc;
  if (sm) {
    if ((rc = msig_sam_make_args(sm, b->shape.C, b->shape.K, sam))) return rc;
    if (sm->kind != s->kind) return MSIG_E_SHAPE;
    if (sm->rho == 0.f) sm = nullptr;
  }
  SoftArgs soft; bool use; if ((rc = make_soft(s, fc.n, soft, use))) return rc;
  if (!b) return MSIG_E_NULL;
  DaArgs da;
  if (a && (rc = make_da(a, fc, b->shape.B, soft.lam, da))) return rc;
  KdArgs kd;
  if (k && (rc = msig_kd_make_args(k, fc, b->shape.B, b->shape.K, soft.lam, kd))) return rc;
  const bool distil = k && k->alpha != 0.f;
  DroArgs dro;                             // include/msig_dro.h: a blended row has no group
  if (dr) {
    if ((rc = msig_dro_make_args(dr, fc, b->shape.B, b->shape.K, soft.eps, dro))) return rc;
    for (int i = 0; i < fc.n; ++i) if (soft.lam[i] != 1.f) return MSIG_E_SHAPE;
  }
  ScArgs sc;                               // include/msig_sc.h: a blended row has no label to contrast
  if (sk) {
    if ((rc = msig_sc_make_args(sk, fc, b->shape.B, b->shape.K, sc))) return rc;
    for (int i = 0; i < fc.n; ++i) if (soft.lam[i] != 1.f) return MSIG_E_SHAPE;
    if ((rc = msig_sc_check_align(sk, fc, b->shape.B))) return rc;
  }
  ClipArgs cl;
  if (s->clip) {
    if (s->clip->kind != s->kind) return MSIG_E_SHAPE;
    if ((rc = make_clip(b, s->clip, fc.n, cl))) return rc;
  }
  return train_step_fc(b, fc, lrs, steps, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, step, st,
                       StepOpts{s->class_weight, s->kind == MSIG_GC_KIND_CNN_GRU, s->clip ? &cl : nullptr, use ? &soft : nullptr, a ? &da : nullptr,
                                distil ? &kd : nullptr, sm ? &sam : nullptr, dr ? &dro : nullptr, sk ? &sc : nullptr});
}
extern "C" int msig_st_forward(const msig_batch* b, const msig_st* s, void* stream) {
  return st_forward(b, single_fold(b), s, (hipStream_t)stream);
}
extern "C" int msig_st_forward_multi(const msig_batch* b, const msig_multi* m, const msig_st* s, void* stream) {
  if (!s) return MSIG_E_NULL;
  FoldCtx fc; int rc = make_fold_ctx(b, m, fc); if (rc) return rc;
  return st_forward(b, fc, s, (hipStream_t)stream);
}
extern "C" int msig_st_train_step(const msig_batch* b, const msig_st* s, float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2,
                                  float eps, float weight_decay, int64_t step, void* stream) {
  return st_train_step(b, single_fold(b), s, StepTerms{}, &lr, nullptr, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, step, (hipStream_t)stream);
}
// the *_multi forms share their first checks: msig_st, then msig_multi's own
static int st_train_step_multi(const msig_batch* b, const msig_multi* m, const msig_st* s, const StepTerms& t, float* exp_avg, float* exp_avg_sq,
                               float beta1, float beta2, float eps, float weight_decay, int64_t step, void* stream) {
  if (!s) return MSIG_E_NULL;
  FoldCtx fc; int rc = make_fold_ctx(b, m, fc); if (rc) return rc;
  return st_train_step(b, fc, s, t, m->lr, m->step, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, step, (hipStream_t)stream);
}
extern "C" int msig_st_train_step_multi(const msig_batch* b, const msig_multi* m, const msig_st* s, float* exp_avg, float* exp_avg_sq,
                                        float beta1, float beta2, float eps, float weight_decay, int64_t step, void* stream) {
  return st_train_step_multi(b, m, s, StepTerms{}, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, step, stream);
}

// ---- subject-adversarial training (include/msig_da.h; kernel: adversary.hip) ---------------------------------------------------------
extern "C" int msig_da_abi_version(void) { return MSIG_DA_ABI_VERSION; }
extern "C" int64_t msig_da_struct_bytes(void) { return (int64_t)sizeof(msig_da); }
extern "C" int64_t msig_da_param_floats(int32_t S) {
  if (S < 2 || S > MSIG_MAX_K) return MSIG_E_SHAPE;
  return 64 * 128 + 64 + ((int64_t)S * 64 + 3) / 4 * 4 + (S + 3) / 4 * 4;
}
// every check of msig_da.h's own arguments, before any launch; fc: the folds of the launch (stride != 0: a fold batch); lam per fold
static int make_da(const msig_da* a, const FoldCtx& fc, int32_t B, const float* lam, DaArgs& da) {
  if (!a || !lam) return MSIG_E_NULL;
  if (!a->dom || !a->params || !a->exp_avg || !a->exp_avg_sq) return MSIG_E_NULL;
  if (a->S < 2 || a->S > MSIG_MAX_K || B < 1 || B > MSIG_DA_MAX_BATCH) return MSIG_E_SHAPE;
  const bool multi = fc.stride != 0;
  if (multi && a->idx && a->idx_row_stride < B) return MSIG_E_SHAPE;
  da = DaArgs{};
  for (int i = 0; i < fc.n; ++i) {
    if (a->step[i] < 1) return MSIG_E_SHAPE;
    if (!(a->lambda[i] >= 0.f) || !(a->lr[i] >= 0.f) || !(lam[i] >= 0.f && lam[i] <= 1.f)) return MSIG_E_SHAPE;      // NaN included
    const double bc1 = 1.0 - pow((double)a->beta1, (double)a->step[i]), bc2 = 1.0 - pow((double)a->beta2, (double)a->step[i]);
    da.lambda[i] = a->lambda[i]; da.lam[i] = lam[i];
    da.lr_over_bc1[i] = (float)((double)a->lr[i] / bc1);
    da.inv_sqrt_bc2[i] = (float)(1.0 / sqrt(bc2));
  }
  if (((uintptr_t)a->params | (uintptr_t)a->exp_avg | (uintptr_t)a->exp_avg_sq) & 15) return MSIG_E_ALIGN;
  if (((uintptr_t)a->stats | (uintptr_t)a->idx) & 7) return MSIG_E_ALIGN;
  if ((uintptr_t)a->dom & 3) return MSIG_E_ALIGN;
  if (multi && (a->stride_bytes <= 0 || (a->stride_bytes & 255))) return MSIG_E_ALIGN;
  da.S = a->S; da.B = B;
  da.dom = a->dom; da.idx = a->idx; da.idx_row_stride = multi ? a->idx_row_stride : 0;
  da.params = a->params; da.exp_avg = a->exp_avg; da.exp_avg_sq = a->exp_avg_sq; da.stats = a->stats;
  da.stride = multi ? a->stride_bytes : 0;
  da.b1 = a->beta1; da.b2 = a->beta2; da.eps = a->eps; da.wd = a->weight_decay;
  return 0;
}
static int da_step(const msig_da* a, const FoldCtx& fc, const float* feat, float* dfeat, int32_t B, const float* lam, hipStream_t st) {
  if (!feat || !dfeat) return MSIG_E_NULL;
  DaArgs da; int rc = make_da(a, fc, B, lam, da); if (rc) return rc;
  if (((uintptr_t)feat | (uintptr_t)dfeat) & 15) return MSIG_E_ALIGN;
  return launch_da_step(da, feat, dfeat, fc, st);
}
extern "C" int msig_da_step(const msig_da* a, const float* feat, float* dfeat, int32_t B, float lam, void* stream) {
  return da_step(a, single_fold(nullptr), feat, dfeat, B, &lam, (hipStream_t)stream);
}
extern "C" int msig_da_step_multi(const msig_da* a, const msig_multi* m, const float* feat, float* dfeat, int32_t B, const float* lam,
                                  void* stream) {
  if (!a || !m) return MSIG_E_NULL;
  FoldCtx fc; int rc = msig_multi_fold_ctx(m, fc); if (rc) return rc;
  return da_step(a, fc, feat, dfeat, B, lam, (hipStream_t)stream);
}
extern "C" int msig_da_train_step(const msig_batch* b, const msig_st* s, const msig_da* a, float* exp_avg, float* exp_avg_sq, float lr,
                                  float beta1, float beta2, float eps, float weight_decay, int64_t step, void* stream) {
  return st_train_step(b, single_fold(b), s, StepTerms{a}, &lr, nullptr, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, step, (hipStream_t)stream);
}
extern "C" int msig_da_train_step_multi(const msig_batch* b, const msig_multi* m, const msig_st* s, const msig_da* a, float* exp_avg,
                                        float* exp_avg_sq, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                                        void* stream) {
  return st_train_step_multi(b, m, s, StepTerms{a}, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, step, stream);
}

// ---- distillation (include/msig_kd.h; kernels and the stand-alone calls: distill.hip) -----------------------------------------------
extern "C" int msig_kd_train_step(const msig_batch* b, const msig_st* s, const msig_da* da, const msig_kd* kd, float* exp_avg,
                                  float* exp_avg_sq, float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                                  void* stream) {
  return st_train_step(b, single_fold(b), s, StepTerms{da, kd}, &lr, nullptr, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, step,
                       (hipStream_t)stream);
}
extern "C" int msig_kd_train_step_multi(const msig_batch* b, const msig_multi* m, const msig_st* s, const msig_da* da, const msig_kd* kd,
                                        float* exp_avg, float* exp_avg_sq, float beta1, float beta2, float eps, float weight_decay,
                                        int64_t step, void* stream) {
  return st_train_step_multi(b, m, s, StepTerms{da, kd}, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, step, stream);
}

// ---- sharpness-aware minimisation (include/msig_sam.h; kernels and the stand-alone calls: sam.hip) --------------------------------
extern "C" int msig_sam_train_step(const msig_batch* b, const msig_st* s, const msig_kd* kd, const msig_sam* sam, float* exp_avg,
                                   float* exp_avg_sq, float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                                   void* stream) {
  return st_train_step(b, single_fold(b), s, StepTerms{nullptr, kd, sam}, &lr, nullptr, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, step,
                       (hipStream_t)stream);
}
extern "C" int msig_sam_train_step_multi(const msig_batch* b, const msig_multi* m, const msig_st* s, const msig_kd* kd, const msig_sam* sam,
                                         float* exp_avg, float* exp_avg_sq, float beta1, float beta2, float eps, float weight_decay,
                                         int64_t step, void* stream) {
  return st_train_step_multi(b, m, s, StepTerms{nullptr, kd, sam}, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, step, stream);
}

// ---- group-DRO (include/msig_dro.h; kernel and the stand-alone calls: dro.hip) -------------------------------------------------------
extern "C" int msig_dro_train_step(const msig_batch* b, const msig_st* s, const msig_da* da, const msig_kd* kd, const msig_sam* sam,
                                   const msig_dro* dro, float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2, float eps,
                                   float weight_decay, int64_t step, void* stream) {
  return st_train_step(b, single_fold(b), s, StepTerms{da, kd, sam, dro}, &lr, nullptr, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, step,
                       (hipStream_t)stream);
}
extern "C" int msig_dro_train_step_multi(const msig_batch* b, const msig_multi* m, const msig_st* s, const msig_da* da, const msig_kd* kd,
                                         const msig_sam* sam, const msig_dro* dro, float* exp_avg, float* exp_avg_sq, float beta1,
                                         float beta2, float eps, float weight_decay, int64_t step, void* stream) {
  return st_train_step_multi(b, m, s, StepTerms{da, kd, sam, dro}, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, step, stream);
}

// ---- supervised contrastive term (include/msig_sc.h; kernels and the stand-alone calls: supcon.hip) ---------------------------------
extern "C" int msig_sc_train_step(const msig_batch* b, const msig_st* s, const msig_da* da, const msig_kd* kd, const msig_sam* sam,
                                  const msig_dro* dro, const msig_sc* sc, float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2,
                                  float eps, float weight_decay, int64_t step, void* stream) {
  return st_train_step(b, single_fold(b), s, StepTerms{da, kd, sam, dro, sc}, &lr, nullptr, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, step,
                       (hipStream_t)stream);
}
extern "C" int msig_sc_train_step_multi(const msig_batch* b, const msig_multi* m, const msig_st* s, const msig_da* da, const msig_kd* kd,
                                        const msig_sam* sam, const msig_dro* dro, const msig_sc* sc, float* exp_avg, float* exp_avg_sq,
                                        float beta1, float beta2, float eps, float weight_decay, int64_t step, void* stream) {
  return st_train_step_multi(b, m, s, StepTerms{da, kd, sam, dro, sc}, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, step, stream);
}

// ---- window embeddings and classifier-only training (include/msig_ft.h) ---------------------------------------------------------
extern "C" int msig_ft_abi_version(void) { return MSIG_FT_ABI_VERSION; }
extern "C" int64_t msig_ft_struct_bytes(int32_t which) {
  return which == 0 ? (int64_t)sizeof(msig_ft_head) : which == 1 ? (int64_t)sizeof(msig_ft_multi) : -1;
}

// the front end and the GRU of an eval-mode forward, no head launch, then MSIG_WS_FEAT of every fold copied out
static int features_fc(const msig_batch* b, const FoldCtx& fc, int kind, float* out, int64_t out_stride_bytes, hipStream_t st) {
  if (!out) return MSIG_E_NULL;
  if (kind != MSIG_FT_KIND_ATTENTION && kind != MSIG_FT_KIND_CNN_GRU) return MSIG_E_SHAPE;
  if (b->training) return MSIG_E_SHAPE;
  if ((uintptr_t)out & 15) return MSIG_E_ALIGN;
  if (fc.n > 1 && (out_stride_bytes < (int64_t)b->shape.B * 512 || (out_stride_bytes & 15))) return MSIG_E_SHAPE;
  const bool cg = kind == MSIG_FT_KIND_CNN_GRU;
  int rc = forward_fc(b, fc, st, StepOpts{nullptr, cg}, false);         // every argument check of the forward before its first launch
  if (rc) return rc;
  Ctx c;
  if ((rc = make_ctx(b, c, false, cg))) return rc;
  return launch_ft_feat_copy(c.w.p<float>(MSIG_WS_FEAT), out, out_stride_bytes, c.d.B, fc, st);
}
extern "C" int msig_ft_features(const msig_batch* b, int kind, float* out, void* stream) {
  if (!b) return MSIG_E_NULL;
  return features_fc(b, single_fold(b), kind, out, 0, (hipStream_t)stream);
}
extern "C" int msig_ft_features_multi(const msig_batch* b, const msig_multi* m, int kind, float* out, int64_t out_stride_bytes, void* stream) {
  FoldCtx fc; int rc = make_fold_ctx(b, m, fc); if (rc) return rc;
  return features_fc(b, fc, kind, out, out_stride_bytes, (hipStream_t)stream);
}

static int check_ft_head(const msig_ft_head* h) {
  if (!h) return MSIG_E_NULL;
  if (!h->feat || !h->labels || !h->order || !h->params || !h->exp_avg || !h->exp_avg_sq) return MSIG_E_NULL;
  if (h->K < 2 || h->K > MSIG_MAX_K || h->batch < 1 || h->batch > MSIG_FT_MAX_BATCH) return MSIG_E_SHAPE;
  if (h->N < 1 || h->N > MSIG_FT_MAX_N || h->n_order < 1 || h->n_order > h->N) return MSIG_E_SHAPE;
  if (h->first_step < 0 || h->n_steps < 1) return MSIG_E_SHAPE;
  if ((int64_t)h->first_step + h->n_steps > ((int64_t)h->n_order + h->batch - 1) / h->batch) return MSIG_E_SHAPE;
  if (h->dropout_thr < 0 || h->dropout_thr > 256) return MSIG_E_SHAPE;
  if (h->cls_offset < 0 || (h->cls_offset & 3)) return MSIG_E_SHAPE;
  if (((uintptr_t)h->feat | (uintptr_t)h->params | (uintptr_t)h->exp_avg | (uintptr_t)h->exp_avg_sq) & 15) return MSIG_E_ALIGN;
  if (((uintptr_t)h->labels | (uintptr_t)h->loss_acc) & 7) return MSIG_E_ALIGN;
  if (((uintptr_t)h->order | (uintptr_t)h->class_weight) & 3) return MSIG_E_ALIGN;
  return 0;
}
extern "C" int msig_ft_head_epoch(const msig_ft_head* h, void* stream) {
  int rc = check_ft_head(h); if (rc) return rc;
  if (h->step0 < 1) return MSIG_E_SHAPE;
  FtFolds ff{};
  ff.n = 1; ff.lr[0] = h->lr; ff.step0[0] = h->step0; ff.seed[0] = h->seed;
  return launch_head_epoch(*h, ff, (hipStream_t)stream);
}
extern "C" int msig_ft_head_epoch_multi(const msig_ft_head* h, const msig_ft_multi* m, void* stream) {
  if (!m) return MSIG_E_NULL;
  int rc = check_ft_head(h); if (rc) return rc;
  if (m->n < 1 || m->n > MSIG_MAX_FOLDS) return MSIG_E_SHAPE;
  if (m->stride_bytes <= 0 || (m->stride_bytes & 255)) return MSIG_E_ALIGN;
  FtFolds ff{};
  ff.n = m->n; ff.stride = m->stride_bytes;
  for (int i = 0; i < m->n; ++i) {
    if (m->slot[i] < 0 || m->step0[i] < 1) return MSIG_E_SHAPE;
    for (int j = 0; j < i; ++j) if (m->slot[j] == m->slot[i]) return MSIG_E_SHAPE;        // two workgroups in one arena would race
    ff.slot[i] = m->slot[i]; ff.lr[i] = m->lr[i]; ff.step0[i] = m->step0[i]; ff.seed[i] = m->seed[i];
  }
  return launch_head_epoch(*h, ff, (hipStream_t)stream);
}

// ---- label-free BatchNorm adaptation (include/msig_ab.h; kernels: adapt_bn.hip) ---------------------------------------------------
extern "C" int msig_ab_abi_version(void) { return MSIG_AB_ABI_VERSION; }

// one batch into stage `stage` of every fold's accumulator: the front end up to that stage's convolution with its partial sums on
// (launch_frontend_fwd's stats_stage), then the merge.  Every argument check before the first launch.
static int ab_accumulate_fc(const msig_batch* b, const FoldCtx& fc, int kind, int stage, double* acc, hipStream_t st) {
  if (!b || !acc) return MSIG_E_NULL;
  if (kind != MSIG_FT_KIND_ATTENTION && kind != MSIG_FT_KIND_CNN_GRU) return MSIG_E_SHAPE;
  if (stage != 1 && stage != 2) return MSIG_E_SHAPE;
  if (b->training) return MSIG_E_SHAPE;
  if ((uintptr_t)acc & 7) return MSIG_E_ALIGN;
  const bool cg = kind == MSIG_FT_KIND_CNN_GRU;
  Ctx c; int rc = make_ctx(b, c, false, cg); if (rc) return rc;
  int rows = 0;
  if ((rc = launch_frontend_fwd(b, c.d, c.w, c.po, fc, st, !cg, stage, &rows))) return rc;
  const bool s1 = stage == 1;
  return launch_ab_merge(c.w.p<float>(s1 ? MSIG_WS_BN1_PART : MSIG_WS_BN2_PART), rows, stage, (double)c.d.B * (s1 ? c.d.L1 : c.d.L2), acc, fc, st);
}
extern "C" int msig_ab_accumulate(const msig_batch* b, int kind, int stage, double* acc, void* stream) {
  if (!b) return MSIG_E_NULL;
  return ab_accumulate_fc(b, single_fold(b), kind, stage, acc, (hipStream_t)stream);
}
extern "C" int msig_ab_accumulate_multi(const msig_batch* b, const msig_multi* m, int kind, int stage, double* acc, void* stream) {
  FoldCtx fc; int rc = make_fold_ctx(b, m, fc); if (rc) return rc;
  return ab_accumulate_fc(b, fc, kind, stage, acc, (hipStream_t)stream);
}

static int ab_commit_fc(const double* acc, int stage, float alpha, const float* bn_src, float* bn_dst, const FoldCtx& fc, hipStream_t st) {
  if (!acc || !bn_src || !bn_dst) return MSIG_E_NULL;
  if (stage != 1 && stage != 2) return MSIG_E_SHAPE;
  if (!(alpha >= 0.0f && alpha <= 1.0f)) return MSIG_E_SHAPE;          // NaN fails both comparisons
  if ((uintptr_t)acc & 7) return MSIG_E_ALIGN;
  if (((uintptr_t)bn_src | (uintptr_t)bn_dst) & 3) return MSIG_E_ALIGN;
  return launch_ab_commit(acc, stage, alpha, bn_src, bn_dst, fc, st);
}
extern "C" int msig_ab_commit(const double* acc, int stage, float alpha, const float* bn_src, float* bn_dst, void* stream) {
  return ab_commit_fc(acc, stage, alpha, bn_src, bn_dst, single_fold(nullptr), (hipStream_t)stream);
}
extern "C" int msig_ab_commit_multi(const double* acc, int stage, float alpha, const float* bn_src, float* bn_dst, const msig_multi* m, void* stream) {
  FoldCtx fc; int rc = msig_multi_fold_ctx(m, fc); if (rc) return rc;
  return ab_commit_fc(acc, stage, alpha, bn_src, bn_dst, fc, (hipStream_t)stream);
}

// ---- entropy-minimisation adaptation (include/msig_tt.h; kernels and the stand-alone calls: tta.hip) ------------------------------
// One step: the eval forward kept for a backward, the objective's launch on WS_LOGITS -> WS_DLOGITS, msig_backward's arithmetic over
// the folds of the launch, the selective Adam.  Every argument check, in the header's order, before the first launch.
static int tt_step_fc(const msig_batch* b, FoldCtx fc, const msig_tt* t, const float* lrs, const int64_t* steps, int64_t step, hipStream_t st) {
  if (!b || !t) return MSIG_E_NULL;
  if (b->training || !b->keep_for_backward || b->dx) return MSIG_E_SHAPE;
  TtSel sel;
  int rc = msig_tt_make_sel(b->shape.C, b->shape.K, t->kind, t->select, sel); if (rc) return rc;
  if (msig_tt_bad_diversity(t->diversity) || b->shape.B > MSIG_TT_MAX_BATCH) return MSIG_E_SHAPE;
  if (!t->exp_avg || !t->exp_avg_sq) return MSIG_E_NULL;
  if (step < 1) return MSIG_E_SHAPE;
  if (steps)
    for (int i = 0; i < fc.n; ++i) if (steps[i] < 0) return MSIG_E_SHAPE;
  if (((uintptr_t)t->exp_avg | (uintptr_t)t->exp_avg_sq) & 15) return MSIG_E_ALIGN;
  if ((uintptr_t)t->stats & 7) return MSIG_E_ALIGN;
  const StepOpts o{nullptr, t->kind == MSIG_FT_KIND_CNN_GRU};
  Ctx c;
  if ((rc = make_ctx(b, c, true, o.cg))) return rc;
  if ((rc = msig_check_call_forms(b, c.d.NT, fc))) return rc;
  if ((rc = forward_fc(b, fc, st, o))) return rc;
  if ((rc = launch_tt_objective(c.w.p<float>(MSIG_WS_LOGITS), c.w.p<float>(MSIG_WS_DLOGITS), t->stats, c.d.B, c.d.K, t->diversity, fc, st))) return rc;
  if ((rc = backward_fc(b, nullptr, fc, st, o))) return rc;
  msig_tt_fill_adam(fc, lrs, steps, step, t->beta1, t->beta2);
  return launch_tt_adam((float*)b->params, b->grads, t->exp_avg, t->exp_avg_sq, sel, t->beta1, t->beta2, t->eps, t->weight_decay, fc, st);
}
extern "C" int msig_tt_step(const msig_batch* b, const msig_tt* t, float lr, int64_t step, void* stream) {
  return tt_step_fc(b, single_fold(b), t, &lr, nullptr, step, (hipStream_t)stream);
}
extern "C" int msig_tt_step_multi(const msig_batch* b, const msig_multi* m, const msig_tt* t, int64_t step, void* stream) {
  if (!b || !m || !t) return MSIG_E_NULL;
  FoldCtx fc; int rc = make_fold_ctx(b, m, fc); if (rc) return rc;
  return tt_step_fc(b, fc, t, m->lr, m->step, step, (hipStream_t)stream);
}

// ---- Monte-Carlo dropout (include/msig_mc.h; kernels of its own: mc.hip) ------------------------------------------------------------
// An eval forward cut at the first dropout site.  Both halves are launch orders of the forward's own kernels (launch_gru_fwd's
// `part`, launch_head_fwd's `mc_tail`); every argument check before the first launch.
static int mc_check(const msig_batch* b, int32_t kind) {
  if (!b) return MSIG_E_NULL;
  if (kind != MSIG_MC_KIND_ATTENTION && kind != MSIG_MC_KIND_CNN_GRU) return MSIG_E_SHAPE;
  if (b->training || b->keep_for_backward || b->dx) return MSIG_E_SHAPE;
  return 0;
}
extern "C" int msig_mc_trunk(const msig_batch* b, int32_t kind, void* stream) {
  int rc = mc_check(b, kind); if (rc) return rc;
  const bool cg = kind == MSIG_MC_KIND_CNN_GRU;
  const FoldCtx fc = single_fold(b);
  hipStream_t st = (hipStream_t)stream;
  Ctx c; if ((rc = make_ctx(b, c, false, cg))) return rc;
  if ((rc = msig_check_call_forms(b, c.d.NT, fc))) return rc;
  if ((rc = launch_frontend_fwd(b, c.d, c.w, c.po, fc, st, !cg))) return rc;
  return launch_gru_fwd(b, c.d, c.w, c.po, fc, st, GRU_PART_L0);
}
extern "C" int msig_mc_tail(const msig_batch* b, int32_t kind, void* stream) {
  int rc = mc_check(b, kind); if (rc) return rc;
  if ((rc = check_shape(&b->shape))) return rc;
  if ((int64_t)b->shape.B * make_dims(b->shape).TP * 128 > (int64_t)1 << 31) return MSIG_E_SHAPE;      // the mask index is 32-bit
  msig_batch t = *b;
  if (!t.x) t.x = t.params;                  // the tail reads no input: x may be NULL (params: any checked pointer, never read as x)
  t.labels = nullptr;
  const bool cg = kind == MSIG_MC_KIND_CNN_GRU;
  const FoldCtx fc = single_fold(&t);
  hipStream_t st = (hipStream_t)stream;
  Ctx c; if ((rc = make_ctx(&t, c, false, cg))) return rc;
  if ((rc = msig_check_call_forms(&t, c.d.NT, fc))) return rc;
  if ((rc = launch_gru_fwd(&t, c.d, c.w, c.po, fc, st, GRU_PART_L1, true))) return rc;
  return launch_head_fwd(&t, c.d, c.w, c.po, fc, st, StepOpts{}, true);
}

extern "C" uint32_t msig_dropout_key(uint64_t seed, uint64_t step, uint32_t stream_id) {
  return dropout_key(seed, step, stream_id);
}

extern "C" int msig_gather_windows(const float* store, const int64_t* store_labels, const int64_t* idx, int32_t B,
                                   int64_t window_floats, float* out_x, int64_t* out_y, void* stream) {
  if (!store || !idx || !out_x) return MSIG_E_NULL;
  if (B < 1 || window_floats < 1) return MSIG_E_SHAPE;
  if (!(window_floats & 3) && (((uintptr_t)store | (uintptr_t)out_x) & 15)) return MSIG_E_ALIGN;      // the float4 copy; any other length goes element by element
  return launch_gather(store, store_labels, idx, B, B, window_floats, out_x, out_y, single_fold(nullptr), (hipStream_t)stream);
}

extern "C" int msig_gather_windows_multi(const float* store, const int64_t* store_labels, const int64_t* idx, int64_t idx_row_stride, int32_t B,
                                         int64_t window_floats, float* out_x, int64_t* out_y, const msig_multi* m, void* stream) {
  if (!store || !idx || !out_x || !m) return MSIG_E_NULL;
  if (B < 1 || idx_row_stride < B || window_floats < 1) return MSIG_E_SHAPE;
  if (!(window_floats & 3) && (((uintptr_t)store | (uintptr_t)out_x) & 15)) return MSIG_E_ALIGN;
  msig_batch dummy{};
  FoldCtx fc; int rc = make_fold_ctx(&dummy, m, fc); if (rc) return rc;
  return launch_gather(store, store_labels, idx, idx_row_stride, B, window_floats, out_x, out_y, fc, (hipStream_t)stream);
}

int launch_channel_attention(const float* x, const float* W1, const float* W2, int B, int C, int T, float* out, float* s, float* scratch,
                             hipStream_t st);
extern "C" int msig_channel_attention(const float* x, const float* w1, const float* w2, int32_t B, int32_t C, int32_t T, float* out, float* s,
                                      float* scratch, void* stream) {
  if (!x || !out || !s || !scratch) return MSIG_E_NULL;
  if (B < 1 || C < 1 || C > MSIG_MAX_C || T < 1) return MSIG_E_SHAPE;
  if (C >= 4 && (!w1 || !w2)) return MSIG_E_NULL;
  return launch_channel_attention(x, w1, w2, B, C, T, out, s, scratch, (hipStream_t)stream);
}
