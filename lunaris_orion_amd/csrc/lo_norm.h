// The GroupNorm(8) + Mish family (private to the library; lo_norm.hip): a call names the layer (LoGnLayer) and what it asks of it
// (LoGnFwd / LoGnBwd), lo_gn_bwd_choose() is the ONE place that decides which backward form runs and how many P1 / P2 rows per
// sample it leaves for lo_gn_finalize_all.  Also the layout transposes that live in the same unit.
#pragma once
#include "lo_common.h"

int lo_gn_nchunk(int HW, int C);     // pixel chunks per sample of the streaming passes = rows of P1 / P2 they write
// where one (sample, group) fits a workgroup: reduce + apply in one pass, and the forms that consume split-K slabs
bool lo_gn_bwd_local_applies(int HW, int C);

// one GroupNorm layer: raw conv output v [B][HW][C], saved statistics [B][8][2] (mean, rstd), affine parameters.  The forward
// writes stats (and, from split-K slabs, v); the backward reads both
struct LoGnLayer { const f16* v; const float* stats; const float* gamma; const float* beta; int B, HW, C; };

// ---- forward: y = GroupNorm + Mish (mode 0), + other (1: skip add), mish(.. + other) (2: ResBlock tail) -----------------------------
// Source: the conv epilogue's partial sums `partial` [B][MT][8][2] beside v, or the fp32 slabs [nsplit][B*HW][C] of a split-K conv,
// which are summed here (+ bias) into v first (one (sample, group)-local pass: lo_gn_bwd_local_applies, no y8)
struct LoGnFwd {
  const float* partial = nullptr; int MT = 0;
  const float* slab = nullptr; int nsplit = 0; const float* bias = nullptr;
  const f16* other = nullptr;
  int mode = 0;
  f16* y = nullptr;
  uint8_t* y8 = nullptr;         // optional e4m3 copy of y * LO_F8_ACT_SCALE
};
int lo_gn_forward(const LoGnLayer& l, const LoGnFwd& op, hipStream_t st);

// ---- backward: dv = gradient wrt v (+ ds, mode 2: gradient wrt mish(u) + identity); P1 / P2 rows for lo_gn_finalize_all ----------------
// Source: the activation gradient dy, or the fp32 slabs of the split-K data gradient that produces it (+ add_src; the fp16 sum is
// stored to dy_out when somebody else reads it)
struct LoGnBwd {
  const f16* dy = nullptr;
  const float* slab = nullptr; int nsplit = 0; const f16* add_src = nullptr; f16* dy_out = nullptr;
  const f16* other = nullptr;
  int mode = 0;
  f16* ds = nullptr;
  f16* dv = nullptr;
  float* P1 = nullptr;           // [B][rows.p1][C][2] (sum du, sum du*xhat)
  float* P2 = nullptr;           // [B][rows.p2][C]    (sum dv: the conv bias gradient)
  int rows_in_P1 = 0;            // rows per sample a fused data-gradient epilogue has already left in P1; 0 = none
  bool allow_local = false;      // the one-pass (sample, group)-local form may replace reduce + apply (LO_GN_LOCAL)
};
struct LoGnRows { int p1, p2; };    // rows per sample a launch leaves valid in P1 / P2 (0: it does not write that buffer)
enum LoGnBwdForm {
  LO_GNB_SLAB_LOCAL,    // slab sum + one-pass backward (plain mode); a slab use on a layer it does not fit gets one of the other
                        // three, which no slab call can run: ask before planning a split-K data gradient
  LO_GNB_APPLY_ONLY,    // P1 holds rows_in_P1 rows: the apply pass alone
  LO_GNB_LOCAL,         // reduce + apply in one pass
  LO_GNB_TWO_PASS       // reduce, then apply
};
struct LoGnUse { bool slab = false; int rows_in_P1 = 0; bool allow_local = false; };
static inline LoGnUse lo_gn_use(const LoGnBwd& op) { return {op.slab != nullptr, op.rows_in_P1, op.allow_local}; }
struct LoGnChoice { LoGnBwdForm form; LoGnRows rows; };
LoGnChoice lo_gn_bwd_choose(int HW, int C, const LoGnUse& use);
int lo_gn_backward(const LoGnLayer& l, const LoGnBwd& op, hipStream_t st, LoGnRows* rows = nullptr);   // rows: what the chosen form left
// the two-pass form + this layer's own parameter-gradient finalize (the C ABI's op-level entry point)
int lo_gn_bwd(const LoGnLayer& l, const LoGnBwd& op, float* dgamma, float* dbeta, float* dbias, float scale, hipStream_t st);

// GroupNorm affine + conv bias gradients of up to LO_GN_FIN_MAX layers in one launch: nblk1 / nblk2 = B * rows of P1 / P2
struct LoGnFinJob { const float* P1; const float* P2; float* dgamma; float* dbeta; float* dbias; int nblk1, nblk2, C, block0; };
#define LO_GN_FIN_MAX 16
struct LoGnFinJobs { LoGnFinJob j[LO_GN_FIN_MAX]; int n; };
int lo_gn_finalize_all(const LoGnFinJobs& jobs, float scale, hipStream_t st);

// ---- per-sample layout transposes [HW][C] <-> [C][HW] --------------------------------------------------------------------------------
int lo_nhwc_to_nchw_f16(const f16* src, f16* dst, int B, int HW, int C, hipStream_t st);
int lo_nchw_to_nhwc_f16(const f16* src, f16* dst, int B, int HW, int C, hipStream_t st, uint8_t* dst8 = nullptr);
int lo_nhwc_f16_to_nchw_f32(const f16* src, float* dst, int B, int HW, int C, float scale, hipStream_t st);   // module-boundary forms
int lo_nchw_f32_to_nhwc_f16(const float* src, f16* dst, int B, int HW, int C, float scale, hipStream_t st);
