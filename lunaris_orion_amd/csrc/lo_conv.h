// The convolution family (private to the library): geometry and weight packing (lo_conv_geom.hip), the implicit-GEMM kernel
// (lo_igemm.hip), the fused-tap and patch-resident kernels (lo_conv3.hip), fp8 packing (lo_conv_f8.hip), the weight gradients
// (lo_wgrad.hip, lo_wgrad3.hip, lo_wgrad2.hip) and the ONE place that decides which kernel runs an op (lo_conv_select.hip).
// The GroupNorm + Mish passes between the convs have the same shape of header: lo_norm.h.
#pragma once
#include "lo_common.h"

// ---- lo_conv_geom.hip: geometry, fp16 weight packing ------------------------------------------------------------------------
int lo_pack_weight(const float* w, f16* wp, const LoGeom& g, hipStream_t st);
int lo_pack_all(const LoPackJob* jobs_dev, int njobs, int nblocks, hipStream_t st, int block_base = 0);   // block_base: a sub-range of the table
int lo_pack_blocks(const LoGeom& g);   // blocks of one job in the fused pack launch
size_t lo_packed_weight_elems(const LoGeom& g);
static inline int lo_geom_packed_elems(const LoGeom& g) {
  int off = 0;
  for (int p = 0; p < g.n_phase; ++p) off += g.Cout * g.T[p] * g.Cin;
  return off;
}
static inline double lo_geom_flops(const LoGeom& g) {
  double f = 0;
  for (int p = 0; p < g.n_phase; ++p) f += 2.0 * g.B * g.GH * g.GW * (double)g.Cout * g.T[p] * g.Cin;
  return f;
}
// algorithmic bytes: input read once + output written once (fp16) + packed weights once
static inline double lo_geom_bytes(const LoGeom& g) {
  return 2.0 * ((double)g.B * g.Hin * g.Win * g.Cin + (double)g.B * g.Hout * g.Wout * g.Cout + lo_geom_packed_elems(g));
}

// ---- what a call asks of the op ---------------------------------------------------------------------------------------------
// Data-gradient epilogue that also runs the GroupNorm backward of the layer whose activation gradient it produces.  P1: the
// reduction (per-tile, per-channel sum du / sum du*xhat).  dv != null: the APPLY pass too -- the workgroups of a sample exchange
// their P1 rows (sc1 stores, arrival counter per (sample, n tile): lo_common.h lo_arrive_and_wait), form the group sums in the
// order lo_gn_bwd_apply uses and write dv (+ P2 = per-tile sums of dv for the conv bias gradient) instead of the activation
// gradient, which is then never stored.  LoConvChoice::gnb_apply: whether the chosen kernel supports it.
struct LoGnBwdFuse {
  const f16* v; const float* stats; const float* gamma; const float* beta; float* P1;
  f16* dv = nullptr; float* P2 = nullptr; unsigned int* counter = nullptr; unsigned int target = 0; unsigned int* fail = nullptr;
  bool keep_out = false;    // with dv: store the activation gradient too (somebody else reads it: the decoder's skip gradients)
};
// teacher epilogue: LeakyReLU(0.2), per-channel BN partial sums; out_pitch > 0: the output tensor has out_pitch channels per pixel
// and this op writes its Cout channels starting at channel out_choff (writing straight into a concatenated tensor)
struct LoConvExtra { int act; float* bn_partial; int out_pitch = 0; int out_choff = 0; };
// One conv-like op, fp16 operands.  slab + nsplit > 1: split-K (output = fp32 partials, the caller reduces).  gf: GroupNorm + Mish
// of the output inside the epilogue (LoGnFuse, lo_common.h) with the tile grid of LoConvChoice::mts / nt in gf->MTs / gf->NT.
struct LoConvOp {
  const f16* in = nullptr;
  const f16* w = nullptr;            // packed weights
  const float* bias = nullptr;       // [Cout]
  const f16* add_src = nullptr;      // residual / skip gradient, layout of out
  f16* out = nullptr;
  float* gn_partial = nullptr;       // [B][mts][8][2]
  float* slab = nullptr;
  int nsplit = 1;
  const LoGnBwdFuse* gb = nullptr;
  const LoConvExtra* ex = nullptr;
  const LoGnFuse* gf = nullptr;
};
// The same request as flags: everything the kernel choice depends on besides the geometry.
struct LoConvUse {
  bool bias = false, gn_partial = false, add = false;
  bool gb = false, gb_apply = false;   // GroupNorm-backward reduce in the epilogue; its apply form (LoGnBwdFuse::dv)
  bool ex = false, concat = false;     // teacher epilogue (activation / BatchNorm partials); concatenated output (out_pitch > 0)
  bool gf = false;                     // fused GroupNorm forward
  int nsplit = 1;
  bool f8 = false;                     // e4m3 operands (lo_conv_run_f8)
};
static inline LoConvUse lo_conv_use(const LoConvOp& op) {
  LoConvUse u;
  u.bias = op.bias != nullptr; u.gn_partial = op.gn_partial != nullptr; u.add = op.add_src != nullptr;
  u.gb = op.gb != nullptr; u.gb_apply = op.gb && op.gb->dv;
  u.ex = op.ex != nullptr; u.concat = op.ex && op.ex->out_pitch > 0;
  u.gf = op.gf != nullptr;
  u.nsplit = op.nsplit < 1 ? 1 : op.nsplit;
  return u;
}

// ---- lo_conv_select.hip: which kernel runs (g, use), and what callers size their buffers by ------------------------------------
enum LoConvKernel { LO_CK_NONE = 0, LO_CK_IGEMM, LO_CK_IGEMM_SPLITK, LO_CK_IGEMM_F8, LO_CK_CONV3_PP, LO_CK_CONVT4_PATCH, LO_CK_CONVS2D_PATCH };
struct LoConvChoice {
  int kernel;        // LoConvKernel; LO_CK_NONE: no kernel serves the request (fp8 operands on a geometry the e4m3 K step does not fit)
  int bm, bn, bk;    // lo_igemm_nt tile; lo_conv3x3_pp: bn output channels
  int th, tw;        // lo_conv3x3_pp: pixel tile
  int grid;          // workgroups
  int mts;           // partial-sum rows per sample the epilogue writes: GroupNorm partials, P1 rows of the fused GroupNorm backward
  int rows;          // the same over the batch: BatchNorm partial rows of the teacher epilogue
  int nt;            // n tiles per row
  bool gn_fuse;      // use.gf: the kernel takes the fused GroupNorm forward, with gf->MTs = mts and gf->NT = nt
  bool gnb_apply;    // use.gb_apply: the kernel takes the fused GroupNorm-backward apply, with mts P1 rows per sample and nt n tiles
};
LoConvChoice lo_conv_choose(const LoGeom& g, const LoConvUse& use);
int lo_conv_splitk_plan(const LoGeom& g);     // K splits for the few-rows convolutions (128 x 128 split-K tiles + a fused slab pass), 0 = no
int lo_conv_run(const LoGeom& g, const LoConvOp& op, hipStream_t st, LoConvChoice* chosen = nullptr);   // chosen: the choice it made
// the same op with both operands in e4m3: in8 = fp8(activation * LO_F8_ACT_SCALE) in the fp16 tensor's layout, w8 / wscale from
// lo_pack_f8_all; bias, add_src, out, gn_partial of `op` as in the fp16 form, and the teacher epilogue op.ex (activation, BatchNorm
// partial rows; no concatenated output).  chosen: the choice it made (the rows the launch wrote)
int lo_conv_run_f8(const LoGeom& g, const uint8_t* in8, const uint8_t* w8, const float* wscale, const LoConvOp& op, hipStream_t st,
                   LoConvChoice* chosen = nullptr);

// ---- lo_igemm.hip -----------------------------------------------------------------------------------------------------------
int lo_igemm_run(const LoGeom& g, const LoConvOp& op, const LoConvChoice& c, hipStream_t st);
int lo_igemm_run_f8(const LoGeom& g, const uint8_t* in8, const uint8_t* w8, const float* wscale, const LoConvOp& op, const LoConvChoice& c,
                    hipStream_t st);
int lo_splitk_reduce(const float* slab, const float* bias, float* out32, f16* out16, int M, int N, int nsplit, hipStream_t st);

// ---- lo_conv3.hip: fused-tap 3x3 kernel, patch-resident stride-2 kernels ------------------------------------------------------
int lo_conv3_run(const LoGeom& g, const LoConvOp& op, const LoConvChoice& c, hipStream_t st);
int lo_convt4_patch_run(const LoGeom& g, const LoConvOp& op, const LoConvChoice& c, hipStream_t st);
int lo_convs2d_patch_run(const LoGeom& g, const LoConvOp& op, const LoConvChoice& c, hipStream_t st);
// forced-kernel entry points of the teacher: the 16x16-pixel x 128-channel fused-tap kernel at any batch size
bool lo_conv3_pp_applies(const LoGeom& g);
bool lo_conv3_pp_f8_applies(const LoGeom& g);
int lo_conv3_pp_rows(const LoGeom& g);   // BatchNorm partial rows the two entry points below write (one per 16x16 tile)
int lo_conv3_run_pp_xf(const LoGeom& g, const f16* in, const f16* xc, const f16* kx, int nlev, const f16* wp, const float* bias,
                       f16* out, hipStream_t st, const LoConvExtra* ex);
int lo_conv3_run_pp_f8(const LoGeom& g, const uint8_t* in8, const uint8_t* w8, const float* wscale, const float* bias, f16* out,
                       hipStream_t st, const LoConvExtra* ex);

// ---- lo_conv_f8.hip: fp8 (e4m3) operand path of the forward convs ------------------------------------------------------------
struct LoPackF8Job { const f16* src; uint8_t* dst; float* scale; int K[LO_MAX_PHASE]; int wofs[LO_MAX_PHASE]; int Cout, n_phase, block0; };
void lo_pack_f8_job(LoPackF8Job* j, const LoGeom& g, const f16* src, uint8_t* dst, float* scale, int block0);   // blocks: n_phase * Cout
int lo_pack_f8_all(const LoPackF8Job* jobs_dev, int njobs, int nblocks, hipStream_t st, int block_base = 0);
int lo_pack_f8_one(const LoGeom& g, const f16* wp, uint8_t* w8, float* wscale, hipStream_t st);
int lo_quantize_f8(const f16* x, uint8_t* x8, size_t n, hipStream_t st);

// ---- weight gradients: lo_wgrad.hip (per-tap kernel, reduce, selection), lo_wgrad3.hip, lo_wgrad2.hip ---------------------------
enum LoWgradKernel { LO_WK_WGRAD3 = 0, LO_WK_WGRAD2, LO_WK_TN };
enum LoWgradReduce { LO_WR_NONE = 0, LO_WR_ROWS, LO_WR_CONVT, LO_WR_SCATTER };
// The whole plan of the weight gradient of g, computed by lo_wgrad_choose and nowhere else: a GEMM launch whose workgroups each own
// one channel tile over one range of K units and write one fp32 slab per split, then a reduce launch that sums the slabs.
struct LoWgradChoice {
  int kernel;                   // LoWgradKernel
  int bmw, bnw, bkp, stages;    // lo_wgrad_tn: output x reduced channels of a tile, pixels per K step, LDS stages
  int taps;                     // lo_wgrad_tn: (phase, tap) pairs, a workgroup each
  int tw;                       // lo_wgrad3x3_mt: chunk width (16: 2 x 16 pixels, 8: 4 x 8)
  bool convt;                   // lo_wgrad_s2_mt: the transposed-convolution form
  int tiles;                    // workgroups per split
  int units, units_per_split;   // K units (lo_wgrad_tn: bkp-pixel steps; multi-tap kernels: 32-position chunks)
  int nsplit;                   // splits launched = slabs written = slabs the reduce reads; none is empty
  int slabs;                    // slabs the caller provides (lo_wgrad_slab_bytes); >= nsplit
  dim3 grid, block;             // the GEMM launch
  bool direct;                  // the GEMM launch writes the scaled gradient itself: no slab, no reduce
  int reduce;                   // LoWgradReduce
  dim3 rgrid, rblock;           // the reduce launch
};
LoWgradChoice lo_wgrad_choose(const LoGeom& g);
int lo_wgrad_run(const LoGeom& g, const f16* x, const f16* dy, float* slab, float* grad, float scale, hipStream_t st);
size_t lo_wgrad_slab_bytes(const LoGeom& g);
int lo_wgrad3_run(const LoGeom& g, const LoWgradChoice& p, const f16* x, const f16* dy, float* slab, hipStream_t st);
int lo_wgrad2_run(const LoGeom& g, const LoWgradChoice& p, const f16* x, const f16* dy, float* slab, hipStream_t st);
