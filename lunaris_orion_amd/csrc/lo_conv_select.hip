// Kernel selection for the convolution family: lo_conv_choose() is the one place that decides which kernel runs (geometry, use),
// with which tile and grid, and how many partial-sum rows its epilogue writes.  lo_conv_run / lo_conv_run_f8 launch what it says;
// the planners and executors size their buffers and decide their fusions from the same answer, made with the use the later call has.
#include "lo_conv.h"
#include "lo_norm.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>

// Split-K plan for a single-phase convolution whose GroupNorm groups are (sample, group)-local (lo_gn_bwd_local_applies on ITS
// OUTPUT): 128 x 128 tiles, K split so that about two workgroups per CU run.  Returns the number of splits, or 0 when the op
// should stay on its one-launch kernel (long grids, fused-tap geometry that already fills the chip, too few K steps).
int lo_conv_splitk_plan(const LoGeom& g) {
  if (g.n_phase != 1 || g.T[0] < 9 || g.Cin % 64 != 0 || g.Cout % 128 != 0) return 0;
  const long M = (long)g.B * g.GH * g.GW;
  if (M % 128 != 0 || !lo_gn_bwd_local_applies(g.GH * g.GW, g.Cout)) return 0;
  const long tiles = (M / 128) * (g.Cout / 128);
  if (tiles >= 256) return 0;                         // the one-launch kernels already put a workgroup on every CU
  const int ksteps = g.T[0] * (g.Cin / 64);
  int ns = (int)((512 + tiles - 1) / tiles);
  while (ns > 1 && ksteps / ns < 8) --ns;             // at least 8 K steps per split
  return ns >= 2 ? ns : 0;
}

// Largest tile (BM=128 preferred) that still gives >= 512 workgroups (two per CU); measured on MI355X at B=64:
// 128x128 wins at M=65536/N=128, 128x64 at M=16384/N=256, 64x64 at M=4096/N=512.
static void pick_tile(const LoGeom& g, int* bm_out, int* bn_out) {
  const int per_sample = g.GH * g.GW;
  const size_t M = (size_t)g.B * per_sample;
  const int BK = (g.Cin % 64 == 0) ? 64 : 32;
  constexpr int min_wgs = 512;     // 256 / 384 / 512 / 768 / 1024 swept twice (rounds 1, 2): a plateau, 512 kept
  const int cand[4][2] = {{128, 128}, {128, 64}, {64, 128}, {64, 64}};
  int bm = 64, bn = (g.Cout % 64 == 0) ? 64 : 32;
  if (BK == 32) {
    bn = 64;
    bm = (per_sample % 128 == 0 && (M / 128) * (g.Cout / 64) * g.n_phase >= (size_t)min_wgs) ? 128 : 64;
  } else if (g.Cout % 64 != 0) {
    bm = (per_sample % 128 == 0 && (M / 128) * (g.Cout / 32) * g.n_phase >= (size_t)min_wgs) ? 128 : 64;
  } else {
    for (int i = 0; i < 4; ++i) {
      int cm = cand[i][0], cn = cand[i][1];
      if (per_sample % cm || g.Cout % cn || (g.Cout >> 3) > cn) continue;   // whole tiles per sample; GN group inside a tile
      bm = cm; bn = cn;
      if (((M + cm - 1) / cm) * (g.Cout / cn) * g.n_phase >= (size_t)min_wgs) break;
    }
  }
  *bm_out = bm; *bn_out = bn;
}

// ---- lo_conv3x3_pp (fused-tap 3x3 stride-1 kernel, lo_conv3.hip) --------------------------------------------------------------
// LO_HALO: 0 = never, 2 = default (the shapes where it measured faster than lo_igemm_nt), 3 = every shape it can tile (what the
// forced parity test uses: small batches run on it too)
static inline int conv3_mode() {
  static const int m = getenv("LO_HALO") ? atoi(getenv("LO_HALO")) : 2;
  return m;
}
// tile of the 8-wave ping-pong kernel that gives >= 256 workgroups at batch 64: 16x16 pixels x 128 channels, 8x16 x 128 when that
// would leave CUs idle, 16x16 x 64 for 64 output channels
static inline bool conv3_tile(const LoGeom& g, int* th, int* tw, int* bn) {
  if (g.n_phase != 1 || g.T[0] != 9 || g.in_stride != 1 || g.out_stride != 1) return false;
  if (g.Cin % 64 || g.Cout % 64 || g.Win % 16 || g.Hin % 16) return false;
  const long t16 = (long)g.B * (g.Hin / 16) * (g.Win / 16);
  if (g.Cout % 128 == 0 && t16 * (g.Cout / 128) >= 256) { *th = 16; *tw = 16; *bn = 128; }
  else if (g.Cout % 128 == 0) { *th = 8; *tw = 16; *bn = 128; }
  else if (g.Cout == 64) { *th = 16; *tw = 16; *bn = 64; }
  else return false;
  return (g.Cout >> 3) <= *bn;   // a GroupNorm group must fit inside the N tile
}
// is the fused-tap kernel selected for g?  need_bn: the launch carries the teacher's BatchNorm epilogue
static bool conv3_selected(const LoGeom& g, bool need_bn, int* th, int* tw, int* bn) {
  const int mode = conv3_mode();
  if (mode == 0 || !conv3_tile(g, th, tw, bn)) return false;
  if (mode == 2) {
    // default: where it measured faster than lo_igemm_nt -- the 16x16-pixel x 128-channel workgroup on
    // long grids (>= 4 tiles per CU: the teacher), and, for launches without the BatchNorm epilogue, any tile choice above that
    // puts a workgroup on every CU (the VAE's 64 / 128 / 256-channel ResBlock convolutions at batch 64: 44 -> 36, 34 -> 28,
    // 36 -> 33 us; +1.0 % on the step over three interleaved pairs)
    const long tiles = (long)g.B * (g.Hin / *th) * (g.Win / *tw) * (g.Cout / *bn);
    const bool long_grid = *th == 16 && *bn == 128 && tiles >= 1024;
    if (!(long_grid || (!need_bn && tiles >= 256))) return false;
  }
  return true;
}

// ---- patch-resident stride-2 kernels (lo_conv3.hip) ---------------------------------------------------------------------------
// ConvTranspose2d k4 s2 p1 forward geometry with 64 -> 32 or 128 -> 64 channels on a map of whole 16 x 16 tiles
static bool convt4_patch_geom(const LoGeom& g) {
  if (g.n_phase != 4 || g.in_stride != 1 || g.out_stride != 2) return false;
  if (!((g.Cin == 64 && g.Cout == 32) || (g.Cin == 128 && g.Cout == 64))) return false;
  for (int p = 0; p < 4; ++p) if (g.T[p] != 4) return false;
  return g.Hin % 16 == 0 && g.Win % 16 == 0 && g.Hout == 2 * g.Hin && g.Wout == 2 * g.Win;
}
// Data gradient of the stride-2 3x3 convolution 64 -> 128 (lunar_generate.py:102): dy [B][32][32][128] -> dx [B][64][64][64] (+ add_src)
static bool convs2d_patch_geom(const LoGeom& g) {
  if (g.n_phase != 4 || g.in_stride != 1 || g.out_stride != 2 || g.Cin != 128 || g.Cout != 64) return false;
  if (g.T[0] != 1 || g.T[1] != 2 || g.T[2] != 2 || g.T[3] != 4) return false;
  for (int p = 0; p < 4; ++p)
    for (int t = 0; t < g.T[p]; ++t) if (g.dy[p][t] < 0 || g.dy[p][t] > 1 || g.dx[p][t] < 0 || g.dx[p][t] > 1) return false;
  return g.Hin % 16 == 0 && g.Win % 16 == 0 && g.Hout == 2 * g.Hin && g.Wout == 2 * g.Win;
}

// ---- the choice ---------------------------------------------------------------------------------------------------------------
static void set_rows(LoConvChoice& c, const LoGeom& g, int mts, int nt) {   // kernels whose tiles lie inside one sample
  c.mts = mts; c.nt = nt;
  c.rows = g.B * mts;
}
static void choose_igemm_tile(LoConvChoice& c, const LoGeom& g, int n_z) {   // bm / bn are set; n_z: phases, or K splits
  const long M = (long)g.B * g.GH * g.GW;
  c.mts = (g.GH * g.GW / c.bm) * g.n_phase; c.nt = g.Cout / c.bn;
  c.rows = (int)((M / c.bm) * g.n_phase);      // M tiles may span samples (the teacher's 1x1 convs, the Linear layers)
  c.grid = (int)((M + c.bm - 1) / c.bm) * c.nt * n_z;
}

// e4m3 operands: every shape the e4m3 K step fits, also where a fused-tap fp16 kernel owns the fp16 form (conv by conv the e4m3 implicit
// GEMM is the faster launch there too: profiles/r04_fp8_per_layer.txt; on the step +0.5 %).  LO_F8_FORCE=0: the round-2 selection (those
// shapes stay fp16).  Always lo_igemm_nt's tiles, whatever fp16 kernel owns the geometry.
// The wide teacher's 3x3 convs at 128 x 128 (feature_dim 256 / 512, teacher epilogue: use.ex) were measured against the fp16 launch
// that owns each geometry (lo_conv3x3_pp), batch 8, three interleaved pairs, e4m3 ahead in every pair -- 128 -> 256: 68-77 us against
// 95-103; 256 -> 256: 97-101 against 154-158; 128 -> 512: 118-122 against 170-176; 512 -> 512: 313-316 against 535-538
// (profiles/teacher_fp8_wide_ab.md) -- so none of them is routed back to fp16 here; LoTeacher::fp8a / fp8b follow this answer.
static LoConvChoice choose_f8(const LoGeom& g) {
  static const bool force = !(getenv("LO_F8_FORCE") && atoi(getenv("LO_F8_FORCE")) == 0);
  LoConvChoice c{};
  int th, tw, bn;
  if (!(g.Cin % 128 == 0 && g.Cout % 64 == 0 && (force || !conv3_selected(g, false, &th, &tw, &bn)))) return c;
  c.kernel = LO_CK_IGEMM_F8;
  pick_tile(g, &c.bm, &c.bn);
  c.bk = 128;
  choose_igemm_tile(c, g, g.n_phase);
  return c;
}

// Precedence: lo_convt4_patch (a bare forward: bias and GroupNorm partials only), lo_convs2d_patch (a bare data gradient: residual add
// only; where the grid fills at least half the chip), lo_conv3x3_pp (every epilogue but the concatenated output), split-K lo_igemm_nt,
// lo_igemm_nt with the tile of pick_tile.
LoConvChoice lo_conv_choose(const LoGeom& g, const LoConvUse& u) {
  if (u.f8) return choose_f8(g);
  LoConvChoice c{};
  const int nsplit = u.nsplit < 1 ? 1 : u.nsplit;
  const int per_sample = g.GH * g.GW;
  const bool bare = nsplit == 1 && !u.gb && !u.ex && !u.gf;
  const int tiles16 = (g.Hin / 16) * (g.Win / 16);
  if (bare && !u.add && convt4_patch_geom(g)) {
    // last transposed convs of the decoder, patch-resident
    c.kernel = LO_CK_CONVT4_PATCH;
    set_rows(c, g, tiles16, 1);
    c.grid = g.B * tiles16;
  } else if (bare && !u.bias && !u.gn_partial && convs2d_patch_geom(g) && g.B * tiles16 >= 128) {
    // data gradient of the 64 -> 128 stride-2 conv, patch-resident, where the grid fills at least half the chip (batch >= 32):
    // +0.65 % on the step against the four-phase lo_igemm_nt launch (24 403-24 510 against 24 257-24 324 sprites/s, interleaved)
    c.kernel = LO_CK_CONVS2D_PATCH;
    set_rows(c, g, 0, 1);
    c.grid = g.B * tiles16;
  } else if (int th, tw, bn; nsplit == 1 && conv3_selected(g, u.ex, &th, &tw, &bn)) {
    // fused-tap kernel for 3x3 stride-1 (it always carries the GroupNorm-backward epilogue, so use.gb never sends an op elsewhere)
    c.kernel = LO_CK_CONV3_PP;
    c.th = th; c.tw = tw; c.bn = bn;
    set_rows(c, g, (g.Hin / c.th) * (g.Win / c.tw), g.Cout / c.bn);
    c.grid = c.rows * c.nt;
    c.gn_fuse = u.gf && c.mts * c.nt <= LO_GNF_MAX_TILES;
    c.gnb_apply = u.gb_apply && (g.Cout >> 3) >= 8 && c.mts * c.nt <= LO_GNF_MAX_TILES;
  } else if (nsplit > 1) {
    // convolutions with few output rows (the 8 x 8 stage: M = 4 096): 128 x 128 tiles halve the L2 -> LDS operand traffic of the
    // 64 x 64 tiles that the tile heuristic would need to fill the chip, and the K split fills it instead (lo_conv_splitk_plan)
    c.kernel = LO_CK_IGEMM_SPLITK;
    c.bm = c.bn = (g.T[0] > 1 && ((long)g.B * per_sample) % 128 == 0 && g.Cout % 128 == 0) ? 128 : 64;
    c.bk = (g.Cin % 64 == 0) ? 64 : 32;
    choose_igemm_tile(c, g, nsplit);
    c.mts = c.rows = 0;      // fp32 partial products only: no epilogue sums
  } else {
    c.kernel = LO_CK_IGEMM;
    pick_tile(g, &c.bm, &c.bn);
    c.bk = (g.Cin % 64 == 0) ? 64 : 32;
    choose_igemm_tile(c, g, g.n_phase);
    const bool whole = g.Cin % 64 == 0 && g.Cout % 64 == 0 && per_sample % c.bm == 0 && (g.Cout >> 3) <= c.bn;
    // the patch-resident transposed conv owns its geometry and has no fused GroupNorm epilogue (not built): no fusion there
    c.gn_fuse = u.gf && whole && !convt4_patch_geom(g) && c.mts * c.nt <= LO_GNF_MAX_TILES;
    // tiles inside one sample, 8-channel chunks inside one GroupNorm group
    c.gnb_apply = u.gb_apply && whole && g.n_phase == 1 && (g.Cout >> 3) >= 8 && c.nt <= 8 && c.mts <= LO_GNF_MAX_TILES;
  }
  return c;
}

// Run one conv-like op on the kernel lo_conv_choose names for (g, the use of op).  chosen: where to leave that choice (the rows the launch wrote)
int lo_conv_run(const LoGeom& g, const LoConvOp& op, hipStream_t st, LoConvChoice* chosen) {
  const LoGnFuse* gf = op.gf;
  const LoGnBwdFuse* gb = op.gb;
  LO_REQUIRE(g.Cin % 32 == 0, "lo_conv_run: Cin=%d must be a multiple of 32", g.Cin);
  LO_REQUIRE(g.Cout % 32 == 0, "lo_conv_run: Cout=%d must be a multiple of 32", g.Cout);
  const LoConvUse u = lo_conv_use(op);
  const LoConvChoice c = lo_conv_choose(g, u);
  if (chosen) *chosen = c;
  if (gf) {
    LO_REQUIRE(u.nsplit <= 1 && !u.add && !gb && !u.ex && gf->y && gf->xbuf && gf->counter && gf->fail && gf->gamma && gf->beta &&
               (gf->mode == 0 || gf->other), "lo_conv_run: bad fused-GroupNorm arguments");
    LO_REQUIRE(c.gn_fuse && c.mts == gf->MTs && c.nt == gf->NT,
               "lo_conv_run: fused GroupNorm asked for a geometry / tile grid the kernel does not have (check LoConvChoice::gn_fuse)");
  }
  if (u.gb_apply)
    LO_REQUIRE(gb->P2 && gb->counter && gb->fail && c.gnb_apply,
               "lo_conv_run: fused GroupNorm-backward apply asked for a geometry the kernel does not support (check LoConvChoice::gnb_apply)");
  LO_REQUIRE(!u.concat || (!u.add && !gb && op.ex->out_pitch % 8 == 0 && op.ex->out_choff % 8 == 0), "lo_conv_run: bad concatenated-output arguments");
  switch (c.kernel) {
    case LO_CK_CONVT4_PATCH: return lo_convt4_patch_run(g, op, c, st);
    case LO_CK_CONVS2D_PATCH: return lo_convs2d_patch_run(g, op, c, st);
    case LO_CK_CONV3_PP: return lo_conv3_run(g, op, c, st);
    case LO_CK_IGEMM_SPLITK:
    case LO_CK_IGEMM: return lo_igemm_run(g, op, c, st);
    default: break;
  }
  lo_set_error("lo_conv_run: no kernel for this op");
  return LO_ERR_ARG;
}

int lo_conv_run_f8(const LoGeom& g, const uint8_t* in8, const uint8_t* w8, const float* wscale, const LoConvOp& op, hipStream_t st,
                   LoConvChoice* chosen) {
  LO_REQUIRE(!op.gb && !op.gf && !op.slab && op.nsplit <= 1 && !(op.ex && op.ex->out_pitch > 0),
             "lo_conv_run_f8: the e4m3 path has bias, residual add, GroupNorm partials and the teacher epilogue (activation, BatchNorm partials) only");
  LoConvUse u = lo_conv_use(op);
  u.f8 = true;
  const LoConvChoice c = lo_conv_choose(g, u);
  if (chosen) *chosen = c;
  LO_REQUIRE(c.kernel == LO_CK_IGEMM_F8, "lo_conv_run_f8: geometry not supported (Cin %% 128, Cout %% 64)");
  return lo_igemm_run_f8(g, in8, w8, wscale, op, c, st);
}
