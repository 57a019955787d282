// Private header of the native teacher executor: LunarMoETeacher.forward AS EXECUTED by the reference (lunar_evaluator.py:57-462;
// SURVEY §3.4, §8 row A12) -- fp16 NHWC activations, fp32 BatchNorm statistics -- and its backward.
//   lo_teacher_plan.hip       state table, parameter offsets, workspace plan, create / destroy, queries, pack
//   lo_teacher_kernels.hip    kernels every path shares (first conv, BatchNorm finalize / apply, depthwise convs, the generic
//                             attention, dropout glue) behind host launchers; the BatchNorm ones take an op struct (TBnFinalize, TBnApply)
//   lo_teacher_f128.hip       feature_dim 128: the sparse / dense / dropout forms of an ExpertBlock and their kernels
//   lo_teacher_heads.hip      gate / quality / semantic / embedding heads, their backward, reward bookkeeping
//   lo_teacher_forward.hip    feature extractor forward, plain ExpertBlock forward, lo_teacher_forward
//   lo_teacher_bwd_block.hip  full backward: BatchNorm (op struct TbBnBwd) and ExpertBlock backward
//   lo_teacher_bwd.hip        full backward: plan, feature extractor backward, executor, clip + AdamW
// There is no relocatable device code: a kernel is launched only from the unit that defines it; the ones other units need sit
// behind a one-line host launcher, which is also where feature_dim picks the template argument.
#pragma once
#include "lo_internal.h"
#include "../../include/lunaris_hip.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <optional>
#include <string>
#include <vector>

#define T_HW 16384
#define T_W 128
#define BN_EPS 1e-5f
#define LN_EPS 1e-5f
#define T_FMAX 512   // largest feature_dim

// flat parameter / flat gradient / workspace / backward-scratch addressing: expect `P`, `G`, `ws`, `bws` in scope
#define TP(o) (P + (o))
#define TG(o) (G + (o))
#define TW(T, o) reinterpret_cast<T*>(reinterpret_cast<unsigned char*>(ws) + (o))
#define TB(T, o) reinterpret_cast<T*>(reinterpret_cast<unsigned char*>(bws) + (o))
#define LO_TRYT(call) do { int _r = (call); if (_r != LO_OK) return _r; } while (0)
// a teacher igemm launch reported under its own profiler name
#define LO_TAGGED(tag, call) do { g_lo_prof_tag = (tag); int _r = (call); g_lo_prof_tag = nullptr; if (_r != LO_OK) return _r; } while (0)

// a profiler scope whose name the caller of a shared launch sequence supplies; null: that caller reports none at this site
struct TOptScope {
  std::optional<LoProfScope> s;
  TOptScope(const char* name, double flops, double bytes, hipStream_t st) { if (name) s.emplace(name, flops, bytes, st); }
};

// the dropout of one teacher call: threshold on the 16 mask bits of an element (keep <=> bits >= thr), 1 / (1 - p), call seed
struct LoDropCfg {
  bool on; uint32_t thr; float inv_keep; uint64_t seed;      // off: thr = 0, inv_keep = 1
  LoDropSite site(uint32_t s) const { return lo_drop_site_keys(seed, s); }
};
static inline LoDropCfg lo_drop_cfg(float p, uint64_t seed) {
  LoDropCfg d{p > 0.f, 0u, 1.0f, seed};
  if (d.on) {
    d.thr = (uint32_t)lrintf(p * 65536.f);
    if (d.thr == 0) d.thr = 1;
    d.inv_keep = 1.0f / (1.0f - p);
  }
  return d;
}

// ---- offsets (in floats) of the parameters inside the flat state, resolved from the state table's names once, in create ----------
struct TBnOff { size_t weight = 0, bias = 0, running_mean = 0, running_var = 0; };
struct TBlockOff {
  size_t layer_scale = 0, conv1_w = 0, conv1_b = 0; TBnOff bn1;
  size_t qkv_w = 0, qkv_b = 0, proj_w = 0, proj_b = 0, conv2_w = 0, conv2_b = 0; TBnOff bn2;
  size_t sc_w = 0, sc_b = 0; TBnOff bn_sc;   // ExpertBlock.shortcut = Conv1x1 + BatchNorm: exists when in_channels != out_channels only
};
struct TBranchOff { size_t dw_w = 0, dw_b = 0, pw_w = 0, pw_b = 0; TBnOff bn; };
struct TFeOff { size_t conv1_w = 0, conv1_b = 0; TBnOff bn1; TBranchOff br[3]; size_t fus_w = 0, fus_b = 0; TBnOff bn_fus; };
struct THeadOff { size_t ln_w = 0, ln_b = 0, w1 = 0, b1 = 0, w2 = 0, b2 = 0; };
struct THeadsOff { size_t g_w1 = 0, g_b1 = 0, g_w2 = 0, g_b2 = 0; THeadOff q[8], sem, style, prompt; };

struct LoTeacher {
  int B = 0, E = 0, I = 256, emb = 0, layers = 3;
  int F = 128;                // feature_dim: 128 (fast paths) or 256 / 512 (plain form: every tensor at full resolution)
  // plain form of a block (feature_dim 256 / 512, and any feature_dim in the full-backward mode): conv 128->F, conv F->F, qkv F->3F,
  // shortcut 128->F (1x1), proj on the compact rows; gfw: a 64-channel slice of the fusion conv 192 -> 128 (its weight gradient)
  LoGeom g3a{}, g3b{}, gqF{}, gsc{}, gpc{}, gfw{};
  size_t o_wsc[8] = {}, o_sc = 0, o_ss_sc = 0, o_attc = 0;   // packed shortcut weights per expert, raw shortcut output, its (scale, shift), compact attention rows
  // state table (the reference's state_dict order) and where its named parameters sit
  std::vector<std::string> names;
  std::vector<size_t> off, numel;
  std::vector<char> is_float;
  size_t flat_elems = 0;
  TFeOff fe;
  TBlockOff blk[8][3];
  THeadsOff heads;
  // workspace offsets
  size_t o_raw32 = 0, o_dw = 0, o_br[3] = {}, o_cat = 0, o_feat = 0, o_x0 = 0, o_x1 = 0, o_rawA = 0, o_bnA = 0, o_qkv = 0, o_att = 0, o_proj = 0, o_rawB = 0;
  size_t o_bnp = 0, o_bnpre = 0, o_ss = 0, o_poolp = 0, o_pool_f = 0, o_pool_e = 0, o_rawq = 0;
  size_t o_wp3[8][3][2] = {};   // packed 3x3 weights (expert, layer, conv1/conv2)
  size_t o_wqkv[8][3] = {}, o_wproj[8][3] = {}, o_wpw[3] = {}, o_wfus = 0;
  size_t o_wfus_fold = 0, o_bfus_fold = 0, o_ss_cat = 0;   // fusion conv with the three branch BatchNorms folded in (per call)
  LoGeom g3{}, gq{}, gp{}, gpw{}, gfus{};
  // sparse expert path (default; LO_T_DENSE=1 selects the dense one): folded attention (no k / v tensors), proj and
  // conv2 on the 8 image rows per sample that are not a constant field
  bool sparse = true;
  LoGeom gU{}, gZ{}, g3c{};
  size_t o_qin = 0, o_U = 0, o_Z = 0, o_projc = 0, o_rawBc = 0, o_cvec[8][3] = {}, o_wu[8][3] = {}, o_ub[8][3] = {}, o_wz[8][3] = {};
  int qrows = 0;              // query rows of the U GEMM: B * 543 rounded up to a multiple of 128
  bool fuse_tail = false;     // block tail folded into the next conv1 (LO_T_FUSE_TAIL=0 turns it off)
  size_t o_xc[2] = {}, o_kx[8] = {};   // compact rows of x_l (ping-pong), transform constants [3][6][128] fp16 per expert (contiguous)
  size_t o_xc3 = 0, o_poolpe = 0;      // compact rows of x_3 of every expert [E][B][1024][128]; pool partials [E][B][64][128]
  size_t o_ssb = 0;           // per-sample (scale, shift) of a BatchNorm followed by Dropout2d: [B][128][2]
  // fp8 mode (LO_TEACHER_FP8_CONV): e4m3 weights + row scales of the 24 3x3 convs, e4m3 activations.  feature_dim 128: the dropout
  // path only; 256 / 512: every train-mode lo_teacher_forward, per geometry (fp8a: the 128 -> F conv1 of a first block, fp8b: the F -> F
  // convs), each where lo_conv_choose serves the teacher epilogue on e4m3 operands; fp8 = either
  bool fp8 = false, fp8a = false, fp8b = false;
  size_t o_w8[8][3][2] = {}, o_ws8[8][3][2] = {}, o_feat8 = 0, o_x8[2] = {}, o_proj8 = 0;
  size_t ws_bytes = 0;
  bool att_zeroed = false;
  const void* att_zeroed_ws = nullptr;
  // dropout of the last forward (lo_teacher_heads_backward replays the head masks), and which path it took:
  // 0 sparse (constant-field shortcuts), 1 dense (LO_T_DENSE=1), 2 dropout (train mode, dropout_p > 0)
  float last_p = 0.f; uint64_t last_seed = 0; int last_path = -1;
  // full-backward mode (lo_teacher_bwd.hip): lo_teacher_forward_keep is a forward of its own (plain form, every tensor of every block
  // kept inside the backward's scratch `kept_bws`); lo_teacher_full_backward on the same scratch then recomputes nothing
  // kept_eval: which mode left the tensors (lo_teacher_forward_keep_eval: running statistics, no dropout); a backward of the other
  // mode recomputes instead of consuming them
  const void* kept_bws = nullptr; bool kept = false, kept_eval = false;
  bool bwd_shared = false;    // LO_T_BWD_SHARED=1: the full backward's shared-tensor-set plan (one recomputation per block) at any size
};

// ---- lo_teacher_kernels.hip ---------------------------------------------------------------------------------------------------------
// BatchNorm finalize of `nrow` partial rows into (scale, shift): the shared slot o_ss, or ss_dst; mr: (mean, rstd) kept for the backward.
// training: 1 batch statistics + running-statistics update, 2 batch statistics only, 0 running statistics.  tps / vtps / cvec: the
// sparse path's compact rows (tiles per sample, of which valid; the constant vectors that stand for the rest)
struct TBnFinalize {
  const float* partial; int nrow, C; const TBnOff& bn; int training;
  int tps = 1, vtps = 1; const float* cvec = nullptr; float* ss_dst = nullptr; float* mr = nullptr;
};
int t_bn_finalize(LoTeacher* h, float* P, void* ws, const TBnFinalize& op, hipStream_t st);
// BatchNorm apply from the (scale, shift) of the last finalize (per_sample: the Dropout2d table o_ssb), BnApplyArgs::mode:
enum TBnMode { T_BN_PLAIN = 0, T_BN_TAIL = 1, T_BN_TAIL_SPARSE = 2 };   // y = BN(raw); ExpertBlock tail; the tail on the sparse raw tensor + cvec
struct TBnApply {
  const f16* raw; const float* ls = nullptr; const f16* identity = nullptr; f16* y = nullptr; int C;
  int dst_pitch = C, dst_off = 0;      // y has dst_pitch channels per pixel and gets its C from channel dst_off
  int mode = T_BN_PLAIN; float* pool_partial = nullptr; const float* cvec = nullptr; bool per_sample = false;
  uint8_t* y8 = nullptr; const float* id_ss = nullptr;       // e4m3 copy of y; (scale, shift) of a BatchNorm on the identity branch
};
int t_bn_apply(LoTeacher* h, void* ws, const TBnApply& op, hipStream_t st);
int t_pool_finalize(const float* partial, float* pooled, int nblk, int C, int total, hipStream_t st);
int t_pool(LoTeacher* h, float* pooled, int C, void* ws, hipStream_t st);      // from the pool partials of the last t_bn_apply (o_poolp)
int t_conv1(const float* x, const float* w, const float* bias, f16* out, float* bn_partial, int B, hipStream_t st);
int t_dwconv(int K, const f16* raw, const float* ss, const float* w, const float* bias, f16* out, int B, hipStream_t st);   // K = 3 or 5
int t_attn_generic(int F, const f16* qkv, f16* attc, int B, LoDropSite ds, uint32_t thr, float inv_keep, hipStream_t st);
int t_projdrop(int C, const f16* projc, const float* pbias, f16* out, uint8_t* out8, size_t nchunk, LoDropSite ds, uint32_t thr,
               float inv_keep, hipStream_t st);
int t_cat_bn_drop(f16* cat, const float* ss, size_t nchunk, LoDropSite ds, uint32_t thr, float inv_keep, hipStream_t st);
int t_fold_fusion(const float* w, const float* bias, const float* ss, f16* w16, float* bias_out, hipStream_t st);
// Dropout2d after a BatchNorm: o_ss (C channels) -> o_ssb, the per-sample table with the kept channels scaled and the dropped ones zero
int t_drop2d(LoTeacher* h, void* ws, int C, const LoDropCfg& d, uint32_t site, hipStream_t st);

// ---- lo_teacher_forward.hip ---------------------------------------------------------------------------------------------------------
// where one feature extractor forward leaves its tensors.  dw: the depthwise outputs (one shared buffer three times, or three kept);
// catd != null: Dropout(BN(cat)) goes there and cat stays raw (else in place); feat8, the (mean, rstd) tables and pool_partial may be null
struct TFeDst {
  f16* raw32; f16* dw[3]; f16* cat; f16* catd; f16* rawF; f16* feat; uint8_t* feat8;
  float* ss32;                                  // (scale, shift) of the 32-channel BatchNorm, read by the depthwise convs
  float *mr32, *mr_br[3], *mr_fus;
  float* pool_partial;
};
struct TFeNames { const char *conv1, *dw3, *dw5, *cat_bn_drop; };   // LoProfScope names
// fold: the branch BatchNorms fold into the fusion conv (no dropout between them); else normalise + drop (d.thr = 0: normalise only)
int t_fe_forward(LoTeacher* h, const float* x, float* P, void* ws, int train, const LoDropCfg& d, bool fold, const TFeDst& t,
                 const TFeNames& nm, hipStream_t st);
// the tensors of one ExpertBlock in plain form (what its backward reads); scraw / ssS / mrS: shortcut branch (feature_dim != 128, layer 0);
// the (mean, rstd) tables may be null
struct TBlkT { f16 *rawA, *bnA, *qkv, *attc, *projc, *a2, *rawB, *scraw; float *mrA, *mrB, *mrS, *ssS; };
struct TBlkNames { const char *shortcut, *conv1, *qkv, *proj, *conv2;    // LO_TAGGED tags of the five convolutions
                   const char *attn, *projdrop; };                      // LoProfScope names
// e4m3 operands of the block's two 3x3 convs (fp8 mode of the wide teacher), each conv on its own: xin8 = the e4m3 copy of xin and
// w8[0] / ws8[0] conv1's weights (null: conv1 stays fp16); a28 = where proj_drop writes conv2's input as e4m3 INSTEAD of t.a2 and
// w8[1] / ws8[1] conv2's weights (null: fp16); xout8: the tail also emits the e4m3 copy of xout (null: not wanted)
struct TBlk8 { const uint8_t* xin8; uint8_t* a28; uint8_t* xout8; const uint8_t* w8[2]; const float* ws8[2]; };
// ExpertBlock (e, l) in plain form from xin into the tensor set t; xout = the block output (null: not wanted), pool_partial: its
// per-sample column sums (null: not wanted); both null skips the tail.  train: 1 the step's forward (running statistics move), 2 a
// recomputation (they do not), 0 eval
int t_block_plain(LoTeacher* h, float* P, void* ws, int e, int l, const LoDropCfg& d, const TBlkT& t, const f16* xin, f16* xout, int train,
                  float* pool_partial, const TBlkNames& nm, hipStream_t st, const TBlk8* f8 = nullptr);

// one lo_teacher_forward call, as the block forms see it
struct TFwd { LoTeacher* h; float* P; void* ws; hipStream_t st; int training; LoDropCfg d; bool stats_only, f8; };

// ---- lo_teacher_f128.hip ------------------------------------------------------------------------------------------------------------
int t_pack_f128(LoTeacher* h, const float* P, void* ws, int e, int l, hipStream_t st);   // weight-only products of the folded attention + constant vectors
int t_block_dropout(const TFwd& c, int e, int l);
int t_block_sparse(const TFwd& c, int e, int l);
int t_block_dense(const TFwd& c, int e, int l);
int t_pool_fused(const TFwd& c);           // fused tail: x_3 of every expert pooled in one pass over feat

// ---- lo_teacher_heads.hip -----------------------------------------------------------------------------------------------------------
int t_run_heads(LoTeacher* h, float* P, void* ws, float* quality, float* weights, float* style, float* prompt, float* semantic,
                const LoDropCfg& d, hipStream_t st);
int t_heads_backward(LoTeacher* h, const float* P, const float* pooled_f, const float* pooled_e, const float* raw_q,
                     const float* expert_weights, const float* dq_up, const float* dw_up, float coef, const LoDropCfg& d, float* rows,
                     float* grads, hipStream_t st, float* d_pool_f = nullptr, float* d_pool_e = nullptr);

// ---- full backward (lo_teacher_bwd.hip, lo_teacher_bwd_block.hip) -----------------------------------------------------------------------
// the tensors of one ExpertBlock that its backward reads, as offsets into the backward's scratch.  saved plan: one set per block, filled
// once by the forward (lo_teacher_forward_keep) or by the backward's own first pass; otherwise ONE shared set, refilled in front of
// every block's backward
struct TbBlk { size_t rawA, bnA, qkv, attc, projc, a2, rawB, scraw, mrA, mrB, mrS, ssS; };
struct TbPlan {
  size_t o_raw32, o_dwb[3], o_cat, o_catd, o_rawF, o_feat, o_xs[8][3];
  bool saved;
  TbBlk blk[8][3];
  size_t o_mr[8], o_ssx[4];                  // feature extractor: (mean, rstd) tables 3 conv1, 4..6 branches, 7 fusion; o_ssx[3] = conv1's (scale, shift)
  size_t o_dA, o_dB, o_dC, o_dqkv, o_dattc, o_dprojc, o_dfeat, o_dcat, o_d32a, o_d32b;
  size_t o_part, o_bpart, o_coef, o_wslab, o_wd, o_wt, o_tmpw, o_dpool_f, o_dpool_e, o_cat64;
  size_t bytes;
};
struct TbCtx {
  LoTeacher* h; float* P; void* ws; void* bws; float* G; hipStream_t st; TbPlan pl;
  LoDropCfg d; float gscale, inv_g;
  int frozen = 0;                         // 1: eval mode -- every BatchNorm with its running statistics, differentiated as constants
  const LoImgSeed* seed = nullptr;        // lo_teacher_eval_backward_seed: the image data gradient stores dx_factor * (d / dx) + seed->c (x - seed->target)
  float dx_factor = 1.0f;
  LoGeom d1a, d1b, dq, dpc, dsc;          // data gradients of a block's conv 128->F, conv F->F, qkv, proj on the compact rows, shortcut
};
// BatchNorm backward of one layer: upstream din -> gradient wrt the conv output (out), parameter gradients into G (dbias: the bias
// gradient of the conv in front).  A view = C channels of a [pix][pitch] tensor from channel `off`.  frozen (default: the call's mode,
// TbCtx::frozen): statistics are constants, out = gamma rstd ls g slope.  Without a gradient buffer (TbCtx::G null, frozen only) the
// layer is ONE streaming pass; tail_y set, that pass is also the ExpertBlock tail in front of it: din.p = dy (null: the broadcast of
// tail_dpool) and tail_ds receives dS = dy slope(y), the value the BatchNorm then reads
struct TbView { const f16* p; int pitch, off = 0; };
struct TbViewOut { f16* p; int pitch, off = 0; };
enum TbAct { TB_ACT_NONE = 0, TB_ACT_LRELU = 1 };                          // TbBnArgs::act: the stored tensor is LeakyReLU(conv)
enum TbDropMode { TB_DROP_NONE = 0, TB_DROP_2D = 1, TB_DROP_ELEM = 2 };    // TbBnArgs::dmode: Dropout2d (index b*C + c), Dropout (pix*idx_pitch + idx_off + c)
struct TbDrop { int mode = TB_DROP_NONE; uint32_t site = 0; int idx_pitch = 0, idx_off = 0; };   // behind the BatchNorm; off when the call has no dropout
struct TbBnBwd {
  TbView din, raw; const float* mr; const TBnOff& bn; const float* ls = nullptr; float* dls = nullptr;
  TbViewOut out; int C; int act = TB_ACT_NONE; TbDrop drop = {}; float* dbias = nullptr;
  const f16* tail_y = nullptr; const float* tail_dpool = nullptr; f16* tail_ds = nullptr;
};
int tb_bn_backward(TbCtx& c, const TbBnBwd& op);
// backward of ExpertBlock (e, l): scratch holds its recomputation; y = the block output, dy / dpool = its gradient.
// dx_out = gradient wrt the block input (conv1's data gradient + the identity branch's)
int tb_block_backward(TbCtx& c, int e, int l, const f16* xin, const f16* y, const f16* dy, const float* dpool, f16* dx_out);
