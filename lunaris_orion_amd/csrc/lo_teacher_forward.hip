// Teacher forward executor: the feature extractor forward and the plain ExpertBlock forward (both shared with the full-backward mode,
// lo_teacher_bwd.hip), and lo_teacher_forward, which picks one of four block forms per call.
#include "lo_teacher.h"
#include "lo_conv.h"

// feature extractor (lunar_evaluator.py:105-112) from the images x into the tensors of t
int t_fe_forward(LoTeacher* h, const float* x, float* P, void* ws, int train, const LoDropCfg& d, bool fold, const TFeDst& t,
                 const TFeNames& nm, hipStream_t st) {
  const TFeOff& fe = h->fe;
  const int B = h->B;
  const size_t px = (size_t)B * T_HW;
  float* bnp = TW(float, h->o_bnp);
  LoConvExtra ex{1, bnp};
  {
    TOptScope _p(nm.conv1, 2.0 * px * 32 * 27, 0, st);
    LO_TRYT(t_conv1(x, TP(fe.conv1_w), TP(fe.conv1_b), t.raw32, bnp, B, st));
  }
  // the depthwise convs read BN(conv1) through its (scale, shift): kept in a private slot, the shared one is reused below
  LO_TRYT(t_bn_finalize(h, P, ws, {.partial = bnp, .nrow = B * 128, .C = 32, .bn = fe.bn1, .training = train, .ss_dst = t.ss32, .mr = t.mr32}, st));
  float* ss_cat = TW(float, h->o_ss_cat);
  for (int b = 0; b < 3; ++b) {
    const TBranchOff& br = fe.br[b];
    {
      TOptScope _p(b == 1 ? nm.dw5 : nm.dw3, 0, 4.0 * px * 32, st);
      LO_TRYT(t_dwconv(b == 1 ? 5 : 3, t.raw32, t.ss32, TP(br.dw_w), TP(br.dw_b), t.dw[b], B, st));
    }
    // the pointwise conv writes its (LeakyReLU'd, not yet normalised) 64 channels straight into the concatenated tensor
    LoConvExtra exb{1, bnp, 192, 64 * b};
    const LoConvOp pw{.in = t.dw[b], .w = TW(f16, h->o_wpw[b]), .bias = TP(br.pw_b), .out = t.cat, .ex = &exb};
    LoConvChoice ch;
    LO_TRYT(lo_conv_run(h->gpw, pw, st, &ch));
    LO_TRYT(t_bn_finalize(h, P, ws, {.partial = bnp, .nrow = ch.rows, .C = 64, .bn = br.bn, .training = train, .ss_dst = ss_cat + 128 * b,
                                     .mr = t.mr_br[b]}, st));
  }
  LoConvOp fus{.out = t.rawF, .ex = &ex};
  if (fold) {
    // the branch BatchNorms fold into the fusion conv (see lo_t_fold_fusion_kernel)
    LO_TRYT(t_fold_fusion(TP(fe.fus_w), TP(fe.fus_b), ss_cat, TW(f16, h->o_wfus_fold), TW(float, h->o_bfus_fold), st));
    fus.in = t.cat; fus.w = TW(f16, h->o_wfus_fold); fus.bias = TW(float, h->o_bfus_fold);
  } else {
    // Dropout sits between the branch BatchNorms and the fusion conv (lunar_evaluator.py:108-111): normalise + drop, in place -- on a
    // copy where the raw tensor is kept
    f16* catd = t.cat;
    if (t.catd) {
      LO_HIP(hipMemcpyAsync(t.catd, t.cat, px * 192 * 2, hipMemcpyDeviceToDevice, st));
      catd = t.catd;
    }
    {
      TOptScope _p(nm.cat_bn_drop, 0, 4.0 * px * 192, st);
      LO_TRYT(t_cat_bn_drop(catd, ss_cat, px * 24, d.site(LO_DS_FE), d.thr, d.inv_keep, st));
    }
    fus.in = catd; fus.w = TW(f16, h->o_wfus); fus.bias = TP(fe.fus_b);
  }
  LoConvChoice ch;
  LO_TRYT(lo_conv_run(h->gfus, fus, st, &ch));
  LO_TRYT(t_bn_finalize(h, P, ws, {.partial = bnp, .nrow = ch.rows, .C = 128, .bn = fe.bn_fus, .training = train, .mr = t.mr_fus}, st));
  return t_bn_apply(h, ws, {.raw = t.rawF, .y = t.feat, .C = 128, .pool_partial = t.pool_partial, .y8 = t.feat8}, st);
}

// Plain form of an ExpertBlock (lunar_evaluator.py:260-275): every tensor at full resolution; the attention keeps the reference's "only
// 543 positions are ever written" behaviour through compact rows (attc / projc) + one expansion pass, which is also where proj_drop
// is applied
int t_block_plain(LoTeacher* h, float* P, void* ws, int e, int l, const LoDropCfg& d, const TBlkT& t, const f16* xin, f16* xout, int train,
                  float* pool_partial, const TBlkNames& nm, hipStream_t st, const TBlk8* f8) {
  const TBlockOff& k = h->blk[e][l];
  const int B = h->B, F = h->F;
  const size_t px = (size_t)B * T_HW;
  float* bnp = TW(float, h->o_bnp);
  LoConvExtra ex{1, bnp};
  const LoGeom& g1 = l == 0 ? h->g3a : h->g3b;
  const bool sc = F != 128 && l == 0;
  LoConvChoice ch;     // of the launch that just ran: its BatchNorm partial rows
  if (sc) {
    // shortcut = BatchNorm(Conv1x1(x)) (in_channels 128 != out_channels F): raw output + its (scale, shift), applied in the tail
    LoConvExtra exs{0, bnp};
    const LoConvOp op{.in = xin, .w = TW(f16, h->o_wsc[e]), .bias = TP(k.sc_b), .out = t.scraw, .ex = &exs};
    LO_TAGGED(nm.shortcut, lo_conv_run(h->gsc, op, st, &ch));
    LO_TRYT(t_bn_finalize(h, P, ws, {.partial = bnp, .nrow = ch.rows, .C = F, .bn = k.bn_sc, .training = train, .ss_dst = t.ssS, .mr = t.mrS}, st));
  }
  const LoConvOp c1{.in = xin, .w = TW(f16, h->o_wp3[e][l][0]), .bias = TP(k.conv1_b), .out = t.rawA, .ex = &ex};
  const bool c1_f8 = f8 && f8->xin8 && f8->w8[0], c2_f8 = f8 && f8->a28 && f8->w8[1];
  if (c1_f8) LO_TAGGED(nm.conv1, lo_conv_run_f8(g1, f8->xin8, f8->w8[0], f8->ws8[0], c1, st, &ch));
  else LO_TAGGED(nm.conv1, lo_conv_run(g1, c1, st, &ch));
  LO_TRYT(t_bn_finalize(h, P, ws, {.partial = bnp, .nrow = ch.rows, .C = F, .bn = k.bn1, .training = train, .mr = t.mrA}, st));
  if (d.on) LO_TRYT(t_drop2d(h, ws, F, d, LO_DS_BLOCK(e, l, 0), st));
  LO_TRYT(t_bn_apply(h, ws, {.raw = t.rawA, .y = t.bnA, .C = F, .per_sample = d.on}, st));
  LO_TAGGED(nm.qkv, lo_conv_run(h->gqF, {.in = t.bnA, .w = TW(f16, h->o_wqkv[e][l]), .bias = TP(k.qkv_b), .out = t.qkv}, st));
  {
    TOptScope _p(nm.attn, 0, 0, st);
    LO_TRYT(t_attn_generic(F, t.qkv, t.attc, B, d.site(LO_DS_BLOCK(e, l, 1)), d.thr, d.inv_keep, st));
  }
  LO_TAGGED(nm.proj, lo_conv_run(h->gpc, {.in = t.attc, .w = TW(f16, h->o_wproj[e][l]), .bias = TP(k.proj_b), .out = t.projc}, st));
  {
    TOptScope _p(nm.projdrop, 0, 2.0 * px * F, st);
    LO_TRYT(t_projdrop(F, t.projc, TP(k.proj_b), t.a2, c2_f8 ? f8->a28 : nullptr, px * (F / 8), d.site(LO_DS_BLOCK(e, l, 2)), d.thr, d.inv_keep, st));
  }
  const LoConvOp c2{.in = t.a2, .w = TW(f16, h->o_wp3[e][l][1]), .bias = TP(k.conv2_b), .out = t.rawB, .ex = &ex};
  if (c2_f8) LO_TAGGED(nm.conv2, lo_conv_run_f8(h->g3b, f8->a28, f8->w8[1], f8->ws8[1], c2, st, &ch));
  else LO_TAGGED(nm.conv2, lo_conv_run(h->g3b, c2, st, &ch));
  LO_TRYT(t_bn_finalize(h, P, ws, {.partial = bnp, .nrow = ch.rows, .C = F, .bn = k.bn2, .training = train, .mr = t.mrB}, st));
  if (d.on) LO_TRYT(t_drop2d(h, ws, F, d, LO_DS_BLOCK(e, l, 3), st));
  // a block output that feeds nothing but the global average pool is only summed (xout null); a caller that wants neither skips the tail
  if (xout || pool_partial)
    LO_TRYT(t_bn_apply(h, ws, {.raw = t.rawB, .ls = TP(k.layer_scale), .identity = sc ? t.scraw : xin, .y = xout, .C = F, .mode = T_BN_TAIL,
                               .pool_partial = pool_partial, .per_sample = d.on, .y8 = f8 && xout ? f8->xout8 : nullptr,
                               .id_ss = sc ? t.ssS : nullptr}, st));
  return LO_OK;
}

// feature_dim 256 / 512 (README High-End recipe) inside lo_teacher_forward: the plain form with its tensors in the workspace
static int t_block_wide(const TFwd& c, int e, int l) {
  LoTeacher* h = c.h; void* ws = c.ws;
  const TBlkT t{TW(f16, h->o_rawA), TW(f16, h->o_bnA), TW(f16, h->o_qkv), TW(f16, h->o_attc), TW(f16, h->o_projc), TW(f16, h->o_proj), TW(f16, h->o_rawB),
                TW(f16, h->o_sc), nullptr, nullptr, nullptr, TW(float, h->o_ss_sc)};
  static const TBlkNames nm{"t_shortcut (igemm)", "t_conv1 (generic)", "t_qkv (igemm)", "t_proj (igemm)", "t_conv2 (generic)", "lo_t_attn (generic)", "lo_t_projdrop"};
  const f16* xin = l == 0 ? TW(f16, h->o_feat) : TW(f16, ((l - 1) & 1) ? h->o_x1 : h->o_x0);
  // the last block's output feeds nothing but the global average pool: a statistics-only call skips its tail, a full call only sums it
  f16* xout = l < 2 ? TW(f16, (l & 1) ? h->o_x1 : h->o_x0) : nullptr;
  float* poolp = (l == 2 && !c.stats_only) ? TW(float, h->o_poolp) : nullptr;
  if (!c.f8) return t_block_plain(h, c.P, ws, e, l, c.d, t, xin, xout, c.training, poolp, nm, c.st);
  // fp8 mode: conv1 reads the e4m3 copy of its input (feat8, or the y8 of the previous tail), conv2 the e4m3 output of proj_drop
  const bool c1 = l == 0 ? h->fp8a : h->fp8b, c2 = h->fp8b;
  TBlkNames nm8 = nm;
  if (c1) nm8.conv1 = "t_conv1 (generic, e4m3)";
  if (c2) nm8.conv2 = "t_conv2 (generic, e4m3)";
  const TBlk8 f8{c1 ? (l == 0 ? TW(uint8_t, h->o_feat8) : TW(uint8_t, h->o_x8[(l - 1) & 1])) : nullptr, c2 ? TW(uint8_t, h->o_proj8) : nullptr,
                 (l < 2 && h->fp8b) ? TW(uint8_t, h->o_x8[l & 1]) : nullptr,
                 {c1 ? TW(uint8_t, h->o_w8[e][l][0]) : nullptr, c2 ? TW(uint8_t, h->o_w8[e][l][1]) : nullptr},
                 {TW(float, h->o_ws8[e][l][0]), TW(float, h->o_ws8[e][l][1])}};
  return t_block_plain(h, c.P, ws, e, l, c.d, t, xin, xout, c.training, poolp, nm8, c.st, &f8);
}

// what must be zero once per workspace: rows / positions that no kernel ever writes
static int t_zero_once(LoTeacher* h, void* ws, hipStream_t st) {
  if (h->att_zeroed && h->att_zeroed_ws == ws) return LO_OK;
  const int B = h->B;
  LO_HIP(hipMemsetAsync(TW(void, h->o_att), 0, (size_t)B * T_HW * 128 * 2, st));   // positions >= 543 are never written again
  LO_HIP(hipMemsetAsync(TW(void, h->o_Z), 0, (size_t)B * 1024 * 1088 * 2, st));    // rows >= 543 of every sample stay zero
  LO_HIP(hipMemsetAsync(TW(void, h->o_qin), 0, (size_t)h->qrows * 128 * 2, st));
  if (h->F != 128) LO_HIP(hipMemsetAsync(TW(void, h->o_attc), 0, (size_t)B * 1024 * h->F * 2, st));   // rows >= 543 of every sample stay zero
  h->att_zeroed = true; h->att_zeroed_ws = ws;
  return LO_OK;
}

// x: fp32 NCHW images.  P: flat state (parameters AND BatchNorm running statistics; the latter are updated in place when
// training != 0).  outputs: quality_scores [B,4], expert_weights [B,E], style/prompt embeddings [B,emb], semantic [B,1].
// dropout_p / drop_seed: train mode applies the reference's six dropout sites with probability dropout_p from the counter RNG
// stream drop_seed (lo_common.h); the constant-field shortcuts of the sparse path do not survive proj_drop, so that call runs
// every convolution in full (path 2).  Eval mode, or dropout_p = 0: no dropout, sparse path.
extern "C" int lo_teacher_forward(LoTeacher* h, const float* x, float* P, void* ws, int training, float dropout_p, uint64_t drop_seed,
                                  float* quality, float* weights, float* style, float* prompt, float* semantic, void* stream) {
  // all five output pointers null = statistics-only call: everything that feeds a BatchNorm layer runs (the running
  // statistics are the call's side effect), the pooling of the last block and the heads do not.  This is the first
  // teacher call of _process_batch (train_hybrid.py:853-855), whose outputs the reference overwrites before use.
  const bool stats_only = !quality && !weights && !style && !prompt && !semantic;
  LO_REQUIRE(h && x && P && ws && (stats_only || (quality && weights && style && prompt && semantic)), "lo_teacher_forward: null argument");
  LO_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "lo_teacher_forward: dropout_p %g outside [0, 1)", (double)dropout_p);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int B = h->B, F = h->F;
  const LoDropCfg d = lo_drop_cfg(training ? dropout_p : 0.f, drop_seed);
  LO_REQUIRE(!d.on || (size_t)B * T_HW * (size_t)(F > 192 ? F : 192) <= 0xFFFFFFFFull,
             "lo_teacher_forward: batch %d x feature_dim %d exceeds the 32-bit element index of the dropout mask generator", B, F);
  h->last_p = d.on ? dropout_p : 0.f; h->last_seed = drop_seed;
  h->last_path = d.on ? 2 : (h->sparse && F == 128 ? 0 : 1);
  // f8: e4m3 operands in the 24 3x3 convolutions -- feature_dim 128: of the dropout path; 256 / 512: of every train-mode call
  const TFwd c{h, P, ws, st, training, d, stats_only, h->fp8 && (F == 128 ? d.on : training != 0)};
  LO_TRYT(t_zero_once(h, ws, st));
  // ---- feature extractor: the branch BatchNorms fold into the fusion conv unless dropout sits between them
  const TFeDst fd{TW(f16, h->o_raw32), {TW(f16, h->o_dw), TW(f16, h->o_dw), TW(f16, h->o_dw)}, TW(f16, h->o_cat), nullptr, TW(f16, h->o_rawA), TW(f16, h->o_feat),
                  c.f8 && (F == 128 || h->fp8a) ? TW(uint8_t, h->o_feat8) : nullptr, TW(float, h->o_ss) + 2 * T_FMAX + 2 * 192, nullptr, {nullptr, nullptr, nullptr}, nullptr,
                  TW(float, h->o_poolp)};
  static const TFeNames fe_names{"lo_t_conv1", "lo_t_dwconv<3>", "lo_t_dwconv<5>", "lo_t_cat_bn_drop"};
  LO_TRYT(t_fe_forward(h, x, P, ws, training, d, !d.on, fd, fe_names, st));
  LO_TRYT(t_pool(h, TW(float, h->o_pool_f), 128, ws, st));
  // ---- experts (lunar_evaluator.py:260-275, 422-428): one block form per call
  h->kept = false;                      // whatever lo_teacher_forward_keep left in a backward scratch no longer belongs to the last forward
  int (*block)(const TFwd&, int, int) = F != 128 ? t_block_wide : (h->last_path == 2 ? t_block_dropout : (h->last_path == 0 ? t_block_sparse : t_block_dense));
  const bool fused_pool = block == t_block_sparse && h->fuse_tail;
  // per-expert pooling of x_3 from the last tail's partial sums: not with the fused tail (pooled below, for all experts at once), and
  // not where a statistics-only call has skipped that tail
  const bool pool_each = (block == t_block_sparse || block == t_block_dense) ? !fused_pool : !stats_only;
  for (int e = 0; e < h->E; ++e) {
    for (int l = 0; l < 3; ++l) LO_TRYT(block(c, e, l));
    if (pool_each) LO_TRYT(t_pool(h, TW(float, h->o_pool_e) + (size_t)e * B * F, F, ws, st));
  }
  if (stats_only) return LO_OK;
  if (fused_pool) LO_TRYT(t_pool_fused(c));
  // ---- heads (lunar_evaluator.py:417, 425, 431-449)
  return t_run_heads(h, P, ws, quality, weights, style, prompt, semantic, d, st);
}

// the keep decisions of one dropout site as bytes (what lo_teacher_forward applies for this call seed): checked bit for bit
// against oracle/dropout_ref.py by the tests
__global__ void lo_dropout_mask_kernel(uint8_t* __restrict__ keep, size_t n, LoDropSite ds, uint32_t thr) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) keep[i] = lo_drop_keep(ds, (uint32_t)i, thr) ? 1 : 0;
}
extern "C" int lo_dropout_mask(uint64_t drop_seed, int site, float dropout_p, size_t n, uint8_t* keep, void* stream) {
  LO_REQUIRE(keep && site >= 0 && dropout_p > 0.f && dropout_p < 1.f && n < ((size_t)1 << 32), "lo_dropout_mask: bad argument");
  const LoDropCfg d = lo_drop_cfg(dropout_p, drop_seed);
  hipLaunchKernelGGL(lo_dropout_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), keep, n,
                     d.site((uint32_t)site), d.thr);
  LO_LAUNCH_CHECK("dropout_mask");
  return LO_OK;
}
