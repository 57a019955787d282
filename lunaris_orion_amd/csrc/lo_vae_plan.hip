// VAE step executor: the plan (parameter table, workspace layout, which kernels own which layer), create / destroy and the queries.
#include "lo_vae.h"
#include <memory>

namespace {
struct Arena {
  size_t off = 0;
  size_t take(size_t bytes) {
    size_t o = off;
    off += (bytes + 255) & ~(size_t)255;
    return o;
  }
};
bool env_is_zero(const char* v) { return v && atoi(v) == 0; }      // v: what getenv gave for a knob whose "0" turns a default off
const int kEncCh[5] = {3, 64, 128, 256, 512};
const int kDecCh[5] = {512, 256, 128, 64, 32};
}  // namespace

// The ONE place that decides whether a layer's forward conv takes e4m3 operands in the fp8 mode: the e4m3 implicit GEMM covers the
// geometry (Cin % 128 == 0, Cout % 64 == 0) and no patch-resident fp16 kernel owns the layer (the 128 -> 64 transposed conv)
static bool layer_takes_f8(const LoGeom& gf) {
  if (lo_conv_choose(gf, {.bias = true, .gn_partial = true, .f8 = true}).kernel == LO_CK_NONE) return false;
  return lo_conv_choose(gf, {.bias = true, .gn_partial = true}).kernel != LO_CK_CONVT4_PATCH;
}

static int setup_conv_layer(ConvLayer& c, int kind, int B, int H, int W, int Cin, int Cout, int p_w, Arena& ar, bool first, bool fp8_fwd) {
  c.kind = kind; c.H = H; c.W = W; c.Cin = Cin; c.Cout = Cout;
  c.p_w = p_w; c.p_b = p_w + 1; c.p_gw = p_w + 2; c.p_gb = p_w + 3;
  if (!first) {
    LO_TRY(lo_make_geom(&c.gf, kind, B, H, W, Cin, Cout));
    int dk = kind == LO_CONV3_S1 ? LO_CONV3_S1_DGRAD : (kind == LO_CONV3_S2 ? LO_CONV3_S2_DGRAD : LO_CONVT4_S2_DGRAD);
    c.Ho = c.gf.Hout; c.Wo = c.gf.Wout;
    // the data-gradient op READS the forward output tensor [B,Ho,Wo,Cout] and WRITES Cin channels
    LO_TRY(lo_make_geom(&c.gd, dk, B, c.Ho, c.Wo, Cout, Cin));
    c.o_wp_f = ar.take(lo_packed_weight_elems(c.gf) * 2);
    c.o_wp_d = ar.take(lo_packed_weight_elems(c.gd) * 2);
    // partial-sum rows per sample of conv_gn's launch (lo_vae_step.hip), asked with the use that launch really has: the e4m3 launch
    // runs lo_igemm_nt's tiles whatever fp16 kernel owns the geometry (conv_gn checks the count against the launch's own answer)
    c.f8 = fp8_fwd && layer_takes_f8(c.gf);
    c.MT = lo_conv_choose(c.gf, {.bias = true, .gn_partial = true, .f8 = c.f8}).mts;
  } else {
    c.Ho = H / 2; c.Wo = W / 2;
    c.MT = 64;
  }
  size_t act = (size_t)B * c.Ho * c.Wo * Cout * 2;
  c.o_v = ar.take(act);
  c.o_a = ar.take(act);
  c.o_part = ar.take((size_t)B * c.MT * 16 * 4);
  c.o_stats = ar.take((size_t)B * 16 * 4);
  int nchunk = lo_gn_nchunk(c.Ho * c.Wo, Cout);
  c.prow_cap = nchunk > (c.Ho * c.Wo) / 64 ? nchunk : (c.Ho * c.Wo) / 64;   // >= tiles per sample of any data-gradient epilogue
  c.o_P1 = ar.take((size_t)B * c.prow_cap * Cout * 2 * 4);
  c.o_P2 = ar.take((size_t)B * c.prow_cap * Cout * 4);     // nchunk rows (lo_gn_bwd_apply) or one row per tile (fused apply)
  c.o_dv = ar.take(act);
  c.o_xbuf = ar.take((size_t)B * LO_GNF_MAX_TILES * 128);
  c.o_xcnt = ar.take((size_t)B * 4);
  c.o_bcnt = ar.take((size_t)B * 8 * 4);
  return LO_OK;
}

// parameter table in state_dict order (lunar_generate.py:91-125, 162-192); returns the index of the decoder's first conv weight
static int plan_parameters(LoVae* h) {
  const int L = h->L;
  std::vector<size_t>& numel = h->p_numel;
  for (int s = 0; s < 4; ++s) {
    size_t ci = kEncCh[s], co = kEncCh[s + 1];
    numel.push_back(co * ci * 9); numel.push_back(co); numel.push_back(co); numel.push_back(co);
    for (int k = 0; k < 2; ++k) { numel.push_back(co * co * 9); numel.push_back(co); numel.push_back(co); numel.push_back(co); }
  }
  // SelfAttention2d(512) in state_dict order: the module's own parameter (gamma) first, then the three 1x1 convs (weight, bias)
  auto push_attn = [&](LoAttnSite& a) {
    if (!h->attn) return;
    a.p_gamma = (int)numel.size(); numel.push_back(1);
    a.p_w = (int)numel.size(); a.p_b = a.p_w + 1;
    numel.push_back(64 * 512); numel.push_back(64);
    numel.push_back(64 * 512); numel.push_back(64);
    numel.push_back(512 * 512); numel.push_back(512);
  };
  push_attn(h->att[0]);
  h->idx_fc_mu_w = (int)numel.size(); numel.push_back((size_t)L * 32768);
  h->idx_fc_mu_b = (int)numel.size(); numel.push_back(L);
  h->idx_fc_lv_w = (int)numel.size(); numel.push_back((size_t)L * 32768);
  h->idx_fc_lv_b = (int)numel.size(); numel.push_back(L);
  h->idx_dfc_w = (int)numel.size(); numel.push_back((size_t)32768 * L);
  h->idx_dfc_b = (int)numel.size(); numel.push_back(32768);
  push_attn(h->att[1]);
  const int dec_first = (int)numel.size();
  for (int s = 0; s < 4; ++s) {
    size_t ci = kDecCh[s], co = kDecCh[s + 1];
    numel.push_back(ci * co * 16); numel.push_back(co); numel.push_back(co); numel.push_back(co);
  }
  h->idx_final_w = (int)numel.size(); numel.push_back(3 * 32 * 9);
  h->idx_final_b = (int)numel.size(); numel.push_back(3);
  h->nparam = (int)numel.size();
  h->p_off.assign(h->nparam, 0);
  // flat layout: state_dict order, except that fc_logvar.weight directly follows fc_mu.weight and the two head
  // biases are adjacent, so the encoder head is ONE [2L, 32768] matrix; every tensor starts on a 64-element boundary.
  // An attention site is gamma | Wq | Wk | Wv | bq | bk | bv (the three weights one [640][512] matrix, the biases one [640] vector: all
  // multiples of 64, no padding between them).  The encoder's site sits before fc_mu.weight -- inside the encoder range, which the
  // serial norm tail and the optimizer's stage-4 level cover -- and the decoder's behind decoder.fc.bias, inside "everything behind
  // decoder.fc.weight" of the early norm and the optimizer's decoder level: no range of lo_vae_opt.hip / early_norm needs a new case.
  size_t off = 0;
  auto place = [&](int i) { h->p_off[i] = off; off += (numel[i] + 63) & ~(size_t)63; };
  auto place_attn = [&](const LoAttnSite& a) {
    if (!h->attn) return;
    place(a.p_gamma);
    for (int k = 0; k < 3; ++k) place(a.p_w + 2 * k);
    for (int k = 0; k < 3; ++k) place(a.p_b + 2 * k);
  };
  auto in_attn = [&](int i) { return h->attn && ((i >= h->att[0].p_gamma && i < h->att[0].p_gamma + 7) || (i >= h->att[1].p_gamma && i < h->att[1].p_gamma + 7)); };
  for (int i = 0; i < h->nparam; ++i) {
    if (i == h->idx_fc_mu_b || i == h->idx_fc_lv_w || i == h->idx_fc_lv_b || in_attn(i)) continue;
    if (i == h->idx_fc_mu_w) place_attn(h->att[0]);
    place(i);
    if (i == h->idx_fc_mu_w) { place(h->idx_fc_lv_w); place(h->idx_fc_mu_b); place(h->idx_fc_lv_b); }
    if (i == h->idx_dfc_b) place_attn(h->att[1]);
  }
  h->flat_elems = off;
  return dec_first;
}

// workspace plan, forward part: the conv layers with everything they own, the skip maps, the latent
static int plan_forward_buffers(LoVae* h, Arena& ar, int dec_first) {
  const int B = h->B, L = h->L;
  int Hs = 128;
  int pidx = 0;
  for (int s = 0; s < 4; ++s) {
    int ci = kEncCh[s], co = kEncCh[s + 1];
    LO_TRY(setup_conv_layer(h->enc[s][0], LO_CONV3_S2, B, Hs, Hs, ci, co, pidx, ar, s == 0, h->fp8_fwd));
    pidx += 4;
    Hs /= 2;
    LO_TRY(setup_conv_layer(h->enc[s][1], LO_CONV3_S1, B, Hs, Hs, co, co, pidx, ar, false, h->fp8_fwd));
    pidx += 4;
    LO_TRY(setup_conv_layer(h->enc[s][2], LO_CONV3_S1, B, Hs, Hs, co, co, pidx, ar, false, h->fp8_fwd));
    pidx += 4;
    h->o_eout[s] = ar.take((size_t)B * Hs * Hs * co * 2);
  }
  Hs = 8;
  for (int s = 0; s < 4; ++s) {
    LO_TRY(setup_conv_layer(h->dec[s], LO_CONVT4_S2, B, Hs, Hs, kDecCh[s], kDecCh[s + 1], dec_first + 4 * s, ar, false, h->fp8_fwd));
    Hs *= 2;
  }
  for (int k = 0; k < 3; ++k) h->o_skipin[k] = ar.take((size_t)B * (64 >> k) * (64 >> k) * (64 << k) * 2);
  // latent
  LO_TRY(lo_make_geom(&h->g_head, LO_LINEAR, B, 1, 1, 32768, 2 * L));     // [mu|logvar] = xflat W^T
  LO_TRY(lo_make_geom(&h->g_head_d, LO_LINEAR, B, 1, 1, 2 * L, 32768));   // dxflat = dml Wt^T  (Wt = W^T packed)
  LO_TRY(lo_make_geom(&h->g_dfc, LO_LINEAR, B, 1, 1, L, 32768));          // y = z Wd^T
  LO_TRY(lo_make_geom(&h->g_dfc_d, LO_LINEAR, B, 1, 1, 32768, L));        // dz = dy Wdt^T
  h->o_wp_head = ar.take((size_t)2 * L * 32768 * 2);
  h->o_wp_head_t = ar.take((size_t)2 * L * 32768 * 2);
  h->o_wp_dfc = ar.take((size_t)L * 32768 * 2);
  h->o_wp_dfc_t = ar.take((size_t)L * 32768 * 2);
  h->o_xflat = ar.take((size_t)B * 32768 * 2);
  h->o_slab_head = ar.take((size_t)h->head_split * B * 2 * L * 4);
  h->o_eps = ar.take((size_t)B * L * 4);
  h->o_mu = ar.take((size_t)B * L * 4);
  h->o_lv = ar.take((size_t)B * L * 4);
  h->o_z = ar.take((size_t)B * L * 2);
  h->o_klp = ar.take((size_t)((B * L + 255) / 256) * 4);
  h->o_yfc = ar.take((size_t)B * 32768 * 2);
  h->o_h0 = ar.take((size_t)B * 32768 * 2);
  h->o_msep = ar.take((size_t)B * 64 * 4);
  h->o_losses = ar.take(16 * 4);
  h->o_coefs = ar.take(16 * 4);
  return LO_OK;
}

// workspace plan, backward part: gradient ping-pong buffers, slabs, job tables, the Linear layers' factors
static void plan_backward_buffers(LoVae* h, Arena& ar) {
  const int B = h->B, L = h->L;
  size_t max_act = (size_t)B * 128 * 128 * 32 * 2;
  for (int i = 0; i < 4; ++i) h->o_G[i] = ar.take(max_act);
  h->o_skipg[0] = ar.take((size_t)B * 64 * 64 * 64 * 2);    // grad wrt (up3.act + enc1.out)
  h->o_skipg[1] = ar.take((size_t)B * 32 * 32 * 128 * 2);   // grad wrt (up2.act + enc2.out)
  h->o_skipg[2] = ar.take((size_t)B * 16 * 16 * 256 * 2);   // grad wrt (up1.act + enc3.out)
  h->o_P1 = ar.take((size_t)B * 64 * 512 * 2 * 4);
  h->o_P2 = ar.take((size_t)B * 64 * 512 * 4);
  size_t wslab = 0;
  for_each_layer(h, [&](ConvLayer& c) {
    if (&c == &h->enc[0][0]) return;
    size_t b = lo_wgrad_slab_bytes(c.gf);
    wslab = b > wslab ? b : wslab;
  });
  h->o_wslab = ar.take(wslab);
  // The two Linear weight gradients run on the MAIN stream while the decoder's conv weight gradients may still be running on
  // the side stream: they get their own slab.  (Found by the buffer audit of round 2: at latent 512 / 256 both Linear
  // gradients are written directly and never touch a slab, but at latent 64 / 128 lo_wgrad_choose() gives decoder.fc two
  // pixel splits, and sharing o_wslab with the side stream was a write-write race on those shapes.)
  size_t b = lo_wgrad_slab_bytes(h->g_head), b2 = lo_wgrad_slab_bytes(h->g_dfc);
  h->o_wslab_lin = ar.take(b > b2 ? b : b2);
  h->o_fcw_part = ar.take((size_t)B * 16 * 1728 * 4);
  h->o_lc_part = ar.take((size_t)B * 64 * 867 * 4);
  h->o_dz = ar.take((size_t)B * L * 2);
  h->o_dml = ar.take((size_t)B * 2 * L * 2);
  h->o_gfc = ar.take((size_t)B * 32768 * 2);    // dy of decoder.fc, channel-major: its own buffer (the side-stream weight gradient reads it while the chain reuses Gb)
  h->o_slab_dz = ar.take((size_t)h->dfcd_split * B * L * 4);
  h->o_packjobs = ar.take(sizeof(LoPackJob) * 64);
  h->o_sync_fail = ar.take(256);
  h->Bp = lo_lowrank_bp(B);
  h->o_fac_dmlT = ar.take((size_t)2 * L * h->Bp * 2);
  h->o_fac_xT = ar.take((size_t)32768 * h->Bp * 2);
  h->o_fac_gfcT = ar.take((size_t)32768 * h->Bp * 2);
  h->o_fac_zT = ar.take((size_t)L * h->Bp * 2);
  h->o_gram = ar.take((size_t)2 * 128 * 128 * 4);
}

// few-rows convolutions as split-K GEMMs + a fused slab pass (LO_SPLITK_CONV=0: every convolution on its one-launch kernel), and the
// fp8 operand mode: every forward conv whose geometry the e4m3 igemm covers (Cin % 128 == 0: the 128 / 256 / 512 channel ResBlock
// and stride-2 convs, the 512 / 256 / 128 channel transposed convs) reads an e4m3 copy of its input, written by the kernel that
// produces the fp16 activation (which the backward still uses)
static void plan_splitk_and_fp8(LoVae* h, Arena& ar) {
  const int B = h->B;
  size_t slab = 0;
  if (!env_is_zero(getenv("LO_SPLITK_CONV")) && !h->fp8_fwd)
    for_each_layer(h, [&](ConvLayer& c) {
      if (&c == &h->enc[0][0]) return;
      c.sk_fwd = lo_conv_splitk_plan(c.gf);
      c.sk_dgrad = lo_conv_splitk_plan(c.gd);
      const size_t bf = (size_t)c.sk_fwd * B * c.gf.GH * c.gf.GW * c.gf.Cout * 4, bd = (size_t)c.sk_dgrad * B * c.gd.GH * c.gd.GW * c.gd.Cout * 4;
      slab = bf > slab ? bf : slab;
      slab = bd > slab ? bd : slab;
    });
  h->o_skslab = ar.take(slab > 0 ? slab : 256);
  if (!h->fp8_fwd) return;
  auto enable = [&](ConvLayer& c, size_t* producer_copy) {      // operands of an e4m3 layer: weights, scales, the producer's e4m3 copy of its input
    if (!c.f8) return;      // decided with the layer's row count (setup_conv_layer)
    c.o_wp8 = ar.take(lo_packed_weight_elems(c.gf));
    c.o_wscale = ar.take((size_t)c.gf.n_phase * c.Cout * 4);
    if (!*producer_copy) *producer_copy = ar.take((size_t)B * c.H * c.W * c.Cin);
  };
  for (int s = 0; s < 4; ++s) {
    if (s > 0) enable(h->enc[s][0], &h->o_eout8[s - 1]);
    enable(h->enc[s][1], &h->enc[s][0].o_a8);
    enable(h->enc[s][2], &h->enc[s][1].o_a8);
  }
  enable(h->dec[0], &h->o_h08);
  for (int s = 1; s < 4; ++s) enable(h->dec[s], &h->dec[s - 1].o_a8);
  h->o_packjobs8 = ar.take(sizeof(LoPackF8Job) * 32);
}

// bottleneck self-attention: the two GEMM geometries and, per site, the operand copies and the workspace of both directions
static int plan_attention(LoVae* h, Arena& ar) {
  if (!h->attn) return LO_OK;
  const int B = h->B;
  LO_TRY(lo_make_geom(&h->g_att_qkv, LO_LINEAR, B, 8, 8, 512, 640));     // qkv = x Wqkv^T + b
  LO_TRY(lo_make_geom(&h->g_att_dx, LO_LINEAR, B, 8, 8, 640, 512));      // dx = dy + dqkv Wqkv  (the transposed copy as the operand)
  for (LoAttnSite& a : h->att) {
    a.o_w = ar.take((size_t)640 * 512 * 2);
    a.o_wt = ar.take((size_t)640 * 512 * 2);
    a.o_qkv = ar.take((size_t)B * 64 * 640 * 2);
    a.o_y = ar.take((size_t)B * 64 * 512 * 2);
    a.o_dy = ar.take((size_t)B * 64 * 512 * 2);
    a.o_dqkv = ar.take((size_t)B * 64 * 640 * 2);
    a.o_dx = ar.take((size_t)B * 64 * 512 * 2);
    a.o_dgpart = ar.take((size_t)B * 4);
  }
  const size_t slab = lo_wgrad_slab_bytes(h->g_att_qkv);
  h->o_att_wslab = ar.take(slab > 0 ? slab : 256);
  return LO_OK;
}

// which GroupNorm passes are fused into conv epilogues
static void plan_gn_fusions(LoVae* h) {
  // GroupNorm-backward reduction fused into the producing data-gradient epilogue (+1.4 % on the step; LO_GNB_FUSE=0 runs the
  // separate reduction kernel).  The epilogue accumulates (sum du, sum du*v) and forms sum du*xhat = rstd * (sum du*v - mean *
  // sum du) after its store loop: the first version multiplied by xhat inside the loop, with mean / rstd live across it, and
  // was not bitwise reproducible while a weight-gradient kernel ran beside it (tools/gnb_det.py: 1365 mismatching tensors
  // in 24 runs; 0 with this form) -- the determinism tests of tests/test_fullsize_gpu.py and test_vae_gpu.py guard it
  h->fuse_gnb = !env_is_zero(getenv("LO_GNB_FUSE"));
  h->gn_local = !env_is_zero(getenv("LO_GN_LOCAL"));
  // GroupNorm + Mish in the conv epilogue (LO_GN_FUSE=1; the default is the separate lo_gn_fwd pass after every conv).  Built,
  // bitwise equal to the separate pass (tests/test_gn_fuse_gpu.py) and measured at batch 64 in two interleaved rounds: 20 403 /
  // 20 414 sprites/s against 20 821 / 20 859 -- 2 % SLOWER.  Per layer the fused conv launches take 7-22 us longer than before while
  // the passes they replace took 8-23 us: every workgroup of a sample waits for the slowest tile of that sample (on two-round grids
  // the second round starts staggered, so the skew of a whole round is paid twice), the hand-off is a chain of dependent memory
  // round trips (publish, count, poll, read the lines: ~5 us on an otherwise idle CU), and the Mish of the tile (25 VALU operations
  // per element) runs on 2 waves per SIMD with nothing to overlap it, where the separate pass spreads the same arithmetic over
  // every wave slot of the chip.  Which layers qualify is a property of the kernel lo_conv_run picks for the
  // geometry (LoConvChoice::gn_fuse); the fp8 operand mode keeps the separate pass (it also writes the e4m3 copy of the activation).
  h->fuse_gnf = getenv("LO_GN_FUSE") && atoi(getenv("LO_GN_FUSE")) != 0 && !h->fp8_fwd;
  // ... and the backward's apply pass in the data-gradient epilogue of the consuming layer (LO_GNB_APPLY_FUSE=0: separate
  // lo_gn_bwd_apply launches); needs the fused reduction.  Same mechanism, but here it WINS (+0.8 %: 21 002 / 21 021 against
  // 20 821 / 20 859): the epilogue already holds the activation gradient and has read v for the reduction, so the apply pass it
  // removes (a read of dy and v, a write of dv: 12-27 us per layer) costs more than the wait, and dy is never stored at all
  h->fuse_gna = h->fuse_gnb && !env_is_zero(getenv("LO_GNB_APPLY_FUSE"));
  // Workgroups that wait for each other inside an ordinary launch (sample rendezvous) make progress only if every workgroup of the
  // grid can be resident: each fused kernel fits at least one workgroup per CU, workgroups of other kernels on the same CUs (the side
  // stream's weight gradients) finish without waiting for anybody, so a grid of at most one workgroup per compute unit OF THIS
  // DEVICE -- 256 in SPX mode, 32 on a CPX partition -- always drains.  The count is the device's own, not a constant.
  int dev = 0, ncu = 0;
  if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess) h->n_cu = ncu;
  else (void)hipGetLastError();
  if (h->n_cu < 256) h->fuse_gnf = false;      // the forward fusion's two-round rule (LoConvChoice::gn_fuse) was only ever checked on 256 CUs
  for_each_layer(h, [&](ConvLayer& c) {
    if (!h->fuse_gnf || &c == &h->enc[0][0] || c.sk_fwd) return;
    const LoConvChoice ch = lo_conv_choose(c.gf, {.bias = true, .gf = true});
    c.gnf = ch.gn_fuse; c.gnf_mts = ch.mts; c.gnf_nt = ch.nt;
  });
}

// The side stream carries work that has slack (weight gradients, the tail of the optimizer step, operand refresh); the
// caller's stream carries the dependent chain that decides the step time.  Lowest queue priority for the side stream: when both
// have workgroups ready, the dispatcher serves the chain first and the side work fills what it leaves (default priority was the
// round-1 behaviour).  Timeline before (tools/timeline.py): the first GroupNorm pass of a step took 302 us instead of
// 17 beside the side stream's AdamW, data-gradient launches 55-65 us instead of 36-44 beside the weight gradients.
// (A CU-masked side stream -- hipExtStreamCreateWithCUMask with 64 / 128 / 192 / all 256 bits set -- was tried in round 3 to
// fence the side work off: 10 300-12 700 sprites/s against 22 300 with ANY mask, the full one included, so the masked queue
// itself is the cost on this stack; what does help is fewer, longer side workgroups: see the multi-tap split policy in lo_wgrad.hip.)
static void create_side_stream(LoVae* h) {
  h->overlap = getenv("LO_NO_OVERLAP") == nullptr;
  if (!h->overlap) return;
  int prio_least = 0, prio_greatest = 0;
  bool ok;
  if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) == hipSuccess && prio_least != prio_greatest)
    ok = hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, prio_least) == hipSuccess;
  else
    ok = hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking) == hipSuccess;
  // every event below orders two streams of THIS device: no system-scope fence at the recording kernel's end (the flag only
  // gives up visibility to the host and to other devices).  +0.5 % on the step (23 872-23 941 against 23 761-23 789); ev_range
  // keeps the fence: behind it RCCL sends the range to other devices
  constexpr unsigned evf = hipEventDisableTiming | hipEventDisableSystemFence;
  for (int i = 0; i < 4 && ok; ++i)
    ok = hipEventCreateWithFlags(&h->ev_dv[i], evf) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&h->ev_range, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&h->ev_join, evf) == hipSuccess &&
       hipEventCreateWithFlags(&h->ev_pre, evf) == hipSuccess;
  for (int l = 1; l < 6 && ok; ++l) ok = hipEventCreateWithFlags(&h->ev_lvl[l], evf) == hipSuccess;
  if (!ok) { (void)hipGetLastError(); h->overlap = false; }   // no GPU in this process (CPU-side planning only)
}

extern "C" int lo_vae_create(int B, int L, LoVae** out) { return lo_vae_create_ex(B, L, 0u, out); }

extern "C" int lo_vae_create_ex(int B, int L, unsigned flags, LoVae** out) {
  LO_REQUIRE(out, "lo_vae_create: null out");
  LO_REQUIRE((flags & ~(unsigned)(LO_VAE_FP8_FWD | LO_VAE_ATTN)) == 0, "lo_vae_create_ex: unknown flag bits 0x%x", flags);
  LO_REQUIRE((flags & (LO_VAE_FP8_FWD | LO_VAE_ATTN)) != (LO_VAE_FP8_FWD | LO_VAE_ATTN),
             "lo_vae_create_ex: LO_VAE_ATTN cannot be combined with LO_VAE_FP8_FWD (up1 would read an e4m3 copy of the attention's output)");
  LO_REQUIRE(B >= 1 && B <= 4096, "lo_vae_create: batch %d out of range", B);
  LO_REQUIRE(L >= 64 && L % 64 == 0 && L <= 4096, "lo_vae_create: latent_dim %d must be a multiple of 64", L);
  std::unique_ptr<LoVae> h(new LoVae());      // freed again if the plan fails
  h->B = B; h->L = L;
  h->fp8_fwd = (flags & LO_VAE_FP8_FWD) != 0;
  h->attn = (flags & LO_VAE_ATTN) != 0;
  Arena ar;
  LO_TRY(plan_forward_buffers(h.get(), ar, plan_parameters(h.get())));
  plan_backward_buffers(h.get(), ar);
  plan_splitk_and_fp8(h.get(), ar);
  LO_TRY(plan_attention(h.get(), ar));
  h->ws_bytes = ar.off;
  plan_gn_fusions(h.get());
  create_side_stream(h.get());
  *out = h.release();
  return LO_OK;
}

extern "C" void lo_vae_destroy(LoVae* h) {
  if (!h) return;
  if (h->overlap) {
    (void)vae_flush_deferred(h, nullptr);     // an optimizer step must not be lost with its engine
    (void)hipStreamDestroy(h->side);
    for (int i = 0; i < 4; ++i) (void)hipEventDestroy(h->ev_dv[i]);
    (void)hipEventDestroy(h->ev_join); (void)hipEventDestroy(h->ev_pre); (void)hipEventDestroy(h->ev_range);
    for (int l = 1; l < 6; ++l) (void)hipEventDestroy(h->ev_lvl[l]);
  }
  delete h;
}
// Single-call backward only, and only when the side stream exists: once every gradient from fc_mu.weight to the end of the
// buffer is final (decoder weight gradients included), its sum of squares is taken on the side stream, beside the encoder
// backward, into scratch[512 .. 1024) -- lo_clip_adamw_step_presummed then reads just the encoder range (31 of 244 MB) on the
// critical path.  NULL turns it off (e.g. when the gradients are still to be exchanged between ranks).
extern "C" int lo_vae_set_gradnorm_scratch(LoVae* h, float* scratch) {
  LO_REQUIRE(h, "lo_vae_set_gradnorm_scratch: null handle");
  h->norm_scratch = scratch;
  return LO_OK;
}
extern "C" int lo_vae_gradnorm_presummed(const LoVae* h) { return h && h->norm_scratch && (vae_side_on(h) || vae_single_leaves_factors(h)); }
// Factored Linear-layer gradients (lo_lowrank.hip): with the mode on, a FUSED single-call lo_vae_backward does not write the weight
// gradients of fc_mu | fc_logvar and decoder.fc into flat_grads (those ranges keep whatever they held); it leaves their factors and
// their share of the gradient norm (needs lo_vae_set_gradnorm_scratch), and lo_vae_optimizer_step forms the gradient tiles inside
// its AdamW pass.  Batch <= 128.  Explicit-gradient (autograd) backwards and the phased data-parallel backward are not affected.
extern "C" int lo_vae_set_linear_factored(LoVae* h, int on) {
  LO_REQUIRE(h, "lo_vae_set_linear_factored: null handle");
  LO_REQUIRE(on >= 0 && on <= 3, "lo_vae_set_linear_factored: mode must be 0 (off), 1 (single process), 2 (data parallel: factors only) "
             "or 3 (data parallel: factored AdamW and norm from the gathered factors)");
  if (on) LO_REQUIRE(lo_lowrank_applies(h->B, 2 * h->L, 32768) && lo_lowrank_applies(h->B, 32768, h->L),
                     "lo_vae_set_linear_factored: batch %d is above the rank the factored update is built for (128)", h->B);
  h->lin_mode = (LoLinearMode)on;
  h->fac = LoFactorStep{};
  return LO_OK;
}
// Mode 3: the gathered blocks stay the only form of the two Linear weight gradients (block addressing: lo_vae.h)
extern "C" size_t lo_vae_gathered_scratch_bytes(const LoVae* h, int world) {
  if (!h || !lo_lowrank_gathered_applies(world, h->B)) return 0;
  return lo_lowrank_gathered_gram_elems(world, h->B) * sizeof(float);
}
// Gradient accumulation on one GPU: the k micro-batches of a window are k "ranks" that arrive one after the other, and their
// gradients -- each already carrying lo_vae_loss's 1 / accum -- are added, not averaged: on != 0 drops the 1 / world from every pass
// that reads gathered blocks (norm, AdamW tiles, the matrices written out).  Survives lo_vae_set_linear_factored.
extern "C" int lo_vae_set_gathered_sum(LoVae* h, int on) {
  LO_REQUIRE(h, "lo_vae_set_gathered_sum: null handle");
  h->gathered_sum = on != 0;
  return LO_OK;
}
// Called behind the all-gather of the factor blocks AND the exchange of the rest of the phase-1 range, on the stream that ran them:
// fills scratch[512..1024) the way the single-process backward's early norm does (VaeBackward::early_norm) -- [512, 767) everything
// behind decoder.fc.weight and [767] the two head biases from the AVERAGED flat buffer, [768, 896) and [896, 1024) the two matrices
// from the Gram matrices of the gathered factors, cross-rank terms included -- and remembers the buffer for the optimizer step.
// Lifetime of `gathered`: the pipelined step's factored AdamW reads it on the side stream; the caller overwrites it with the next
// step's all-gather on its communication stream.  That stream is ordered behind a point of the compute stream that follows
// lo_vae_backward_phase(1) of the next step, that backward begins with a wait for operand-refresh level 5 (VaeBackward::begin), and
// level 5 is recorded on the side stream behind the factored AdamW (level 3, vae_flush_deferred): the all-gather cannot start
// before the AdamW has read the buffer.  No further event is needed.
extern "C" int lo_vae_gathered_early_norm(LoVae* h, const void* gathered, int world, float* gram_scratch, const float* G, float* scratch,
                                          void* stream) {
  LO_REQUIRE(h && gathered && gram_scratch && G && scratch, "lo_vae_gathered_early_norm: null argument");
  if (!vae_factors_gathered(h)) { lo_set_error("lo_vae_gathered_early_norm: needs mode 3 of lo_vae_set_linear_factored"); return LO_ERR_STATE; }
  LO_REQUIRE(lo_lowrank_gathered_applies(world, h->B), "lo_vae_gathered_early_norm: world %d x padded batch %d is above the combined rank "
             "the gathered update is built for (512): use mode 2", world, h->Bp);
  hipStream_t st = S(stream);
  const int L = h->L;
  const size_t bh = h->p_off[h->idx_fc_mu_w], nh = (size_t)2 * L * 32768, bd = h->p_off[h->idx_dfc_w], nd = (size_t)32768 * L;
  const f16* base = reinterpret_cast<const f16*>(gathered);
  LO_TRY(lo_sumsq_blocks(G + bd + nd, h->flat_elems - (bd + nd), scratch + 512, 255, st));
  LO_TRY(lo_sumsq_blocks(G + bh + nh, bd - (bh + nh), scratch + 767, 1, st));
  const size_t kt = (size_t)world * h->Bp;
  const LoLowrankNorm nl[2] = {
      {vae_fac_in_block(h, base, h->o_fac_dmlT), 2 * L, vae_fac_in_block(h, base, h->o_fac_xT), 32768, gram_scratch, scratch + 768, 128},
      {vae_fac_in_block(h, base, h->o_fac_zT), L, vae_fac_in_block(h, base, h->o_fac_gfcT), 32768, gram_scratch + kt * kt, scratch + 896, 128}};
  LO_TRY(lo_lowrank_sumsq_gathered(nl, 2, vae_fac_block_elems(h), world, h->B, vae_gathered_scale(h, world), st));
  h->fac.gathered = base;
  h->fac.world = world;
  h->fac.ready = true;
  return LO_OK;
}
// data parallel (mode 2): where the factor block -- dml^T | xflat^T | Gfc^T | z^T, transposed and batch-padded fp16, one contiguous
// range of the workspace -- lives: what the ranks all-gather instead of exchanging the Linear layers' 201 MB of weight gradients
extern "C" int lo_vae_factor_block(const LoVae* h, size_t* byte_offset, size_t* bytes) {
  LO_REQUIRE(h && byte_offset && bytes, "lo_vae_factor_block: null argument");
  *byte_offset = h->o_fac_dmlT;
  *bytes = h->o_gram - h->o_fac_dmlT;       // the arena places the four factors back to back (256-byte granules), o_gram follows
  return LO_OK;
}
// ... and the averaged Linear weight gradients from `world` gathered blocks (block r at gathered + r * lo_vae_factor_block bytes):
// flat_grads[fc_mu.weight | fc_logvar.weight] and [decoder.fc.weight] = (1 / world) sum_r dY_r^T X_r / loss scale
extern "C" int lo_vae_materialize_gathered_linear_grads(LoVae* h, const void* gathered, int world, float* G, void* stream) {
  LO_REQUIRE(h && gathered && G && world >= 1, "lo_vae_materialize_gathered_linear_grads: bad argument");
  hipStream_t st = S(stream);
  const int L = h->L;
  const size_t blk = vae_fac_block_elems(h);
  const f16* base = reinterpret_cast<const f16*>(gathered);
  const float sc = vae_gathered_scale(h, world);
  LO_TRY(lo_lowrank_materialize_gathered(G + h->p_off[h->idx_fc_mu_w], vae_fac_in_block(h, base, h->o_fac_xT), vae_fac_in_block(h, base, h->o_fac_dmlT),
                                         blk, world, 2 * L, 32768, h->B, sc, st));
  return lo_lowrank_materialize_gathered(G + h->p_off[h->idx_dfc_w], vae_fac_in_block(h, base, h->o_fac_zT), vae_fac_in_block(h, base, h->o_fac_gfcT),
                                         blk, world, 32768, L, h->B, sc, st);
}
// non-zero: the flat gradient buffer does not hold the two matrices after a step (1 or 3 = the mode; lo_vae_materialize_linear_grads
// writes them out).  Mode 2 materialises them itself: 0
extern "C" int lo_vae_linear_factored(const LoVae* h) { return h ? vae_flat_lacks_linear(h) : 0; }
extern "C" int lo_vae_num_params(const LoVae* h) { return h->nparam; }
extern "C" size_t lo_vae_param_offset(const LoVae* h, int i) { return (i >= 0 && i < h->nparam) ? h->p_off[i] : (size_t)-1; }
extern "C" size_t lo_vae_param_numel(const LoVae* h, int i) { return (i >= 0 && i < h->nparam) ? h->p_numel[i] : 0; }
extern "C" size_t lo_vae_flat_elems(const LoVae* h) { return h->flat_elems; }
extern "C" size_t lo_vae_workspace_bytes(const LoVae* h) { return h->ws_bytes; }

// where a forward left one of its intermediate tensors inside the workspace (fp16 NHWC [B][H][W][C]); for parity tests that
// compare per-layer activations with the reference's hooked module outputs.  which: 0 = raw output (bias included) of encoder
// conv (stage s, k = 0 strided conv / 1, 2 the ResBlock convs), 1 = raw output of transposed conv s of the decoder,
// 2 = ResBlock output of encoder stage s (the stage output), 3 = activation (GroupNorm + Mish [+ skip]) of decoder layer s
extern "C" int lo_vae_debug_tensor(const LoVae* h, int which, int s, int k, size_t* byte_offset, int* dims4) {
  LO_REQUIRE(h && byte_offset && dims4 && s >= 0 && s < 4 && k >= 0 && k < 3, "lo_vae_debug_tensor: bad argument");
  const ConvLayer* c = which == 0 ? &h->enc[s][k] : ((which == 1 || which == 3) ? &h->dec[s] : (which == 2 ? &h->enc[s][2] : nullptr));
  LO_REQUIRE(c, "lo_vae_debug_tensor: unknown tensor kind %d", which);
  *byte_offset = which == 2 ? h->o_eout[s] : (which == 3 ? c->o_a : c->o_v);
  dims4[0] = h->B; dims4[1] = c->Ho; dims4[2] = c->Wo; dims4[3] = c->Cout;
  return LO_OK;
}

// ... and what a forward plus a backward leave behind, for tests that check every layer IN SITU (each layer against a plain reference of
// its own stored operands, at the batch size and with the kernels the step really selected; tests/test_vae_insitu_gpu.py).  which 0..3
// as above; 4 = activation (GroupNorm + Mish) of encoder conv (s, k) -- k = 2 has none, the ResBlock tail writes the stage output (2);
// 5 / 6 = saved GroupNorm statistics of encoder conv (s, k) / decoder layer s: FP32 [B][8][2] (mean, rstd), dims4 = B, 8, 2, 1;
// 7 / 8 = gradient wrt the raw conv output of encoder conv (s, k) / decoder layer s (carries the backward's loss scale); 9 = the
// decoder's input h0 [B][8][8][512]; 10 = skip gradient s (0: 64 x 64 x 64, 1: 32 x 32 x 128, 2: 16 x 16 x 256; loss scale as 7 / 8).
// elem_bytes: 2 = fp16, 4 = fp32.  The first conv's dv has no fixed home (the ping-pong buffer, unless conv1's data gradient wrote it):
// the answer for (7, 0, 0) holds for the backward that ran last.
extern "C" int lo_vae_debug_tensor_ex(const LoVae* h, int which, int s, int k, size_t* byte_offset, int* dims4, int* elem_bytes) {
  LO_REQUIRE(h && byte_offset && dims4 && elem_bytes && s >= 0 && s < 4 && k >= 0 && k < 3, "lo_vae_debug_tensor_ex: bad argument");
  *elem_bytes = 2;
  if (which >= 0 && which <= 3) return lo_vae_debug_tensor(h, which, s, k, byte_offset, dims4);
  dims4[0] = h->B;
  if (which == 9) { *byte_offset = h->o_h0; dims4[1] = dims4[2] = 8; dims4[3] = 512; return LO_OK; }
  if (which == 10) {
    LO_REQUIRE(s < 3, "lo_vae_debug_tensor_ex: three skip gradients, asked for %d", s);
    *byte_offset = h->o_skipg[s]; dims4[1] = dims4[2] = 64 >> s; dims4[3] = 64 << s;
    return LO_OK;
  }
  if (which >= 11 && which <= 22) {      // the attention sites: odd = encoder, even = decoder
    LO_REQUIRE(h->attn, "lo_vae_debug_tensor_ex: tensor kind %d needs a plan made with LO_VAE_ATTN", which);
    const int site = (which & 1) ? 0 : 1, what = (which - 11) / 2;
    const LoAttnSite& a = h->att[site];
    const size_t o[6] = {a.o_qkv, vae_attn_input(h, site), a.o_y, a.o_dy, a.o_dqkv, a.o_dx};
    *byte_offset = o[what];
    dims4[1] = dims4[2] = 8; dims4[3] = (what == 0 || what == 4) ? 640 : 512;
    return LO_OK;
  }
  LO_REQUIRE(which >= 4 && which <= 8 && !(which == 4 && k == 2), "lo_vae_debug_tensor_ex: unknown tensor kind %d (k = %d)", which, k);
  const ConvLayer* c = (which == 6 || which == 8) ? &h->dec[s] : &h->enc[s][k];
  if (which == 5 || which == 6) {
    *byte_offset = c->o_stats; *elem_bytes = 4;
    dims4[1] = 8; dims4[2] = 2; dims4[3] = 1;
    return LO_OK;
  }
  *byte_offset = which == 4 ? c->o_a : ((c == &h->enc[0][0] && !c->dv_done) ? h->o_G[3] : c->o_dv);
  dims4[1] = c->Ho; dims4[2] = c->Wo; dims4[3] = c->Cout;
  return LO_OK;
}
// how the plan runs conv + GroupNorm layer (dec ? up(s+1) : encoder conv (s, k)): info4 = forward conv on e4m3 operands (0 / 1),
// GroupNorm partial-sum rows per sample its epilogue writes, K splits of the forward, of the data gradient (0 = one-launch kernel)
extern "C" int lo_vae_layer_plan(const LoVae* h, int dec, int s, int k, int* info4) {
  LO_REQUIRE(h && info4 && s >= 0 && s < 4 && k >= 0 && k < 3, "lo_vae_layer_plan: bad argument");
  const ConvLayer& c = dec ? h->dec[s] : h->enc[s][k];
  info4[0] = c.f8 ? 1 : 0; info4[1] = c.MT; info4[2] = c.sk_fwd; info4[3] = c.sk_dgrad;
  return LO_OK;
}

// A handle made where no device is visible (n_cu = 0) plans nothing that waits across workgroups, so its answers are not those of any
// real device.  This names the device to plan for instead; such a handle can launch nothing.  Refused on a handle that has a device.
extern "C" int lo_vae_plan_assume_cus(LoVae* h, int n_cu) {
  LO_REQUIRE(h && n_cu >= 1, "lo_vae_plan_assume_cus: bad argument");
  if (h->n_cu != 0 && !h->n_cu_assumed) {
    lo_set_error("lo_vae_plan_assume_cus: the handle was made on a device with %d compute units", h->n_cu);
    return LO_ERR_STATE;
  }
  h->n_cu = n_cu;
  h->n_cu_assumed = true;
  return LO_OK;
}

// The launches of conv + GroupNorm layer (dec, s, k) in the fused single-call step (lo_vae_forward, lo_vae_backward with fused = 1),
// field order as documented in include/lunaris_hip.h.  Every choice comes from the helper the executor asks (lo_vae.h); what the
// executor keeps as state between launches -- the P1 rows a data-gradient epilogue has left for the GroupNorm backward of the layer
// before it -- is replayed here from the chain's topology.
extern "C" int lo_vae_layer_plan_ex(const LoVae* h, int dec, int s, int k, int* info, int cap) {
  LO_REQUIRE(h && info && s >= 0 && s < 4 && k >= 0 && k < 3 && !(dec && k), "lo_vae_layer_plan_ex: bad argument");
  LO_REQUIRE(cap >= LO_VAE_PLAN_FIELDS, "lo_vae_layer_plan_ex: room for %d fields, the plan has %d", cap, LO_VAE_PLAN_FIELDS);
  const ConvLayer& c = dec ? h->dec[s] : h->enc[s][k];
  const bool first = &c == &h->enc[0][0];      // its conv, weight gradient and (image) data gradient are kernels of their own
  for (int i = 0; i < LO_VAE_PLAN_FIELDS; ++i) info[i] = 0;
  auto put_conv = [&](int at, const LoConvChoice& ch, int ksplit) {
    const int f[9] = {ch.kernel, ch.bm, ch.bn, ch.bk, ch.th, ch.tw, ch.mts, ch.nt, ksplit};
    for (int i = 0; i < 9; ++i) info[at + i] = f[i];
  };
  // ---- forward
  if (first) info[6] = c.MT;
  else {
    bool y8 = c.o_a8 != 0;      // conv_gn's o_y8: the ResBlock tail writes the stage output and its e4m3 copy
    for (int t = 0; t < 4; ++t) if (&c == &h->enc[t][2]) y8 = h->o_eout8[t] != 0;
    const VaeFwdPlan f = vae_fwd_plan(c, y8);
    put_conv(c.f8 ? 9 : 0, f.choice, f.splitk ? c.sk_fwd : 0);
  }
  // ---- data gradient
  if (!first) {
    const VaeDgradPlan d = vae_dgrad_plan(h, c, vae_dgrad_prod(h, c), vae_dgrad_adds(h, c));
    put_conv(18, d.choice, d.splitk ? c.sk_dgrad : 0);
    info[27] = d.apply ? 1 : 0;
  }
  // ---- GroupNorm backward: what the data gradient of the consuming layer has left decides the form
  {
    const VaeGnBwdPlan g = vae_gn_bwd_replay(h, c);      // every single-call backward ends by checking this replay against what it did
    info[28] = g.form; info[29] = g.p1; info[30] = g.p2;
  }
  // ---- weight gradient
  if (first) info[31] = -1;
  else {
    const LoWgradChoice w = lo_wgrad_choose(c.gf);
    const int f[9] = {w.kernel, w.tw, w.convt ? 1 : 0, w.nsplit, w.slabs, w.units_per_split, w.direct ? 1 : 0, w.reduce, w.units};
    for (int i = 0; i < 9; ++i) info[31 + i] = f[i];
  }
  return LO_OK;
}

// byte offset (inside the workspace) of the word a fused-GroupNorm workgroup sets when its rendezvous poll ran out; 0 = never
extern "C" int lo_vae_sync_fail_word(const LoVae* h, size_t* byte_offset, int* fused_layers) {
  LO_REQUIRE(h && byte_offset, "lo_vae_sync_fail_word: null argument");
  *byte_offset = h->o_sync_fail;
  if (fused_layers) {
    int n = 0;
    for_each_layer(h, [&](const ConvLayer& c) { n += c.gnf ? 1 : 0; });
    *fused_layers = n;
  }
  return LO_OK;
}

extern "C" int lo_vae_set_async_handover(LoVae* h, int on) {
  LO_REQUIRE(h, "lo_vae_set_async_handover: null handle");
  h->async_handover = on != 0;
  return LO_OK;
}
extern "C" int lo_vae_wait_handover(LoVae* h, void* stream) {
  LO_REQUIRE(h, "lo_vae_wait_handover: null handle");
  if (h->range_pending) {
    LO_HIP(hipStreamWaitEvent(S(stream), h->ev_range, 0));
    h->range_pending = false;
  }
  return LO_OK;
}
extern "C" int lo_gradnorm_early_range(const float* flat_grads, size_t begin, size_t end, float* scratch, void* stream) {
  LO_REQUIRE(flat_grads && scratch && end > begin, "lo_gradnorm_early_range: bad argument");
  // the kernel issues 16-byte loads from flat_grads + begin on: the pointer is 16-byte aligned by the ABI, so begin must keep that
  LO_REQUIRE(begin % 4 == 0, "lo_gradnorm_early_range: begin=%zu must be a multiple of 4 elements (16-byte loads start there)", begin);
  return lo_sumsq_range(flat_grads, begin, end, scratch, S(stream));
}

// op level: the two gathered-factor passes on plain pointers (tests, tools/op_bench.py)
extern "C" size_t lo_lowrank_gathered_scratch_bytes(int world, int batch) {
  return lo_lowrank_gathered_applies(world, batch) ? lo_lowrank_gathered_gram_elems(world, batch) / 2 * sizeof(float) : 0;   // one layer
}
extern "C" int lo_lowrank_gathered_sumsq(const void* fshort_t, int n_short, const void* flong_t, int n_long, size_t rank_stride_elems, int world,
                                         int batch, float scale, float* gram_scratch, float* partial, void* stream) {
  LO_REQUIRE(fshort_t && flong_t && gram_scratch && partial, "lo_lowrank_gathered_sumsq: null argument");
  const LoLowrankNorm nl = {reinterpret_cast<const f16*>(fshort_t), n_short, reinterpret_cast<const f16*>(flong_t), n_long, gram_scratch, partial, 128};
  return lo_lowrank_sumsq_gathered(&nl, 1, rank_stride_elems, world, batch, scale, S(stream));
}
extern "C" int lo_lowrank_gathered_adamw(float* p, float* m, float* v, void* cast, void* cast_t, const void* xt, const void* yt,
                                         size_t rank_stride_elems, int world, int N, int K, int batch, float gscale, const float* norm, float lr,
                                         float beta1, float beta2, float eps, float weight_decay, int step, void* stream) {
  LO_REQUIRE(p && m && v && xt && yt && step >= 1, "lo_lowrank_gathered_adamw: bad argument");
  const LoLowrankMat mt = {p, m, v, reinterpret_cast<f16*>(cast), reinterpret_cast<f16*>(cast_t), reinterpret_cast<const f16*>(xt),
                           reinterpret_cast<const f16*>(yt), N, K};
  return lo_adamw_lowrank_gathered(&mt, 1, rank_stride_elems, world, batch, gscale, {norm, lr, beta1, beta2, eps, weight_decay, step}, S(stream));
}

// ... and the two passes of the optimizer's materialised path they are measured against (tools/op_bench.py --op lowrank_gathered)
extern "C" int lo_adamw_range(float* p, const float* g, float* m, float* v, size_t n, const float* norm, float lr, float beta1, float beta2,
                              float eps, float weight_decay, int step, void* cast, void* stream) {
  LO_REQUIRE(p && g && m && v && n > 0 && step >= 1, "lo_adamw_range: bad argument");
  return lo_adamw(p, g, m, v, n, norm, lr, beta1, beta2, eps, weight_decay, step, S(stream), reinterpret_cast<f16*>(cast));
}
extern "C" int lo_transpose_f16(const void* src, void* dst, int rows, int cols, void* stream) {
  LO_REQUIRE(src && dst && rows > 0 && cols > 0 && rows % 64 == 0 && cols % 64 == 0, "lo_transpose_f16: rows=%d, cols=%d must be positive multiples of 64", rows, cols);
  return lo_nhwc_to_nchw_f16(reinterpret_cast<const f16*>(src), reinterpret_cast<f16*>(dst), 1, rows, cols, S(stream));
}

extern "C" int lo_vae_fp8_layers(const LoVae* h, int* layers) {
  LO_REQUIRE(h && layers, "lo_vae_fp8_layers: null argument");
  int n = 0;
  for_each_layer(h, [&](const ConvLayer& c) { n += c.f8 ? 1 : 0; });
  *layers = n;
  return LO_OK;
}
extern "C" int lo_vae_linear_grad_range(const LoVae* h, size_t* begin, size_t* end) {
  LO_REQUIRE(h && begin && end, "lo_vae_linear_grad_range: null argument");
  *begin = h->p_off[h->idx_fc_mu_w];
  *end = h->p_off[h->idx_dfc_b] + ((h->p_numel[h->idx_dfc_b] + 63) & ~(size_t)63);
  return LO_OK;
}

// everything from fc_mu.weight to the end of the flat buffer (the three Linear layers, the decoder convs and the final
// conv: 90 % of the bytes) is final after phase 1
extern "C" int lo_vae_phase1_grad_range(const LoVae* h, size_t* begin, size_t* end) {
  LO_REQUIRE(h && begin && end, "lo_vae_phase1_grad_range: null argument");
  *begin = h->p_off[h->idx_fc_mu_w];
  *end = h->flat_elems;
  return LO_OK;
}

// the last encoder stage (down4: strided conv + ResBlock at 512 channels) holds 94 % of the encoder's gradient bytes and is the
// first to be complete in the backward: the three-call form (phases 1, 3, 4) hands it over before stages 3..1 run
extern "C" int lo_vae_stage4_grad_range(const LoVae* h, size_t* begin, size_t* end) {
  LO_REQUIRE(h && begin && end, "lo_vae_stage4_grad_range: null argument");
  *begin = h->p_off[h->enc[3][0].p_w];
  *end = h->p_off[h->idx_fc_mu_w];
  return LO_OK;
}
