// VAE step executor: forward, loss and backward.
#include "lo_vae.h"

// The arrival counters of the fused GroupNorm epilogues live in the caller's workspace: zero them (and the failure word) the first
// time a workspace is seen; from then on they only ever count up (ConvLayer::gnf_epoch follows them on the host).
static int vae_ensure_sync_init(LoVae* h, void* ws, hipStream_t st) {
  if (h->sync_for_ws == ws) return LO_OK;
  hipError_t e = hipSuccess;
  for_each_layer(h, [&](ConvLayer& c) {
    if (e == hipSuccess) e = hipMemsetAsync(WSP(void, c.o_xcnt), 0, (size_t)h->B * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(WSP(void, c.o_bcnt), 0, (size_t)h->B * 8 * 4, st);
    c.gnf_epoch = 0; c.gba_epoch = 0;
  });
  LO_HIP(e);
  LO_HIP(hipMemsetAsync(WSP(void, h->o_sync_fail), 0, 256, st));
  h->sync_for_ws = ws;
  return LO_OK;
}

// in8: e4m3 copy of `in` (fp8 mode, layers with c.f8); y8: where to leave the e4m3 copy of y (0 = nobody reads it)
static int conv_gn(LoVae* h, ConvLayer& c, const f16* in, const f16* other, f16* y, int mode, const float* P, void* ws,
                   hipStream_t st, size_t o_in8 = 0, size_t o_y8 = 0) {
  LoProfTag tag("fwd kind%d %dx%d %d->%d", c.kind, c.Ho, c.Wo, c.gf.Cin, c.gf.Cout);     // names the conv launch below
  // GroupNorm + Mish inside the conv's own epilogue (the workgroups of a sample exchange their sums: LoGnFuse) where the kernel that
  // owns this geometry supports it; the separate lo_gn_fwd pass below is then not run.  Same statistics, same arithmetic, same bits.
  const VaeFwdPlan plan = vae_fwd_plan(c, o_y8 != 0);
  LoConvChoice ran{};       // the choice the launch made: the plan's, and its partial-sum rows are what lo_gn_forward reads below
  if (plan.splitk) {
    // few output rows: K-split GEMM into fp32 slabs, then ONE (sample, group)-local pass: slab sum + bias -> v, statistics, GroupNorm + Mish
    LO_TRY(lo_conv_run(c.gf, {.in = in, .w = WSP(f16, c.o_wp_f), .slab = WSP(float, h->o_skslab), .nsplit = c.sk_fwd}, st, &ran));
    tag.end();
    LO_TRY(vae_require_planned(ran, plan.choice, "forward conv (split-K)", c.gf));
    return lo_gn_forward(vae_gn_layer(h, c, P, ws),
                         {.slab = WSP(float, h->o_skslab), .nsplit = c.sk_fwd, .bias = PRM(c.p_b), .other = other, .mode = mode, .y = y}, st);
  }
  const bool fuse = plan.fuse;
  LoGnFuse gf;
  if (fuse) {
    memset(&gf, 0, sizeof(gf));
    gf.xbuf = WSP(float, c.o_xbuf); gf.counter = WSP(unsigned int, c.o_xcnt);
    gf.MTs = c.gnf_mts; gf.NT = c.gnf_nt;
    gf.target = (++c.gnf_epoch) * (unsigned)(c.gnf_mts * c.gnf_nt);
    gf.gamma = PRM(c.p_gw); gf.beta = PRM(c.p_gb); gf.other = other; gf.y = y; gf.stats = WSP(float, c.o_stats); gf.mode = mode;
    gf.fail = WSP(unsigned int, h->o_sync_fail);
  }
  int r_;
  if (c.f8) {
    LO_REQUIRE(o_in8, "fp8 mode: no e4m3 copy of the input of a conv %d->%d", c.Cin, c.Cout);
    r_ = lo_conv_run_f8(c.gf, WSP(uint8_t, o_in8), WSP(uint8_t, c.o_wp8), WSP(float, c.o_wscale),
                        {.bias = PRM(c.p_b), .out = WSP(f16, c.o_v), .gn_partial = WSP(float, c.o_part)}, st, &ran);
  } else {
    r_ = lo_conv_run(c.gf, {.in = in, .w = WSP(f16, c.o_wp_f), .bias = PRM(c.p_b), .out = WSP(f16, c.o_v),
                            .gn_partial = fuse ? nullptr : WSP(float, c.o_part), .gf = fuse ? &gf : nullptr}, st, &ran);
  }
  tag.end();
  if (r_ != LO_OK) { if (fuse) --c.gnf_epoch; return r_; }
  LO_TRY(vae_require_planned(ran, plan.choice, c.f8 ? "forward conv (e4m3)" : "forward conv", c.gf));
  if (fuse) return LO_OK;
  // o_part is sized for c.MT rows per sample and lo_gn_fwd sums c.MT rows: a launch that wrote another count has overrun the one and
  // is misread by the other (the plan and the launch asked lo_conv_choose with different uses)
  LO_REQUIRE(ran.mts == c.MT, "conv + GroupNorm %dx%d %d->%d: the conv launch wrote %d partial-sum rows per sample, the plan has %d",
             c.Ho, c.Wo, c.Cin, c.Cout, ran.mts, c.MT);
  return lo_gn_forward(vae_gn_layer(h, c, P, ws), {.partial = WSP(float, c.o_part), .MT = c.MT, .other = other, .mode = mode, .y = y,
                                                   .y8 = o_y8 ? WSP(uint8_t, o_y8) : nullptr}, st);
}

// bottleneck self-attention, forward of one site: qkv = x Wqkv^T + b on the GEMM family, then the fused core (lo_attn8.hip)
static int vae_attn_forward(LoVae* h, int site, const f16* x, const float* P, void* ws, hipStream_t st) {
  const LoAttnSite& a = h->att[site];
  {
    LoProfTag tag("attn%d qkv", site);
    LO_TRY(lo_conv_run(h->g_att_qkv, {.in = x, .w = WSP(f16, a.o_w), .bias = PRM(a.p_b), .out = WSP(f16, a.o_qkv)}, st));
  }
  return lo_attn8_fwd(x, WSP(f16, a.o_qkv), PRM(a.p_gamma), WSP(f16, a.o_y), h->B, st);
}

// decoder (lunar_generate.py:194-229) from the latent z (fp16, in the workspace); use_skips=false is the `skips=[]`
// call of LunarisCoreVAE.sample (:278-291)
// skips[k] (fp16 NHWC, k = 0: 64 x 64 x 64, 1: 32 x 32 x 128, 2: 16 x 16 x 256) is added after up(3-k); NULL = not added
static int vae_decoder_forward(LoVae* h, const f16* const skips[3], const float* P, void* ws, float* recon, const float* target,
                               hipStream_t st) {
  const int B = h->B;
  LO_TRY(vae_ensure_sync_init(h, ws, st));
  LO_TRY(vae_wait_level(h, st, 4));
  LO_TRY(lo_conv_run(h->g_dfc, {.in = WSP(f16, h->o_z), .w = WSP(f16, h->o_wp_dfc), .bias = PRM(h->idx_dfc_b), .out = WSP(f16, h->o_yfc)}, st));
  LO_TRY(lo_nchw_to_nhwc_f16(WSP(f16, h->o_yfc), WSP(f16, h->o_h0), B, 64, 512, st, h->o_h08 ? WSP(uint8_t, h->o_h08) : nullptr));
  const f16* cur = WSP(f16, h->o_h0);
  size_t cur8 = h->o_h08;
  if (h->attn) {      // up1 reads the attention's output in place of h0 (level 4 has refreshed the site's operand)
    LO_TRY(vae_attn_forward(h, 1, cur, P, ws, st));
    cur = WSP(f16, h->att[1].o_y);
  }
  for (int s = 0; s < 4; ++s) {
    ConvLayer& c = h->dec[s];
    const f16* skip = s < 3 ? skips[2 - s] : nullptr;
    LO_TRY(conv_gn(h, c, cur, skip, WSP(f16, c.o_a), skip ? 1 : 0, P, ws, st, cur8, c.o_a8));
    cur = WSP(f16, c.o_a);
    cur8 = c.o_a8;
  }
  h->dec_done = true;
  h->dec_skips = (skips[0] ? 1 : 0) + (skips[1] ? 1 : 0) + (skips[2] ? 1 : 0);
  return lo_final_conv_fwd(cur, PRM(h->idx_final_w), PRM(h->idx_final_b), target, recon, target ? WSP(float, h->o_msep) : nullptr,
                           B, st);
}

static int vae_encoder_forward(LoVae* h, const float* x, const float* eps, uint64_t seed, const float* P, void* ws, float* mu,
                               float* logvar, hipStream_t st);

extern "C" int lo_vae_forward(LoVae* h, const float* x, const float* eps, uint64_t seed, const float* P, void* ws,
                              float* recon, float* mu, float* logvar, const float* target, void* stream) {
  LO_REQUIRE(h && x && P && ws && recon && mu && logvar, "lo_vae_forward: null argument");
  hipStream_t st = S(stream);
  LO_TRY(vae_encoder_forward(h, x, eps, seed, P, ws, mu, logvar, st));
  const f16* skips[3] = {WSP(f16, h->o_eout[0]), WSP(f16, h->o_eout[1]), WSP(f16, h->o_eout[2])};
  LO_TRY(vae_decoder_forward(h, skips, P, ws, recon, target, st));
  h->forward_done = true;
  h->loss_done = false;
  return LO_OK;
}

// encoder + heads + reparameterisation (lunar_generate.py:127-153, 259-261): stage outputs in o_eout, mu / logvar / z / eps / KL partials
static int vae_encoder_forward(LoVae* h, const float* x, const float* eps, uint64_t seed, const float* P, void* ws, float* mu,
                               float* logvar, hipStream_t st) {
  const int B = h->B, L = h->L;
  LO_TRY(vae_ensure_sync_init(h, ws, st));
  // ---- encoder (lunar_generate.py:127-153)
  const f16* cur = nullptr;
  size_t cur8 = 0;
  for (int s = 0; s < 4; ++s) {
    ConvLayer& c0 = h->enc[s][0];
    ConvLayer& c1 = h->enc[s][1];
    ConvLayer& c2 = h->enc[s][2];
    if (s == 0) {
      LO_TRY(lo_first_conv_fwd(x, PRM(c0.p_w), PRM(c0.p_b), WSP(f16, c0.o_v), WSP(float, c0.o_part), B, st));
      LO_TRY(lo_gn_forward(vae_gn_layer(h, c0, P, ws), {.partial = WSP(float, c0.o_part), .MT = c0.MT, .y = WSP(f16, c0.o_a),
                                                        .y8 = c0.o_a8 ? WSP(uint8_t, c0.o_a8) : nullptr}, st));
      LO_TRY(vae_wait_level(h, st, 1));
    } else {
      // the last stage's packed weights are refreshed at the END of the side-stream chain of a pipelined optimizer step
      // (after the AdamW of everything from this stage on): same event as the Linear casts
      if (s == 3) LO_TRY(vae_wait_level(h, st, 2));
      LO_TRY(conv_gn(h, c0, cur, nullptr, WSP(f16, c0.o_a), 0, P, ws, st, cur8, c0.o_a8));
    }
    LO_TRY(conv_gn(h, c1, WSP(f16, c0.o_a), nullptr, WSP(f16, c1.o_a), 0, P, ws, st, c0.o_a8, c1.o_a8));
    // ResBlock tail: out = mish(mish(GN(conv2)) + identity); c2.o_a is unused, the result is the stage output
    LO_TRY(conv_gn(h, c2, WSP(f16, c1.o_a), WSP(f16, c0.o_a), WSP(f16, h->o_eout[s]), 2, P, ws, st, c1.o_a8, h->o_eout8[s]));
    cur = WSP(f16, h->o_eout[s]);
    cur8 = h->o_eout8[s];
  }
  if (h->attn) {      // the flatten reads the attention's output in place of the stage-4 output (level 2 has refreshed the site's operand)
    LO_TRY(vae_attn_forward(h, 0, cur, P, ws, st));
    cur = WSP(f16, h->att[0].o_y);
  }
  // ---- heads + reparameterisation (lunar_generate.py:150-152, 259-261)
  LO_TRY(lo_nhwc_to_nchw_f16(cur, WSP(f16, h->o_xflat), B, 64, 512, st));
  LO_TRY(vae_wait_level(h, st, 3));
  LO_TRY(lo_conv_run(h->g_head, {.in = WSP(f16, h->o_xflat), .w = WSP(f16, h->o_wp_head), .slab = WSP(float, h->o_slab_head), .nsplit = h->head_split}, st));
  LO_REQUIRE(h->p_off[h->idx_fc_lv_b] == h->p_off[h->idx_fc_mu_b] + (size_t)L, "flat layout: head biases not adjacent");
  LO_TRY(lo_head_reduce(WSP(float, h->o_slab_head), PRM(h->idx_fc_mu_b), eps, seed, WSP(float, h->o_mu), WSP(float, h->o_lv),
                        WSP(f16, h->o_z), WSP(float, h->o_eps), WSP(float, h->o_klp), B, L, h->head_split, st, mu, logvar));
  h->enc_done = true;
  return LO_OK;
}

// Encoder.forward (lunar_generate.py:127-153) on its own: mu, logvar and the skip list as fp32 NCHW tensors (NULL = not wanted)
extern "C" int lo_vae_encode(LoVae* h, const float* x, const float* P, void* ws, float* mu, float* logvar, float* skip0, float* skip1,
                             float* skip2, void* stream) {
  LO_REQUIRE(h && x && P && ws && mu && logvar, "lo_vae_encode: null argument");
  hipStream_t st = S(stream);
  LO_TRY(vae_encoder_forward(h, x, nullptr, 0, P, ws, mu, logvar, st));     // the z it leaves in the workspace is not used
  float* sk[3] = {skip0, skip1, skip2};
  for (int k = 0; k < 3; ++k)
    if (sk[k]) LO_TRY(lo_nhwc_f16_to_nchw_f32(WSP(f16, h->o_eout[k]), sk[k], h->B, (64 >> k) * (64 >> k), 64 << k, 1.0f, st));
  h->forward_done = false;   // a fused backward needs a whole lo_vae_forward
  return LO_OK;
}

// Decoder.forward(z, skips) (lunar_generate.py:194-229).  n_skips = len(skips): the reference adds skips[2] after up1 when
// len >= 3, skips[1] after up2 when len >= 2, skips[0] after up3 when len >= 1.  skip maps: fp32 NCHW.
extern "C" int lo_vae_decode_skips(LoVae* h, const float* z, int n_skips, const float* skip0, const float* skip1, const float* skip2,
                                   const float* P, void* ws, float* recon, void* stream) {
  LO_REQUIRE(h && z && P && ws && recon && n_skips >= 0 && n_skips <= 3, "lo_vae_decode_skips: bad argument");
  const float* sk[3] = {skip0, skip1, skip2};
  for (int k = 0; k < n_skips; ++k) LO_REQUIRE(sk[k], "lo_vae_decode_skips: skip %d is NULL but n_skips = %d", k, n_skips);
  hipStream_t st = S(stream);
  LO_TRY(lo_cast_f32_f16(z, WSP(f16, h->o_z), (size_t)h->B * h->L, st));
  const f16* skips[3] = {nullptr, nullptr, nullptr};
  for (int k = 0; k < n_skips; ++k) {
    LO_TRY(lo_nchw_f32_to_nhwc_f16(sk[k], WSP(f16, h->o_skipin[k]), h->B, (64 >> k) * (64 >> k), 64 << k, 1.0f, st));
    skips[k] = WSP(f16, h->o_skipin[k]);
  }
  LO_TRY(vae_decoder_forward(h, skips, P, ws, recon, nullptr, st));
  h->forward_done = false;
  return LO_OK;
}

extern "C" int lo_vae_decode(LoVae* h, const float* z, const float* P, void* ws, float* recon, void* stream) {
  LO_REQUIRE(h && z && P && ws && recon, "lo_vae_decode: null argument");
  hipStream_t st = S(stream);
  LO_TRY(lo_cast_f32_f16(z, WSP(f16, h->o_z), (size_t)h->B * h->L, st));
  const f16* skips[3] = {nullptr, nullptr, nullptr};
  LO_TRY(vae_decoder_forward(h, skips, P, ws, recon, nullptr, st));
  h->forward_done = false;   // activations no longer belong to a full forward: a fused backward must not follow
  return LO_OK;
}

extern "C" int lo_vae_loss(LoVae* h, void* ws, float recon_weight, float kl_weight, float mean_advantage, const float* adv_dev,
                           float accum, float loss_scale, float* losses_dev, void* stream) {
  LO_REQUIRE(h && ws && losses_dev, "lo_vae_loss: null argument");
  if (!h->forward_done) { lo_set_error("lo_vae_loss: no forward with a target has run"); return LO_ERR_STATE; }
  hipStream_t st = S(stream);
  const int B = h->B, L = h->L;
  LO_TRY(lo_loss_finalize(WSP(float, h->o_msep), B * 64, WSP(float, h->o_klp), (B * L + 255) / 256, recon_weight, kl_weight,
                          mean_advantage, adv_dev, accum, loss_scale, losses_dev, WSP(float, h->o_coefs),
                          (float)B * 3.f * 128.f * 128.f, (float)B * (float)L, st));   // the four scalars go straight to the caller's buffer
  h->loss_done = true;
  return LO_OK;
}
// the hybrid step's reward-gradient term behind lo_vae_loss (the kernel sits beside lo_hybrid_reward's)
extern "C" int lo_vae_reward_term(LoVae* h, void* ws, const float* q_eval, float weight, float accum, float loss_scale, float* losses_dev,
                                  float* out2, float* seed_coef, void* stream) {
  LO_REQUIRE(h && ws && q_eval && losses_dev && out2 && seed_coef, "lo_vae_reward_term: null argument");
  if (!h->loss_done) { lo_set_error("lo_vae_reward_term: lo_vae_loss has not run"); return LO_ERR_STATE; }
  return lo_reward_term(q_eval, h->B, weight, accum, loss_scale, WSP(float, h->o_coefs), losses_dev, out2, seed_coef, S(stream));
}

// GroupNorm affine + conv bias gradients of a set of layers in one launch (enc_mask: bit s = encoder stage s)
static int vae_gn_finalize(LoVae* h, unsigned enc_mask, bool dec, float* G, void* ws, float inv, hipStream_t st) {
  const int B = h->B;
  LoGnFinJobs jobs;
  jobs.n = 0;
  int blocks = 0;
  bool rows_ok = true;        // every layer summed here has gone through vae_record_rows in this backward
  auto add = [&](ConvLayer& c) {
    LoGnFinJob& j = jobs.j[jobs.n++];
    j.P1 = WSP(float, c.o_P1); j.P2 = WSP(float, c.o_P2);
    j.dgamma = GRD(c.p_gw); j.dbeta = GRD(c.p_gb); j.dbias = GRD(c.p_b);
    rows_ok = rows_ok && c.np1 > 0 && c.np2 > 0;
    j.nblk1 = B * c.np1; j.nblk2 = B * c.np2;
    j.C = c.Cout; j.block0 = blocks;
    blocks += (c.Cout + 3) / 4;
  };
  for (int s = 0; s < 4; ++s)
    if (enc_mask & (1u << s)) for (int k = 0; k < 3; ++k) add(h->enc[s][k]);
  if (dec) for (int s = 0; s < 4; ++s) add(h->dec[s]);
  LO_REQUIRE(rows_ok, "GroupNorm finalize: a layer's backward has not run (no P1 / P2 rows recorded)");
  return lo_gn_finalize_all(jobs, inv, st);
}

// the alignment gaps of the flat gradient buffer (every tensor starts on a 64-element boundary): the only elements no gradient
// kernel writes.  One small launch instead of a 244 MB memset per step.
struct LoGapTable { unsigned long long off[96]; int len[96]; int n; };
__global__ void lo_zero_gaps_kernel(float* G, LoGapTable t) {
  const int i = blockIdx.x;
  if (i < t.n && (int)threadIdx.x < t.len[i]) G[t.off[i] + threadIdx.x] = 0.f;
}
static int vae_zero_gaps(LoVae* h, float* G, hipStream_t st) {
  LoGapTable t;
  t.n = 0;
  LO_REQUIRE(h->nparam <= 96, "gap table too small");
  for (int i = 0; i < h->nparam; ++i) {
    const size_t n = h->p_numel[i], padded = (n + 63) & ~(size_t)63;
    if (padded > n) { t.off[t.n] = h->p_off[i] + n; t.len[t.n] = (int)(padded - n); ++t.n; }
  }
  if (t.n == 0) return LO_OK;
  hipLaunchKernelGGL(lo_zero_gaps_kernel, dim3(t.n), dim3(64), 0, st, G, t);
  LO_LAUNCH_CHECK("zero_gaps");
  return LO_OK;
}

// ---------------------------------------------------------------------------------------------
// Backward.  One VaeBackward lives on the stack of an entry point, which composes the parts below; the dependent chain runs on `st`,
// weight / bias gradients beside it on the side stream when there is one (`side`).
// ---------------------------------------------------------------------------------------------
namespace {
struct VaeBackward {
  LoVae* h; const float* P; float* G; void* ws; float loss_scale; hipStream_t st;
  float inv;        // 1 / loss scale: what every parameter gradient is multiplied by
  bool side;
  f16 *Ga, *Gb, *Gc, *Gd;
  VaeBackward(LoVae* h_, const float* P_, float* G_, void* ws_, float loss_scale_, void* stream)
      : h(h_), P(P_), G(G_), ws(ws_), loss_scale(loss_scale_), st(S(stream)), inv(1.0f / loss_scale_), side(vae_side_on(h_)),
        Ga(WSP(f16, h_->o_G[0])), Gb(WSP(f16, h_->o_G[1])), Gc(WSP(f16, h_->o_G[2])), Gd(WSP(f16, h_->o_G[3])) {}

  int begin(bool first_call);
  int gn_backward(ConvLayer& c, const LoGnBwd& op);
  int layer(ConvLayer& c, const f16* dy, const f16* other, int mode, const f16* layer_in, f16* ds, f16* din, const f16* add_src,
            ConvLayer* prod = nullptr, bool din_has_other_readers = false);
  int dgrad_splitk(ConvLayer& c, int k, const VaeDgradPlan& plan, const f16* dv, f16* din, const f16* add_src, ConvLayer& prod,
                   bool din_has_other_readers);
  int dgrad(ConvLayer& c, int k, const VaeDgradPlan& plan, const f16* dv, f16* din, const f16* add_src, ConvLayer* prod,
            bool din_has_other_readers);
  int decoder_chain(int fused, const float* recon, const float* target, const float* drecon, bool fac, float* dz32);
  int latent_and_heads(int fused, const float* gmu, const float* glv, bool fac, bool beside, bool hand_to_side);
  int attention(int site, const f16* dy, f16* dx, bool beside);
  int early_norm(bool fac1);
  int encoder_stages(int s_hi, int s_lo, const float* x, float* dx);
  int finalize(unsigned enc_mask, bool dec, hipStream_t on) { return vae_gn_finalize(h, enc_mask, dec, G, ws, inv, on); }
  int publish_range(unsigned enc_mask, bool dec);
  // the caller's stream waits for the side stream (all weight gradients written) before anything that consumes the gradient buffer
  int join() { return side ? vae_order(st, h->side, h->ev_join) : LO_OK; }
};

// `st` waits for the transposed Linear copies (and, after a lo_vae_pack between forward and backward, everything); the first call of
// a backward also resets what the layers remember of the last one
int VaeBackward::begin(bool first_call) {
  LO_TRY(vae_wait_level(h, st, 5));
  if (!first_call) return LO_OK;
  h->bwd_layer = 0;
  for_each_layer(h, [](ConvLayer& c) { c.np1 = 0; c.dv_done = false; c.np2 = 0; c.ev_ready = nullptr; c.gnb_ran = -2; });
  return LO_OK;
}

// GroupNorm backward of layer c in the form lo_gn_bwd_choose picks for (c, op); op.P1 / P2, rows_in_P1 and allow_local are filled here
int VaeBackward::gn_backward(ConvLayer& c, const LoGnBwd& op_in) {
  LoGnBwd op = op_in;
  op.P1 = WSP(float, c.o_P1); op.P2 = WSP(float, c.o_P2);
  op.rows_in_P1 = c.np1; op.allow_local = h->gn_local;
  const LoGnChoice plan = vae_gn_bwd_choice(h, c, op.slab != nullptr, c.np1);
  LO_TRY(vae_record_rows(c, plan.rows));
  c.gnb_ran = (int)plan.form;
  LoGnRows left{};
  LO_TRY(lo_gn_backward(vae_gn_layer(h, c, P, ws), op, st, &left));
  if (left.p1 != plan.rows.p1 || left.p2 != plan.rows.p2) {
    lo_set_error("GroupNorm backward %dx%dx%d: the launch left %d / %d rows of P1 / P2 per sample, the plan has %d / %d", c.Ho, c.Wo, c.Cout,
                 left.p1, left.p2, plan.rows.p1, plan.rows.p2);
    return LO_ERR_STATE;
  }
  return LO_OK;
}

// backward of one conv+GN+Mish layer.  dy: gradient wrt the layer's activation output (after mish, before any skip add).
// Produces the parameter gradients and, when din != null, the gradient wrt the layer input (+ add_src).
// prod: the conv+GN+Mish layer (mode plain / skip) whose activation gradient this layer's data gradient produces;
// its GroupNorm-backward reduction is then fused into the data-gradient epilogue (vae_record_rows keeps the row count).
int VaeBackward::layer(ConvLayer& c, const f16* dy, const f16* other, int mode, const f16* layer_in, f16* ds, f16* din,
                       const f16* add_src, ConvLayer* prod, bool din_has_other_readers) {
  // every layer has its own dv buffer: the side-stream weight gradient of layer k may still be reading it while the main
  // stream produces the dv of the following layers (no event back from the side stream: two host calls per layer less)
  const int k = h->bwd_layer++;
  f16* dv = WSP(f16, c.o_dv);
  // c.dv_done: the data gradient of the consuming layer has already turned this layer's activation gradient into dv (and P2) in
  // its epilogue -- `dy` was never stored
  hipEvent_t ready = nullptr;         // completes when dv is final
  if (c.dv_done) { ready = c.ev_ready; c.ev_ready = nullptr; }
  else {
    LoHandover ho(h, side);
    // apply only where the consumer's data gradient has reduced this layer already; else ONE pass where a (sample, group) fits a
    // workgroup (the ResBlock tails of the 16 x 16 and 8 x 8 stages), else reduce + apply
    LO_TRY(gn_backward(c, {.dy = dy, .other = other, .mode = mode, .ds = ds, .dv = dv}));
    LO_TRY(ho.finish(st));
    ready = ho.ev;
  }
  {
    if (side && ready) LO_HIP(hipStreamWaitEvent(h->side, ready, 0));
    else if (side) LO_TRY(vae_order(h->side, st, h->ev_dv[(h->nevent++) & 3]));   // dv came from a launch that carried no event: classic record
    LoProfTag tag("wgrad L%02d kind%d %dx%d %d->%d", k, c.kind, c.Ho, c.Wo, c.gf.Cin, c.gf.Cout);
    LO_TRY(lo_wgrad_run(c.gf, layer_in, dv, WSP(float, h->o_wslab), GRD(c.p_w), inv, side ? h->side : st));
  }
  if (!din) return LO_OK;
  // the plan query describes this launch from the chain's topology alone: what the caller passed must be that
  LO_REQUIRE(prod == vae_dgrad_prod(h, c) && (add_src != nullptr) == vae_dgrad_adds(h, c),
             "data gradient %dx%d %d->%d: producer / added gradient differ from the chain's topology (lo_vae.h)", c.Ho, c.Wo, c.gd.Cin, c.gd.Cout);
  const VaeDgradPlan plan = vae_dgrad_plan(h, c, prod, add_src != nullptr);
  if (plan.splitk) return dgrad_splitk(c, k, plan, dv, din, add_src, *prod, din_has_other_readers);
  return dgrad(c, k, plan, dv, din, add_src, prod, din_has_other_readers);
}

// few output rows: the data gradient as a K-split GEMM into fp32 slabs, then ONE (sample, group)-local pass that sums them
// (+ the residual gradient) and runs the whole GroupNorm backward of the producing layer: dv, one P1 / P2 row per sample
int VaeBackward::dgrad_splitk(ConvLayer& c, int k, const VaeDgradPlan& plan, const f16* dv, f16* din, const f16* add_src, ConvLayer& prod,
                              bool din_has_other_readers) {
  {
    LoProfTag tag("dgrad L%02d kind%d %dx%d %d->%d", k, c.kind, c.Ho, c.Wo, c.gd.Cin, c.gd.Cout);
    LoConvChoice ran{};
    LO_TRY(lo_conv_run(c.gd, {.in = dv, .w = WSP(f16, c.o_wp_d), .slab = WSP(float, h->o_skslab), .nsplit = c.sk_dgrad}, st, &ran));
    LO_TRY(vae_require_planned(ran, plan.choice, "data gradient (split-K)", c.gd));
  }
  LoHandover ho(h, side);       // the pass below writes prod's dv: its launch carries prod's hand-over event
  LO_TRY(gn_backward(prod, {.slab = WSP(float, h->o_skslab), .nsplit = c.sk_dgrad, .add_src = add_src,
                            .dy_out = din_has_other_readers ? din : nullptr, .dv = WSP(f16, prod.o_dv)}));
  LO_TRY(ho.finish(st));
  prod.ev_ready = ho.ev;
  prod.dv_done = true;
  return LO_OK;
}

// the data gradient on its one-launch kernel, with the GroupNorm backward of the producing layer in its epilogue where that applies
int VaeBackward::dgrad(ConvLayer& c, int k, const VaeDgradPlan& plan, const f16* dv, f16* din, const f16* add_src, ConvLayer* prod,
                       bool din_has_other_readers) {
  LoGnBwdFuse gb, *gbp = nullptr;
  if (plan.reduce) {
    gb.v = WSP(f16, prod->o_v); gb.stats = WSP(float, prod->o_stats); gb.gamma = PRM(prod->p_gw); gb.beta = PRM(prod->p_gb);
    gb.P1 = WSP(float, prod->o_P1);
    // plan.rows rows of P1 per sample; the apply form where the plan has it (vae_dgrad_plan)
    const int mts = plan.rows;
    const bool apply = plan.apply;
    LO_TRY(vae_record_rows(*prod, {mts, apply ? mts : 0}));      // without the apply this launch leaves P2 alone: prod's own layer() runs that pass
    if (apply) {
      gb.dv = WSP(f16, prod->o_dv); gb.P2 = WSP(float, prod->o_P2);
      gb.counter = WSP(unsigned int, prod->o_bcnt);
      gb.target = (++prod->gba_epoch) * (unsigned)mts;
      gb.fail = WSP(unsigned int, h->o_sync_fail);
      gb.keep_out = din_has_other_readers;      // the decoder's data gradients are also the encoder's skip gradients
      prod->dv_done = true;
      prod->gnb_ran = -1;
    }
    gbp = &gb;
  }
  const bool writes_dv = gbp && gbp->dv;      // this launch writes prod's dv: it carries prod's event
  LoProfTag tag("dgrad L%02d kind%d %dx%d %d->%d", k, c.kind, c.Ho, c.Wo, c.gd.Cin, c.gd.Cout);
  LoHandover ho(h, side && writes_dv);
  LoConvChoice ran{};
  int r_ = lo_conv_run(c.gd, {.in = dv, .w = WSP(f16, c.o_wp_d), .add_src = add_src, .out = din, .gb = gbp}, st, &ran);
  if (r_ != LO_OK) { if (writes_dv) { --prod->gba_epoch; prod->dv_done = false; } return r_; }
  LO_TRY(vae_require_planned(ran, plan.choice, "data gradient", c.gd));
  // the P1 (and P2) rows recorded above are the ones this launch wrote
  if (gbp) LO_REQUIRE(ran.mts == prod->np1, "data gradient %dx%d %d->%d: the launch wrote %d P1 rows per sample, %d were recorded",
                      c.Ho, c.Wo, c.gd.Cin, c.gd.Cout, ran.mts, prod->np1);
  if (writes_dv) { LO_TRY(ho.finish(st)); prod->ev_ready = ho.ev; }
  return LO_OK;
}

// Backward of one attention site from dy = gradient wrt its output (fp16, loss-scaled): the fused core leaves dqkv and the per-sample
// shares of dgamma; dx = dy + dqkv Wqkv (the residual's gradient is the GEMM's added tensor) continues the chain; dgamma, the three
// bias gradients (one column sum) and dWqkv = dqkv^T x run beside it, where the Linear layers' own do.  Shared by every entry point:
// decoder_chain runs site 1, latent_and_heads site 0.  beside: the parameter gradients go to the side stream (if there is one), as the
// caller's own Linear-layer gradients do; else everything stays on the caller's stream.
int VaeBackward::attention(int site, const f16* dy, f16* dx, bool beside) {
  const LoAttnSite& a = h->att[site];
  const int B = h->B;
  beside = beside && side;
  hipStream_t gs = beside ? h->side : st;
  f16* dqkv = WSP(f16, a.o_dqkv);
  {
    LoHandover ho(h, beside);
    LO_TRY(lo_attn8_bwd(WSP(f16, a.o_qkv), PRM(a.p_gamma), dy, dqkv, WSP(float, a.o_dgpart), B, st));
    LO_TRY(ho.finish(st));
    if (beside) LO_HIP(hipStreamWaitEvent(h->side, ho.ev, 0));
  }
  {
    LoProfTag tag("attn%d params", site);
    LO_TRY(lo_attn8_dgamma(WSP(float, a.o_dgpart), B, inv, GRD(a.p_gamma), gs));
    LO_TRY(lo_colsum_f16(dqkv, GRD(a.p_b), B * 64, 640, inv, gs));
    LO_TRY(lo_wgrad_run(h->g_att_qkv, WSP(f16, vae_attn_input(h, site)), dqkv, WSP(float, h->o_att_wslab), GRD(a.p_w), inv, gs));
  }
  LoProfTag tag("attn%d dx", site);
  return lo_conv_run(h->g_att_dx, {.in = dqkv, .w = WSP(f16, a.o_wt), .add_src = dy, .out = dx}, st);
}

// Final conv, up4..up1, decoder.fc, dz: the gradients from decoder.fc.weight to the end of the buffer are complete afterwards (the
// decoder's GroupNorm / bias gradients after their finalize).  dz32 (Decoder.forward's own backward): dz also as fp32
int VaeBackward::decoder_chain(int fused, const float* recon, const float* target, const float* drecon, bool fac, float* dz32) {
  const int B = h->B, L = h->L;
  // ---- final conv (+tanh, + fused MSE gradient; fused == 2: the reconstruction's gradient is the explicit drecon, only the latent seeds are lo_vae_loss's)
  const bool fr = fused == 1;
  if (fr || drecon) {
    LoHandover ho(h, side && !lo_event_marker());     // rides on the kernel; the dw / db column sums follow it on the side stream
    LO_TRY(lo_final_conv_bwd(WSP(f16, h->dec[3].o_a), PRM(h->idx_final_w), recon, fr ? target : nullptr, fr ? nullptr : drecon,
                             fr ? WSP(float, h->o_coefs) : nullptr, loss_scale, Ga, WSP(float, h->o_lc_part),
                             GRD(h->idx_final_w), GRD(h->idx_final_b), B, inv, st, ho.ev ? h->side : nullptr, ho.ev));
  } else {
    LO_HIP(hipMemsetAsync(Ga, 0, (size_t)B * 128 * 128 * 32 * 2, st));
  }
  // ---- decoder: up4..up1.  Ga holds the gradient wrt the stage's (activation [+ skip]) output.
  const f16* gout = Ga;
  for (int s = 3; s >= 0; --s) {
    // with the attention site, up1 read its output y, and the gradient wrt y gets a buffer of its own (it stays inspectable)
    const f16* layer_in = s > 0 ? WSP(f16, h->dec[s - 1].o_a) : WSP(f16, h->attn ? h->att[1].o_y : h->o_h0);
    f16* din = s > 0 ? WSP(f16, h->o_skipg[3 - s]) : (h->attn ? WSP(f16, h->att[1].o_dy) : Ga);   // up4->skipg[0] (wrt up3 out), up3->skipg[1], up2->skipg[2], up1->Ga
    // mode 1 (skip add) has the same du as mode 0; the skip branch receives gout unchanged (kept in skipg)
    LO_TRY(layer(h->dec[s], gout, nullptr, 0, layer_in, nullptr, din, nullptr, vae_dgrad_prod(h, h->dec[s]), true));
    gout = din;
  }
  // gout == Ga: gradient wrt h0 [B,8,8,512] NHWC (with the attention site: wrt its output; its backward leaves the one wrt h0)
  if (h->attn) {
    LO_TRY(attention(1, gout, WSP(f16, h->att[1].o_dx), true));
    gout = WSP(f16, h->att[1].o_dx);
  }
  // ---- decoder.fc
  // The bias and weight gradients of the two Linear layers feed nothing on the dependent chain (72 us of it in round 2): with a
  // side stream they run there, behind an event that rides on the launch producing their operand (LO_LAUNCH_STOP).  o_wslab_lin
  // stays theirs alone (two launches, in order on one stream); Gfc is a buffer of its own because the chain reuses Gb.
  hipStream_t gs = side ? h->side : st;
  f16* Gfc = WSP(f16, h->o_gfc);
  {
    LoHandover ho(h, side);
    LO_TRY(lo_nhwc_to_nchw_f16(gout, Gfc, B, 64, 512, st));                 // Gfc = dy of decoder.fc, [B][32768] c-major
    LO_TRY(ho.finish(st));
    if (side) LO_HIP(hipStreamWaitEvent(h->side, ho.ev, 0));
  }
  LO_TRY(lo_colsum_f16(Gfc, GRD(h->idx_dfc_b), B, 32768, inv, gs));
  if (!fac)      // factored mode: dW = Gfc^T z is never formed (its factors are transposed with the encoder heads')
    LO_TRY(lo_wgrad_run(h->g_dfc, WSP(f16, h->o_z), Gfc, WSP(float, h->o_wslab_lin), GRD(h->idx_dfc_w), inv, gs));
  LO_TRY(lo_conv_run(h->g_dfc_d, {.in = Gfc, .w = WSP(f16, h->o_wp_dfc_t), .slab = WSP(float, h->o_slab_dz), .nsplit = h->dfcd_split}, st));
  return lo_splitk_reduce(WSP(float, h->o_slab_dz), nullptr, dz32, WSP(f16, h->o_dz), B, L, h->dfcd_split, st);
}

// KL + reparameterisation backward (train_hybrid.py:862; lunar_generate.py:259-261) from dz, then the encoder heads: Ga = gradient wrt
// the encoder's output.  beside: the heads' bias and weight gradients run on the side stream (see decoder.fc above).  hand_to_side:
// the side stream is then ordered behind the last launch here as well (ev_pre rides on it).
int VaeBackward::latent_and_heads(int fused, const float* gmu, const float* glv, bool fac, bool beside, bool hand_to_side) {
  const int B = h->B, L = h->L;
  beside = beside && side;
  hipStream_t gs = beside ? h->side : st;
  {
    LoHandover ho(h, beside);
    LO_TRY(lo_latent_bwd(WSP(f16, h->o_dz), WSP(float, h->o_mu), WSP(float, h->o_lv), WSP(float, h->o_eps),
                         fused ? WSP(float, h->o_coefs) : nullptr, fused ? nullptr : gmu, fused ? nullptr : glv, loss_scale,
                         WSP(f16, h->o_dml), B, L, st));
    LO_TRY(ho.finish(st));
    if (beside) LO_HIP(hipStreamWaitEvent(h->side, ho.ev, 0));
  }
  LO_TRY(lo_colsum_f16(WSP(f16, h->o_dml), GRD(h->idx_fc_mu_b), B, 2 * L, inv, gs));
  if (fac) {
    // the four factors, transposed and batch-padded, are what the optimizer's AdamW pass multiplies: one launch
    const f16* src[4] = {WSP(f16, h->o_dml), WSP(f16, h->o_xflat), WSP(f16, h->o_gfc), WSP(f16, h->o_z)};
    f16* dst[4] = {WSP(f16, h->o_fac_dmlT), WSP(f16, h->o_fac_xT), WSP(f16, h->o_fac_gfcT), WSP(f16, h->o_fac_zT)};
    const int Cs[4] = {2 * L, 32768, 32768, L};
    LO_TRY(lo_transpose_pad_f16_multi(src, dst, Cs, 4, B, h->Bp, gs));
  } else {
    LO_TRY(lo_wgrad_run(h->g_head, WSP(f16, h->o_xflat), WSP(f16, h->o_dml), WSP(float, h->o_wslab_lin), GRD(h->idx_fc_mu_w), inv, gs));
  }
  LO_TRY(lo_conv_run(h->g_head_d, {.in = WSP(f16, h->o_dml), .w = WSP(f16, h->o_wp_head_t), .out = Gb}, st));
  // with the attention site this is the gradient wrt ITS output; its backward leaves the one wrt the stage-4 output in the site's dx,
  // where encoder_stages picks it up
  f16* genc = h->attn ? WSP(f16, h->att[0].o_dy) : Ga;
  {
    LoHandover ho(h->ev_pre, beside && hand_to_side);
    LO_TRY(lo_nchw_to_nhwc_f16(Gb, genc, B, 64, 512, st));                // Ga = gradient wrt enc4 output, NHWC
    LO_TRY(ho.finish(st));
    if (ho.ev) LO_HIP(hipStreamWaitEvent(h->side, ho.ev, 0));
  }
  if (h->attn) LO_TRY(attention(0, genc, WSP(f16, h->att[0].o_dx), beside));
  return LO_OK;
}

// Single-call backward with lo_vae_set_gradnorm_scratch: everything from fc_mu.weight on is final once the decoder's side-stream
// weight gradients are, so its sum of squares is taken here -- on the side stream (which latent_and_heads has ordered behind the
// chain) beside the encoder backward.  The decoder's GroupNorm / bias gradients belong to the range: finalized here.
int VaeBackward::early_norm(bool fac1) {
  const int L = h->L;
  hipStream_t ns = side ? h->side : st;
  LO_TRY(finalize(0u, true, ns));
  if (!fac1) return lo_sumsq_range(G, h->p_off[h->idx_fc_mu_w], h->flat_elems, h->norm_scratch, ns);
  // scratch[512..1024) = partial sums of squares of the range: [512, 767) everything behind decoder.fc.weight (decoder.fc.bias,
  // the decoder's convs and GroupNorms, the final conv), [767] the two head biases, [768, 896) fc_mu | fc_logvar weights and
  // [896, 1024) decoder.fc.weight from the Gram matrices of their factors -- no pass over the 50 M elements they stand for
  const size_t bh = h->p_off[h->idx_fc_mu_w], nh = (size_t)2 * L * 32768, bd = h->p_off[h->idx_dfc_w], nd = (size_t)32768 * L;
  float* sc = h->norm_scratch;
  LO_TRY(lo_sumsq_blocks(G + bd + nd, h->flat_elems - (bd + nd), sc + 512, 255, ns));
  LO_TRY(lo_sumsq_blocks(G + bh + nh, bd - (bh + nh), sc + 767, 1, ns));
  const LoLowrankNorm nl[2] = {{WSP(f16, h->o_dml), 2 * L, WSP(f16, h->o_xflat), 32768, WSP(float, h->o_gram), sc + 768, 128},
                               {WSP(f16, h->o_z), L, WSP(f16, h->o_gfc), 32768, WSP(float, h->o_gram) + 128 * 128, sc + 896, 128}};
  LO_TRY(lo_lowrank_sumsq(nl, 2, h->B, inv, ns));
  h->fac.scale = inv;
  h->fac.ready = true;
  return LO_OK;
}

// encoder stages s_hi+1 .. s_lo+1 (4..1: s = 3..0) from Ga = gradient wrt the output of stage s_hi+1; dx (with stage 1; NULL = not
// wanted): the gradient wrt the images, fp32 NCHW [B,3,128,128]
int VaeBackward::encoder_stages(int s_hi, int s_lo, const float* x, float* dx) {
  const int B = h->B;
  for (int s = s_hi; s >= s_lo; --s) {
    ConvLayer& c0 = h->enc[s][0];
    ConvLayer& c1 = h->enc[s][1];
    ConvLayer& c2 = h->enc[s][2];
    // ResBlock tail + conv2:  dy = Ga -> ds = Gb (identity branch) ; dgrad -> Gd (grad wrt conv1 activation)
    const f16* gtop = (s == 3 && h->attn) ? WSP(f16, h->att[0].o_dx) : Ga;      // stage 4 behind the attention site: see latent_and_heads
    LO_TRY(layer(c2, gtop, WSP(f16, c0.o_a), 2, WSP(f16, c1.o_a), Gb, Gd, nullptr, vae_dgrad_prod(h, c2)));
    // conv1: dy = Gd ; dgrad (+ ds) -> Gc (grad wrt the block input = c0 activation)
    LO_TRY(layer(c1, Gd, nullptr, 0, WSP(f16, c0.o_a), nullptr, Gc, Gb, vae_dgrad_prod(h, c1)));
    if (s > 0) {
      // strided conv: dy = Gc ; dgrad (+ decoder skip gradient) -> Ga (grad wrt the previous stage output)
      LO_TRY(layer(c0, Gc, nullptr, 0, WSP(f16, h->o_eout[s - 1]), nullptr, Ga, WSP(f16, h->o_skipg[s - 1]), vae_dgrad_prod(h, c0)));
      continue;
    }
    // (the first conv's weight gradient on the side stream with the finalize beside it: neutral in round 2 and again in round 3
    // with launch-bound events, 22 900-23 137 against 22 864-23 106 -- it stays on this stream)
    const f16* dv0 = Gd;
    if (c0.dv_done) dv0 = WSP(f16, c0.o_dv);      // conv1's data gradient has already applied this layer's GroupNorm backward
    else
      LO_TRY(gn_backward(c0, {.dy = Gc, .dv = Gd}));
    LO_TRY(lo_first_conv_wgrad(x, dv0, WSP(float, h->o_fcw_part), GRD(c0.p_w), B, inv, st));
    // the images' gradient (lo_vae_backward_dx / lo_vae_encoder_backward_dx): the same dv0 through the transposed first conv
    if (dx) LO_TRY(lo_image_dgrad(dv0, 64, 2, PRM(c0.p_w), B, inv, dx, st));
  }
  return LO_OK;
}

// Asynchronous hand-over of a finished gradient range (lo_vae_set_async_handover): the caller's stream is NOT held up until the side
// stream's weight gradients have finished; the side stream -- ordered behind the chain by the caller -- finalizes the range's
// GroupNorm / bias gradients and leaves "the range is final" as an event that lo_vae_wait_handover puts in front of the exchange
int VaeBackward::publish_range(unsigned enc_mask, bool dec) {
  LO_TRY(finalize(enc_mask, dec, h->side));
  LO_HIP(hipEventRecord(h->ev_range, h->side));
  h->range_pending = true;
  return LO_OK;
}

// what every backward entry point checks first (fwd_ran: the forward whose activations it reads)
int vae_backward_checks(const LoVae* h, bool args_ok, bool fwd_ran, int fused, const float* target, float loss_scale) {
  LO_REQUIRE(args_ok, "lo_vae_backward: null argument");
  LO_REQUIRE(fused >= 0 && fused <= 2, "lo_vae_backward: fused must be 0 (explicit), 1 (lo_vae_loss) or 2 (lo_vae_loss's latent seeds, explicit drecon), got %d", fused);
  if (!fwd_ran) { lo_set_error("lo_vae_backward: the forward this backward belongs to has not run"); return LO_ERR_STATE; }
  if (fused && (!h->loss_done || !target)) { lo_set_error("lo_vae_backward: fused mode needs lo_vae_loss and a target"); return LO_ERR_STATE; }
  LO_REQUIRE(loss_scale > 0.f, "lo_vae_backward: loss_scale must be positive");
  return LO_OK;
}
}  // namespace

// dx (NULL = not wanted): the gradient wrt the images, fp32 NCHW [B,3,128,128]
extern "C" int lo_vae_backward_dx(LoVae* h, const float* x, const float* P, void* ws, const float* recon, const float* target,
                                  int fused, const float* drecon, const float* gmu, const float* glv, float loss_scale,
                                  float* G, float* dx, void* stream) {
  const bool args_ok = h && P && ws && G && x && recon;
  LO_TRY(vae_backward_checks(h, args_ok, args_ok && h->forward_done, fused, target, loss_scale));
  LO_REQUIRE(fused != 2 || drecon, "lo_vae_backward: fused = 2 needs the explicit drecon");
  VaeBackward b(h, P, G, ws, loss_scale, stream);
  LO_TRY(b.begin(true));
  // the Linear layers' weight gradients stay factored (lo_lowrank.hip): the fused single-call backward of a stepper only
  const bool fac1 = vae_single_leaves_factors(h) && fused;
  if (fac1 && !h->norm_scratch) { lo_set_error("lo_vae_backward: the factored Linear-gradient mode needs lo_vae_set_gradnorm_scratch"); return LO_ERR_STATE; }
  h->fac.ready = false;
  // decoder layers finalized early, norm of [fc_mu.weight, end) taken beside the encoder backward
  const bool early = h->norm_scratch && (b.side || fac1);
  LO_TRY(vae_zero_gaps(h, G, (b.side && fused) ? h->side : b.st));
  LO_TRY(b.decoder_chain(fused, recon, target, drecon, fac1, nullptr));
  LO_TRY(b.latent_and_heads(fused, gmu, glv, fac1, true, h->norm_scratch != nullptr));
  if (early) LO_TRY(b.early_norm(fac1));
  LO_TRY(b.encoder_stages(3, 0, x, dx));
  // GroupNorm affine + conv bias gradients of all 16 layers in one launch.  Reads P1 / P2 rows only (all written on this stream):
  // before the join, beside the side stream's last weight gradients
  LO_TRY(b.finalize(0xFu, !early, b.st));
  LO_TRY(b.join());
  return vae_check_gn_replay(h);      // what lo_vae_layer_plan_ex reports of the GroupNorm backwards is what this backward did
}
extern "C" int lo_vae_backward(LoVae* h, const float* x, const float* P, void* ws, const float* recon, const float* target,
                               int fused, const float* drecon, const float* gmu, const float* glv, float loss_scale,
                               float* G, void* stream) {
  return lo_vae_backward_dx(h, x, P, ws, recon, target, fused, drecon, gmu, glv, loss_scale, G, nullptr, stream);
}

// The backward in two calls (phase 1: final conv, decoder, Linear layers; 2: the whole encoder) or three (1; 3: encoder stage 4;
// 4: stages 3..1), so that a data-parallel caller can exchange each finished gradient range while the next phase runs
extern "C" int lo_vae_backward_phase(LoVae* h, int phase, const float* x, const float* P, void* ws, const float* recon,
                                     const float* target, int fused, const float* drecon, const float* gmu, const float* glv,
                                     float loss_scale, float* G, void* stream) {
  LO_REQUIRE(phase >= 1 && phase <= 4, "lo_vae_backward_phase: phase must be 1 (final conv, decoder, Linear layers), 2 (whole encoder), "
             "3 (encoder stage 4) or 4 (encoder stages 3..1, after 3)");
  const bool args_ok = h && P && ws && G && x && recon;
  LO_TRY(vae_backward_checks(h, args_ok, args_ok && h->forward_done, fused, target, loss_scale));
  LO_REQUIRE(fused != 2 || drecon, "lo_vae_backward: fused = 2 needs the explicit drecon");
  VaeBackward b(h, P, G, ws, loss_scale, stream);
  LO_TRY(b.begin(phase == 1));
  const bool async = b.side && h->async_handover;
  if (phase == 1) {
    const bool facdp = vae_phased_leaves_factors(h) && fused;    // data parallel: the factors leave this rank, not the gradients
    h->fac.ready = false;
    LO_TRY(vae_zero_gaps(h, G, (b.side && fused) ? h->side : b.st));
    LO_TRY(b.decoder_chain(fused, recon, target, drecon, facdp, nullptr));
    LO_TRY(b.latent_and_heads(fused, gmu, glv, facdp, true, async));
    if (facdp) h->fac.scale = b.inv;
    // every gradient from fc_mu.weight to the end of the buffer is complete now: hand the range over, or join the side stream
    // (decoder weight gradients) and finish the decoder's GroupNorm / bias gradients, so that the caller can start exchanging
    // that range while the encoder backward runs
    if (async) return b.publish_range(0u, true);
    LO_TRY(b.join());
    return b.finalize(0u, true, b.st);
  }
  LO_TRY(b.encoder_stages(phase == 4 ? 2 : 3, phase == 3 ? 3 : 0, x, nullptr));
  if (phase == 3 && async) {      // see phase 1: the stage-4 range, without a join
    LO_TRY(vae_order(h->side, b.st, h->ev_pre));
    return b.publish_range(0x8u, false);
  }
  // the GroupNorm / bias gradients of the stages this call ran, before the join (see lo_vae_backward_dx)
  LO_TRY(b.finalize(phase == 3 ? 0x8u : (phase == 4 ? 0x7u : 0xFu), false, b.st));
  return b.join();
}

// Backward of lo_vae_decode_skips (Decoder.forward, lunar_generate.py:194-229): drecon [B,3,128,128] -> dz [B,L], the gradients
// of the skip maps that were added (fp32 NCHW, NULL = not wanted) and the decoder's parameter gradients (decoder.fc.weight to
// the end of flat_grads; the encoder range is not written).
extern "C" int lo_vae_decoder_backward(LoVae* h, const float* P, void* ws, const float* recon, const float* drecon, float loss_scale,
                                       float* dz, float* dskip0, float* dskip1, float* dskip2, float* G, void* stream) {
  LO_REQUIRE(h && drecon && dz, "lo_vae_decoder_backward: null argument");
  LO_TRY(vae_backward_checks(h, P && ws && G && recon, h->dec_done, 0, nullptr, loss_scale));
  VaeBackward b(h, P, G, ws, loss_scale, stream);
  const int B = h->B;
  float* dskip[3] = {dskip0, dskip1, dskip2};
  LO_TRY(b.begin(true));
  // G is a fresh block of PyTorch's caching allocator here, which is ordered with respect to the CALLER's stream only: the gaps are
  // zeroed on that stream (see vae_zero_gaps)
  LO_TRY(vae_zero_gaps(h, G, b.st));
  LO_TRY(b.decoder_chain(0, recon, nullptr, drecon, false, dz));
  // dz and the skip-map gradients leave un-scaled as fp32 (the gradient of skips[k] is the gradient of the sum it was added into,
  // which the data gradient of the next transposed conv has left in skipg[k])
  LO_TRY(lo_scale_f32(dz, (size_t)B * h->L, b.inv, b.st));
  for (int k = 0; k < 3; ++k)
    if (dskip[k]) LO_TRY(lo_nhwc_f16_to_nchw_f32(WSP(f16, h->o_skipg[k]), dskip[k], B, (64 >> k) * (64 >> k), 64 << k, b.inv, b.st));
  LO_TRY(b.join());
  return b.finalize(0u, true, b.st);
}
// Backward of lo_vae_encode (Encoder.forward, lunar_generate.py:127-153): upstream gradients of mu, logvar [B,L] and of the skip
// maps (fp32 NCHW; any of them may be NULL = zero) -> the encoder's parameter gradients ([0, decoder.fc.weight) of flat_grads).
// lo_vae_encoder_backward_dx also writes the gradient wrt x (fp32 NCHW [B,3,128,128]; NULL = not wanted).
extern "C" int lo_vae_encoder_backward_dx(LoVae* h, const float* x, const float* P, void* ws, const float* gmu, const float* glv,
                                          const float* gskip0, const float* gskip1, const float* gskip2, float loss_scale, float* G,
                                          float* dx, void* stream) {
  const bool args_ok = h && P && ws && G && x;
  LO_TRY(vae_backward_checks(h, args_ok, args_ok && h->enc_done, 0, nullptr, loss_scale));
  VaeBackward b(h, P, G, ws, loss_scale, stream);
  const int B = h->B;
  const float* gskip[3] = {gskip0, gskip1, gskip2};
  LO_TRY(b.begin(true));
  LO_TRY(vae_zero_gaps(h, G, b.st));
  for (int k = 0; k < 3; ++k) {
    const size_t n = (size_t)B * (64 >> k) * (64 >> k) * (64 << k);
    if (gskip[k]) LO_TRY(lo_nchw_f32_to_nhwc_f16(gskip[k], WSP(f16, h->o_skipg[k]), B, (64 >> k) * (64 >> k), 64 << k, loss_scale, b.st));
    else LO_HIP(hipMemsetAsync(WSP(f16, h->o_skipg[k]), 0, n * 2, b.st));
  }
  LO_HIP(hipMemsetAsync(WSP(f16, h->o_dz), 0, (size_t)B * h->L * 2, b.st));      // no decoder behind the latent: dz = 0
  LO_TRY(b.latent_and_heads(0, gmu, glv, false, false, false));                   // everything on the caller's stream
  LO_TRY(b.encoder_stages(3, 0, x, dx));
  LO_TRY(b.finalize(0xFu, false, b.st));
  return b.join();
}
extern "C" int lo_vae_encoder_backward(LoVae* h, const float* x, const float* P, void* ws, const float* gmu, const float* glv,
                                       const float* gskip0, const float* gskip1, const float* gskip2, float loss_scale, float* G,
                                       void* stream) {
  return lo_vae_encoder_backward_dx(h, x, P, ws, gmu, glv, gskip0, gskip1, gskip2, loss_scale, G, nullptr, stream);
}
