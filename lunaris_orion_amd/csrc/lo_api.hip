// C ABI (include/lunaris_hip.h): the single-op entry points.  The native VAE step executor is in lo_vae_*.hip.
#include "lo_internal.h"
#include "lo_conv.h"
#include "lo_norm.h"
#include "../../include/lunaris_hip.h"
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <vector>


extern "C" const char* lo_last_error(void) { return lo_get_error(); }
extern "C" int lo_version(void) { return 1; }

// =============================================================================================
// single-op entry points
// =============================================================================================
extern "C" size_t lo_packed_weight_elems_for(int kind, int B, int H, int W, int Cin, int Cout) {
  LoGeom g;
  if (lo_make_geom(&g, kind, B, H, W, Cin, Cout) != LO_OK) return 0;
  return lo_packed_weight_elems(g);
}
extern "C" int lo_pack_weight_for(int kind, int B, int H, int W, int Cin, int Cout, const float* w, void* wp, void* stream) {
  LoGeom g;
  LO_TRY(lo_make_geom(&g, kind, B, H, W, Cin, Cout));
  return lo_pack_weight(w, (f16*)wp, g, S(stream));
}
extern "C" int lo_conv_forward(int kind, int B, int H, int W, int Cin, int Cout, const void* in, const void* wp,
                               const float* bias, const void* add_src, void* out, float* gn_partial, int* mt_out,
                               void* stream) {
  LoGeom g;
  LO_TRY(lo_make_geom(&g, kind, B, H, W, Cin, Cout));
  const LoConvOp op{.in = (const f16*)in, .w = (const f16*)wp, .bias = bias, .add_src = (const f16*)add_src, .out = (f16*)out, .gn_partial = gn_partial};
  if (mt_out) *mt_out = lo_conv_choose(g, lo_conv_use(op)).mts;
  return lo_conv_run(g, op, S(stream));
}
// fp8 (e4m3) operand forms of the same op: see LO_VAE_FP8_FWD in the header
extern "C" int lo_quantize_act_f8(const void* x16, void* x8, size_t n, void* stream) {
  LO_REQUIRE(x16 && x8, "lo_quantize_act_f8: null argument");
  return lo_quantize_f8((const f16*)x16, (uint8_t*)x8, n, S(stream));
}
extern "C" int lo_pack_weight_f8_for(int kind, int B, int H, int W, int Cin, int Cout, const void* wp16, void* wp8, float* wscale,
                                     void* stream) {
  LO_REQUIRE(wp16 && wp8 && wscale, "lo_pack_weight_f8_for: null argument");
  LoGeom g;
  LO_TRY(lo_make_geom(&g, kind, B, H, W, Cin, Cout));
  return lo_pack_f8_one(g, (const f16*)wp16, (uint8_t*)wp8, wscale, S(stream));
}
extern "C" int lo_conv_forward_f8(int kind, int B, int H, int W, int Cin, int Cout, const void* in8, const void* wp8,
                                  const float* wscale, const float* bias, const void* add_src, void* out, float* gn_partial,
                                  int* mt_out, void* stream) {
  LO_REQUIRE(in8 && wp8 && wscale && out, "lo_conv_forward_f8: null argument");
  LoGeom g;
  LO_TRY(lo_make_geom(&g, kind, B, H, W, Cin, Cout));
  const LoConvOp op{.bias = bias, .add_src = (const f16*)add_src, .out = (f16*)out, .gn_partial = gn_partial};
  LoConvUse use = lo_conv_use(op);
  use.f8 = true;
  if (mt_out) *mt_out = lo_conv_choose(g, use).mts;
  return lo_conv_run_f8(g, (const uint8_t*)in8, (const uint8_t*)wp8, wscale, op, S(stream));
}
// the teacher's 3x3 stride-1 convolution kernel (lo_conv3x3_pp) with its epilogue: bias, optional LeakyReLU(0.2), optional
// BatchNorm partial sums [B * (H/16) * (W/16)][Cout][2]; operands fp16 (fp8 == 0: in / wp as for lo_conv_forward) or e4m3
// (fp8 != 0: in / wp / wscale as for lo_conv_forward_f8)
extern "C" int lo_conv3x3_fused_tap_forward(int B, int H, int W, int Cin, int Cout, int fp8, const void* in, const void* wp, const float* wscale,
                                            const float* bias, int leaky_relu, void* out, float* bn_partial, void* stream) {
  LO_REQUIRE(in && wp && out && (!fp8 || wscale), "lo_conv3x3_fused_tap_forward: null argument");
  LoGeom g;
  LO_TRY(lo_make_geom(&g, LO_CONV3_S1, B, H, W, Cin, Cout));
  LoConvExtra ex{leaky_relu ? 1 : 0, bn_partial};
  if (fp8) return lo_conv3_run_pp_f8(g, (const uint8_t*)in, (const uint8_t*)wp, wscale, bias, (f16*)out, S(stream), &ex);
  return lo_conv3_run_pp_xf(g, (const f16*)in, nullptr, nullptr, 0, (const f16*)wp, bias, (f16*)out, S(stream), &ex);
}
// the wide teacher's 3x3 stride-1 convolution (feature_dim 256 / 512: 128 -> F, F -> F) on e4m3 operands, implicit-GEMM form, with the
// teacher epilogue; operands as for lo_conv_forward_f8.  rows_out: the BatchNorm partial rows the launch wrote
extern "C" int lo_teacher_conv3x3_forward_f8(int B, int H, int W, int Cin, int Cout, const void* in8, const void* wp8, const float* wscale,
                                             const float* bias, int leaky_relu, void* out, float* bn_partial, int* rows_out, void* stream) {
  LO_REQUIRE(in8 && wp8 && wscale && out, "lo_teacher_conv3x3_forward_f8: null argument");
  LoGeom g;
  LO_TRY(lo_make_geom(&g, LO_CONV3_S1, B, H, W, Cin, Cout));
  const LoConvExtra ex{leaky_relu ? 1 : 0, bn_partial};
  const LoConvOp op{.bias = bias, .out = (f16*)out, .ex = &ex};
  LoConvUse use = lo_conv_use(op);
  use.f8 = true;
  const LoConvChoice c = lo_conv_choose(g, use);
  LO_REQUIRE(c.kernel == LO_CK_IGEMM_F8 && (B * H * W) % c.bm == 0,
             "lo_teacher_conv3x3_forward_f8: %d -> %d channels on %d x %d x %d is not served on e4m3 operands (Cin %% 128, Cout %% 64, whole M tiles)",
             Cin, Cout, B, H, W);
  if (rows_out) *rows_out = c.rows;
  return lo_conv_run_f8(g, (const uint8_t*)in8, (const uint8_t*)wp8, wscale, op, S(stream));
}
extern "C" int lo_linear_splitk(int M, int K, int N, const void* x, const void* wp, const float* bias, float* slab,
                                int nsplit, float* out32, void* out16, void* stream) {
  LoGeom g;
  LO_TRY(lo_make_geom(&g, LO_LINEAR, M, 1, 1, K, N));
  LO_TRY(lo_conv_run(g, {.in = (const f16*)x, .w = (const f16*)wp, .slab = slab, .nsplit = nsplit}, S(stream)));
  return lo_splitk_reduce(slab, bias, out32, (f16*)out16, M, N, nsplit, S(stream));
}
extern "C" size_t lo_wgrad_slab_bytes_for(int kind, int B, int H, int W, int Cin, int Cout) {
  LoGeom g;
  if (lo_make_geom(&g, kind, B, H, W, Cin, Cout) != LO_OK) return 0;
  return lo_wgrad_slab_bytes(g);
}
extern "C" int lo_conv_wgrad(int kind, int B, int H, int W, int Cin, int Cout, const void* x, const void* dy, float* slab,
                             float* grad, float scale, void* stream) {
  LoGeom g;
  LO_REQUIRE(kind == LO_CONV3_S1 || kind == LO_CONV3_S2 || kind == LO_CONVT4_S2 || kind == LO_LINEAR,
             "lo_conv_wgrad: kind %d is not a forward op", kind);
  LO_TRY(lo_make_geom(&g, kind, B, H, W, Cin, Cout));
  return lo_wgrad_run(g, (const f16*)x, (const f16*)dy, slab, grad, scale, S(stream));
}
extern "C" int lo_gn_mish_forward(const void* v, const float* gn_partial, int MT, const float* gamma, const float* beta,
                                  const void* other, void* y, float* stats, int B, int HW, int C, int mode, void* stream) {
  return lo_gn_forward({(const f16*)v, stats, gamma, beta, B, HW, C},
                       {.partial = gn_partial, .MT = MT, .other = (const f16*)other, .mode = mode, .y = (f16*)y}, S(stream));
}
extern "C" int lo_gn_nchunk_for(int HW, int C) { return lo_gn_nchunk(HW, C); }
extern "C" int lo_gn_mish_backward(const void* dy, const void* v, const void* other, const float* stats, const float* gamma,
                                   const float* beta, void* ds, void* dv, float* P1, float* P2, float* dgamma, float* dbeta,
                                   float* dbias, int B, int HW, int C, int mode, float scale, void* stream) {
  return lo_gn_bwd({(const f16*)v, stats, gamma, beta, B, HW, C},
                   {.dy = (const f16*)dy, .other = (const f16*)other, .mode = mode, .ds = (f16*)ds, .dv = (f16*)dv, .P1 = P1, .P2 = P2},
                   dgamma, dbeta, dbias, scale, S(stream));
}
extern "C" int lo_first_conv_forward(const float* x, const float* w, const float* bias, void* v, float* gn_partial, int B,
                                     void* stream) {
  return lo_first_conv_fwd(x, w, bias, (f16*)v, gn_partial, B, S(stream));
}
extern "C" int lo_first_conv_wgrad_op(const float* x, const void* dv, float* partial, float* dw, int B, float scale, void* stream) {
  return lo_first_conv_wgrad(x, (const f16*)dv, partial, dw, B, scale, S(stream));
}
extern "C" int lo_image_dgrad_op(const void* dy, int cout, int stride, const float* w, int B, float scale, float* dx, void* stream) {
  return lo_image_dgrad((const f16*)dy, cout, stride, w, B, scale, dx, S(stream));
}
extern "C" int lo_image_dgrad_seed_op(const void* dy, int cout, int stride, const float* w, int B, float scale, const float* seed_coef,
                                      const float* recon, const float* target, float* dx, void* stream) {
  const LoImgSeed seed{seed_coef, recon, target};
  return lo_image_dgrad((const f16*)dy, cout, stride, w, B, scale, dx, S(stream), &seed);
}
extern "C" int lo_final_conv_forward(const void* a4, const float* w, const float* bias, const float* target, float* recon,
                                     float* mse_partial, int B, void* stream) {
  return lo_final_conv_fwd((const f16*)a4, w, bias, target, recon, mse_partial, B, S(stream));
}
extern "C" int lo_final_conv_backward(const void* a4, const float* w, const float* recon, const float* target,
                                      const float* drecon, const float* coef_dev, float gscale, void* da4, float* partial,
                                      float* dw, float* db, int B, float scale, void* stream) {
  return lo_final_conv_bwd((const f16*)a4, w, recon, target, drecon, coef_dev, gscale, (f16*)da4, partial, dw, db, B, scale,
                           S(stream));
}
extern "C" int lo_clip_adamw_step(float* p, const float* g, float* m, float* v, size_t n, float max_norm, float lr,
                                  float beta1, float beta2, float eps, float weight_decay, int step, float* scratch,
                                  void* stream) {
  LO_TRY(lo_gradnorm(g, n, max_norm, scratch, scratch + 1024, S(stream)));
  return lo_adamw(p, g, m, v, n, scratch + 1024, lr, beta1, beta2, eps, weight_decay, step, S(stream));
}

// The same step for a caller whose lo_vae_backward already left the sum of squares of [presummed_begin, n) in the scratch
// (lo_vae_set_gradnorm_scratch): only the head of the buffer is read for the norm.
extern "C" int lo_clip_adamw_step_presummed(float* p, const float* g, float* m, float* v, size_t n, size_t presummed_begin, float max_norm,
                                            float lr, float beta1, float beta2, float eps, float weight_decay, int step, float* scratch,
                                            void* stream) {
  LO_REQUIRE(p && g && m && v && scratch && presummed_begin <= n && presummed_begin % 4 == 0, "lo_clip_adamw_step_presummed: bad argument");
  LO_TRY(lo_gradnorm_split(g, presummed_begin, max_norm, scratch, scratch + 1024, S(stream)));
  return lo_adamw(p, g, m, v, n, scratch + 1024, lr, beta1, beta2, eps, weight_decay, step, S(stream));
}

// one micro-batch's gradients into the accumulator of its window (see lo_train.hip)
extern "C" int lo_grad_accumulate(float* acc, const float* g, size_t n, float scale, int first, void* stream) {
  return lo_grad_accumulate_run(acc, g, n, scale, first != 0, S(stream));
}

extern "C" int lo_decode_sprites_u8(const void* u8_hwc, float* out_chw, int B, void* stream) {
  LO_REQUIRE(u8_hwc && out_chw && B > 0, "lo_decode_sprites_u8: bad argument");
  return lo_decode_sprites((const uint8_t*)u8_hwc, out_chw, B, S(stream));
}

// op level: the latent / loss / column-sum launchers of the step (lo_train.hip) and its noise generator, as the executor calls them
extern "C" int lo_reparam_noise(uint64_t seed, size_t first, size_t n, float* out, void* stream) {
  LO_REQUIRE(out && n > 0, "lo_reparam_noise: bad argument");
  return lo_randn_fill(seed, first, n, out, S(stream));
}
extern "C" int lo_latent_forward_op(const float* slab, const float* bias, const float* eps_in, uint64_t seed, float* mu, float* logvar,
                                    void* z, float* eps_out, float* kl_partial, int B, int L, int nsplit, float* mu_user,
                                    float* logvar_user, void* stream) {
  LO_REQUIRE(slab && bias && mu && logvar && z && eps_out && kl_partial && B > 0 && L > 0 && nsplit > 0 && !mu_user == !logvar_user,
             "lo_latent_forward_op: bad argument");
  return lo_head_reduce(slab, bias, eps_in, seed, mu, logvar, (f16*)z, eps_out, kl_partial, B, L, nsplit, S(stream), mu_user, logvar_user);
}
extern "C" int lo_latent_backward_op(const void* dz, const float* mu, const float* logvar, const float* eps, const float* coefs,
                                     const float* gmu, const float* glv, float gscale, void* dml, int B, int L, void* stream) {
  LO_REQUIRE(dz && mu && logvar && eps && dml && B > 0 && L > 0, "lo_latent_backward_op: bad argument");
  return lo_latent_bwd((const f16*)dz, mu, logvar, eps, coefs, gmu, glv, gscale, (f16*)dml, B, L, S(stream));
}
extern "C" int lo_loss_finalize_op(const float* mse_partial, int n_mse, const float* kl_partial, int n_kl, float recon_weight,
                                   float kl_weight, float mean_advantage, const float* adv_dev, float accum, float loss_scale,
                                   float* losses, float* coefs, float n_rec, float n_lat, void* stream) {
  LO_REQUIRE(mse_partial && kl_partial && losses && coefs && n_mse > 0 && n_kl > 0, "lo_loss_finalize_op: bad argument");
  return lo_loss_finalize(mse_partial, n_mse, kl_partial, n_kl, recon_weight, kl_weight, mean_advantage, adv_dev, accum, loss_scale,
                          losses, coefs, n_rec, n_lat, S(stream));
}
extern "C" int lo_colsum_f16_op(const void* x, float* out, int M, int N, float scale, void* stream) {
  LO_REQUIRE(x && out && M > 0 && N > 0, "lo_colsum_f16_op: bad argument");
  return lo_colsum_f16((const f16*)x, out, M, N, scale, S(stream));
}

extern "C" int lo_selfattn2d_forward(const float* x, const float* wq, const float* bq, const float* wk, const float* bk,
                                     const float* wv, const float* bv, const float* gamma, float* q, float* k, float* v,
                                     float* out, int B, int C, int N, void* stream) {
  LO_REQUIRE(x && wq && bq && wk && bk && wv && bv && gamma && q && k && v && out, "lo_selfattn2d_forward: null argument");
  return lo_selfattn2d_fwd(x, wq, bq, wk, bk, wv, bv, gamma, q, k, v, out, B, C, N, S(stream));
}

extern "C" size_t lo_selfattn2d_backward_scratch_elems(int B, int C, int N) { return lo_selfattn2d_bwd_scratch(B, C, N); }
extern "C" int lo_selfattn2d_backward(const float* x, const float* wq, const float* wk, const float* wv, const float* gamma,
                                      const float* q, const float* k, const float* v, const float* dy, float* scratch, float* dx,
                                      float* dwq, float* dbq, float* dwk, float* dbk, float* dwv, float* dbv, float* dgamma, int B,
                                      int C, int N, void* stream) {
  LO_REQUIRE(x && wq && wk && wv && gamma && q && k && v && dy && scratch && dx && dwq && dbq && dwk && dbk && dwv && dbv && dgamma,
             "lo_selfattn2d_backward: null argument");
  return lo_selfattn2d_bwd(x, wq, wk, wv, gamma, q, k, v, dy, scratch, dx, dwq, dbq, dwk, dbk, dwv, dbv, dgamma, B, C, N, S(stream));
}

// data-parallel gradient exchange helpers (see lo_train.hip)
extern "C" int lo_dp_pack_f16(const float* g, void* wire, size_t n, float scale, void* stream) {
  LO_REQUIRE(g && wire, "lo_dp_pack_f16: null argument");
  return lo_dp_pack_f16_run(g, (f16*)wire, n, scale, S(stream));
}
extern "C" int lo_dp_unpack_f16_sumsq(const void* wire, float* g, size_t n, float inv_scale, float* scratch, void* stream) {
  LO_REQUIRE(g && wire && scratch, "lo_dp_unpack_f16_sumsq: null argument");
  return lo_dp_unpack_f16_sumsq_run((const f16*)wire, g, n, inv_scale, scratch, S(stream));
}
extern "C" int lo_dp_unpack_f16(const void* wire, float* g, size_t n, float inv_scale, void* stream) {
  LO_REQUIRE(g && wire, "lo_dp_unpack_f16: null argument");
  return lo_dp_unpack_f16_run((const f16*)wire, g, n, inv_scale, S(stream));
}
extern "C" int lo_dp_sum_shares(const void* recv, void* share, int world, size_t chunk, int is_f16, void* stream) {
  LO_REQUIRE(recv && share && world >= 1, "lo_dp_sum_shares: bad argument");
  return lo_dp_sum_shares_run(recv, share, world, chunk, is_f16, 1.0f / (float)world, S(stream));
}

// upstream-gradient normalisation of the nn.Module boundary (see lo_train.hip)
extern "C" int lo_grad_scale_pick(const float* g0, size_t n0, const float* g1, size_t n1, const float* g2, size_t n2, const float* g3,
                                  size_t n3, const float* g4, size_t n4, float* scratch, void* stream) {
  LO_REQUIRE(scratch, "lo_grad_scale_pick: null scratch");
  const float* g[5] = {g0, g1, g2, g3, g4};
  const size_t n[5] = {n0, n1, n2, n3, n4};
  return lo_grad_scale_pick_run(g, n, scratch, S(stream));
}
extern "C" int lo_scale_copy_dev(const float* src, float* dst, size_t n, const float* scale_dev, void* stream) {
  LO_REQUIRE(src && dst && scale_dev, "lo_scale_copy_dev: null argument");
  return lo_scale_copy_dev_run(src, dst, n, scale_dev, S(stream));
}
extern "C" int lo_grad_unscale_dev(float* x, size_t n, const float* scale_dev, const void* fail_word, void* stream) {
  LO_REQUIRE(x && scale_dev, "lo_grad_unscale_dev: null argument");
  return lo_scale_dev_run(x, n, scale_dev, (const unsigned int*)fail_word, S(stream));
}
