// C ABI (include/lunaris_hip.h) + the native VAE step executor: one C call enqueues every kernel of
// LunarisCoreVAE.forward (lunar_generate.py:263-276) or of its backward on the given HIP stream.
#include "lo_internal.h"
#include "../../include/lunaris_hip.h"
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <vector>

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
#define LO_TRY(call)            \
  do {                          \
    int _r = (call);            \
    if (_r != LO_OK) return _r; \
  } while (0)

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
  if (mt_out) *mt_out = lo_conv_mt(g);
  return lo_conv_run(g, (const f16*)in, (const f16*)wp, bias, (const f16*)add_src, (f16*)out, gn_partial, nullptr, 1, S(stream));
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
  if (mt_out) *mt_out = lo_conv_mt_f8(g);
  return lo_conv_run_f8(g, (const uint8_t*)in8, (const uint8_t*)wp8, wscale, bias, (const f16*)add_src, (f16*)out, gn_partial, S(stream));
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
extern "C" int lo_linear_splitk(int M, int K, int N, const void* x, const void* wp, const float* bias, float* slab,
                                int nsplit, float* out32, void* out16, void* stream) {
  LoGeom g;
  LO_TRY(lo_make_geom(&g, LO_LINEAR, M, 1, 1, K, N));
  LO_TRY(lo_conv_run(g, (const f16*)x, (const f16*)wp, nullptr, nullptr, nullptr, nullptr, slab, nsplit, S(stream)));
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
  return lo_gn_fwd((const f16*)v, gn_partial, MT, gamma, beta, (const f16*)other, (f16*)y, stats, B, HW, C, mode, S(stream));
}
extern "C" int lo_gn_nchunk_for(int HW, int C) { return lo_gn_nchunk(HW, C); }
extern "C" int lo_gn_mish_backward(const void* dy, const void* v, const void* other, const float* stats, const float* gamma,
                                   const float* beta, void* ds, void* dv, float* P1, float* P2, float* dgamma, float* dbeta,
                                   float* dbias, int B, int HW, int C, int mode, float scale, void* stream) {
  return lo_gn_bwd((const f16*)dy, (const f16*)v, (const f16*)other, stats, gamma, beta, (f16*)ds, (f16*)dv, P1, P2, dgamma,
                   dbeta, dbias, B, HW, C, mode, scale, S(stream));
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

extern "C" int lo_decode_sprites_u8(const void* u8_hwc, float* out_chw, int B, void* stream) {
  LO_REQUIRE(u8_hwc && out_chw && B > 0, "lo_decode_sprites_u8: bad argument");
  return lo_decode_sprites((const uint8_t*)u8_hwc, out_chw, B, S(stream));
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

// =============================================================================================
// VAE executor
// =============================================================================================
namespace {

struct ConvLayer {           // conv + GroupNorm + Mish
  int kind;                  // forward kind
  int H, W, Cin, Cout;       // input spatial dims / channels
  int Ho, Wo;                // output spatial dims
  LoGeom gf, gd;             // forward / data-gradient geometry
  int p_w, p_b, p_gw, p_gb;  // parameter indices (state_dict order)
  size_t o_wp_f, o_wp_d;     // workspace offsets: packed fp16 weights (fwd, dgrad)
  size_t o_v, o_a;           // raw conv output, activation after GN+Mish(+...)
  size_t o_part, o_stats;    // GN partial sums, saved stats
  size_t o_P1, o_P2;         // GN backward partial sums (kept until the fused finalize at the end of backward)
  int np1;                   // >0: P1 rows per sample written by the consumer's fused data-gradient epilogue
  int MT;
  size_t o_dv;               // gradient wrt the raw conv output (GroupNorm backward -> data / weight gradient); one per layer, so the
                             // side-stream weight gradient of layer k never shares a buffer with what the main stream writes next
  // fp8 operand mode (LO_VAE_FP8_FWD): e4m3 weights + per-row scales of the forward op, e4m3 copy of the activation o_a
  bool f8;                   // this layer's forward conv runs on e4m3 operands
  size_t o_wp8, o_wscale, o_a8;   // o_a8 = 0: no consumer needs the copy
  // GroupNorm + Mish fused into the forward conv's epilogue (LoGnFuse, lo_common.h): exchange lines, arrival counters, and how many
  // launches have used them (the counters are monotonic: launch k leaves them at k * tiles per sample)
  bool gnf; int gnf_mts, gnf_nt;
  size_t o_xbuf, o_xcnt;
  unsigned gnf_epoch;
  // GroupNorm-backward APPLY fused into the data-gradient epilogue of the layer that CONSUMES this layer's activation (LoGnBwdFuse):
  // arrival counters [B][8], launches so far, and -- per backward -- whether o_dv / P2 were already produced that way
  size_t o_bcnt;
  unsigned gba_epoch;
  bool dv_done; int np2;
  hipEvent_t ev_ready;   // dv_done: the event bound to the launch that wrote this layer's dv (null: none was bound)
  // few-rows layers (the 8 x 8 stage): forward / data gradient as a K-split 128 x 128-tile GEMM into fp32 slabs + ONE fused
  // (sample, group)-local pass (slab sum + bias + GroupNorm [+ Mish | backward]); 0 = the one-launch kernel
  int sk_fwd, sk_dgrad;
};

struct Arena {
  size_t off = 0;
  size_t take(size_t bytes) {
    size_t o = off;
    off += (bytes + 255) & ~(size_t)255;
    return o;
  }
};

}  // namespace

struct LoVae {
  int B, L;
  // parameters
  int nparam;
  std::vector<size_t> p_off, p_numel;
  size_t flat_elems;
  // layers: encoder stage s: enc[s][0] = strided conv, enc[s][1] = res.conv1, enc[s][2] = res.conv2
  ConvLayer enc[4][3];
  ConvLayer dec[4];
  size_t o_eout[4];          // ResBlock outputs (stage outputs)
  size_t o_skipin[3];        // skip feature maps handed to Decoder.forward from outside (lo_vae_decode_skips), fp16 NHWC
  // latent
  LoGeom g_head, g_head_d, g_dfc, g_dfc_d;
  int head_split, dfcd_split;
  size_t o_wp_head, o_wp_head_t, o_wp_dfc, o_wp_dfc_t;
  size_t o_xflat, o_slab_head, o_eps, o_z, o_klp, o_mu, o_lv, o_yfc, o_h0;
  size_t o_msep, o_losses, o_coefs;
  // backward scratch
  size_t o_G[6], o_skipg[3], o_P1, o_P2, o_wslab, o_wslab_lin, o_fcw_part, o_lc_part, o_dz, o_dml, o_slab_dz, o_gfc;
  size_t o_packjobs;
  std::vector<LoPackJob> packjobs_host;   // kept alive: source of the asynchronous table upload
  int n_packjobs, pack_blocks;
  int n_packjobs_enc, pack_blocks_enc;   // the early share of the table: encoder stages 1..3 (their jobs come first)
  const void* packjobs_for_ws;     // workspace / parameter pointers the uploaded job table was built for
  const void* packjobs_for_params;
  size_t ws_bytes;
  int idx_fc_mu_w, idx_fc_mu_b, idx_fc_lv_w, idx_fc_lv_b, idx_dfc_w, idx_dfc_b, idx_final_w, idx_final_b;
  bool forward_done, loss_done;
  bool enc_done, dec_done;   // activations of an encoder / decoder forward are in the workspace (split module calls)
  int dec_skips;             // how many skip maps the last decoder forward added (3 inside lo_vae_forward)
  // weight-gradient GEMMs run on a side stream, concurrently with the data-gradient / GroupNorm chain
  hipStream_t side;
  hipEvent_t ev_dv[4], ev_join, ev_pre, ev_range;
  bool async_handover, range_pending;   // lo_vae_set_async_handover: phase 1 / 3 leave their range's completion as an event on the side stream
  // Operand refresh on the side stream in five levels, one event each, recorded in this order (waiting for a level implies the
  // lower ones): 1 packed convs of encoder stages 1..3; 2 encoder stage 4 (parameters + packs); 3 the encoder heads (fc_mu /
  // fc_logvar: parameters + fp16 copy); 4 decoder.fc + decoder convs; 5 the transposed Linear copies only the backward reads
  hipEvent_t ev_lvl[6];
  bool lvl_pending[6];
  // pipelined optimizer step: levels 2..5 (AdamW of 97 % of the parameters + their operand refresh) are ENQUEUED by the next
  // forward once its first stage has run -- see lo_vae_optimizer_step
  struct { bool pending; float* P; const float* G; float* M; float* V; void* ws; const float* norm; float lr, beta1, beta2, eps, wd; int step; } defer;
  int n_packjobs_s4, pack_blocks_s4, n_packjobs8_s4, pack_blocks8_s4;   // job-table prefix up to and including encoder stage 4
  int bwd_layer;      // conv layers processed so far in the current backward (selects the dv buffer / events)
  size_t o_skslab;    // slabs of the split-K convolutions (one launch at a time on the caller's stream)
  bool gn_local;      // LO_GN_LOCAL=0: never use the one-pass (sample, group)-local GroupNorm backward
  int nevent;         // hand-over events handed out so far (ev_dv[nevent & 3])
  bool overlap;
  float* norm_scratch;   // lo_vae_set_gradnorm_scratch: where a single-call backward leaves the early part of the gradient norm
  bool fuse_gnb;      // fuse the GroupNorm-backward reduction into the producing data-gradient epilogue
  bool fuse_gnf;      // fuse GroupNorm + Mish of a conv output into that conv's epilogue (sample rendezvous between its workgroups)
  bool fuse_gna;      // fuse the GroupNorm-backward APPLY pass into the data-gradient epilogue that already carries its reduction
  size_t o_sync_fail; // one word: set by a workgroup whose rendezvous poll ran out (never, unless a launch was lost)
  // rank-B Linear-layer weight gradients kept as their factors (lo_lowrank.hip): transposed, batch-padded factor copies
  // dml^T [2L][Bp], xflat^T [32768][Bp], Gfc^T [32768][Bp], z^T [L][Bp] (one contiguous block), Gram scratch; fac_ready: a fused
  // backward has left this step's factors and the Gram part of the gradient norm; fac_scale: 1 / loss scale of that backward
  bool lin_factored, fac_ready;
  bool lin_factored_dp;      // data parallel: phase 1 leaves the factors (no Linear weight gradients); the ranks all-gather them
  int Bp;
  size_t o_fac_dmlT, o_fac_xT, o_fac_gfcT, o_fac_zT, o_gram;
  float fac_scale;
  int n_cu;           // compute units of the device (partition) this plan was made on; 0 = no device: nothing that waits across workgroups is planned
  const void* sync_for_ws;
  // fp8 operand mode of the forward convs (lo_vae_create_ex flag LO_VAE_FP8_FWD)
  bool fp8_fwd;
  size_t o_eout8[4], o_h08, o_packjobs8;
  std::vector<LoPackF8Job> packjobs8_host;
  int n_packjobs8, pack_blocks8;
  int n_packjobs8_enc, pack_blocks8_enc;
};

static int setup_conv_layer(ConvLayer& c, int kind, int B, int H, int W, int Cin, int Cout, int p_w, Arena& ar, bool first) {
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
    c.MT = lo_conv_mt(c.gf);
  } else {
    c.Ho = H / 2; c.Wo = W / 2;
    c.o_wp_f = c.o_wp_d = 0;
    c.MT = 64;
  }
  size_t act = (size_t)B * c.Ho * c.Wo * Cout * 2;
  c.o_v = ar.take(act);
  c.o_a = ar.take(act);
  c.o_part = ar.take((size_t)B * c.MT * 16 * 4);
  c.o_stats = ar.take((size_t)B * 16 * 4);
  int nchunk = lo_gn_nchunk(c.Ho * c.Wo, Cout);
  int p1rows = nchunk > (c.Ho * c.Wo) / 64 ? nchunk : (c.Ho * c.Wo) / 64;   // >= tiles per sample of any data-gradient epilogue
  c.np1 = 0;
  c.o_P1 = ar.take((size_t)B * p1rows * Cout * 2 * 4);
  c.o_P2 = ar.take((size_t)B * p1rows * Cout * 4);     // nchunk rows (lo_gn_bwd_apply) or one row per tile (fused apply)
  c.o_dv = ar.take(act);
  c.f8 = false;
  c.o_wp8 = c.o_wscale = c.o_a8 = 0;
  c.gnf = false; c.gnf_mts = c.gnf_nt = 0; c.gnf_epoch = 0;
  c.o_xbuf = ar.take((size_t)B * LO_GNF_MAX_TILES * 128);
  c.o_xcnt = ar.take((size_t)B * 4);
  c.o_bcnt = ar.take((size_t)B * 8 * 4);
  c.gba_epoch = 0; c.dv_done = false; c.np2 = 0; c.ev_ready = nullptr;
  c.sk_fwd = c.sk_dgrad = 0;
  return LO_OK;
}

extern "C" int lo_vae_create(int B, int L, LoVae** out) { return lo_vae_create_ex(B, L, 0u, out); }

extern "C" int lo_vae_create_ex(int B, int L, unsigned flags, LoVae** out) {
  LO_REQUIRE(out, "lo_vae_create: null out");
  LO_REQUIRE((flags & ~(unsigned)LO_VAE_FP8_FWD) == 0, "lo_vae_create_ex: unknown flag bits 0x%x", flags);
  LO_REQUIRE(B >= 1 && B <= 4096, "lo_vae_create: batch %d out of range", B);
  LO_REQUIRE(L >= 64 && L % 64 == 0 && L <= 4096, "lo_vae_create: latent_dim %d must be a multiple of 64", L);
  LoVae* h = new LoVae();
  h->B = B; h->L = L;
  h->forward_done = h->loss_done = h->enc_done = h->dec_done = false;
  h->dec_skips = 0;
  // ---- parameter table in state_dict order (lunar_generate.py:91-125, 162-192)
  std::vector<size_t> numel;
  const int ench[5] = {3, 64, 128, 256, 512};
  for (int s = 0; s < 4; ++s) {
    size_t ci = ench[s], co = ench[s + 1];
    numel.push_back(co * ci * 9); numel.push_back(co); numel.push_back(co); numel.push_back(co);
    for (int k = 0; k < 2; ++k) { numel.push_back(co * co * 9); numel.push_back(co); numel.push_back(co); numel.push_back(co); }
  }
  h->idx_fc_mu_w = (int)numel.size(); numel.push_back((size_t)L * 32768);
  h->idx_fc_mu_b = (int)numel.size(); numel.push_back(L);
  h->idx_fc_lv_w = (int)numel.size(); numel.push_back((size_t)L * 32768);
  h->idx_fc_lv_b = (int)numel.size(); numel.push_back(L);
  h->idx_dfc_w = (int)numel.size(); numel.push_back((size_t)32768 * L);
  h->idx_dfc_b = (int)numel.size(); numel.push_back(32768);
  const int dech[5] = {512, 256, 128, 64, 32};
  int dec_first = (int)numel.size();
  for (int s = 0; s < 4; ++s) {
    size_t ci = dech[s], co = dech[s + 1];
    numel.push_back(ci * co * 16); numel.push_back(co); numel.push_back(co); numel.push_back(co);
  }
  h->idx_final_w = (int)numel.size(); numel.push_back(3 * 32 * 9);
  h->idx_final_b = (int)numel.size(); numel.push_back(3);
  h->nparam = (int)numel.size();
  h->p_numel = numel;
  h->p_off.assign(h->nparam, 0);
  // flat layout: state_dict order, except that fc_logvar.weight directly follows fc_mu.weight and the two head
  // biases are adjacent, so the encoder head is ONE [2L, 32768] matrix; every tensor starts on a 64-element boundary.
  {
    size_t off = 0;
    auto place = [&](int i) { h->p_off[i] = off; off += (numel[i] + 63) & ~(size_t)63; };
    for (int i = 0; i < h->nparam; ++i) {
      if (i == h->idx_fc_mu_b || i == h->idx_fc_lv_w || i == h->idx_fc_lv_b) continue;
      place(i);
      if (i == h->idx_fc_mu_w) { place(h->idx_fc_lv_w); place(h->idx_fc_mu_b); place(h->idx_fc_lv_b); }
    }
    h->flat_elems = off;
  }
  // ---- workspace plan
  Arena ar;
  int Hs = 128;
  int pidx = 0;
  for (int s = 0; s < 4; ++s) {
    int ci = ench[s], co = ench[s + 1];
    LO_TRY(setup_conv_layer(h->enc[s][0], LO_CONV3_S2, B, Hs, Hs, ci, co, pidx, ar, s == 0));
    pidx += 4;
    Hs /= 2;
    LO_TRY(setup_conv_layer(h->enc[s][1], LO_CONV3_S1, B, Hs, Hs, co, co, pidx, ar, false));
    pidx += 4;
    LO_TRY(setup_conv_layer(h->enc[s][2], LO_CONV3_S1, B, Hs, Hs, co, co, pidx, ar, false));
    pidx += 4;
    h->o_eout[s] = ar.take((size_t)B * Hs * Hs * co * 2);
  }
  Hs = 8;
  for (int s = 0; s < 4; ++s) {
    LO_TRY(setup_conv_layer(h->dec[s], LO_CONVT4_S2, B, Hs, Hs, dech[s], dech[s + 1], dec_first + 4 * s, ar, false));
    Hs *= 2;
  }
  for (int k = 0; k < 3; ++k) h->o_skipin[k] = ar.take((size_t)B * (64 >> k) * (64 >> k) * (64 << k) * 2);
  // latent
  LO_TRY(lo_make_geom(&h->g_head, LO_LINEAR, B, 1, 1, 32768, 2 * L));     // [mu|logvar] = xflat W^T
  LO_TRY(lo_make_geom(&h->g_head_d, LO_LINEAR, B, 1, 1, 2 * L, 32768));   // dxflat = dml Wt^T  (Wt = W^T packed)
  LO_TRY(lo_make_geom(&h->g_dfc, LO_LINEAR, B, 1, 1, L, 32768));          // y = z Wd^T
  LO_TRY(lo_make_geom(&h->g_dfc_d, LO_LINEAR, B, 1, 1, 32768, L));        // dz = dy Wdt^T
  h->head_split = h->dfcd_split = 32;      // K splits of the two K = 32768 Linear GEMMs (8 / 16 / 32 / 64 measured in round 2: 32)
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
  // backward scratch
  size_t max_act = (size_t)B * 128 * 128 * 32 * 2;
  for (int i = 0; i < 4; ++i) h->o_G[i] = ar.take(max_act);
  h->o_G[4] = h->o_G[5] = 0;
  h->o_skipg[0] = ar.take((size_t)B * 64 * 64 * 64 * 2);    // grad wrt (up3.act + enc1.out)
  h->o_skipg[1] = ar.take((size_t)B * 32 * 32 * 128 * 2);   // grad wrt (up2.act + enc2.out)
  h->o_skipg[2] = ar.take((size_t)B * 16 * 16 * 256 * 2);   // grad wrt (up1.act + enc3.out)
  h->o_P1 = ar.take((size_t)B * 64 * 512 * 2 * 4);
  h->o_P2 = ar.take((size_t)B * 64 * 512 * 4);
  size_t wslab = 0;
  for (int s = 0; s < 4; ++s) {
    for (int k = 0; k < 3; ++k) {
      if (s == 0 && k == 0) continue;
      size_t b = lo_wgrad_slab_bytes(h->enc[s][k].gf);
      wslab = b > wslab ? b : wslab;
    }
    size_t b = lo_wgrad_slab_bytes(h->dec[s].gf);
    wslab = b > wslab ? b : wslab;
  }
  h->o_wslab = ar.take(wslab);
  // The two Linear weight gradients run on the MAIN stream while the decoder's conv weight gradients may still be running on
  // the side stream: they get their own slab.  (Found by the buffer audit of round 2: at latent 512 / 256 both Linear
  // gradients are written directly and never touch a slab, but at latent 64 / 128 lo_wgrad_nsplit() gives decoder.fc two
  // pixel splits, and sharing o_wslab with the side stream was a write-write race on those shapes.)
  {
    size_t b = lo_wgrad_slab_bytes(h->g_head), b2 = lo_wgrad_slab_bytes(h->g_dfc);
    h->o_wslab_lin = ar.take(b > b2 ? b : b2);
  }
  h->o_fcw_part = ar.take((size_t)B * 16 * 1728 * 4);
  h->o_lc_part = ar.take((size_t)B * 64 * 867 * 4);
  h->o_dz = ar.take((size_t)B * L * 2);
  h->o_dml = ar.take((size_t)B * 2 * L * 2);
  h->o_gfc = ar.take((size_t)B * 32768 * 2);    // dy of decoder.fc, channel-major: its own buffer (the side-stream weight gradient reads it while the chain reuses Gb)
  h->o_slab_dz = ar.take((size_t)h->dfcd_split * B * L * 4);
  h->o_packjobs = ar.take(sizeof(LoPackJob) * 64);
  h->packjobs_for_ws = h->packjobs_for_params = nullptr;
  h->o_sync_fail = ar.take(256);
  h->Bp = lo_lowrank_bp(B);
  h->o_fac_dmlT = ar.take((size_t)2 * L * h->Bp * 2);
  h->o_fac_xT = ar.take((size_t)32768 * h->Bp * 2);
  h->o_fac_gfcT = ar.take((size_t)32768 * h->Bp * 2);
  h->o_fac_zT = ar.take((size_t)L * h->Bp * 2);
  h->o_gram = ar.take((size_t)2 * 128 * 128 * 4);
  h->lin_factored = h->fac_ready = h->lin_factored_dp = false;
  h->fac_scale = 1.f;

  // ---- fp8 operand mode: every forward conv whose geometry the e4m3 igemm covers (Cin % 128 == 0: the 128 / 256 / 512
  // channel ResBlock and stride-2 convs, the 512 / 256 / 128 channel transposed convs) reads an e4m3 copy of its input,
  // written by the kernel that produces the fp16 activation (which the backward still uses)
  h->fp8_fwd = (flags & LO_VAE_FP8_FWD) != 0;
  {
    // few-rows convolutions as split-K GEMMs + a fused slab pass (LO_SPLITK_CONV=0: every convolution on its one-launch kernel)
    const bool sk_on = !(getenv("LO_SPLITK_CONV") && atoi(getenv("LO_SPLITK_CONV")) == 0) && !h->fp8_fwd;
    size_t slab = 0;
    auto plan_sk = [&](ConvLayer& c, bool first) {
      if (first || !sk_on) return;
      c.sk_fwd = lo_conv_splitk_plan(c.gf);
      c.sk_dgrad = lo_conv_splitk_plan(c.gd);
      const size_t bf = (size_t)c.sk_fwd * B * c.gf.GH * c.gf.GW * c.gf.Cout * 4, bd = (size_t)c.sk_dgrad * B * c.gd.GH * c.gd.GW * c.gd.Cout * 4;
      slab = bf > slab ? bf : slab;
      slab = bd > slab ? bd : slab;
    };
    for (int s = 0; s < 4; ++s) { for (int k = 0; k < 3; ++k) plan_sk(h->enc[s][k], s == 0 && k == 0); plan_sk(h->dec[s], false); }
    h->o_skslab = ar.take(slab > 0 ? slab : 256);
  }
  for (int s = 0; s < 4; ++s) h->o_eout8[s] = 0;
  h->o_h08 = 0; h->o_packjobs8 = 0; h->n_packjobs8 = h->pack_blocks8 = 0;
  h->n_packjobs8_enc = h->pack_blocks8_enc = 0;
  if (h->fp8_fwd) {
    auto enable = [&](ConvLayer& c, size_t* producer_copy) {
      if (!lo_conv_f8_applies(c.gf) || lo_convt4_patch_applies(c.gf)) return;   // a patch-resident fp16 kernel owns the layer (and its partial-sum rows)
      c.f8 = true;
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
  h->ws_bytes = ar.off;
  h->side = nullptr;
  for (int l = 0; l < 6; ++l) h->lvl_pending[l] = false;
  h->defer.pending = false;
  h->n_packjobs_s4 = h->pack_blocks_s4 = h->n_packjobs8_s4 = h->pack_blocks8_s4 = 0;
  h->norm_scratch = nullptr;
  h->overlap = getenv("LO_NO_OVERLAP") == nullptr;
  // GroupNorm-backward reduction fused into the producing data-gradient epilogue (+1.4 % on the step; LO_GNB_FUSE=0 runs the
  // separate reduction kernel).  The epilogue accumulates (sum du, sum du*v) and forms sum du*xhat = rstd * (sum du*v - mean *
  // sum du) after its store loop: the first version multiplied by xhat inside the loop, with mean / rstd live across it, and
  // was not bitwise reproducible while a weight-gradient kernel ran beside it (tools/gnb_det.py: 1365 mismatching tensors
  // in 24 runs; 0 with this form) -- the determinism tests of tests/test_fullsize_gpu.py and test_vae_gpu.py guard it
  h->fuse_gnb = !(getenv("LO_GNB_FUSE") && atoi(getenv("LO_GNB_FUSE")) == 0);
  h->gn_local = !(getenv("LO_GN_LOCAL") && atoi(getenv("LO_GN_LOCAL")) == 0);
  h->nevent = 0;
  h->async_handover = false; h->range_pending = false;
  // GroupNorm + Mish in the conv epilogue (LO_GN_FUSE=1; the default is the separate lo_gn_fwd pass after every conv).  Built,
  // bitwise equal to the separate pass (tests/test_gn_fuse_gpu.py) and measured at batch 64 in two interleaved rounds: 20 403 /
  // 20 414 sprites/s against 20 821 / 20 859 -- 2 % SLOWER.  Per layer the fused conv launches take 7-22 us longer than before while
  // the passes they replace took 8-23 us: every workgroup of a sample waits for the slowest tile of that sample (on two-round grids
  // the second round starts staggered, so the skew of a whole round is paid twice), the hand-off is a chain of dependent memory
  // round trips (publish, count, poll, read the lines: ~5 us on an otherwise idle CU), and the Mish of the tile (25 VALU operations
  // per element) runs on 2 waves per SIMD with nothing to overlap it, where the separate pass spreads the same arithmetic over
  // every wave slot of the chip.  Which layers qualify is a property of the kernel lo_conv_run picks for the
  // geometry (lo_conv_gn_fuse_tiles); the fp8 operand mode keeps the separate pass (it also writes the e4m3 copy of the activation).
  h->fuse_gnf = getenv("LO_GN_FUSE") && atoi(getenv("LO_GN_FUSE")) != 0 && !h->fp8_fwd;
  // ... and the backward's apply pass in the data-gradient epilogue of the consuming layer (LO_GNB_APPLY_FUSE=0: separate
  // lo_gn_bwd_apply launches); needs the fused reduction.  Same mechanism, but here it WINS (+0.8 %: 21 002 / 21 021 against
  // 20 821 / 20 859): the epilogue already holds the activation gradient and has read v for the reduction, so the apply pass it
  // removes (a read of dy and v, a write of dv: 12-27 us per layer) costs more than the wait, and dy is never stored at all
  h->fuse_gna = h->fuse_gnb && !(getenv("LO_GNB_APPLY_FUSE") && atoi(getenv("LO_GNB_APPLY_FUSE")) == 0);
  h->sync_for_ws = nullptr;
  // Workgroups that wait for each other inside an ordinary launch (sample rendezvous) make progress only if every workgroup of the
  // grid can be resident: each fused kernel fits at least one workgroup per CU, workgroups of other kernels on the same CUs (the side
  // stream's weight gradients) finish without waiting for anybody, so a grid of at most one workgroup per compute unit OF THIS
  // DEVICE -- 256 in SPX mode, 32 on a CPX partition -- always drains.  The count is the device's own, not a constant.
  h->n_cu = 0;
  {
    int dev = 0, ncu = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess) h->n_cu = ncu;
    else (void)hipGetLastError();
  }
  if (h->n_cu < 256) h->fuse_gnf = false;      // the forward fusion's two-round rule (lo_conv_gn_fuse_tiles) was only ever checked on 256 CUs
  {
    auto plan = [&](ConvLayer& c, bool first) {
      c.gnf = h->fuse_gnf && !first && !c.sk_fwd && lo_conv_gn_fuse_tiles(c.gf, &c.gnf_mts, &c.gnf_nt);
    };
    for (int s = 0; s < 4; ++s) { for (int k = 0; k < 3; ++k) plan(h->enc[s][k], s == 0 && k == 0); plan(h->dec[s], false); }
  }
  if (h->overlap) {
    // The side stream carries work that has slack (weight gradients, the tail of the optimizer step, operand refresh); the
    // caller's stream carries the dependent chain that decides the step time.  Lowest queue priority for the side stream: when both
    // have workgroups ready, the dispatcher serves the chain first and the side work fills what it leaves (default priority was the
    // round-1 behaviour).  Timeline before (tools/timeline.py): the first GroupNorm pass of a step took 302 us instead of
    // 17 beside the side stream's AdamW, data-gradient launches 55-65 us instead of 36-44 beside the weight gradients.
    // (A CU-masked side stream -- hipExtStreamCreateWithCUMask with 64 / 128 / 192 / all 256 bits set -- was tried in round 3 to
    // fence the side work off: 10 300-12 700 sprites/s against 22 300 with ANY mask, the full one included, so the masked queue
    // itself is the cost on this stack; what does help is fewer, longer side workgroups: see lo_wgrad3_nsplit / lo_wgrad2_nsplit.)
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
  *out = h;
  return LO_OK;
}

static int vae_flush_deferred(LoVae* h, hipStream_t after_main);
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
extern "C" int lo_vae_gradnorm_presummed(const LoVae* h) { return h && h->norm_scratch && ((h->overlap && !g_lo_prof_on) || h->lin_factored); }
// Factored Linear-layer gradients (lo_lowrank.hip): with the mode on, a FUSED single-call lo_vae_backward does not write the weight
// gradients of fc_mu | fc_logvar and decoder.fc into flat_grads (those ranges keep whatever they held); it leaves their factors and
// their share of the gradient norm (needs lo_vae_set_gradnorm_scratch), and lo_vae_optimizer_step forms the gradient tiles inside
// its AdamW pass.  Batch <= 128.  Explicit-gradient (autograd) backwards and the phased data-parallel backward are not affected.
extern "C" int lo_vae_set_linear_factored(LoVae* h, int on) {
  LO_REQUIRE(h, "lo_vae_set_linear_factored: null handle");
  LO_REQUIRE(on >= 0 && on <= 2, "lo_vae_set_linear_factored: mode must be 0 (off), 1 (single process) or 2 (data parallel: factors only)");
  if (on) LO_REQUIRE(lo_lowrank_applies(h->B, 2 * h->L, 32768) && lo_lowrank_applies(h->B, 32768, h->L),
                     "lo_vae_set_linear_factored: batch %d is above the rank the factored update is built for (128)", h->B);
  h->lin_factored = on == 1;
  h->lin_factored_dp = on == 2;
  h->fac_ready = false;
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
  const size_t blk = (h->o_gram - h->o_fac_dmlT) / 2;     // elements per rank block
  const f16* base = reinterpret_cast<const f16*>(gathered);
  const float sc = h->fac_scale / (float)world;
  LO_TRY(lo_lowrank_materialize_gathered(G + h->p_off[h->idx_fc_mu_w], base + (h->o_fac_xT - h->o_fac_dmlT) / 2, base, blk, world, 2 * L, 32768, h->B, sc, st));
  return lo_lowrank_materialize_gathered(G + h->p_off[h->idx_dfc_w], base + (h->o_fac_zT - h->o_fac_dmlT) / 2, base + (h->o_fac_gfcT - h->o_fac_dmlT) / 2,
                                         blk, world, 32768, L, h->B, sc, st);
}
extern "C" int lo_vae_linear_factored(const LoVae* h) { return h && h->lin_factored ? 1 : 0; }
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

// byte offset (inside the workspace) of the word a fused-GroupNorm workgroup sets when its rendezvous poll ran out; 0 = never
extern "C" int lo_vae_sync_fail_word(const LoVae* h, size_t* byte_offset, int* fused_layers) {
  LO_REQUIRE(h && byte_offset, "lo_vae_sync_fail_word: null argument");
  *byte_offset = h->o_sync_fail;
  if (fused_layers) {
    int n = 0;
    for (int s = 0; s < 4; ++s) { for (int k = 0; k < 3; ++k) n += h->enc[s][k].gnf ? 1 : 0; n += h->dec[s].gnf ? 1 : 0; }
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
  return lo_sumsq_range(flat_grads, begin, end, scratch, S(stream));
}

extern "C" int lo_vae_fp8_layers(const LoVae* h, int* layers) {
  LO_REQUIRE(h && layers, "lo_vae_fp8_layers: null argument");
  int n = 0;
  for (int s = 0; s < 4; ++s) { for (int k = 0; k < 3; ++k) n += h->enc[s][k].f8 ? 1 : 0; n += h->dec[s].f8 ? 1 : 0; }
  *layers = n;
  return LO_OK;
}

// an armed event never outlives the function that armed it (error returns included)
struct LoStopEventGuard { ~LoStopEventGuard() { g_lo_stop_event = nullptr; } };
static bool lo_event_marker() {   // LO_EVENT_MARKER=1: hipEventRecord behind the launch, as before round 3 (A/B: -0.5 %)
  static const bool on = getenv("LO_EVENT_MARKER") != nullptr;
  return on;
}
#define WSP(T, off) reinterpret_cast<T*>(reinterpret_cast<unsigned char*>(ws) + (off))
#define PRM(i) (P + h->p_off[(i)])
#define GRD(i) (G + h->p_off[(i)])

// (re)build the job tables of the fused pack launches and upload them into the workspace (once per workspace / parameter buffer)
static int vae_ensure_pack_jobs(LoVae* h, const float* P, void* ws, hipStream_t st) {
  if (h->packjobs_for_ws != ws || h->packjobs_for_params != (const void*)P) {
    // (re)build the job table of the fused pack launch and upload it into the workspace
    std::vector<LoPackJob>& jobs = h->packjobs_host;
    jobs.clear();
    int blocks = 0;
    auto add = [&](ConvLayer& c, const LoGeom& g, size_t o_dst) {
      LoPackJob j;
      j.src = PRM(c.p_w); j.dst = WSP(f16, o_dst); j.total = (int)lo_packed_weight_elems(g); j.block0 = blocks; j.g = g;
      blocks += lo_pack_blocks(g);
      jobs.push_back(j);
    };
    for (int s = 0; s < 4; ++s) {
      if (s == 3) { h->n_packjobs_enc = (int)jobs.size(); h->pack_blocks_enc = blocks; }   // "early" share: encoder stages 1..3
      for (int k = 0; k < 3; ++k) {
        if (s == 0 && k == 0) continue;
        add(h->enc[s][k], h->enc[s][k].gf, h->enc[s][k].o_wp_f);
        add(h->enc[s][k], h->enc[s][k].gd, h->enc[s][k].o_wp_d);
      }
    }
    h->n_packjobs_s4 = (int)jobs.size(); h->pack_blocks_s4 = blocks;
    for (int s = 0; s < 4; ++s) {
      add(h->dec[s], h->dec[s].gf, h->dec[s].o_wp_f);
      add(h->dec[s], h->dec[s].gd, h->dec[s].o_wp_d);
    }
    LO_REQUIRE(jobs.size() <= 64, "too many pack jobs");
    LO_HIP(hipMemcpyAsync(WSP(void, h->o_packjobs), jobs.data(), jobs.size() * sizeof(LoPackJob), hipMemcpyHostToDevice, st));
    h->n_packjobs = (int)jobs.size();
    h->pack_blocks = blocks;
    if (h->fp8_fwd) {
      std::vector<LoPackF8Job>& j8 = h->packjobs8_host;
      j8.clear();
      int blocks8 = 0;
      auto add8 = [&](ConvLayer& c) {
        if (!c.f8) return;
        LoPackF8Job j;
        lo_pack_f8_job(&j, c.gf, WSP(f16, c.o_wp_f), WSP(uint8_t, c.o_wp8), WSP(float, c.o_wscale), blocks8);
        blocks8 += c.gf.n_phase * c.Cout;
        j8.push_back(j);
      };
      for (int s = 0; s < 4; ++s) {
        if (s == 3) { h->n_packjobs8_enc = (int)j8.size(); h->pack_blocks8_enc = blocks8; }
        for (int k = 0; k < 3; ++k) add8(h->enc[s][k]);
      }
      h->n_packjobs8_s4 = (int)j8.size(); h->pack_blocks8_s4 = blocks8;
      for (int s = 0; s < 4; ++s) add8(h->dec[s]);
      LO_REQUIRE(j8.size() <= 32, "too many fp8 pack jobs");
      if (!j8.empty())
        LO_HIP(hipMemcpyAsync(WSP(void, h->o_packjobs8), j8.data(), j8.size() * sizeof(LoPackF8Job), hipMemcpyHostToDevice, st));
      h->n_packjobs8 = (int)j8.size();
      h->pack_blocks8 = blocks8;
    }
    h->packjobs_for_ws = ws;
    h->packjobs_for_params = (const void*)P;
  }
  return LO_OK;
}

// side-stream bookkeeping: one event per operand-refresh level (see LoVae::ev_lvl)
static int vae_side_record(LoVae* h, int lvl, hipStream_t on) {
  LO_HIP(hipEventRecord(h->ev_lvl[lvl], on));
  h->lvl_pending[lvl] = true;
  return LO_OK;
}

// The transposed fp16 copies of the two Linear weights (operands of their data gradients), made from the fp16 forward copies that
// the same stream has just refreshed: 4 bytes of traffic per element instead of the 6 of a transposing cast from fp32, and the
// same bits (LO_TRANSPOSE_F32=1: from the fp32 parameters).  2L and 32768 are multiples of 64 (L is 128, 256 or 512).
static int vae_linear_transposes(LoVae* h, const float* P, void* ws, hipStream_t st) {
  constexpr bool from_f32 = false;
  const int L = h->L;
  if (from_f32 || (2 * L) % 64 != 0 || L % 64 != 0) {
    LO_TRY(lo_transpose_cast(PRM(h->idx_fc_mu_w), WSP(f16, h->o_wp_head_t), 2 * L, 32768, st));
    return lo_transpose_cast(PRM(h->idx_dfc_w), WSP(f16, h->o_wp_dfc_t), 32768, L, st);
  }
  LO_TRY(lo_nhwc_to_nchw_f16(WSP(f16, h->o_wp_head), WSP(f16, h->o_wp_head_t), 1, 2 * L, 32768, st));   // [2L][32768] -> [32768][2L]
  return lo_nhwc_to_nchw_f16(WSP(f16, h->o_wp_dfc), WSP(f16, h->o_wp_dfc_t), 1, 32768, L, st);          // [32768][L] -> [L][32768]
}

// Levels 2..5 of a pipelined optimizer step: AdamW of everything from the encoder's last stage on, in the order the forward needs
// the results, each chunk followed by the operand refresh that depends on it.  after_main != null: the side stream first waits
// for what `after_main` has enqueued so far (the forward calls this once its first stage has been issued, so that the 1.5 GB of
// AdamW traffic runs beside the later, MFMA- and L2-bound stages instead of beside the HBM-bound first one).
static int vae_flush_deferred(LoVae* h, hipStream_t after_main) {
  if (!h->defer.pending) return LO_OK;
  h->defer.pending = false;
  float* P = h->defer.P; const float* G = h->defer.G; float* M = h->defer.M; float* V = h->defer.V; void* ws = h->defer.ws;
  const float* norm = h->defer.norm;
  const float lr = h->defer.lr, b1 = h->defer.beta1, b2 = h->defer.beta2, eps = h->defer.eps, wd = h->defer.wd;
  const int step = h->defer.step, L = h->L;
  hipStream_t sd = h->side;
  if (after_main) {
    LO_HIP(hipEventRecord(h->ev_pre, after_main));
    LO_HIP(hipStreamWaitEvent(sd, h->ev_pre, 0));
  }
  const size_t n = h->flat_elems, b4 = h->p_off[h->enc[3][0].p_w], bh = h->p_off[h->idx_fc_mu_w], bd = h->p_off[h->idx_dfc_w];
  const LoPackJob* jobs = WSP(LoPackJob, h->o_packjobs);
  const LoPackF8Job* jobs8 = WSP(LoPackF8Job, h->o_packjobs8);
  auto adam = [&](size_t lo, size_t hi, f16* cast = nullptr) {
    return hi > lo ? lo_adamw(P + lo, G + lo, M + lo, V + lo, hi - lo, norm, lr, b1, b2, eps, wd, step, sd, cast) : LO_OK;
  };
  // the Linear layers' fp16 forward operands come out of the AdamW pass itself (LO_ADAM_CAST=0: separate cast launches)
  constexpr int fuse_cast = 1;
  const size_t nh = (size_t)2 * L * 32768, nd = (size_t)32768 * L;
  // level 2: encoder stage 4 (10 % of the parameters): first consumer ~0.45 ms into the forward
  LO_TRY(adam(b4, bh));
  LO_TRY(lo_pack_all(jobs + h->n_packjobs_enc, h->n_packjobs_s4 - h->n_packjobs_enc, h->pack_blocks_s4 - h->pack_blocks_enc, sd, h->pack_blocks_enc));
  if (h->fp8_fwd)
    LO_TRY(lo_pack_f8_all(jobs8 + h->n_packjobs8_enc, h->n_packjobs8_s4 - h->n_packjobs8_enc, h->pack_blocks8_s4 - h->pack_blocks8_enc, sd, h->pack_blocks8_enc));
  LO_TRY(vae_side_record(h, 2, sd));
  // level 3: fc_mu / fc_logvar (weights + biases are adjacent: [bh, bd)) and their fp16 copy
  // (the transposed fp16 copies [32768][2L] / [L][32768] -- operands of the two Linear data gradients -- leave the same pass)
  // (+0.6 % on the step against the separate transposes: 25 002 / 25 077 / 24 998 vs 24 720 / 25 047 / 24 867)
  const LoLowrankMat lrm[2] = {{P + bh, M + bh, V + bh, WSP(f16, h->o_wp_head), WSP(f16, h->o_wp_head_t), WSP(f16, h->o_fac_xT), WSP(f16, h->o_fac_dmlT), 2 * L, 32768},
                               {P + bd, M + bd, V + bd, WSP(f16, h->o_wp_dfc), WSP(f16, h->o_wp_dfc_t), WSP(f16, h->o_fac_zT), WSP(f16, h->o_fac_gfcT), 32768, L}};
  if (h->lin_factored) {
    // both factored matrices (fc_mu | fc_logvar and decoder.fc: 82 % of the parameters) in one launch: the forward needs neither
    // before the end of the encoder, ~1 ms away, and one launch has one ramp and one tail
    LO_TRY(lo_adamw_lowrank(lrm, 2, h->B, h->fac_scale, norm, lr, b1, b2, eps, wd, step, sd));
    LO_TRY(adam(bh + nh, bd));
  } else if (fuse_cast) {
    LO_TRY(adam(bh, bh + nh, WSP(f16, h->o_wp_head)));
    LO_TRY(adam(bh + nh, bd));
  } else {
    LO_TRY(adam(bh, bd));
    LO_TRY(lo_cast_f32_f16(PRM(h->idx_fc_mu_w), WSP(f16, h->o_wp_head), nh, sd));
  }
  LO_TRY(vae_side_record(h, 3, sd));
  // level 4: decoder.fc, the decoder and final convs
  if (h->lin_factored) {
    LO_TRY(adam(bd + nd, n));          // decoder.fc.weight went with the encoder heads (one launch for both factored matrices)
  } else if (fuse_cast) {
    LO_TRY(adam(bd, bd + nd, WSP(f16, h->o_wp_dfc)));
    LO_TRY(adam(bd + nd, n));
  } else {
    LO_TRY(adam(bd, n));
    LO_TRY(lo_cast_f32_f16(PRM(h->idx_dfc_w), WSP(f16, h->o_wp_dfc), nd, sd));
  }
  LO_TRY(lo_pack_all(jobs + h->n_packjobs_s4, h->n_packjobs - h->n_packjobs_s4, h->pack_blocks - h->pack_blocks_s4, sd, h->pack_blocks_s4));
  if (h->fp8_fwd)
    LO_TRY(lo_pack_f8_all(jobs8 + h->n_packjobs8_s4, h->n_packjobs8 - h->n_packjobs8_s4, h->pack_blocks8 - h->pack_blocks8_s4, sd, h->pack_blocks8_s4));
  LO_TRY(vae_side_record(h, 4, sd));
  // level 5: the transposed copies (data gradients of the Linear layers: backward only); the factored AdamW pass has written them
  if (!h->lin_factored) LO_TRY(vae_linear_transposes(h, P, ws, sd));
  LO_TRY(vae_side_record(h, 5, sd));
  return LO_OK;
}

// `st` waits for operand-refresh level `lvl` (and with it every lower one); a deferred optimizer tail is enqueued first
static int vae_wait_level(LoVae* h, hipStream_t st, int lvl) {
  if (lvl >= 2) LO_TRY(vae_flush_deferred(h, nullptr));
  for (int l = lvl; l >= 1; --l)
    if (h->lvl_pending[l]) {
      LO_HIP(hipStreamWaitEvent(st, h->ev_lvl[l], 0));      // the highest pending level <= lvl: same stream, recorded in order
      for (int k = 1; k <= l; ++k) h->lvl_pending[k] = false;
      break;
    }
  return LO_OK;
}

extern "C" int lo_vae_pack(LoVae* h, const float* P, void* ws, void* stream) {
  LO_REQUIRE(h && P && ws, "lo_vae_pack: null argument");
  hipStream_t st = S(stream);
  LO_TRY(vae_flush_deferred(h, nullptr));     // an optimizer tail still to be enqueued writes the parameters this pack reads
  LO_TRY(vae_ensure_pack_jobs(h, P, ws, st));
  // the four Linear-layer copies (0.15 ms at L=512) are not needed before the end of the encoder: refresh them on the side
  // stream while the conv pack and the encoder forward run; the consumers wait on the level events (vae_wait_level)
  hipStream_t cs = st;
  if (h->overlap && !g_lo_prof_on) {
    if (h->lvl_pending[5]) LO_HIP(hipStreamWaitEvent(st, h->ev_lvl[5], 0));   // order after an optimizer tail already running
    LO_HIP(hipEventRecord(h->ev_pre, st));
    LO_HIP(hipStreamWaitEvent(h->side, h->ev_pre, 0));
    cs = h->side;
  }
  // the conv pack too (LO_SIDE_PACK, default on): the first conv of the encoder reads the fp32 weights directly, so the pack
  // hides behind it and its GroupNorm; every other consumer waits on its level
  hipStream_t ps = cs;
  LO_TRY(lo_pack_all(WSP(LoPackJob, h->o_packjobs), h->n_packjobs, h->pack_blocks, ps));
  if (h->fp8_fwd) LO_TRY(lo_pack_f8_all(WSP(LoPackF8Job, h->o_packjobs8), h->n_packjobs8, h->pack_blocks8, ps));
  if (ps != st) { LO_TRY(vae_side_record(h, 1, ps)); LO_TRY(vae_side_record(h, 2, ps)); }
  const int L = h->L;
  // encoder head: [fc_mu.weight ; fc_logvar.weight] is one contiguous [2L][32768] fp32 matrix in the flat buffer
  LO_REQUIRE(h->p_off[h->idx_fc_lv_w] == h->p_off[h->idx_fc_mu_w] + (size_t)L * 32768, "flat layout: head weights not adjacent");
  LO_TRY(lo_cast_f32_f16(PRM(h->idx_fc_mu_w), WSP(f16, h->o_wp_head), (size_t)2 * L * 32768, cs));
  LO_TRY(lo_cast_f32_f16(PRM(h->idx_dfc_w), WSP(f16, h->o_wp_dfc), (size_t)32768 * L, cs));
  if (cs != st) { LO_TRY(vae_side_record(h, 3, cs)); LO_TRY(vae_side_record(h, 4, cs)); }
  LO_TRY(vae_linear_transposes(h, P, ws, cs));
  if (cs != st) LO_TRY(vae_side_record(h, 5, cs));
  return LO_OK;
}

// ---------------------------------------------------------------------------------------------
// Pipelined optimizer step: clip + AdamW + operand refresh, ordered so that the NEXT forward starts after 3 % of the update and
// the rest runs beside it where it hurts least.
//   stream:  gradient norm -> AdamW [0, b4)          (b4 = offset of the encoder's last stage: stages 1..3 hold 3 % of the bytes)
//   side  :  pack encoder stages 1..3 (level 1) -> AdamW stage 4 + its packs (level 2) -> AdamW fc_mu|fc_logvar + fp16 copy (3)
//            -> AdamW decoder.fc / decoder + copy + packs (4) -> transposed copies (5).  The forward waits for level 2 before
//            encoder stage 4, 3 before the heads, 4 before the decoder; the backward for level 5.
// Until level 4 has completed, parameters [b4, n) and their Adam moments are in flight on the side stream: lo_vae_join orders
// another stream (e.g. before the caller reads the parameters itself).  Without the side stream everything runs in order on
// `stream`.  presummed != 0: scratch[512..1024) already holds the sum of squares of [b, n) (lo_vae_set_gradnorm_scratch).
// ---------------------------------------------------------------------------------------------
extern "C" int lo_vae_optimizer_step(LoVae* h, float* P, const float* G, float* M, float* V, void* ws, float max_norm, float lr,
                                     float beta1, float beta2, float eps, float weight_decay, int step, float* scratch, int flags,
                                     void* stream) {
  LO_REQUIRE(h && P && G && M && V && ws && scratch, "lo_vae_optimizer_step: null argument");
  LO_REQUIRE((flags & ~(LO_OPT_PRESUMMED | LO_OPT_SERIAL)) == 0, "lo_vae_optimizer_step: unknown flag bits 0x%x", flags);
  const int presummed = flags & LO_OPT_PRESUMMED;
  const bool serial = (flags & LO_OPT_SERIAL) != 0;
  // a fused-GroupNorm rendezvous of this step's launches that ran out left garbage in the gradients: the clip kernel reads the word
  // and skips the update on the device, like a non-finite norm (ADVICE r3 / VERDICT r3 item 1b)
  const unsigned int* fail = WSP(unsigned int, h->o_sync_fail);
  hipStream_t st = S(stream);
  if (h->lin_factored) {
    if (!h->fac_ready || !presummed) {
      lo_set_error("lo_vae_optimizer_step: the factored Linear-gradient mode needs a fused lo_vae_backward (with the gradient-norm scratch set) "
                   "before every step, and LO_OPT_PRESUMMED");
      return LO_ERR_STATE;
    }
    h->fac_ready = false;
  }
  LO_TRY(vae_flush_deferred(h, nullptr));     // two optimizer steps without a forward in between
  // b: begin of the range whose sum of squares may be presummed (fc_mu.weight);  b4: begin of the encoder's last stage -- the
  // stream itself only updates stages 1..3 (3 % of the parameters, what the next forward reads in its first 0.45 ms)
  const size_t n = h->flat_elems, b = h->p_off[h->idx_fc_mu_w], b4 = h->p_off[h->enc[3][0].p_w];
  LO_TRY(vae_ensure_pack_jobs(h, P, ws, st));
  if (presummed) LO_TRY(lo_gradnorm_split(G, b, max_norm, scratch, scratch + 1024, st, fail));
  else LO_TRY(lo_gradnorm(G, n, max_norm, scratch, scratch + 1024, st, fail));
  const float* norm = scratch + 1024;
  if (serial || !(h->overlap && !g_lo_prof_on)) {
    if (h->lin_factored) {
      const int L = h->L;
      const size_t bh = h->p_off[h->idx_fc_mu_w], nh = (size_t)2 * L * 32768, bd = h->p_off[h->idx_dfc_w], nd = (size_t)32768 * L;
      const LoLowrankMat lrm[2] = {{P + bh, M + bh, V + bh, nullptr, nullptr, WSP(f16, h->o_fac_xT), WSP(f16, h->o_fac_dmlT), 2 * L, 32768},
                                   {P + bd, M + bd, V + bd, nullptr, nullptr, WSP(f16, h->o_fac_zT), WSP(f16, h->o_fac_gfcT), 32768, L}};
      LO_TRY(lo_adamw(P, G, M, V, bh, norm, lr, beta1, beta2, eps, weight_decay, step, st));
      LO_TRY(lo_adamw_lowrank(lrm, 2, h->B, h->fac_scale, norm, lr, beta1, beta2, eps, weight_decay, step, st));
      LO_TRY(lo_adamw(P + bh + nh, G + bh + nh, M + bh + nh, V + bh + nh, bd - (bh + nh), norm, lr, beta1, beta2, eps, weight_decay, step, st));
      LO_TRY(lo_adamw(P + bd + nd, G + bd + nd, M + bd + nd, V + bd + nd, n - (bd + nd), norm, lr, beta1, beta2, eps, weight_decay, step, st));
    } else {
      LO_TRY(lo_adamw(P, G, M, V, n, norm, lr, beta1, beta2, eps, weight_decay, step, st));
    }
    return lo_vae_pack(h, P, ws, stream);
  }
  LoStopEventGuard stop_guard_;
  if (!lo_event_marker()) g_lo_stop_event = h->ev_pre;    // the hand-over event rides on the AdamW launch (LO_LAUNCH_STOP)
  {
    int r_ = lo_adamw(P, G, M, V, b4, norm, lr, beta1, beta2, eps, weight_decay, step, st);
    if (r_ != LO_OK) { g_lo_stop_event = nullptr; return r_; }
  }
  if (g_lo_stop_event || lo_event_marker()) { g_lo_stop_event = nullptr; LO_HIP(hipEventRecord(h->ev_pre, st)); }
  LO_HIP(hipStreamWaitEvent(h->side, h->ev_pre, 0));
  hipStream_t sd = h->side;
  LO_TRY(lo_pack_all(WSP(LoPackJob, h->o_packjobs), h->n_packjobs_enc, h->pack_blocks_enc, sd));
  if (h->fp8_fwd) LO_TRY(lo_pack_f8_all(WSP(LoPackF8Job, h->o_packjobs8), h->n_packjobs8_enc, h->pack_blocks8_enc, sd));
  LO_TRY(vae_side_record(h, 1, sd));
  h->defer.pending = true;
  h->defer.P = P; h->defer.G = G; h->defer.M = M; h->defer.V = V; h->defer.ws = ws; h->defer.norm = norm;
  h->defer.lr = lr; h->defer.beta1 = beta1; h->defer.beta2 = beta2; h->defer.eps = eps; h->defer.wd = weight_decay; h->defer.step = step;
  // (deferring this tail behind the next forward's first stage was measured in round 2: no difference -- where the AdamW traffic
  // lands only changes WHICH kernels it slows down, not the sum -- so it is enqueued at once)
  LO_TRY(vae_flush_deferred(h, nullptr));
  return LO_OK;
}
// `stream` waits for whatever lo_vae_pack / lo_vae_optimizer_step left running (or still to be enqueued) on the side stream.
extern "C" int lo_vae_join(LoVae* h, void* stream) {
  LO_REQUIRE(h, "lo_vae_join: null handle");
  hipStream_t st = S(stream);
  LO_TRY(vae_flush_deferred(h, nullptr));
  for (int l = 5; l >= 1; --l)
    if (h->lvl_pending[l]) { LO_HIP(hipStreamWaitEvent(st, h->ev_lvl[l], 0)); break; }
  // the flags stay set: the executor's own stream may be a different one and still has to wait
  return LO_OK;
}

// The arrival counters of the fused GroupNorm epilogues live in the caller's workspace: zero them (and the failure word) the first
// time a workspace is seen; from then on they only ever count up (ConvLayer::gnf_epoch follows them on the host).
static int vae_ensure_sync_init(LoVae* h, void* ws, hipStream_t st) {
  if (h->sync_for_ws == ws) return LO_OK;
  auto zero = [&](ConvLayer& c) -> int {
    LO_HIP(hipMemsetAsync(WSP(void, c.o_xcnt), 0, (size_t)h->B * 4, st));
    LO_HIP(hipMemsetAsync(WSP(void, c.o_bcnt), 0, (size_t)h->B * 8 * 4, st));
    c.gnf_epoch = 0; c.gba_epoch = 0;
    return LO_OK;
  };
  for (int s = 0; s < 4; ++s) { for (int k = 0; k < 3; ++k) LO_TRY(zero(h->enc[s][k])); LO_TRY(zero(h->dec[s])); }
  LO_HIP(hipMemsetAsync(WSP(void, h->o_sync_fail), 0, 256, st));
  h->sync_for_ws = ws;
  return LO_OK;
}

// in8: e4m3 copy of `in` (fp8 mode, layers with c.f8); y8: where to leave the e4m3 copy of y (0 = nobody reads it)
static int conv_gn(LoVae* h, ConvLayer& c, const f16* in, const f16* other, f16* y, int mode, const float* P, void* ws,
                   hipStream_t st, size_t o_in8 = 0, size_t o_y8 = 0) {
  static char ftag[64][64];
  static int fcount = 0;
  if (g_lo_prof_on && g_lo_prof_layers) {
    char* tg = ftag[fcount++ & 63];
    snprintf(tg, 64, "fwd kind%d %dx%d %d->%d", c.kind, c.Ho, c.Wo, c.gf.Cin, c.gf.Cout);
    g_lo_prof_tag = tg;
  }
  int r_;
  // GroupNorm + Mish inside the conv's own epilogue (the workgroups of a sample exchange their sums: LoGnFuse) where the kernel that
  // owns this geometry supports it; the separate lo_gn_fwd pass below is then not run.  Same statistics, same arithmetic, same bits.
  if (c.sk_fwd && !c.f8 && !o_y8) {
    // few output rows: K-split GEMM into fp32 slabs, then ONE (sample, group)-local pass: slab sum + bias -> v, statistics, GroupNorm + Mish
    int r2 = lo_conv_run(c.gf, in, WSP(f16, c.o_wp_f), nullptr, nullptr, nullptr, nullptr, WSP(float, h->o_skslab), c.sk_fwd, st);
    g_lo_prof_tag = nullptr;
    if (r2 != LO_OK) return r2;
    return lo_splitk_gn_fwd(WSP(float, h->o_skslab), c.sk_fwd, PRM(c.p_b), PRM(c.p_gw), PRM(c.p_gb), other, WSP(f16, c.o_v), y,
                            WSP(float, c.o_stats), h->B, c.Ho * c.Wo, c.Cout, mode, st);
  }
  const bool fuse = c.gnf && !c.f8 && !o_y8;
  LoGnFuse gf;
  if (fuse) {
    memset(&gf, 0, sizeof(gf));
    gf.xbuf = WSP(float, c.o_xbuf); gf.counter = WSP(unsigned int, c.o_xcnt);
    gf.MTs = c.gnf_mts; gf.NT = c.gnf_nt;
    gf.target = (++c.gnf_epoch) * (unsigned)(c.gnf_mts * c.gnf_nt);
    gf.gamma = PRM(c.p_gw); gf.beta = PRM(c.p_gb); gf.other = other; gf.y = y; gf.stats = WSP(float, c.o_stats); gf.mode = mode;
    gf.fail = WSP(unsigned int, h->o_sync_fail);
  }
  if (c.f8) {
    LO_REQUIRE(o_in8, "fp8 mode: no e4m3 copy of the input of a conv %d->%d", c.Cin, c.Cout);
    r_ = lo_conv_run_f8(c.gf, WSP(uint8_t, o_in8), WSP(uint8_t, c.o_wp8), WSP(float, c.o_wscale), PRM(c.p_b), nullptr, WSP(f16, c.o_v),
                        WSP(float, c.o_part), st);
  } else {
    r_ = lo_conv_run(c.gf, in, WSP(f16, c.o_wp_f), PRM(c.p_b), nullptr, WSP(f16, c.o_v), fuse ? nullptr : WSP(float, c.o_part), nullptr, 1, st,
                     nullptr, nullptr, fuse ? &gf : nullptr);
  }
  g_lo_prof_tag = nullptr;
  if (r_ != LO_OK) { if (fuse) --c.gnf_epoch; return r_; }
  if (fuse) return LO_OK;
  return lo_gn_fwd(WSP(f16, c.o_v), WSP(float, c.o_part), c.MT, PRM(c.p_gw), PRM(c.p_gb), other, y, WSP(float, c.o_stats), h->B,
                   c.Ho * c.Wo, c.Cout, mode, st, o_y8 ? WSP(uint8_t, o_y8) : nullptr);
}

// decoder (lunar_generate.py:194-229) from the latent z (fp16, in the workspace); use_skips=false is the `skips=[]`
// call of LunarisCoreVAE.sample (:278-291)
// skips[k] (fp16 NHWC, k = 0: 64 x 64 x 64, 1: 32 x 32 x 128, 2: 16 x 16 x 256) is added after up(3-k); NULL = not added
static int vae_decoder_forward(LoVae* h, const f16* const skips[3], const float* P, void* ws, float* recon, const float* target,
                               hipStream_t st) {
  const int B = h->B;
  LO_TRY(vae_ensure_sync_init(h, ws, st));
  LO_TRY(vae_wait_level(h, st, 4));
  LO_TRY(lo_conv_run(h->g_dfc, WSP(f16, h->o_z), WSP(f16, h->o_wp_dfc), PRM(h->idx_dfc_b), nullptr, WSP(f16, h->o_yfc), nullptr,
                     nullptr, 1, st));
  LO_TRY(lo_nchw_to_nhwc_f16(WSP(f16, h->o_yfc), WSP(f16, h->o_h0), B, 64, 512, st, h->o_h08 ? WSP(uint8_t, h->o_h08) : nullptr));
  const f16* cur = WSP(f16, h->o_h0);
  size_t cur8 = h->o_h08;
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
      LO_TRY(lo_gn_fwd(WSP(f16, c0.o_v), WSP(float, c0.o_part), c0.MT, PRM(c0.p_gw), PRM(c0.p_gb), nullptr, WSP(f16, c0.o_a),
                       WSP(float, c0.o_stats), B, c0.Ho * c0.Wo, c0.Cout, 0, st, c0.o_a8 ? WSP(uint8_t, c0.o_a8) : nullptr));
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
  // ---- heads + reparameterisation (lunar_generate.py:150-152, 259-261)
  LO_TRY(lo_nhwc_to_nchw_f16(cur, WSP(f16, h->o_xflat), B, 64, 512, st));
  LO_TRY(vae_wait_level(h, st, 3));
  LO_TRY(lo_conv_run(h->g_head, WSP(f16, h->o_xflat), WSP(f16, h->o_wp_head), nullptr, nullptr, nullptr, nullptr,
                     WSP(float, h->o_slab_head), h->head_split, st));
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

// Hand-over of a layer's dv to the side stream.  The event rides on the launch that writes dv (LO_LAUNCH_STOP, lo_common.h): a
// hipEventRecord behind that launch costs the caller's stream 3.5-4.7 us per hand-over (a marker packet the next kernel waits
// for), the kernel's own completion signal 0.9-1.3 us (tools/probe/ev_probe.hip).
//   vae_arm_handover:   call right before the launcher whose LAST launch writes dv; returns the event (null without a side stream)
//   vae_armed_handover: call right after it; records the event the classic way if no launch picked it up
static hipEvent_t vae_arm_handover(LoVae* h, bool ov) {
  if (!ov) return nullptr;
  hipEvent_t e = h->ev_dv[(h->nevent++) & 3];
  if (!lo_event_marker()) g_lo_stop_event = e;
  return e;
}
static int vae_armed_handover(hipEvent_t e, hipStream_t st) {
  if (e && (g_lo_stop_event || lo_event_marker())) {   // nobody consumed it (a launcher path without LO_LAUNCH_STOP): fall back to a marker
    g_lo_stop_event = nullptr;
    LO_HIP(hipEventRecord(e, st));
  }
  return LO_OK;
}

// backward of one conv+GN+Mish layer.  dy: gradient wrt the layer's activation output (after mish, before any skip add).
// Produces the parameter gradients and, when din != null, the gradient wrt the layer input (+ add_src).
// prod: the conv+GN+Mish layer (mode plain / skip) whose activation gradient this layer's data gradient produces;
// its GroupNorm-backward reduction is then fused into the data-gradient epilogue (prod->np1 records the row count).
static int conv_gn_bwd(LoVae* h, ConvLayer& c, const f16* dy, const f16* other, int mode, const f16* layer_in, f16* ds,
                       f16* din, const f16* add_src, const float* P, float* G, void* ws, float inv_scale, hipStream_t st,
                       ConvLayer* prod = nullptr, bool din_has_other_readers = false) {
  // every layer has its own dv buffer: the side-stream weight gradient of layer k may still be reading it while the main
  // stream produces the dv of the following layers (no event back from the side stream: two host calls per layer less)
  LoStopEventGuard stop_guard_;
  const int k = h->bwd_layer++;
  f16* dv = WSP(f16, c.o_dv);
  const bool ov = h->overlap && !g_lo_prof_on;   // per-launch profiling keeps everything on one stream
  // c.dv_done: the data gradient of the consuming layer has already turned this layer's activation gradient into dv (and P2) in
  // its epilogue -- `dy` was never stored
  hipEvent_t ready = nullptr;         // completes when dv is final
  if (c.dv_done) { ready = c.ev_ready; c.ev_ready = nullptr; }
  if (!c.dv_done) {
    ready = vae_arm_handover(h, ov);
    if (c.np1 == 0 && h->gn_local && lo_gn_bwd_local_applies(c.Ho * c.Wo, c.Cout)) {
      // nobody has reduced this layer yet and a (sample, group) fits a workgroup: reduce + apply in ONE pass (the ResBlock tails of
      // the 16 x 16 and 8 x 8 stages), one P1 / P2 row per sample
      LO_TRY(lo_gn_bwd_local(dy, WSP(f16, c.o_v), other, WSP(float, c.o_stats), PRM(c.p_gw), PRM(c.p_gb), ds, dv, WSP(float, c.o_P1),
                             WSP(float, c.o_P2), h->B, c.Ho * c.Wo, c.Cout, mode, st));
      c.np1 = 1; c.np2 = 1;
    } else {
      LO_TRY(lo_gn_bwd_nofinal(dy, WSP(f16, c.o_v), other, WSP(float, c.o_stats), PRM(c.p_gw), PRM(c.p_gb), ds, dv,
                               WSP(float, c.o_P1), WSP(float, c.o_P2), h->B, c.Ho * c.Wo, c.Cout, mode, st, c.np1));
    }
    LO_TRY(vae_armed_handover(ready, st));
  }
  if (ov) {
    if (!ready) {                      // dv came from a launch that carried no event: classic record
      ready = h->ev_dv[(h->nevent++) & 3];
      LO_HIP(hipEventRecord(ready, st));
    }
    LO_HIP(hipStreamWaitEvent(h->side, ready, 0));
    LO_TRY(lo_wgrad_run(c.gf, layer_in, dv, WSP(float, h->o_wslab), GRD(c.p_w), inv_scale, h->side));
  } else {
    static char wtag[32][64];
    if (g_lo_prof_on && g_lo_prof_layers) {
      snprintf(wtag[k & 31], 64, "wgrad L%02d kind%d %dx%d %d->%d", k, c.kind, c.Ho, c.Wo, c.gf.Cin, c.gf.Cout);
      g_lo_prof_tag = wtag[k & 31];
    }
    int r_ = lo_wgrad_run(c.gf, layer_in, dv, WSP(float, h->o_wslab), GRD(c.p_w), inv_scale, st);
    g_lo_prof_tag = nullptr;
    if (r_ != LO_OK) return r_;
  }
  if (din && prod && c.sk_dgrad && lo_gn_bwd_local_applies(prod->Ho * prod->Wo, prod->Cout)) {
    // few output rows: the data gradient as a K-split GEMM into fp32 slabs, then ONE (sample, group)-local pass that sums them
    // (+ the residual gradient) and runs the whole GroupNorm backward of the producing layer: dv, one P1 / P2 row per sample
    static char stag[32][64];
    if (g_lo_prof_on && g_lo_prof_layers) {
      snprintf(stag[k & 31], 64, "dgrad L%02d kind%d %dx%d %d->%d", k, c.kind, c.Ho, c.Wo, c.gd.Cin, c.gd.Cout);
      g_lo_prof_tag = stag[k & 31];
    }
    int r_ = lo_conv_run(c.gd, dv, WSP(f16, c.o_wp_d), nullptr, nullptr, nullptr, nullptr, WSP(float, h->o_skslab), c.sk_dgrad, st);
    g_lo_prof_tag = nullptr;
    if (r_ != LO_OK) return r_;
    hipEvent_t pe = vae_arm_handover(h, ov);       // the pass below writes prod's dv: its launch carries prod's hand-over event
    int r2_ = lo_splitk_gn_bwd(WSP(float, h->o_skslab), c.sk_dgrad, add_src, WSP(f16, prod->o_v), WSP(float, prod->o_stats), PRM(prod->p_gw),
                               PRM(prod->p_gb), din_has_other_readers ? din : nullptr, WSP(f16, prod->o_dv), WSP(float, prod->o_P1),
                               WSP(float, prod->o_P2), h->B, prod->Ho * prod->Wo, prod->Cout, st);
    if (r2_ != LO_OK) { g_lo_stop_event = nullptr; return r2_; }
    LO_TRY(vae_armed_handover(pe, st));
    prod->ev_ready = pe;
    prod->dv_done = true; prod->np1 = 1; prod->np2 = 1;
    return LO_OK;
  }
  if (din) {
    LoGnBwdFuse gb, *gbp = nullptr;
    if (prod && h->fuse_gnb) {
      gb.v = WSP(f16, prod->o_v); gb.stats = WSP(float, prod->o_stats); gb.gamma = PRM(prod->p_gw); gb.beta = PRM(prod->p_gb);
      gb.P1 = WSP(float, prod->o_P1);
      prod->np1 = lo_conv_gnb_rows(c.gd);
      int mts = 0, nt = 0;
      // ... only where the whole grid is resident at once (one workgroup per CU): on the 64-channel 64 x 64 layers (1 024 tiles at
      // batch 64, two rounds of 512) the fused launch is 32-34 us longer than the 27 us pass it replaces, and the step is 0.6 %
      // faster without it there (22 309-22 332 against 22 185-22 202; nowhere: 22 238-22 316)
      if (h->fuse_gna && lo_conv_gnb_apply_tiles(c.gd, &mts, &nt) && mts == prod->np1 && h->B * mts * nt <= h->n_cu) {
        gb.dv = WSP(f16, prod->o_dv); gb.P2 = WSP(float, prod->o_P2);
        gb.counter = WSP(unsigned int, prod->o_bcnt);
        gb.target = (++prod->gba_epoch) * (unsigned)mts;
        gb.fail = WSP(unsigned int, h->o_sync_fail);
        gb.keep_out = din_has_other_readers;      // the decoder's data gradients are also the encoder's skip gradients
        prod->dv_done = true;
        prod->np2 = mts;
      }
      gbp = &gb;
    }
    static char dtag[32][64];
    if (g_lo_prof_on && g_lo_prof_layers) {
      snprintf(dtag[k & 31], 64, "dgrad L%02d kind%d %dx%d %d->%d", k, c.kind, c.Ho, c.Wo, c.gd.Cin, c.gd.Cout);
      g_lo_prof_tag = dtag[k & 31];
    }
    hipEvent_t pe = (gbp && gbp->dv) ? vae_arm_handover(h, ov) : nullptr;   // this launch writes prod's dv: it carries prod's event
    int r_ = lo_conv_run(c.gd, dv, WSP(f16, c.o_wp_d), nullptr, add_src, din, nullptr, nullptr, 1, st, gbp);
    g_lo_prof_tag = nullptr;
    if (r_ != LO_OK) { g_lo_stop_event = nullptr; if (gbp && gbp->dv) { --prod->gba_epoch; prod->dv_done = false; } return r_; }
    if (gbp && gbp->dv) { LO_TRY(vae_armed_handover(pe, st)); prod->ev_ready = pe; }
  }
  return LO_OK;
}

// phase 5 / 6 = Decoder / Encoder backward on their own (the module boundary: lo_vae_decoder_backward / lo_vae_encoder_backward);
// the feature-map gradients cross as fp32 NCHW tensors.  dx (any phase that runs encoder stage 1; NULL = not wanted): the gradient wrt
// the images, fp32 NCHW [B,3,128,128]
struct LoSplitBwd { float* dz; float* dskip[3]; const float* gskip[3]; float* dx; };
static int vae_backward_impl(LoVae* h, int phase, const float* x, const float* P, void* ws, const float* recon, const float* target,
                             int fused, const float* drecon, const float* gmu, const float* glv, float loss_scale,
                             float* G, void* stream, const LoSplitBwd* sp = nullptr);

extern "C" int lo_vae_backward_dx(LoVae* h, const float* x, const float* P, void* ws, const float* recon, const float* target,
                                  int fused, const float* drecon, const float* gmu, const float* glv, float loss_scale,
                                  float* G, float* dx, void* stream) {
  if (!dx) return vae_backward_impl(h, 0, x, P, ws, recon, target, fused, drecon, gmu, glv, loss_scale, G, stream);
  LoSplitBwd sp{nullptr, {nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}, dx};
  return vae_backward_impl(h, 0, x, P, ws, recon, target, fused, drecon, gmu, glv, loss_scale, G, stream, &sp);
}
extern "C" int lo_vae_backward(LoVae* h, const float* x, const float* P, void* ws, const float* recon, const float* target,
                               int fused, const float* drecon, const float* gmu, const float* glv, float loss_scale,
                               float* G, void* stream) {
  return lo_vae_backward_dx(h, x, P, ws, recon, target, fused, drecon, gmu, glv, loss_scale, G, nullptr, stream);
}
extern "C" int lo_vae_backward_phase(LoVae* h, int phase, const float* x, const float* P, void* ws, const float* recon,
                                     const float* target, int fused, const float* drecon, const float* gmu, const float* glv,
                                     float loss_scale, float* G, void* stream) {
  LO_REQUIRE(phase >= 1 && phase <= 4, "lo_vae_backward_phase: phase must be 1 (final conv, decoder, Linear layers), 2 (whole encoder), "
             "3 (encoder stage 4) or 4 (encoder stages 3..1, after 3)");
  return vae_backward_impl(h, phase, x, P, ws, recon, target, fused, drecon, gmu, glv, loss_scale, G, stream);
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

// GroupNorm affine + conv bias gradients of a set of layers in one launch (enc_mask: bit s = encoder stage s)
static int vae_gn_finalize(LoVae* h, unsigned enc_mask, bool dec, float* G, void* ws, float inv, hipStream_t st) {
  const int B = h->B;
  LoGnFinJobs jobs;
  jobs.n = 0;
  int blocks = 0;
  auto add = [&](ConvLayer& c) {
    LoGnFinJob& j = jobs.j[jobs.n++];
    j.P1 = WSP(float, c.o_P1); j.P2 = WSP(float, c.o_P2);
    j.dgamma = GRD(c.p_gw); j.dbeta = GRD(c.p_gb); j.dbias = GRD(c.p_b);
    j.nblk2 = B * (c.np2 > 0 ? c.np2 : lo_gn_nchunk(c.Ho * c.Wo, c.Cout));
    j.nblk1 = c.np1 > 0 ? B * c.np1 : j.nblk2;
    j.C = c.Cout; j.block0 = blocks;
    blocks += (c.Cout + 3) / 4;
  };
  for (int s = 0; s < 4; ++s)
    if (enc_mask & (1u << s)) for (int k = 0; k < 3; ++k) add(h->enc[s][k]);
  if (dec) for (int s = 0; s < 4; ++s) add(h->dec[s]);
  return lo_gn_finalize_all(jobs, inv, st);
}

// the alignment gaps of the flat gradient buffer (every tensor starts on a 64-element boundary): the only elements no gradient
// kernel writes.  One small launch instead of a 244 MB memset per step.
struct LoGapTable { unsigned long long off[80]; int len[80]; int n; };
__global__ void lo_zero_gaps_kernel(float* G, LoGapTable t) {
  const int i = blockIdx.x;
  if (i < t.n && (int)threadIdx.x < t.len[i]) G[t.off[i] + threadIdx.x] = 0.f;
}
static int vae_zero_gaps(LoVae* h, float* G, hipStream_t st) {
  LoGapTable t;
  t.n = 0;
  LO_REQUIRE(h->nparam <= 80, "gap table too small");
  for (int i = 0; i < h->nparam; ++i) {
    const size_t n = h->p_numel[i], padded = (n + 63) & ~(size_t)63;
    if (padded > n) { t.off[t.n] = h->p_off[i] + n; t.len[t.n] = (int)(padded - n); ++t.n; }
  }
  if (t.n == 0) return LO_OK;
  hipLaunchKernelGGL(lo_zero_gaps_kernel, dim3(t.n), dim3(64), 0, st, G, t);
  LO_LAUNCH_CHECK("zero_gaps");
  return LO_OK;
}

static int vae_backward_impl(LoVae* h, int phase, const float* x, const float* P, void* ws, const float* recon, const float* target,
                             int fused, const float* drecon, const float* gmu, const float* glv, float loss_scale,
                             float* G, void* stream, const LoSplitBwd* sp) {
  LO_REQUIRE(h && P && ws && G && (phase == 5 || x) && (phase == 6 || recon), "lo_vae_backward: null argument");
  if (phase == 5 ? !h->dec_done : (phase == 6 ? !h->enc_done : !h->forward_done)) {
    lo_set_error("lo_vae_backward: the forward this backward belongs to has not run");
    return LO_ERR_STATE;
  }
  if (fused && (!h->loss_done || !target)) { lo_set_error("lo_vae_backward: fused mode needs lo_vae_loss and a target"); return LO_ERR_STATE; }
  LO_REQUIRE(loss_scale > 0.f, "lo_vae_backward: loss_scale must be positive");
  hipStream_t st = S(stream);
  LO_TRY(vae_wait_level(h, st, 5));   // the transposed Linear copies (and, after a lo_vae_pack between forward and backward, everything)
  const int B = h->B, L = h->L;
  const float inv = 1.0f / loss_scale;
  // the Linear layers' weight gradients stay factored (lo_lowrank.hip): the fused single-call backward of a stepper only
  const bool fac1 = h->lin_factored && fused && phase == 0;
  const bool facdp = h->lin_factored_dp && fused && phase == 1;     // data parallel: the factors leave this rank, not the gradients
  const bool fac = fac1 || facdp;
  if (fac1 && !h->norm_scratch) { lo_set_error("lo_vae_backward: the factored Linear-gradient mode needs lo_vae_set_gradnorm_scratch"); return LO_ERR_STATE; }
  if (phase == 0 || phase == 1) h->fac_ready = false;
  LoStopEventGuard stop_guard_;
  hipEvent_t early_ev = nullptr;      // ev_pre when part A's last launch carries it (single-call backward with the early gradient norm)
  f16* Ga = WSP(f16, h->o_G[0]);
  f16* Gb = WSP(f16, h->o_G[1]);
  f16* Gc = WSP(f16, h->o_G[2]);
  f16* Gd = WSP(f16, h->o_G[3]);
  if (phase == 0 || phase == 1 || phase == 5 || phase == 6) {
    h->bwd_layer = 0;
    for (int s = 0; s < 4; ++s) {
      for (int k = 0; k < 3; ++k) { h->enc[s][k].np1 = 0; h->enc[s][k].dv_done = false; h->enc[s][k].np2 = 0; h->enc[s][k].ev_ready = nullptr; }
      h->dec[s].np1 = 0; h->dec[s].dv_done = false; h->dec[s].np2 = 0; h->dec[s].ev_ready = nullptr;
    }
  }
  if (phase == 0 || phase == 1 || phase == 5) {   // ---------------- part A: final conv, decoder, Linear layers (their gradients are complete afterwards)
  // padding elements of the flat gradient buffer are zero afterwards; every other element is overwritten (never accumulated
  // into) by exactly one gradient kernel
  // (gradient-only and independent of everything on the chain: on the side stream when there is one -- in order behind the previous
  // optimizer tail there, in front of every weight gradient of this backward, and joined before anybody reads the buffer)
  // Only for the fused step, whose gradient buffer is the stepper's own: behind the module boundary (fused == 0, phase 5) G is a fresh
  // block of PyTorch's caching allocator, which is ordered with respect to the CALLER's stream only -- a side-stream write could land
  // while earlier work of the caller's stream still uses the recycled block.
  LO_TRY(vae_zero_gaps(h, G, (h->overlap && !g_lo_prof_on && fused && phase != 5) ? h->side : st));
  // ---- final conv (+tanh, + fused MSE gradient)
  {
    ConvLayer& u4 = h->dec[3];
    if (fused || drecon) {
      const bool ov0 = h->overlap && !g_lo_prof_on && !lo_event_marker();
      hipEvent_t e = vae_arm_handover(h, ov0);          // rides on the kernel; the dw / db column sums follow it on the side stream
      int r_ = lo_final_conv_bwd(WSP(f16, u4.o_a), PRM(h->idx_final_w), recon, fused ? target : nullptr, fused ? nullptr : drecon,
                                 fused ? WSP(float, h->o_coefs) : nullptr, loss_scale, Ga, WSP(float, h->o_lc_part),
                                 GRD(h->idx_final_w), GRD(h->idx_final_b), B, inv, st, ov0 ? h->side : nullptr, e);
      g_lo_stop_event = nullptr;
      if (r_ != LO_OK) return r_;
    } else {
      LO_HIP(hipMemsetAsync(Ga, 0, (size_t)B * 128 * 128 * 32 * 2, st));
    }
  }
  // ---- decoder: up4..up1.  Ga holds the gradient wrt the stage's (activation [+ skip]) output.
  const f16* gout = Ga;
  for (int s = 3; s >= 0; --s) {
    ConvLayer& c = h->dec[s];
    const f16* layer_in = s > 0 ? WSP(f16, h->dec[s - 1].o_a) : WSP(f16, h->o_h0);
    f16* din = s > 0 ? WSP(f16, h->o_skipg[3 - s]) : Ga;   // up4->skipg[0] (wrt up3 out), up3->skipg[1], up2->skipg[2], up1->Ga
    // mode 1 (skip add) has the same du as mode 0; the skip branch receives gout unchanged (kept in skipg)
    LO_TRY(conv_gn_bwd(h, c, gout, nullptr, 0, layer_in, nullptr, din, nullptr, P, G, ws, inv, st, s > 0 ? &h->dec[s - 1] : nullptr, true));
    gout = din;
  }
  // gout == Ga: gradient wrt h0 [B,8,8,512] NHWC
  // ---- decoder.fc
  // The bias and weight gradients of the two Linear layers feed nothing on the dependent chain (72 us of it in round 2): with a
  // side stream they run there, behind an event that rides on the launch producing their operand (LO_LAUNCH_STOP).  o_wslab_lin
  // stays theirs alone (two launches, in order on one stream); Gfc is a buffer of its own because the chain reuses Gb.
  const bool ovl = h->overlap && !g_lo_prof_on;
  hipStream_t gs = ovl ? h->side : st;
  f16* Gfc = WSP(f16, h->o_gfc);
  {
    hipEvent_t e = vae_arm_handover(h, ovl);
    int r_ = lo_nhwc_to_nchw_f16(Ga, Gfc, B, 64, 512, st);                   // Gfc = dy of decoder.fc, [B][32768] c-major
    if (r_ != LO_OK) { g_lo_stop_event = nullptr; return r_; }
    LO_TRY(vae_armed_handover(e, st));
    if (ovl) LO_HIP(hipStreamWaitEvent(h->side, e, 0));
  }
  LO_TRY(lo_colsum_f16(Gfc, GRD(h->idx_dfc_b), B, 32768, inv, gs));
  if (!fac) {      // factored mode: dW = Gfc^T z is never formed (its factors are transposed below, with the encoder heads')
    LO_TRY(lo_wgrad_run(h->g_dfc, WSP(f16, h->o_z), Gfc, WSP(float, h->o_wslab_lin), GRD(h->idx_dfc_w), inv, gs));
  }
  LO_TRY(lo_conv_run(h->g_dfc_d, Gfc, WSP(f16, h->o_wp_dfc_t), nullptr, nullptr, nullptr, nullptr, WSP(float, h->o_slab_dz),
                     h->dfcd_split, st));
  LO_TRY(lo_splitk_reduce(WSP(float, h->o_slab_dz), nullptr, phase == 5 ? sp->dz : nullptr, WSP(f16, h->o_dz), B, L, h->dfcd_split, st));
  if (phase == 5) {
    // Decoder.forward's backward ends here: dz and the skip-map gradients leave un-scaled as fp32 (the gradient of skips[k] is
    // the gradient of the sum it was added into, which the data gradient of the next transposed conv has left in skipg[k])
    LO_TRY(lo_scale_f32(sp->dz, (size_t)B * L, inv, st));
    for (int k = 0; k < 3; ++k)
      if (sp->dskip[k]) LO_TRY(lo_nhwc_f16_to_nchw_f32(WSP(f16, h->o_skipg[k]), sp->dskip[k], B, (64 >> k) * (64 >> k), 64 << k, inv, st));
    if (h->overlap && !g_lo_prof_on) {
      LO_HIP(hipEventRecord(h->ev_join, h->side));
      LO_HIP(hipStreamWaitEvent(st, h->ev_join, 0));
    }
    return vae_gn_finalize(h, 0u, true, G, ws, inv, st);
  }
  // ---- latent: KL + reparameterisation backward (train_hybrid.py:862; lunar_generate.py:259-261)
  {
    hipEvent_t e = vae_arm_handover(h, ovl);
    int r_ = lo_latent_bwd(WSP(f16, h->o_dz), WSP(float, h->o_mu), WSP(float, h->o_lv), WSP(float, h->o_eps),
                           fused ? WSP(float, h->o_coefs) : nullptr, fused ? nullptr : gmu, fused ? nullptr : glv, loss_scale,
                           WSP(f16, h->o_dml), B, L, st);
    if (r_ != LO_OK) { g_lo_stop_event = nullptr; return r_; }
    LO_TRY(vae_armed_handover(e, st));
    if (ovl) LO_HIP(hipStreamWaitEvent(h->side, e, 0));
  }
  // ---- encoder heads (bias + weight gradient beside the chain, see decoder.fc above)
  LO_TRY(lo_colsum_f16(WSP(f16, h->o_dml), GRD(h->idx_fc_mu_b), B, 2 * L, inv, gs));
  if (fac) {
    // the four factors, transposed and batch-padded, are what the optimizer's AdamW pass multiplies: one launch
    const f16* src[4] = {WSP(f16, h->o_dml), WSP(f16, h->o_xflat), Gfc, WSP(f16, h->o_z)};
    f16* dst[4] = {WSP(f16, h->o_fac_dmlT), WSP(f16, h->o_fac_xT), WSP(f16, h->o_fac_gfcT), WSP(f16, h->o_fac_zT)};
    const int Cs[4] = {2 * L, 32768, 32768, L};
    LO_TRY(lo_transpose_pad_f16_multi(src, dst, Cs, 4, B, h->Bp, gs));
  } else {
    LO_TRY(lo_wgrad_run(h->g_head, WSP(f16, h->o_xflat), WSP(f16, h->o_dml), WSP(float, h->o_wslab_lin), GRD(h->idx_fc_mu_w), inv, gs));
  }
  LO_TRY(lo_conv_run(h->g_head_d, WSP(f16, h->o_dml), WSP(f16, h->o_wp_head_t), nullptr, nullptr, Gb, nullptr, nullptr, 1, st));
  early_ev = (((phase == 0 && h->norm_scratch) || (phase == 1 && h->async_handover)) && ovl && !lo_event_marker()) ? h->ev_pre : nullptr;
  if (early_ev) g_lo_stop_event = early_ev;                                  // the early-norm hand-over rides on part A's last launch
  {
    int r_ = lo_nchw_to_nhwc_f16(Gb, Ga, B, 64, 512, st);                    // Ga = gradient wrt enc4 output, NHWC
    if (r_ != LO_OK) { g_lo_stop_event = nullptr; return r_; }
  }
  if (g_lo_stop_event) { g_lo_stop_event = nullptr; early_ev = nullptr; }    // not picked up: the marker below
  }                   // ---------------- end of part A
  if (phase == 6) {
    // Encoder.forward's backward on its own: upstream gradients of mu / logvar and of the three skip maps (fp32 NCHW; NULL = zero)
    LO_TRY(vae_zero_gaps(h, G, st));
    for (int k = 0; k < 3; ++k) {
      const size_t n = (size_t)B * (64 >> k) * (64 >> k) * (64 << k);
      if (sp->gskip[k]) LO_TRY(lo_nchw_f32_to_nhwc_f16(sp->gskip[k], WSP(f16, h->o_skipg[k]), B, (64 >> k) * (64 >> k), 64 << k, loss_scale, st));
      else LO_HIP(hipMemsetAsync(WSP(f16, h->o_skipg[k]), 0, n * 2, st));
    }
    LO_HIP(hipMemsetAsync(WSP(f16, h->o_dz), 0, (size_t)B * L * 2, st));      // no decoder behind the latent: dz = 0
    LO_TRY(lo_latent_bwd(WSP(f16, h->o_dz), WSP(float, h->o_mu), WSP(float, h->o_lv), WSP(float, h->o_eps), nullptr, gmu, glv, loss_scale,
                         WSP(f16, h->o_dml), B, L, st));
    LO_TRY(lo_colsum_f16(WSP(f16, h->o_dml), GRD(h->idx_fc_mu_b), B, 2 * L, inv, st));
    LO_TRY(lo_wgrad_run(h->g_head, WSP(f16, h->o_xflat), WSP(f16, h->o_dml), WSP(float, h->o_wslab_lin), GRD(h->idx_fc_mu_w), inv, st));
    LO_TRY(lo_conv_run(h->g_head_d, WSP(f16, h->o_dml), WSP(f16, h->o_wp_head_t), nullptr, nullptr, Gb, nullptr, nullptr, 1, st));
    LO_TRY(lo_nchw_to_nhwc_f16(Gb, Ga, B, 64, 512, st));
  }
  const bool side_ok = h->overlap && !g_lo_prof_on;
  if (facdp) h->fac_scale = inv;
  const bool early_norm = phase == 0 && h->norm_scratch && (side_ok || fac1);      // decoder layers finalized here, norm of the phase-1 range taken early
  if (early_norm) {
    // everything from fc_mu.weight on is final once the decoder's side-stream weight gradients are: order the early
    // sum of squares after both streams' part A and let it run on the side stream beside the encoder backward
    hipStream_t ns = side_ok ? h->side : st;
    if (side_ok) {
      if (!early_ev) LO_HIP(hipEventRecord(h->ev_pre, st));
      LO_HIP(hipStreamWaitEvent(h->side, h->ev_pre, 0));
    }
    LO_TRY(vae_gn_finalize(h, 0u, true, G, ws, inv, ns));      // the decoder's GroupNorm / bias gradients belong to the range
    if (fac1) {
      // scratch[512..1024) = partial sums of squares of the range: [512, 767) everything behind decoder.fc.weight (decoder.fc.bias,
      // the decoder's convs and GroupNorms, the final conv), [767] the two head biases, [768, 896) fc_mu | fc_logvar weights and
      // [896, 1024) decoder.fc.weight from the Gram matrices of their factors -- no pass over the 50 M elements they stand for
      const size_t bh = h->p_off[h->idx_fc_mu_w], nh = (size_t)2 * L * 32768, bd = h->p_off[h->idx_dfc_w], nd = (size_t)32768 * L;
      float* sc = h->norm_scratch;
      LO_TRY(lo_sumsq_blocks(G + bd + nd, h->flat_elems - (bd + nd), sc + 512, 255, ns));
      LO_TRY(lo_sumsq_blocks(G + bh + nh, bd - (bh + nh), sc + 767, 1, ns));
      const LoLowrankNorm nl[2] = {{WSP(f16, h->o_dml), 2 * L, WSP(f16, h->o_xflat), 32768, WSP(float, h->o_gram), sc + 768, 128},
                                   {WSP(f16, h->o_z), L, WSP(f16, h->o_gfc), 32768, WSP(float, h->o_gram) + 128 * 128, sc + 896, 128}};
      LO_TRY(lo_lowrank_sumsq(nl, 2, B, inv, ns));
      h->fac_scale = inv;
      h->fac_ready = true;
    } else {
      LO_TRY(lo_sumsq_range(G, h->p_off[h->idx_fc_mu_w], h->flat_elems, h->norm_scratch, ns));
    }
  }
  if (phase == 1) {
    // two-call form: every gradient from fc_mu.weight to the end of the buffer is complete now -> join the side
    // stream (decoder weight gradients) and finish the decoder's GroupNorm / bias gradients, so that the caller can
    // start exchanging that range while the encoder backward runs
    if (h->overlap && !g_lo_prof_on && h->async_handover) {
      // asynchronous hand-over (lo_vae_set_async_handover): this stream is NOT held up until the decoder's side-stream weight
      // gradients have finished; the side stream waits for part A, finalizes the decoder's GroupNorm / bias gradients and leaves
      // "the range is final" as an event that lo_vae_wait_handover puts in front of the exchange
      if (!early_ev) LO_HIP(hipEventRecord(h->ev_pre, st));
      LO_HIP(hipStreamWaitEvent(h->side, h->ev_pre, 0));
      LO_TRY(vae_gn_finalize(h, 0u, true, G, ws, inv, h->side));
      LO_HIP(hipEventRecord(h->ev_range, h->side));
      h->range_pending = true;
      return LO_OK;
    }
    if (h->overlap && !g_lo_prof_on) {
      LO_HIP(hipEventRecord(h->ev_join, h->side));
      LO_HIP(hipStreamWaitEvent(st, h->ev_join, 0));
    }
    return vae_gn_finalize(h, 0u, true, G, ws, inv, st);
  }
  // ---- encoder stages 4..1 (phase 3: stage 4 only; phase 4: the rest; phase 6: all of them)
  const int s_hi = phase == 4 ? 2 : 3, s_lo = phase == 3 ? 3 : 0;
  for (int s = s_hi; s >= s_lo; --s) {
    ConvLayer& c0 = h->enc[s][0];
    ConvLayer& c1 = h->enc[s][1];
    ConvLayer& c2 = h->enc[s][2];
    // ResBlock tail + conv2:  dy = Ga -> ds = Gb (identity branch) ; dgrad -> Gd (grad wrt conv1 activation)
    LO_TRY(conv_gn_bwd(h, c2, Ga, WSP(f16, c0.o_a), 2, WSP(f16, c1.o_a), Gb, Gd, nullptr, P, G, ws, inv, st, &c1));
    // conv1: dy = Gd ; dgrad (+ ds) -> Gc (grad wrt the block input = c0 activation)
    LO_TRY(conv_gn_bwd(h, c1, Gd, nullptr, 0, WSP(f16, c0.o_a), nullptr, Gc, Gb, P, G, ws, inv, st, &c0));
    if (s > 0) {
      // strided conv: dy = Gc ; dgrad (+ decoder skip gradient) -> Ga (grad wrt the previous stage output)
      LO_TRY(conv_gn_bwd(h, c0, Gc, nullptr, 0, WSP(f16, h->o_eout[s - 1]), nullptr, Ga, WSP(f16, h->o_skipg[s - 1]), P, G,
                         ws, inv, st));
    } else {
      // (the first conv's weight gradient on the side stream with the finalize below beside it: neutral in round 2 and again in round 3
      // with launch-bound events, 22 900-23 137 against 22 864-23 106 -- it stays on this stream)
      const f16* dv0 = Gd;
      if (c0.dv_done) dv0 = WSP(f16, c0.o_dv);      // conv1's data gradient has already applied this layer's GroupNorm backward
      else
        LO_TRY(lo_gn_bwd_nofinal(Gc, WSP(f16, c0.o_v), nullptr, WSP(float, c0.o_stats), PRM(c0.p_gw), PRM(c0.p_gb), nullptr, Gd,
                                 WSP(float, c0.o_P1), WSP(float, c0.o_P2), B, 64 * 64, 64, 0, st, c0.np1));
      LO_TRY(lo_first_conv_wgrad(x, dv0, WSP(float, h->o_fcw_part), GRD(c0.p_w), B, inv, st));
      // the images' gradient (lo_vae_backward_dx / lo_vae_encoder_backward_dx): the same dv0 through the transposed first conv
      if (sp && sp->dx) LO_TRY(lo_image_dgrad(dv0, 64, 2, PRM(c0.p_w), B, inv, sp->dx, st));
    }
  }
  // ---- GroupNorm affine + conv bias gradients: all 16 layers in one launch (single call), or those of the stages this call ran.
  // Reads P1 / P2 rows only (all written on this stream): before the join, beside the side stream's last weight gradients
  if (phase == 3 && h->overlap && !g_lo_prof_on && h->async_handover) {      // see phase 1: the stage-4 range, without a join
    LO_HIP(hipEventRecord(h->ev_pre, st));
    LO_HIP(hipStreamWaitEvent(h->side, h->ev_pre, 0));
    LO_TRY(vae_gn_finalize(h, 0x8u, false, G, ws, inv, h->side));
    LO_HIP(hipEventRecord(h->ev_range, h->side));
    h->range_pending = true;
    return LO_OK;
  }
  LO_TRY(vae_gn_finalize(h, phase == 3 ? 0x8u : (phase == 4 ? 0x7u : 0xFu), phase == 0 && !early_norm, G, ws, inv, st));
  // ---- join the side stream (all weight gradients written) before anything that consumes the gradient buffer
  if (h->overlap && !g_lo_prof_on) {
    LO_HIP(hipEventRecord(h->ev_join, h->side));
    LO_HIP(hipStreamWaitEvent(st, h->ev_join, 0));
  }
  return LO_OK;
}

// Backward of lo_vae_decode_skips (Decoder.forward, lunar_generate.py:194-229): drecon [B,3,128,128] -> dz [B,L], the gradients
// of the skip maps that were added (fp32 NCHW, NULL = not wanted) and the decoder's parameter gradients (decoder.fc.weight to
// the end of flat_grads; the encoder range is not written).
extern "C" int lo_vae_decoder_backward(LoVae* h, const float* P, void* ws, const float* recon, const float* drecon, float loss_scale,
                                       float* dz, float* dskip0, float* dskip1, float* dskip2, float* G, void* stream) {
  LO_REQUIRE(h && drecon && dz, "lo_vae_decoder_backward: null argument");
  LoSplitBwd sp{dz, {dskip0, dskip1, dskip2}, {nullptr, nullptr, nullptr}, nullptr};
  return vae_backward_impl(h, 5, nullptr, P, ws, recon, nullptr, 0, drecon, nullptr, nullptr, loss_scale, G, stream, &sp);
}
// Backward of lo_vae_encode (Encoder.forward, lunar_generate.py:127-153): upstream gradients of mu, logvar [B,L] and of the skip
// maps (fp32 NCHW; any of them may be NULL = zero) -> the encoder's parameter gradients ([0, decoder.fc.weight) of flat_grads).
// lo_vae_encoder_backward_dx also writes the gradient wrt x (fp32 NCHW [B,3,128,128]; NULL = not wanted).
extern "C" int lo_vae_encoder_backward_dx(LoVae* h, const float* x, const float* P, void* ws, const float* gmu, const float* glv,
                                          const float* gskip0, const float* gskip1, const float* gskip2, float loss_scale, float* G,
                                          float* dx, void* stream) {
  LoSplitBwd sp{nullptr, {nullptr, nullptr, nullptr}, {gskip0, gskip1, gskip2}, dx};
  return vae_backward_impl(h, 6, x, P, ws, nullptr, nullptr, 0, nullptr, gmu, glv, loss_scale, G, stream, &sp);
}
extern "C" int lo_vae_encoder_backward(LoVae* h, const float* x, const float* P, void* ws, const float* gmu, const float* glv,
                                       const float* gskip0, const float* gskip1, const float* gskip2, float loss_scale, float* G,
                                       void* stream) {
  return lo_vae_encoder_backward_dx(h, x, P, ws, gmu, glv, gskip0, gskip1, gskip2, loss_scale, G, nullptr, stream);
}

// The Linear-layer weight gradients of the last fused backward written out after all (tests, tools, anybody who reads
// parameter_grads() in the factored mode): the same MFMA tiles the AdamW pass forms, stored to flat_grads instead.  `stream` must be
// ordered behind that backward (it is, for the stream the backward ran on).
extern "C" int lo_vae_materialize_linear_grads(LoVae* h, void* ws, float* G, void* stream) {
  LO_REQUIRE(h && ws && G, "lo_vae_materialize_linear_grads: null argument");
  if (!h->lin_factored) return LO_OK;           // the backward wrote them itself
  hipStream_t st = S(stream);
  const int L = h->L;
  LO_TRY(lo_lowrank_materialize(G + h->p_off[h->idx_fc_mu_w], WSP(f16, h->o_fac_xT), WSP(f16, h->o_fac_dmlT), 2 * L, 32768, h->B, h->fac_scale, st));
  return lo_lowrank_materialize(G + h->p_off[h->idx_dfc_w], WSP(f16, h->o_fac_zT), WSP(f16, h->o_fac_gfcT), 32768, L, h->B, h->fac_scale, st);
}
