// Internal launcher prototypes shared by the kernel translation units and the C-ABI layer.
#pragma once
#include "lo_common.h"

// the C ABI units (lo_api.hip, lo_vae_*.hip): the stream behind the void* of an entry point, and early return of an error code
static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
#define LO_TRY(call)            \
  do {                          \
    int _r = (call);            \
    if (_r != LO_OK) return _r; \
  } while (0)

const char* lo_get_error();

// lo_edge.hip
int lo_first_conv_fwd(const float* x, const float* w, const float* bias, f16* v, float* gn_partial, int B, hipStream_t st);
int lo_first_conv_wgrad(const float* x, const f16* dv, float* partial, float* dw, int B, float scale, hipStream_t st);
int lo_colsum(const float* partial, float* out, int nrow, int ncol, int stride, float scale, hipStream_t st);

// lo_imgdgrad.hip: data gradient of a 3x3 / padding 1 conv with 3 input channels onto fp32 NCHW [B,3,128,128] images
// (stride 1 with 32 channels: the teacher's conv1; stride 2 with 64 channels: the VAE's first conv).  dy fp16 NHWC, w fp32 [cout][3][3][3]
// seed (stride 1 / 32 channels only): dx = scale * conv2d_input(dy, w) + c[0] * (recon - target), c on the device, recon / target fp32 NCHW
struct LoImgSeed { const float* c; const float* recon; const float* target; };
int lo_image_dgrad(const f16* dy, int cout, int stride, const float* w, int B, float scale, float* dx, hipStream_t st,
                   const LoImgSeed* seed = nullptr);
// lo_teacher_heads.hip: the reward-gradient term of the hybrid step behind lo_loss_finalize (lo_vae_reward_term)
int lo_reward_term(const float* q_eval, int B, float weight, float accum, float loss_scale, const float* coefs, float* losses, float* out2,
                   float* seed_c, hipStream_t st);
int lo_final_conv_fwd(const f16* a4, const float* w, const float* bias, const float* target, float* recon,
                      float* mse_partial, int B, hipStream_t st);
int lo_final_conv_bwd(const f16* a4, const float* w, const float* recon, const float* target, const float* drecon,
                      const float* coef, float gscale, f16* da4, float* partial, float* dw, float* db, int B, float scale,
                      hipStream_t st, hipStream_t sum_st = nullptr, hipEvent_t sum_after = nullptr);   // sum_st: where the two column sums (dw, db) run

// lo_train.hip
int lo_head_reduce(const float* slab, const float* bias, const float* eps_in, uint64_t seed, float* mu, float* logvar,
                   f16* z, float* eps_out, float* kl_partial, int B, int L, int nsplit, hipStream_t st, float* mu_user = nullptr,
                   float* logvar_user = nullptr);
int lo_loss_finalize(const float* mse_partial, int n_mse, const float* kl_partial, int n_kl, float rw, float kw, float adv,
                     const float* adv_dev, float accum, float ls, float* losses, float* coefs, float n_rec, float n_lat,
                     hipStream_t st);
int lo_latent_bwd(const f16* dz, const float* mu, const float* logvar, const float* eps, const float* coefs,
                  const float* gmu, const float* glv, float gscale, f16* dml, int B, int L, hipStream_t st);
int lo_colsum_f16(const f16* x, float* out, int M, int N, float scale, hipStream_t st);
int lo_randn_fill(uint64_t seed, size_t first, size_t n, float* out, hipStream_t st);   // out[i] = the noise lo_head_reduce draws for element first + i
int lo_cast_f32_f16(const float* src, f16* dst, size_t n, hipStream_t st);
int lo_scale_f32(float* x, size_t n, float scale, hipStream_t st);
int lo_grad_accumulate_run(float* acc, const float* g, size_t n, float scale, bool first, hipStream_t st);   // acc = (first ? 0 : acc) + scale * g
int lo_ema_run(float* ema, const float* p, size_t n, float one_minus_decay, const float* gate, hipStream_t st);   // lo_ema.hip: ema += (p - ema)(1 - decay); gate[2] == 0 skips
int lo_dp_pack_f16_run(const float* g, f16* wire, size_t n, float scale, hipStream_t st);     // data-parallel exchange helpers
int lo_dp_unpack_f16_run(const f16* wire, float* g, size_t n, float inv_scale, hipStream_t st);
int lo_dp_unpack_f16_sumsq_run(const f16* wire, float* g, size_t n, float inv_scale, float* scratch, hipStream_t st);
int lo_dp_sum_shares_run(const void* recv, void* share, int world, size_t chunk, int is_f16, float inv_world, hipStream_t st);
int lo_transpose_cast(const float* src, f16* dst, int R, int C, hipStream_t st);
int lo_gradnorm(const float* g, size_t n, float max_norm, float* partial, float* norm_out, hipStream_t st,
                const unsigned int* fail = nullptr);   // fail: the engine's rendezvous-failure word (non-zero skips the update)
int lo_sumsq_range(const float* g, size_t begin, size_t end, float* partial, hipStream_t st);   // -> partial[512 .. 1024)
int lo_gradnorm_split(const float* g, size_t presummed_begin, float max_norm, float* partial, float* norm_out, hipStream_t st,
                      const unsigned int* fail = nullptr);
// upstream-gradient normalisation of the nn.Module boundary (GradScaler-scaled gradients; see lo_train.hip)
int lo_grad_scale_pick_run(const float* const g[5], const size_t n[5], float* scratch, hipStream_t st);
int lo_scale_copy_dev_run(const float* src, float* dst, size_t n, const float* scale_dev, hipStream_t st);
int lo_scale_dev_run(float* x, size_t n, const float* scale_dev, const unsigned int* fail, hipStream_t st);
int lo_adamw(float* p, const float* g, float* m, float* v, size_t n, const float* norm, float lr, float beta1, float beta2,
             float eps, float wd, int step, hipStream_t st, f16* cast = nullptr);
// what one optimizer step hands to every AdamW launch: norm[1] clip coefficient, norm[2] finite flag (lo_gradnorm); step counts from 1
struct LoAdamHyper { const float* norm; float lr, beta1, beta2, eps, wd; int step; };
static inline int lo_adamw(float* p, const float* g, float* m, float* v, size_t n, const LoAdamHyper& hp, hipStream_t st, f16* cast = nullptr) {
  return lo_adamw(p, g, m, v, n, hp.norm, hp.lr, hp.beta1, hp.beta2, hp.eps, hp.wd, hp.step, st, cast);
}

// lo_attn.hip
int lo_selfattn2d_fwd(const float* x, const float* wq, const float* bq, const float* wk, const float* bk, const float* wv,
                      const float* bv, const float* gamma, float* q, float* k, float* v, float* out, int B, int C, int N,
                      hipStream_t st);
size_t lo_selfattn2d_bwd_scratch(int B, int C, int N);
int lo_selfattn2d_bwd(const float* x, const float* wq, const float* wk, const float* wv, const float* gamma, const float* q,
                      const float* k, const float* v, const float* dy, float* scratch, float* dx, float* dwq, float* dbq,
                      float* dwk, float* dbk, float* dwv, float* dbv, float* dgamma, int B, int C, int N, hipStream_t st);
int lo_decode_sprites(const uint8_t* u8, float* out, int B, hipStream_t st);

// lo_attn8.hip: the VAE's bottleneck self-attention (8 x 8 x 512, q / k width 64) on fp16 NHWC tensors.  x, y, dy [B][64][512];
// qkv, dqkv [B][64][640] (q | k | v per position); dgamma_part [B]: per-sample shares of sum dy . O (they carry dy's loss scale)
int lo_attn8_fwd(const f16* x, const f16* qkv, const float* gamma, f16* y, int B, hipStream_t st);
int lo_attn8_bwd(const f16* qkv, const float* gamma, const f16* dy, f16* dqkv, float* dgamma_part, int B, hipStream_t st);
int lo_attn8_dgamma(const float* part, int B, float scale, float* out, hipStream_t st);     // out[0] = scale * sum, fixed order

// lo_lowrank.hip: rank-B Linear-layer weight gradients as factors (Gram-matrix norm, AdamW that forms the gradient tiles itself)
int lo_lowrank_bp(int B);                          // batch rounded up to the MFMA K step (32)
bool lo_lowrank_applies(int B, int N, int K);
int lo_transpose_pad_f16_multi(const f16* const* src, f16* const* dst, const int* C, int njobs, int R, int Rp, hipStream_t st);
struct LoLowrankNorm { const f16* fshort; int n_short; const f16* flong; int n_long; float* gram; float* partial; int nslots; };
int lo_lowrank_sumsq(const LoLowrankNorm* layers, int nlayers, int B, float scale, hipStream_t st);
struct LoLowrankMat { float* p; float* m; float* v; f16* cast; f16* cast_t; const f16* xt; const f16* yt; int N, K; };   // W [N][K] (cast_t [K][N]); xt [K][Bp], yt [N][Bp]
int lo_adamw_lowrank(const LoLowrankMat* mats, int nmat, int B, float gscale, const LoAdamHyper& hp, hipStream_t st);
int lo_lowrank_materialize_gathered(float* gout, const f16* xt, const f16* yt, size_t rank_stride_elems, int world, int N, int K, int B,
                                    float gscale, hipStream_t st);
// data parallel, mode 3: the same two from `world` gathered factor blocks (rank r's copy of a factor rank_stride_elems * r further on);
// world * lo_lowrank_bp(B) <= 512.  LoLowrankNorm's factors are then the TRANSPOSED ones ([n][Bp]); gram: [KT][KT] per layer
bool lo_lowrank_gathered_applies(int world, int B);
size_t lo_lowrank_gathered_gram_elems(int world, int B);   // fp32 elements of Gram scratch for two layers: 2 (world Bp)^2
int lo_adamw_lowrank_gathered(const LoLowrankMat* mats, int nmat, size_t rank_stride_elems, int world, int B, float gscale,
                              const LoAdamHyper& hp, hipStream_t st);
int lo_lowrank_sumsq_gathered(const LoLowrankNorm* layers, int nlayers, size_t rank_stride_elems, int world, int B, float scale, hipStream_t st);
int lo_sumsq_blocks(const float* g, size_t n, float* partial, int nblocks, hipStream_t st);   // lo_train.hip: partial[0 .. nblocks)
