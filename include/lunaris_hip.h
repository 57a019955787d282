/* lunaris_hip.h — C ABI of liblunaris_hip.so: the MI355X (gfx950) kernels behind the Lunaris-Orion VAE training step.
 *
 * The reference (MeryylleA/Lunaris-Orion) has no FFI / operator-plugin interface: its hot path
 * (TrainingManager._process_batch, /root/reference/train_hybrid.py:838-954) calls PyTorch ATen ops directly.  This
 * header therefore DEFINES the boundary; every entry point cites the reference lines whose arithmetic it replaces.
 * INTEGRATION.md shows the ctypes binding the Python host uses (lunaris_orion_amd/_lib.py).
 *
 * Conventions
 *   - every pointer is a raw DEVICE pointer (tensor.data_ptr()); the caller owns all memory, including workspaces;
 *     the library never allocates or frees device memory and never synchronises the device;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = the default stream);
 *   - return value: 0 = ok, <0 = error class (-1 bad argument/unsupported shape, -2 HIP error, -3 bad state); the
 *     message is available from lo_last_error() (thread-local);
 *   - activations inside the library are fp16 NHWC; tensors crossing the boundary are fp32 in PyTorch's layouts
 *     (images / reconstructions NCHW, parameters in their nn.Module layouts);
 *   - gradients flowing between kernels are multiplied by `loss_scale` (fp16 range); every parameter gradient that
 *     leaves the library is un-scaled (true gradient, fp32).
 *
 * What the caller provides
 *   - alignment: every tensor, scratch and workspace pointer is 16-byte aligned (the kernels' widest access: one 16-byte vector
 *     load / store / LDS-DMA lane, at element offsets that are multiples of 16 bytes from the pointer).  Nothing more is assumed:
 *     not the 256 / 512 bytes an allocator usually gives.  Tensors of 4-byte elements with fewer than four elements (a bias of
 *     three, a device scalar) need only their element's alignment;
 *   - sizes: every buffer needs exactly the number of elements its entry point states below (a size function, a dimension list or
 *     a count in a comment) and the library touches no byte outside them -- neither reads nor writes; there is no hidden padding
 *     requirement;
 *   - contents: inputs are read-only.  Output tensors, scratch buffers (slabs, partial tables, `rows`, `bws`) and workspaces may
 *     hold ANYTHING before a call (recycled allocator blocks, NaN): the library writes whatever it later reads, and zeroes the
 *     few regions of a workspace it relies on being zero the first time a handle sees that workspace pointer.  The exceptions are
 *     named where they occur: the AdamW moments m / v and the 1028-float optimizer `scratch` (its skipped-update counter
 *     accumulates) start zeroed by the caller.
 */
#ifndef LUNARIS_HIP_H
#define LUNARIS_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

const char* lo_last_error(void);
int lo_version(void);

/* Per-launch timing with HIP events recorded on the launch stream (used by bench.py's roofline leg).  Enable, run,
 * synchronise the stream, then read record i: kernel name, elapsed ms, algorithmic FLOPs and bytes of that launch.
 * on = 1: records carry the kernel name; on = 2: conv / GroupNorm launches of the VAE step are named per layer
 * ("fwd kind<k> HxW Cin->Cout", "dgrad L<n> ...", "wgrad L<n> ..."), which is how bench.py sums the encoder conv stack. */
void lo_prof_enable(int on);
int lo_prof_count(void);
int lo_prof_get(int i, char* name, int name_cap, double* ms, double* flops, double* bytes);

/* ---- op kinds for the generic implicit-GEMM entry points ---------------------------------------------------- */
enum {
  LO_KIND_CONV3_S1 = 0,        /* nn.Conv2d(k3,s1,p1)           lunar_generate.py:36,41          */
  LO_KIND_CONV3_S2 = 1,        /* nn.Conv2d(k3,s2,p1)           lunar_generate.py:102,109,116    */
  LO_KIND_CONVT4_S2 = 2,       /* nn.ConvTranspose2d(k4,s2,p1)  lunar_generate.py:169,175,181,187 */
  LO_KIND_CONV3_S1_DGRAD = 3,  /* aten::convolution_backward (input grad) of the above           */
  LO_KIND_CONV3_S2_DGRAD = 4,
  LO_KIND_CONVT4_S2_DGRAD = 5,
  LO_KIND_LINEAR = 6           /* nn.Linear                      lunar_generate.py:124,125,165    */
};

/* ---- single-op entry points (used by the parity tests; the step executor below calls the same launchers) ----- */

/* Packed fp16 weight size (elements) for an op of `kind` reading [B,H,W,Cin] and writing Cout channels. */
size_t lo_packed_weight_elems_for(int kind, int B, int H, int W, int Cin, int Cout);
/* canonical fp32 weight (nn.Module layout) -> packed fp16 operand of the implicit GEMM */
int lo_pack_weight_for(int kind, int B, int H, int W, int Cin, int Cout, const float* w, void* wp, void* stream);
/* out = conv(in) + bias (+ add_src); optional GroupNorm partial sums [B][MT][8][2]; returns MT through *mt_out.
 * in/out/add_src: fp16 NHWC.  Replaces aten::convolution / aten::addmm.  gn_partial: exactly B*MT*16 floats; MT is a function of
 * (kind, B, H, W, Cin, Cout) and of which optional pointers are non-NULL: the same arguments always give the same MT, so a caller
 * sizes the table from the *mt_out of an earlier call with those arguments (the step executor asks the selection function). */
int lo_conv_forward(int kind, int B, int H, int W, int Cin, int Cout, const void* in, const void* wp, const float* bias,
                    const void* add_src, void* out, float* gn_partial, int* mt_out, void* stream);
/* e4m3 operand forms (see LO_VAE_FP8_FWD below; Cin % 128 == 0, Cout % 64 == 0): x8 = fp8(8 * x16) saturating at 448;
 * wp8 / wscale[n_phase][Cout] from the packed fp16 weight (one scale per output channel: amax / 448, folded with 1/8);
 * the conv itself, same outputs as lo_conv_forward. */
int lo_quantize_act_f8(const void* x16, void* x8, size_t n, void* stream);
int lo_pack_weight_f8_for(int kind, int B, int H, int W, int Cin, int Cout, const void* wp16, void* wp8, float* wscale, void* stream);
int lo_conv_forward_f8(int kind, int B, int H, int W, int Cin, int Cout, const void* in8, const void* wp8, const float* wscale,
                       const float* bias, const void* add_src, void* out, float* gn_partial, int* mt_out, void* stream);
/* The fused-tap 3x3 stride-1 convolution of the teacher (lunar_evaluator.py:242-243,249-250: Conv2d k3 p1 + LeakyReLU(0.2), and
 * the per-channel sums its BatchNorm needs) on fp16 or e4m3 operands; H, W % 16 == 0, Cin % 64 == 0 (fp8: % 128), Cout % 128 == 0,
 * Cin <= 128.  bn_partial (may be NULL): [B*(H/16)*(W/16)][Cout][2] = (sum, sum of squares) of the stored values per pixel tile. */
int lo_conv3x3_fused_tap_forward(int B, int H, int W, int Cin, int Cout, int fp8, const void* in, const void* wp, const float* wscale,
                                 const float* bias, int leaky_relu, void* out, float* bn_partial, void* stream);
/* The 3x3 stride-1 convolution of the feature_dim 256 / 512 teacher (lunar_evaluator.py:242-243,249-250: Conv2d k3 p1 + LeakyReLU(0.2),
 * and the per-channel sums its BatchNorm needs) on e4m3 operands, implicit-GEMM form: out = fp16(acc * wscale + bias), LeakyReLU on
 * the rounded value when leaky_relu != 0.  in8 / wp8 / wscale as for lo_conv_forward_f8 (kind LO_KIND_CONV3_S1); Cin % 128 == 0,
 * Cout % 64 == 0, H and W powers of two, B*H*W a whole number of M tiles.  bn_partial (may be NULL): [*rows_out][Cout][2] = (sum, sum
 * of squares) of the stored values per M tile, fixed summation order; at most B*H*W/64 rows.  A shape that is not served returns
 * a non-zero code (lo_last_error says why) and launches nothing. */
int lo_teacher_conv3x3_forward_f8(int B, int H, int W, int Cin, int Cout, const void* in8, const void* wp8, const float* wscale,
                                  const float* bias, int leaky_relu, void* out, float* bn_partial, int* rows_out, void* stream);
/* Linear with split-K: y[M,N] (fp32 and/or fp16) = x[M,K] Wp[N,K]^T + bias.  slab: nsplit*M*N floats. */
int lo_linear_splitk(int M, int K, int N, const void* x, const void* wp, const float* bias, float* slab, int nsplit,
                     float* out32, void* out16, void* stream);
/* weight gradient of a FORWARD op `kind` (0,1,2,6): grad (canonical fp32 layout) = scale * sum_pixels dy (x) x. */
size_t lo_wgrad_slab_bytes_for(int kind, int B, int H, int W, int Cin, int Cout);
int lo_conv_wgrad(int kind, int B, int H, int W, int Cin, int Cout, const void* x, const void* dy, float* slab,
                  float* grad, float scale, void* stream);

/* GroupNorm(8,C)+Mish forward on the raw conv output v (fp16 NHWC): mode 0 y=mish(u); 1 y=mish(u)+other;
 * 2 y=mish(mish(u)+other) (ResBlock tail, lunar_generate.py:49-53).  stats[B][8][2] = (mean, rstd) is written. */
int lo_gn_mish_forward(const void* v, const float* gn_partial, int MT, const float* gamma, const float* beta,
                       const void* other, void* y, float* stats, int B, int HW, int C, int mode, void* stream);
/* backward of the above: dv (fp16), ds (mode 2: gradient of the identity branch), dgamma/dbeta/dbias (fp32 * scale).
 * P1: B*nchunk*C*2 floats, P2: B*nchunk*C floats of scratch (nchunk = lo_gn_nchunk_for(HW,C) <= 256). */
int lo_gn_nchunk_for(int HW, int C);
int lo_gn_mish_backward(const void* dy, const void* v, const void* other, const float* stats, const float* gamma,
                        const float* beta, void* ds, void* dv, float* P1, float* P2, float* dgamma, float* dbeta,
                        float* dbias, int B, int HW, int C, int mode, float scale, void* stream);

/* first conv Conv2d(3,64,k3,s2,p1) on fp32 NCHW images (lunar_generate.py:95) and its weight gradient.  x [B,3,128,128], w [64,3,3,3],
 * bias [64], v fp16 NHWC [B,64,64,64], gn_partial [B][64][8][2] floats (MT = 64), partial B*16*1728 floats, dw [64,3,3,3]. */
int lo_first_conv_forward(const float* x, const float* w, const float* bias, void* v, float* gn_partial, int B, void* stream);
int lo_first_conv_wgrad_op(const float* x, const void* dv, float* partial /*B*16*1728*/, float* dw, int B, float scale, void* stream);
/* data gradient of a 3x3 / padding 1 conv with 3 input channels onto the images: dx fp32 NCHW [B,3,128,128] = scale * conv2d_input(dy, w),
 * dy fp16 NHWC [B][128/stride][128/stride][cout], w fp32 [cout][3][3][3].  Built for (stride 2, cout 64: the VAE's encoder.down1.0) and
 * (stride 1, cout 32: the teacher's feature_extractor.conv1.0).  Deterministic (no atomics). */
int lo_image_dgrad_op(const void* dy, int cout, int stride, const float* w, int B, float scale, float* dx, void* stream);
/* the seeded store of the (stride 1, cout 32) kernel: dx = scale * conv2d_input(dy, w) + seed_coef[0] * (recon - target); seed_coef one float
 * on the device, recon / target fp32 NCHW [B,3,128,128], read at the address of the store.  seed_coef[0] == 0: the bits of lo_image_dgrad_op. */
int lo_image_dgrad_seed_op(const void* dy, int cout, int stride, const float* w, int B, float scale, const float* seed_coef,
                           const float* recon, const float* target, float* dx, void* stream);
/* final conv Conv2d(32,3,k3,p1)+tanh (+MSE partial sums, B*64 floats) (lunar_generate.py:192,227-228; train_hybrid.py:859).
 * a4 / da4 fp16 NHWC [B,128,128,32]; w [3,32,3,3], bias / db [3]; recon, target, drecon fp32 NCHW [B,3,128,128]; coef_dev one float;
 * partial B*64*867 floats of scratch. */
int lo_final_conv_forward(const void* a4, const float* w, const float* bias, const float* target, float* recon,
                          float* mse_partial, int B, void* stream);
int lo_final_conv_backward(const void* a4, const float* w, const float* recon, const float* target, const float* drecon,
                           const float* coef_dev, float gscale, void* da4, float* partial /*B*64*867*/, float* dw,
                           float* db, int B, float scale, void* stream);

/* PixelArtDataset.__getitem__ arithmetic (train_hybrid.py:181-182) for a whole batch on the device:
 * uint8 HWC [B,128,128,3] -> float32 CHW [B,3,128,128] = x/127.5 - 1. */
int lo_decode_sprites_u8(const void* u8_hwc, float* out_chw, int B, void* stream);

/* The latent / loss passes of the step as single ops: each is the launcher lo_vae_forward / lo_vae_loss / lo_vae_backward call, on
 * plain pointers (tests/test_train_ops_gpu.py).
 * lo_reparam_noise: out[i] (n floats), i < n = the N(0,1) sample lo_vae_forward(eps = NULL, seed) applies to flat latent element
 * first + i (b * latent_dim + l): the counter generator of the reparameterisation (torch.randn_like, lunar_generate.py:259-261), a
 * 64-bit hash of (seed, index) into two 24-bit uniforms and one Box-Muller cosine branch; |out| <= sqrt(-2 ln 2^-25) = 5.89.
 * oracle/noise_ref.py restates it.
 * lo_latent_forward_op (fc_mu | fc_logvar split-K reduction + reparameterisation + KL partial sums; lunar_generate.py:124-125,
 * 150-152,259-261; train_hybrid.py:862): slab nsplit*B*2L floats ([nsplit][B][mu | logvar]), bias 2L; eps_in B*L floats or NULL
 * (then the generator above with `seed`); out: mu, logvar, eps_out B*L floats each, z B*L halves = fp16(mu + eps * exp(logvar / 2)),
 * kl_partial ceil(B*L / 256) floats, each the sum of 1 + logvar - mu^2 - exp(logvar) over 256 consecutive elements; mu_user /
 * logvar_user: both NULL, or B*L floats each receiving copies of mu / logvar.
 * lo_latent_backward_op: dz B*L halves; mu, logvar, eps B*L floats; coefs NULL or 2 floats ([1] = the KL coefficient c:
 * dmu = c * mu + dz, dlogvar = c/2 * (exp(logvar) - 1) + dz * eps/2 * exp(logvar / 2)); gmu / glv NULL or B*L floats, added times
 * gscale; dml B*2L halves = per sample [dmu | dlogvar].
 * lo_loss_finalize_op: mse_partial n_mse floats, kl_partial n_kl floats (summed in double, fixed order); adv_dev NULL or 1 float
 * overriding mean_advantage; losses 4 floats = recon (sum mse / n_rec), kl (-0.5 sum kl / n_lat), (rw * recon + kw * kl + pg) / accum,
 * pg = -adv * recon; coefs 2 floats = loss_scale * (rw - adv) / accum * 2 / n_rec, loss_scale * kw / accum / n_lat.
 * lo_colsum_f16_op: x M*N halves, out N floats: out[j] = scale * sum_m x[m][j] (the Linear layers' bias gradients; fp32 sums in a
 * fixed order); N a multiple of 8, else -1. */
int lo_reparam_noise(uint64_t seed, size_t first, size_t n, float* out, void* stream);
int lo_latent_forward_op(const float* slab, const float* bias, const float* eps_in, uint64_t seed, float* mu, float* logvar, void* z,
                         float* eps_out, float* kl_partial, int B, int L, int nsplit, float* mu_user, float* logvar_user, void* stream);
int lo_latent_backward_op(const void* dz, const float* mu, const float* logvar, const float* eps, const float* coefs, const float* gmu,
                          const float* glv, float gscale, void* dml, int B, int L, void* stream);
int lo_loss_finalize_op(const float* mse_partial, int n_mse, const float* kl_partial, int n_kl, float recon_weight, float kl_weight,
                        float mean_advantage, const float* adv_dev, float accum, float loss_scale, float* losses, float* coefs,
                        float n_rec, float n_lat, void* stream);
int lo_colsum_f16_op(const void* x, float* out, int M, int N, float scale, void* stream);

/* SelfAttention2d.forward (lunar_generate.py:68-78; the module is defined but never instantiated by the reference):
 * out = gamma * (V softmax(Q^T K)^T) + x with Q,K = 1x1 convs to C/8 channels, V = 1x1 conv to C channels.  x/out fp32
 * [B,C,N=H*W]; q,k ([B,C/8,N]) and v ([B,C,N]) are caller-provided scratch/outputs.  C and N multiples of 64, C <= 512. */
int lo_selfattn2d_forward(const float* x, const float* wq, const float* bq, const float* wk, const float* bk, const float* wv,
                          const float* bv, const float* gamma, float* q, float* k, float* v, float* out, int B, int C,
                          int N, void* stream);
/* Backward of the same module (autograd of lunar_generate.py:68-78): q, k, v are the forward's outputs; scratch:
 * lo_selfattn2d_backward_scratch_elems(B, C, N) floats.  Writes dx [B,C,N] and the gradients of the three 1x1 convs and of
 * gamma (not accumulated: overwritten).  No N x N tensor is materialised; all sums are in a fixed order. */
size_t lo_selfattn2d_backward_scratch_elems(int B, int C, int N);
int lo_selfattn2d_backward(const float* x, const float* wq, const float* wk, const float* wv, const float* gamma,
                           const float* q, const float* k, const float* v, const float* dy, float* scratch, float* dx,
                           float* dwq, float* dbq, float* dwk, float* dbk, float* dwv, float* dbv, float* dgamma, int B,
                           int C, int N, void* stream);
/* The same block at the VAE's bottleneck (C = 512, N = 64 positions, q / k width 64) as the step executor runs it (LO_VAE_ATTN), on
 * fp16 NHWC tensors: x, y, dy [B][64][512]; qkv, dqkv [B][64][640] = per position the 64 query, 64 key and 512 value channels
 * (qkv = x Wqkv^T + b, one GEMM of the conv family); gamma: one fp32 on the device.  Forward: y = gamma * softmax_j(q_i . k_j) v_j
 * + x.  Backward: from dy (any loss scale that keeps it finite in fp16) the gradient dqkv wrt qkv, recomputing the softmax from qkv,
 * and dgamma_part [B] fp32 = per-sample sum dy . O (same loss scale).  The residual's share of dx is NOT in dqkv: the executor adds
 * dy where it forms dx = dy + dqkv Wqkv; x is not read by the backward and may be NULL.  Both products of either direction run on
 * v_mfma_f32_16x16x32_f16; no 64 x 64 tensor reaches global memory; sums have a fixed order (bitwise reproducible). */
int lo_attn8_forward(const void* x, const void* qkv, const float* gamma, void* y, int B, void* stream);
int lo_attn8_backward(const void* x, const void* qkv, const float* gamma, const void* dy, void* dqkv, float* dgamma_part, int B,
                      void* stream);

/* clip_grad_norm_ + AdamW over one flat fp32 buffer (train_hybrid.py:913,921; :504-509).  scratch: 1024+4 floats;
 * scratch[1024..1026] = (grad norm, clip coef, finite flag) afterwards; scratch[1027] counts the calls whose gradient norm was
 * not finite (those updates are skipped, like a step under torch.cuda.amp.GradScaler, train_hybrid.py:917-923). */
int lo_clip_adamw_step(float* p, const float* g, float* m, float* v, size_t n, float max_norm, float lr, float beta1,
                       float beta2, float eps, float weight_decay, int step, float* scratch, void* stream);

/* lo_clip_adamw_step for a caller whose backward already summed the squares of [presummed_begin, n) into scratch[512..1024)
 * (lo_vae_set_gradnorm_scratch): only [0, presummed_begin) is read for the norm. */
int lo_clip_adamw_step_presummed(float* p, const float* g, float* m, float* v, size_t n, size_t presummed_begin, float max_norm,
                                 float lr, float beta1, float beta2, float eps, float weight_decay, int step, float* scratch,
                                 void* stream);

/* Gradient accumulation: acc[i] = (first ? 0 : acc[i]) + scale * g[i] over n fp32 elements, the pass that adds one micro-batch's
 * gradients to those of its window.  The reference zeroes the gradients at the top of every _process_batch
 * (train_hybrid.py:841-842), divides the losses by gradient_accumulation_steps (:895-896) and steps on every k-th call only (:907), so
 * it keeps one micro-batch of k; with this entry behind every backward the step sees all k (VAEStepper(accumulate_gradients=True),
 * opt-in).  first != 0: acc is NOT read -- whatever it held, NaN included, is overwritten.  acc and g must not overlap (-1); any
 * 4-byte-aligned pointers and any n >= 1.  16-byte loads and stores from acc's first 16-byte boundary on (g as well where it has the
 * same phase, as the same range of two flat buffers has), single elements in front and behind; no atomics: bitwise reproducible. */
int lo_grad_accumulate(float* acc, const float* g, size_t n, float scale, int first, void* stream);

/* Tool level: two passes of the optimizer step as single calls, exported for measurement only (tools/op_bench.py); the training
 * path never calls them and a binding may leave them out.
 * The AdamW pass alone (train_hybrid.py:921) on one flat range of n elements -- p, g, m, v: n floats -- as lo_clip_adamw_step and
 * lo_vae_optimizer_step launch it.  norm: NULL, or 3 floats as scratch[1024..1026] ([1] multiplies the gradient, [2] == 0 skips the
 * update); cast: NULL, or n halves = fp16(p) after the update, written by the same pass.
 * lo_transpose_f16: dst [cols][rows] = src [rows][cols]^T, fp16, rows and cols multiples of 64: the transposed operand copies of the
 * two Linear weights.  Both exist at this level for tools/op_bench.py --op lowrank_gathered (the materialised path, pass by pass). */
int lo_adamw_range(float* p, const float* g, float* m, float* v, size_t n, const float* norm, float lr, float beta1, float beta2,
                   float eps, float weight_decay, int step, void* cast, void* stream);
int lo_transpose_f16(const void* src, void* dst, int rows, int cols, void* stream);

/* ---- the VAE step executor (LunarisCoreVAE.forward / backward, lunar_generate.py:263-276) -------------------- */
typedef struct LoVae LoVae;
int lo_vae_create(int batch, int latent_dim, LoVae** out);
/* The same with mode flags.  LO_VAE_FP8_FWD (BASELINE config 5): the forward convolutions whose input channel count is a
 * multiple of 128 (ResBlock / stride-2 convs at 128-512 channels, transposed convs at 512 / 256 / 128) run on OCP e4m3
 * operands (v_mfma_scale_f32_16x16x128_f8f6f4, fp32 accumulation): activations as fp8(8 * value) written next to the fp16
 * copy by the producing GroupNorm kernel, weights with one scale per output channel.  The backward is unchanged (fp16
 * operands).  No reference counterpart: the reference's low-precision mode is torch.cuda.amp fp16 autocast
 * (train_hybrid.py:850).  Unknown flag bits are an error. */
#define LO_VAE_FP8_FWD 1u
/* LO_VAE_ATTN: the model has the reference's SelfAttention2d(512) (lunar_generate.py:56-78) at both ends of the bottleneck: on the
 * encoder's stage-4 output before the flatten, and on decoder.fc's output before up1.  14 more parameter tensors (86): in state_dict
 * order encoder.attn.{gamma, query_conv.weight, .bias, key_conv.weight, .bias, value_conv.weight, .bias} between down4 and fc_mu,
 * the same under decoder.attn between decoder.fc and up1.  In the flat buffer each site is gamma | Wq | Wk | Wv | bq | bk | bv (one
 * [640][512] matrix and one [640] bias); the encoder site sits before fc_mu.weight, the decoder site behind decoder.fc.bias.
 * Not combinable with LO_VAE_FP8_FWD (up1 would read an e4m3 copy of the attention's output): that is an error. */
#define LO_VAE_ATTN 2u
int lo_vae_create_ex(int batch, int latent_dim, unsigned flags, LoVae** out);
void lo_vae_destroy(LoVae* h);
/* Early gradient norm: with a scratch set (the 1028-float scratch of lo_clip_adamw_step), a single-call lo_vae_backward takes the
 * sum of squares of the range lo_vae_phase1_grad_range names as soon as it is final, beside the encoder backward, and
 * lo_clip_adamw_step_presummed(.., presummed_begin = begin of that range, ..) reads only the rest.  lo_vae_gradnorm_presummed
 * says whether the next backward will do so (it needs the library's side stream).  NULL scratch: off. */
int lo_vae_set_gradnorm_scratch(LoVae* h, float* scratch);
/* The same partial sum for a caller that exchanges gradients between processes (data parallel: the norm is that of the AVERAGED
 * gradients, so the library cannot take it inside the backward): sum of squares of flat_grads[begin, end) into scratch[512..1024),
 * to be enqueued behind the exchange of that range, on whatever stream ran it; lo_clip_adamw_step_presummed / the `presummed` form
 * of lo_vae_optimizer_step then read only [0, begin).  clip_grad_norm_'s norm (train_hybrid.py:913), split in two.  The pass issues
 * 16-byte loads from flat_grads + begin on: begin must be a multiple of 4 elements (every range the library names starts at a multiple
 * of 64); any other begin returns -1 with a message and launches nothing.  end is free (the last (end - begin) % 4 elements are read singly). */
int lo_gradnorm_early_range(const float* flat_grads, size_t begin, size_t end, float* scratch, void* stream);
/* Asynchronous hand-over of the phased backward's gradient ranges (data parallel).  By default lo_vae_backward_phase(1) and (3)
 * return with `stream` ordered behind everything that writes their range (the library's side stream is joined).  With on = 1 they
 * do not hold `stream` up: the range's completion is left as an event, and lo_vae_wait_handover(h, s) makes stream `s` -- the one
 * that runs the exchange -- wait for it.  Call it once per phase 1 / 3, before phase 3 / 4 is enqueued.  Phases 2 and 4 and the
 * single-call backward are unchanged.  No reference counterpart (DDP's bucket hooks are the nearest thing). */
int lo_vae_set_async_handover(LoVae* h, int on);
int lo_vae_wait_handover(LoVae* h, void* stream);
int lo_vae_gradnorm_presummed(const LoVae* h);
/* parameters live in ONE flat fp32 buffer; tensor i (state_dict order, 72 tensors) starts at this element offset */
int lo_vae_num_params(const LoVae* h);
size_t lo_vae_param_offset(const LoVae* h, int index);
size_t lo_vae_param_numel(const LoVae* h, int index);
size_t lo_vae_flat_elems(const LoVae* h);
size_t lo_vae_workspace_bytes(const LoVae* h);
/* refresh the packed fp16 operand copies from the fp32 master parameters (call after every parameter update) */
int lo_vae_pack(LoVae* h, const float* flat_params, void* ws, void* stream);
/* clip_grad_norm_ + AdamW (train_hybrid.py:913,921) + lo_vae_pack in ONE call, pipelined with the next forward: encoder stages
 * 1..3 (3 % of the parameters, what the next forward reads first) are updated on `stream`; the last encoder stage, the Linear
 * layers and the decoder (97 %), their fp16 casts and packs follow on the library's side stream beside the next encoder forward
 * (lo_vae_forward waits where it needs them).  p / g / m / v: the flat fp32 buffers of lo_vae_flat_elems() elements; scratch as for lo_clip_adamw_step; flags:
 * LO_OPT_PRESUMMED as for lo_clip_adamw_step_presummed, LO_OPT_SERIAL for the un-pipelined order.  The clip kernel also reads the
 * plan's rendezvous-failure word (lo_vae_sync_fail_word): when set, the update is skipped on the device like one with a non-finite
 * norm (GradScaler semantics, train_hybrid.py:917-923) -- and stays skipped until the host has looked.  Afterwards parameters from encoder.down4 on may still be in flight: call lo_vae_join before
 * reading them on any stream other than through this executor. */
#define LO_OPT_PRESUMMED 1   /* scratch[512..1024) already holds the sum of squares of the phase-1 range */
#define LO_OPT_SERIAL 2      /* no pipelining: norm, AdamW of everything and lo_vae_pack in order on `stream` */
int lo_vae_optimizer_step(LoVae* h, float* p, const float* g, float* m, float* v, void* ws, float max_norm, float lr, float beta1,
                          float beta2, float eps, float weight_decay, int step, float* scratch, int flags, void* stream);
int lo_vae_join(LoVae* h, void* stream);   /* `stream` waits for the side-stream work of lo_vae_pack / lo_vae_optimizer_step */
/* Weight EMA (no reference counterpart; VAEStepper(ema_decay=...), opt-in).  ema[i] += (p[i] - ema[i]) * one_minus_decay over n fp32
 * elements: subtract, multiply, add, each rounded to fp32 (no fma), so numpy float32 replays it bit for bit and launches over
 * sub-ranges equal one launch.  ema and p 16-byte aligned and not overlapping, any n >= 1.  gate: NULL, or 3 floats as
 * scratch[1024..1026] of lo_clip_adamw_step -- gate[2] == 0 (a skipped update) writes nothing. */
int lo_ema_update(float* ema, const float* p, size_t n, float one_minus_decay, const float* gate, void* stream);
/* The same over all lo_vae_flat_elems() elements, ordered by the engine: behind every parameter write of the last
 * lo_vae_optimizer_step on this handle (on its side stream after a pipelined step, beside the next forward) and ahead of the next
 * one; lo_vae_join covers it.  scratch: that step's scratch (the gate is scratch + 1024), or NULL for no gate. */
int lo_vae_ema_update(LoVae* h, const float* flat_params, float* ema, float one_minus_decay, const float* scratch, void* stream);
/* Factored Linear-layer gradients.  fc_mu | fc_logvar ([2L, 32768]) and decoder.fc ([32768, L]) hold 82 % of the parameters
 * (lunar_generate.py:124-125, 165) and at batch B their weight gradients dW = dY^T X have rank B.  With the mode on (batch <= 128),
 * a FUSED single-call lo_vae_backward does not write those two gradients into flat_grads: it keeps the factors (transposed,
 * batch-padded fp16 copies in the workspace), takes their share of clip_grad_norm_'s norm (train_hybrid.py:913) from two B x B Gram
 * matrices per layer -- ||dY^T X||_F^2 = sum_{b,b'} (dY dY^T)[b,b'] (X X^T)[b,b'] -- into the scratch set by
 * lo_vae_set_gradnorm_scratch (required), and lo_vae_optimizer_step (LO_OPT_PRESUMMED required) forms each gradient tile with MFMA
 * inside its AdamW pass (train_hybrid.py:921).  Same update to fp32 rounding; 12 of 38 bytes of HBM traffic per parameter less.
 * Explicit-gradient backwards (the autograd path) and lo_vae_backward_phase always write every gradient.
 * lo_vae_materialize_linear_grads: writes the two gradients of the last fused backward into flat_grads after all (tests, tools). */
int lo_vae_set_linear_factored(LoVae* h, int mode);   /* 0 off, 1 single process (above), 2 / 3 data parallel (below) */
/* Data parallel (mode 2; no reference counterpart: the reference has no distributed code).  lo_vae_backward_phase(1) then leaves the
 * two Linear layers' factors instead of their weight gradients: one contiguous block of the workspace (lo_vae_factor_block:
 * dml^T | xflat^T | Gfc^T | z^T, transposed, batch-padded fp16; 8.6 MB at batch 64 / latent 512).  The ranks all-gather the blocks
 * (exact, and 8.6 MB per rank on the wire instead of 201 MB of gradients) and each calls lo_vae_materialize_gathered_linear_grads
 * on the gathered buffer (block r at gathered + r * bytes): flat_grads of the two matrices = (1 / world) sum_r dY_r^T X_r / loss
 * scale -- the all-reduce(AVG) of the per-rank gradients to fp32 rounding.  Everything else of the range is exchanged as before. */
int lo_vae_factor_block(const LoVae* h, size_t* byte_offset, size_t* bytes);
int lo_vae_materialize_gathered_linear_grads(LoVae* h, const void* gathered, int world, float* flat_grads, void* stream);
/* Mode 3: as mode 2 up to the all-gather, but the averaged matrices are never written either.  Behind the all-gather and the exchange
 * of the rest of the phase-1 range, on the stream that ran them, the caller enqueues lo_vae_gathered_early_norm: it fills
 * scratch[512..1024) of the 1028-float optimizer scratch -- everything behind decoder.fc.weight and the two head biases from the
 * averaged flat_grads, the two matrices as ||sum_r dY_r^T X_r||_F^2 / (loss scale * world)^2 from Gram matrices over the combined
 * batch axis of world * Bp samples (Bp = batch rounded up to 32), cross-rank terms included -- and remembers `gathered` and `world`.
 * lo_vae_optimizer_step (LO_OPT_PRESUMMED required, serial or pipelined) then forms every gradient tile inside its AdamW pass with
 * the contraction running over all ranks' blocks in rank order (no atomics: every rank gets the same bits from the same buffer),
 * and writes the fp16 operand copies like mode 1.  Limits: world * Bp <= 512 (8 ranks at batch 64); above that the norm call
 * returns -1 and the caller stays in mode 2.
 *   gathered      world * lo_vae_factor_block bytes, block r at r * bytes; it must stay unchanged until the work
 *                 lo_vae_optimizer_step enqueues has read it.  The next step's lo_vae_backward_phase(1) waits for that work, so a
 *                 stream ordered behind that call may overwrite the buffer.
 *   gram_scratch  lo_vae_gathered_scratch_bytes(h, world) bytes = 2 * (world * Bp)^2 floats, contents unspecified
 * lo_vae_linear_factored returns the mode (1 or 3) while flat_grads does not hold the two matrices, 0 otherwise (mode 2 included);
 * lo_vae_materialize_linear_grads writes them out after all: in mode 3 the averaged ones, from the remembered gathered buffer. */
size_t lo_vae_gathered_scratch_bytes(const LoVae* h, int world);   /* 0: world * Bp is above 512 */
int lo_vae_gathered_early_norm(LoVae* h, const void* gathered, int world, float* gram_scratch, const float* flat_grads, float* scratch,
                               void* stream);
int lo_vae_linear_factored(const LoVae* h);
/* Mode 3 for gradient accumulation on one GPU (VAEStepper(accumulate_gradients=True); the reference steps on one micro-batch of k,
 * train_hybrid.py:841-842, 907): the k micro-batches of a window are k "ranks" arriving one after the other, each leaving its factor
 * block behind lo_vae_backward_phase(1), and their gradients -- each already carrying lo_vae_loss's 1 / accum (:895-896) -- are ADDED.
 * on != 0: every pass over gathered blocks (lo_vae_gathered_early_norm, the AdamW tiles, both materialize calls) multiplies by
 * 1 / loss scale instead of 1 / (loss scale * world).  Off by default; lo_vae_set_linear_factored does not reset it. */
int lo_vae_set_gathered_sum(LoVae* h, int on);
int lo_vae_materialize_linear_grads(LoVae* h, void* ws, float* flat_grads, void* stream);
/* The two passes of mode 3 on plain pointers.  W is [N][K] fp32 (N % 64 == 0, K % 64 == 0); its averaged gradient is
 * gscale * sum_r dY_r^T X_r with the factors TRANSPOSED and batch-padded, fp16: xt [K][Bp], yt [N][Bp] per rank, columns
 * batch .. Bp - 1 zero (Bp = batch rounded up to 32, batch <= 128), rank r's copy rank_stride_elems * r elements behind rank 0's
 * (a multiple of 8).  world * Bp <= 512, else -1.
 * lo_lowrank_gathered_adamw: AdamW (train_hybrid.py:921) of W in place.  p, m, v: N * K floats; cast: N * K halves = fp16(p) after
 * the update; cast_t: K * N halves = its transpose (either may be NULL); xt: (world - 1) * rank_stride_elems + K * Bp halves, yt:
 * (world - 1) * rank_stride_elems + N * Bp; norm: NULL, or 3 floats as scratch[1024..1026] of lo_clip_adamw_step -- [1] multiplies
 * the gradient, [2] == 0 skips the update.
 * lo_lowrank_gathered_sumsq: partial[0..127] = 128 partial sums (every one written) of scale^2 * ||sum_r dY_r^T X_r||_F^2.  fshort_t /
 * flong_t: the two factors ([n_short][Bp], [n_long][Bp]; row lengths multiples of 32; which of X, dY is which does not matter), sizes
 * as xt / yt; gram_scratch: lo_lowrank_gathered_scratch_bytes(world, batch) bytes = (world * Bp)^2 floats, contents unspecified. */
size_t lo_lowrank_gathered_scratch_bytes(int world, int batch);   /* 0: unsupported */
int lo_lowrank_gathered_sumsq(const void* fshort_t, int n_short, const void* flong_t, int n_long, size_t rank_stride_elems, int world,
                              int batch, float scale, float* gram_scratch, float* partial, void* stream);
int lo_lowrank_gathered_adamw(float* p, float* m, float* v, void* cast, void* cast_t, const void* xt, const void* yt,
                              size_t rank_stride_elems, int world, int N, int K, int batch, float gscale, const float* norm, float lr,
                              float beta1, float beta2, float eps, float weight_decay, int step, void* stream);
/* forward.  eps: explicit N(0,1) noise [B,L] or NULL (on-device counter RNG with `seed`).  target: images for the fused
 * MSE partial sums or NULL.  Outputs recon [B,3,128,128], mu, logvar [B,L] (fp32). */
int lo_vae_forward(LoVae* h, const float* x, const float* eps, uint64_t seed, const float* flat_params, void* ws,
                   float* recon, float* mu, float* logvar, const float* target, void* stream);
/* decoder only, without skip connections: LunarisCoreVAE.sample (lunar_generate.py:278-291).  z fp32 [B,L]. */
int lo_vae_decode(LoVae* h, const float* z, const float* flat_params, void* ws, float* recon, void* stream);
/* The two halves of that forward as the reference's sub-modules expose them (lunar_generate.py:273-275 calls them in turn;
 * callers may too).  Encoder.forward (:127-153): mu, logvar [B,L] and the skip list [B,64,64,64], [B,128,32,32], [B,256,16,16]
 * (fp32 NCHW; NULL = not wanted).  Decoder.forward(z, skips) (:194-229): n_skips = len(skips) in 0..3 with the reference's
 * guards (skips[2] is added after up1 when len >= 3, skips[1] after up2 when len >= 2, skips[0] after up3 when len >= 1). */
int lo_vae_encode(LoVae* h, const float* x, const float* flat_params, void* ws, float* mu, float* logvar, float* skip0, float* skip1,
                  float* skip2, void* stream);
int lo_vae_decode_skips(LoVae* h, const float* z, int n_skips, const float* skip0, const float* skip1, const float* skip2,
                        const float* flat_params, void* ws, float* recon, void* stream);
/* Their backward passes (autograd of the same lines).  lo_vae_decoder_backward follows lo_vae_decode_skips (or lo_vae_forward):
 * drecon [B,3,128,128] -> dz [B,L], the gradients of the skip maps (fp32 NCHW, NULL = not wanted) and the decoder's parameter
 * gradients (decoder.fc.weight to the end of flat_grads; nothing before it is written except the alignment gaps).
 * lo_vae_encoder_backward follows lo_vae_encode (or lo_vae_forward): upstream gradients of mu / logvar [B,L] and of the skip maps
 * (NULL = zero) -> the encoder's parameter gradients ([0, decoder.fc.weight) of flat_grads).  All gradients leave un-scaled. */
int lo_vae_decoder_backward(LoVae* h, const float* flat_params, void* ws, const float* recon, const float* drecon, float loss_scale,
                            float* dz, float* dskip0, float* dskip1, float* dskip2, float* flat_grads, void* stream);
int lo_vae_encoder_backward(LoVae* h, const float* x, const float* flat_params, void* ws, const float* gmu, const float* glv,
                            const float* gskip0, const float* gskip1, const float* gskip2, float loss_scale, float* flat_grads,
                            void* stream);
/* the same, and the gradient wrt the images x: dx fp32 NCHW [B,3,128,128] (NULL = not wanted; lo_vae_encoder_backward is this with NULL) */
int lo_vae_encoder_backward_dx(LoVae* h, const float* x, const float* flat_params, void* ws, const float* gmu, const float* glv,
                               const float* gskip0, const float* gskip1, const float* gskip2, float loss_scale, float* flat_grads,
                               float* dx, void* stream);
/* reduce the loss partial sums of the last forward; losses_dev[4] = recon_loss, kl_loss, vae_loss, pg_loss.
 * vae_loss = (recon_weight*recon + kl_weight*kl - mean_advantage*recon)/accum  (train_hybrid.py:886-889,895).
 * adv_dev (device scalar) overrides mean_advantage when not NULL.  Also prepares the gradient seeds for
 * lo_vae_backward(fused=1). */
int lo_vae_loss(LoVae* h, void* ws, float recon_weight, float kl_weight, float mean_advantage, const float* adv_dev,
                float accum, float loss_scale, float* losses_dev, void* stream);
/* The reward-gradient term of the hybrid step, behind lo_vae_loss on the same stream: q_eval = quality_scores [B][4] of the eval-mode
 * teacher on the reconstruction.  out2 = {-weight * mean(q_eval) / accum, mean(q_eval)}; the term is added to losses_dev[2] (vae_loss);
 * seed_coef[0] = the un-scaled MSE coefficient of d vae_loss / d recon (lo_vae_loss's, its loss scale divided out) for
 * lo_teacher_eval_backward_seed.  loss_scale: the one lo_vae_loss was given. */
int lo_vae_reward_term(LoVae* h, void* ws, const float* q_eval, float weight, float accum, float loss_scale, float* losses_dev,
                       float* out2, float* seed_coef, void* stream);
/* backward into flat_grads (same layout as the parameters; every element is written).  fused=1: gradients of the
 * vae_loss prepared by lo_vae_loss (needs `target`).  fused=0: explicit upstream gradients drecon/gmu/glv (fp32, may
 * be NULL = zero).  fused=2: the latent seeds (KL) of lo_vae_loss as fused=1, the reconstruction's gradient the explicit, un-scaled
 * drecon (the seed lo_teacher_eval_backward_seed leaves: reward term + MSE term). */
int lo_vae_backward(LoVae* h, const float* x, const float* flat_params, void* ws, const float* recon, const float* target,
                    int fused, const float* drecon, const float* gmu, const float* glv, float loss_scale,
                    float* flat_grads, void* stream);
/* the same, and the gradient wrt the images x: dx fp32 NCHW [B,3,128,128] (NULL = not wanted; lo_vae_backward is this with NULL).  Meant for
 * fused = 0 (the module's autograd node); the steppers do not ask for it. */
int lo_vae_backward_dx(LoVae* h, const float* x, const float* flat_params, void* ws, const float* recon, const float* target,
                       int fused, const float* drecon, const float* gmu, const float* glv, float loss_scale,
                       float* flat_grads, float* dx, void* stream);

/* GroupNorm + Mish run inside the producing convolution's epilogue wherever the kernel that owns the layer supports it (the
 * workgroups holding one sample's tiles exchange their partial sums through the workspace and wait for each other; csrc/lo_common.h,
 * LoGnFuse): fused_layers = how many of the 16 conv + GroupNorm layers of this plan do so.  The wait is bounded: byte_offset names a
 * 32-bit word of the workspace that a workgroup sets to 1 if its wait ran out (results of that step are then invalid); the host
 * reads it with the step's metrics.  No reference counterpart (aten::native_group_norm is a separate op there). */
int lo_vae_sync_fail_word(const LoVae* h, size_t* byte_offset, int* fused_layers);

/* The nn.Module boundary under torch.amp.GradScaler (train_hybrid.py:246-247, 289-297, 899-923: scaler.scale(loss).backward(),
 * unscale_, clip_grad_norm_, step).  The upstream gradients an autograd node receives are already multiplied by the caller's loss
 * scale; the backward carries fp16 activation gradients and needs them in a fixed range.  lo_grad_scale_pick: max |g| over up to five
 * fp32 tensors (NULL = absent) -> scratch[0] = r = 2^k with max|g| * r in [2, 4), scratch[1] = 1 / r, scratch[2] = max |g|
 * (scratch: >= 260 floats, device memory; no host synchronisation).  All-zero gradients, or an infinite one, give r = 1.  NaN
 * elements do not enter the maximum (it is taken with fmaxf, which returns its other operand): r, 1 / r and scratch[2] are those of
 * the remaining elements -- r = 1 when nothing else is non-zero -- and the NaN itself reaches the parameter gradients through
 * lo_scale_copy_dev, where GradScaler.unscale_ finds it.  lo_scale_copy_dev: dst = src * scale_dev[0].
 * lo_grad_unscale_dev: x *= scale_dev[0] in place; fail_word (may be NULL): the plan's rendezvous-failure word -- when it is set
 * the result is NaN instead, which is how a lost launch reaches a foreign training loop (GradScaler.unscale_ /
 * clip_grad_norm_ see it; there is no optimizer kernel of this library behind the autograd path that could skip the update). */
int lo_grad_scale_pick(const float* g0, size_t n0, const float* g1, size_t n1, const float* g2, size_t n2, const float* g3, size_t n3,
                       const float* g4, size_t n4, float* scratch, void* stream);
int lo_scale_copy_dev(const float* src, float* dst, size_t n, const float* scale_dev, void* stream);
int lo_grad_unscale_dev(float* x, size_t n, const float* scale_dev, const void* fail_word, void* stream);
/* fp8 operand mode (LO_VAE_FP8_FWD, train_hybrid.py --mfma_precision fp8; BASELINE.json configs[4]): how many of the plan's 16
 * forward conv layers actually run on e4m3 operands: those with Cin % 128 == 0 and Cout % 64 == 0, except the 128 -> 64 transposed
 * conv, which stays on its patch-resident fp16 kernel (10 at batch 64; LO_F8_FORCE=0 also leaves the shapes of the fused-tap fp16
 * kernel in fp16: 6).  0 when the mode is off. */
int lo_vae_fp8_layers(const LoVae* h, int* layers);
/* where lo_vae_forward left an intermediate tensor inside the workspace (fp16 NHWC; dims4 = B, H, W, C), for parity tests
 * against the reference's hooked module outputs (lunar_generate.py:94-120, 168-190): which 0 = raw encoder conv output
 * (stage s, k = 0 strided conv, 1 / 2 ResBlock convs), 1 = raw decoder transposed-conv output, 2 = encoder stage (ResBlock)
 * output, 3 = decoder layer activation. */
int lo_vae_debug_tensor(const LoVae* h, int which, int s, int k, size_t* byte_offset, int* dims4);
/* ... and what a forward followed by a backward leaves in the workspace, for tests that check every layer in situ against a plain
 * reference of that layer's own stored operands (tests/test_vae_insitu_gpu.py).  which 0..3 as above, and: 4 = activation
 * (GroupNorm + Mish) of encoder conv (s, k), k = 0 / 1 (the ResBlock tail k = 2 writes the stage output, which = 2); 5 / 6 = saved
 * GroupNorm statistics of encoder conv (s, k) / decoder layer s, FP32 [B][8][2] = (mean, rstd) per group (dims4 = B, 8, 2, 1);
 * 7 / 8 = gradient wrt the raw conv output of encoder conv (s, k) / decoder layer s, multiplied by the backward's loss scale;
 * 9 = the decoder's input h0 (B, 8, 8, 512); 10 = skip gradient s = 0..2 (B, 64 >> s, 64 >> s, 64 << s; loss scale as 7 / 8).
 * elem_bytes: 2 = fp16, 4 = fp32.  (7, 0, 0) names where the LAST backward left the first conv's gradient.
 * With LO_VAE_ATTN (s = k = 0; odd = encoder site, even = decoder site): 11 / 12 = qkv (B, 8, 8, 640); 13 / 14 = the site's input x,
 * 15 / 16 = its output y, 17 / 18 = the gradient dy wrt y, 21 / 22 = the gradient dx wrt x (B, 8, 8, 512); 19 / 20 = dqkv
 * (B, 8, 8, 640); 17 .. 22 carry the loss scale as 7 / 8. */
int lo_vae_debug_tensor_ex(const LoVae* h, int which, int s, int k, size_t* byte_offset, int* dims4, int* elem_bytes);
/* how the plan runs conv + GroupNorm layer (dec != 0: decoder layer s; else encoder conv (s, k)): info4 = { forward conv on e4m3
 * operands (0 / 1; their count is lo_vae_fp8_layers), GroupNorm partial-sum rows per sample the conv epilogue writes, K splits of the
 * forward conv, K splits of the data gradient (0 = one-launch kernel) }. */
int lo_vae_layer_plan(const LoVae* h, int dec, int s, int k, int* info4);
/* ... and every launch of that layer in the fused single-call step (lo_vae_forward; lo_vae_backward with fused = 1), as the executor
 * will make it: each field is the answer of the chooser the executor asks, with the use the executor asks it with, and the executor
 * refuses (-3) a launch whose own choice differs.  Needs no device.  info[0 .. LO_VAE_PLAN_FIELDS), cap >= LO_VAE_PLAN_FIELDS:
 *    0.. 8  forward conv on fp16 operands: kernel (0 none -- the layer's forward runs on e4m3 operands, or it is the first conv, which
 *           has a kernel of its own; 1 lo_igemm_nt, 2 its split-K form, 3 its e4m3 form, 4 lo_conv3x3_pp, 5 / 6 the patch-resident
 *           transposed conv / stride-2 data gradient), bm, bn, bk (lo_igemm_nt tile; lo_conv3x3_pp: bn channels), th, tw (lo_conv3x3_pp
 *           pixel tile), partial-sum rows per sample, n tiles, K splits (0 = one launch)
 *    9..17  the same for the forward conv on e4m3 operands (all 0: the layer takes none)
 *   18..26  the same for the data gradient (all 0: the first conv, whose input gradient the step does not form)
 *   27      that launch also applies the GroupNorm backward of the layer before it in its epilogue (0 / 1)
 *   28..30  GroupNorm backward: form (0 slab sum + one pass, 1 apply only -- the consuming layer's data gradient has reduced, 2 one
 *           pass, 3 reduce + apply; -1: no launch of its own, the consuming layer's data gradient applied it), rows of P1, of P2 per sample
 *   31..38  weight gradient: kernel (0 lo_wgrad3x3_mt, 1 lo_wgrad_s2_mt, 2 lo_wgrad_tn; -1: the first conv's own), chunk width tw,
 *           transposed-conv form, splits launched, slabs provided, K units per split, direct (no slab, no reduce), reduce form
 *           (0 none, 1 rows, 2 transposed conv, 3 scatter)
 *   39      K units of the whole weight gradient: the last split has units - (splits - 1) * units per split of them */
#define LO_VAE_PLAN_FIELDS 40
int lo_vae_layer_plan_ex(const LoVae* h, int dec, int s, int k, int* info, int cap);
/* A handle made in a process without a device plans no launch whose workgroups wait for each other, which every device does plan:
 * this tells such a handle how many compute units to plan for (256: MI355X, SPX), so that lo_vae_layer_plan_ex answers as it would
 * there.  -3 on a handle that was made on a device. */
int lo_vae_plan_assume_cus(LoVae* h, int n_cu);

/* ---- LunarMoETeacher.forward as executed (lunar_evaluator.py:408-462; feature_dim 128) ---------------------------- */
typedef struct LoTeacher LoTeacher;
int lo_teacher_create(int batch, int num_experts, int feature_dim, int embedding_dim, LoTeacher** out);
/* flags: LO_TEACHER_FP8_CONV = the 24 full-resolution 3x3 convolutions take OCP e4m3 operands (v_mfma_scale_f32_16x16x128_f8f6f4;
 * activations e4m3(8 x), one weight scale per output channel), fp16 outputs, fp32 BatchNorm statistics; everything else unchanged
 * (BASELINE config 5).  feature_dim 128: on the dropout path (train mode, dropout_p > 0); the default path and eval mode stay fp16.
 * feature_dim 256 / 512: in every train-mode lo_teacher_forward call (statistics-only and dropout_p == 0 included); eval mode,
 * lo_teacher_forward_keep and the full backward stay fp16. */
#define LO_TEACHER_FP8_CONV 1u
int lo_teacher_create_ex(int batch, int num_experts, int feature_dim, int embedding_dim, unsigned flags, LoTeacher** out);
void lo_teacher_destroy(LoTeacher* h);
/* state table in the reference's state_dict order (351 entries at the defaults); float tensors (parameters, BatchNorm
 * running statistics) live in ONE flat fp32 buffer at these element offsets; offset -1 = integer buffer kept by the host */
int lo_teacher_num_tensors(const LoTeacher* h);
const char* lo_teacher_tensor_name(const LoTeacher* h, int index);
size_t lo_teacher_tensor_numel(const LoTeacher* h, int index);
long long lo_teacher_tensor_offset(const LoTeacher* h, int index);
size_t lo_teacher_flat_elems(const LoTeacher* h);
size_t lo_teacher_workspace_bytes(const LoTeacher* h);
int lo_teacher_pack(LoTeacher* h, const float* flat_state, void* ws, void* stream);
/* training != 0: BatchNorm uses batch statistics and updates running_mean / running_var inside flat_state  Passing NULL for all five output
 * pointers makes it a statistics-only call (BatchNorm running statistics updated, pooling of the last block and heads
 * skipped): the first teacher call of _process_batch, train_hybrid.py:853-855, whose outputs are dead in the reference. */
/* dropout_p, drop_seed: the reference's six dropout sites (nn.Dropout after the branch concat lunar_evaluator.py:97-99,108;
 * attn_drop / proj_drop :139-140,212,225; nn.Dropout2d after both ExpertBlock convs :246,253; nn.Dropout in the gate and
 * every head :353-397) with torch semantics (elementwise / per (sample, channel), kept values scaled by 1/(1-p)), active
 * only when training != 0 and dropout_p > 0.  The masks come from a counter RNG keyed by (drop_seed, site, element): pass a
 * fresh drop_seed per call.  With dropout the constant-field shortcuts of the default path do not hold (proj_drop makes the
 * conv2 input a random field) and every 3x3 convolution runs in full; lo_teacher_last_path reports which path the last call
 * took: 0 sparse shortcuts, 1 dense (LO_T_DENSE=1), 2 dropout. */
int lo_teacher_forward(LoTeacher* h, const float* x, float* flat_state, void* ws, int training, float dropout_p,
                       uint64_t drop_seed, float* quality_scores, float* expert_weights, float* style_embedding,
                       float* prompt_embedding, float* semantic_score, void* stream);
int lo_teacher_last_path(const LoTeacher* h);
/* keep[i] (1 / 0) of element i < n of dropout site `site` for call seed drop_seed: the decisions lo_teacher_forward applies
 * (nn.Dropout semantics: lunar_evaluator.py:99,139-140; site numbering in csrc/lo_common.h, oracle/dropout_ref.py). */
int lo_dropout_mask(uint64_t drop_seed, int site, float dropout_p, size_t n, uint8_t* keep, void* stream);

/* gradients of teacher_loss = -(quality_weight/accum) * mean(quality_scores) for the parameters that receive gradients in
 * the reference step (gate.*, quality_heads.*; train_hybrid.py:891-904 with the reentrant-checkpoint quirk):
 * one contiguous range [begin,end) of the flat state layout.  rows: B*(end-begin) floats of scratch.  Replays the dropout
 * masks of the gate / quality-head hidden layers of the lo_teacher_forward call it follows. */
int lo_teacher_grad_range(const LoTeacher* h, size_t* begin_elem, size_t* end_elem);
int lo_teacher_heads_backward(LoTeacher* h, const float* flat_state, void* ws, const float* expert_weights, float coef,
                              float* rows, float* flat_grads, void* stream);
/* The same backward for arbitrary upstream gradients, i.e. what autograd needs to make quality_scores / expert_weights
 * differentiable outputs of LunarMoETeacher.forward (the reference calls teacher_loss.backward() on them,
 * train_hybrid.py:891-904; lunar_evaluator.py:417,431-432,455-462): d_quality [B][4] / d_weights [B][E] (either may be NULL =
 * zero).  The head inputs of the forward being differentiated are passed explicitly — lo_teacher_heads_saved says where
 * lo_teacher_forward left them inside the workspace (byte offsets and element counts of pooled extractor features [B][128],
 * pooled expert features [E][B][F], pre-weighting quality logits [B][E][4]), so a caller may copy them and run this backward
 * after later forward calls — together with that call's dropout_p (0 in eval mode) and drop_seed. */
int lo_teacher_heads_saved(const LoTeacher* h, size_t* byte_offsets3, size_t* elems3);
/* Where a teacher forward leaves an intermediate tensor, for tests that check every layer in situ against a plain reference of that
 * layer's own stored operands (tests/test_teacher_insitu_gpu.py).  Launches nothing, changes nothing.  dims4: NHWC of an fp16 tensor
 * (the compact attention rows [B][1024][F] as B, 8, 128, F: they are image rows 0..7), or 1, 1, C, 2 of an fp32 per-channel table;
 * elem_bytes 2 = fp16, 4 = fp32.  An unknown kind, or e / l outside what the kind takes, is an error (lo_last_error says which).
 * space 1 = bws of lo_teacher_forward_keep / _keep_eval (feature extractor kinds take e = l = 0 unless said otherwise):
 *    0 raw32 = lrelu(conv 3->32)        1 dw[l], l = 0..2: depthwise 3x3, 5x5, 3x3    2 cat: the three pointwise convs, raw, 64 channels each
 *    3 catd = Dropout(BN(cat))          4 rawF = lrelu(fusion conv)                   5 feat = BN(rawF)
 *    6 xs[e][l]: output of ExpertBlock (e, l)
 *    per block (e, l) -- an error under the shared-set plan (LO_T_BWD_SHARED=1), which holds one block at a time:
 *    7 rawA = lrelu(conv1)    8 bnA = Dropout2d(BN(rawA))    9 qkv (3F channels)    10 attc: compact attention rows (rows >= 543 zero)
 *   11 projc = proj(attc)    12 a2 = proj_drop, full resolution    13 rawB = lrelu(conv2)    14 scraw: shortcut conv (feature_dim != 128, l = 0)
 *   15 mrA, 16 mrB: (mean, rstd) of BatchNorm1 / 2    17 mrS, 18 ssS: (mean, rstd) and (scale, shift) of the shortcut BatchNorm (as 14)
 *   19 the feature extractor's (mean, rstd) tables, l = 3 conv1 (32 channels), 4..6 branches (64), 7 fusion (128)
 *   20 conv1's (scale, shift), which the depthwise convs read
 * space 0 = ws of lo_teacher_forward, e = l = 0; the block tensors are those of the LAST block the call ran:
 *    0 o_raw32    1 o_cat    2 o_feat    3 o_x0, 4 o_x1: block outputs, ping-pong    5 o_rawA    6 o_projc (compact)    7 o_proj = proj_drop
 *    8 o_rawB     9 o_ss: (scale, shift) of the last BatchNorm finalize    10 o_ssb: the per-sample Dropout2d table [B][F][2]
 *   11 o_ss_cat: (scale, shift) of the 192 concatenated channels    12 o_wfus_fold fp16 [128][192], 13 o_bfus_fold fp32 [128]: the fusion
 *      conv with the branch BatchNorms folded in (dropout-free calls)
 * The pooled features and pre-weighting logits are where lo_teacher_heads_saved says. */
int lo_teacher_debug_tensor(const LoTeacher* h, int space, int which, int e, int l, size_t* byte_offset, int* dims4, int* elem_bytes);
int lo_teacher_heads_backward_ex(LoTeacher* h, const float* flat_state, const float* pooled_f, const float* pooled_e,
                                 const float* raw_q, const float* expert_weights, const float* d_quality, const float* d_weights,
                                 float dropout_p, uint64_t drop_seed, float* rows, float* flat_grads, void* stream);
/* SURVEY §8 row F2, second half: the teacher trained "as documented" -- gradients for EVERY parameter on the path of the teacher
 * loss, experts and feature extractor included, i.e. what teacher_loss.backward() (train_hybrid.py:891-904) produces when the three
 * torch.utils.checkpoint.checkpoint calls of the model (lunar_evaluator.py:194-197, 266-275, 411-414) are non-reentrant.  Like the
 * reference under checkpointing, the trunk is recomputed block by block (BatchNorm with the batch statistics, running statistics
 * untouched) and then differentiated: 24 3x3 convs + BatchNorm(train) + Dropout2d, the chunk attention as executed (543 live rows,
 * attn_drop / proj_drop replayed from the call's seed), layer_scale, the shortcut conv of feature_dim != 128, the feature extractor's
 * depthwise / pointwise branches.  Must follow lo_teacher_forward(training = 1) on the same images (the heads' inputs and the
 * dropout stream of that call are used); coef = quality_weight / accum; gscale = power of two applied to the fp16 activation
 * gradients (parameter gradients come out unscaled; 64 * B * 16384 is a good value); bws = lo_teacher_full_backward_bytes(h) bytes
 * of scratch; rows as for lo_teacher_heads_backward; flat_grads = the whole state-table layout (lo_teacher_flat_elems floats):
 * every parameter on the loss path is written, everything else (the three heads the loss does not read, the softmax-invariant
 * relative-position tables, BatchNorm buffers) is zero.  After a plain lo_teacher_forward the trunk is recomputed first (one extra
 * forward: the reference's own cost under checkpointing); after lo_teacher_forward_keep on the same bws nothing is. */
size_t lo_teacher_full_backward_bytes(const LoTeacher* h);
/* LunarMoETeacher.forward in train mode (outputs and side effects of lo_teacher_forward(training = 1)) in plain form, with every tensor
 * the backward reads -- feature extractor and all 12 ExpertBlocks -- left inside bws: the forward to use in a step that ends in
 * lo_teacher_full_backward(..., the same bws), which then recomputes nothing (26 GB of kept tensors at batch 64 / feature_dim 128; above
 * 160 GB the plan keeps the block outputs only and the backward recomputes one block at a time). */
int lo_teacher_forward_keep(LoTeacher* h, const float* images_nchw, float* flat_state, void* ws, void* bws, float dropout_p,
                            uint64_t drop_seed, float* quality_scores, float* expert_weights, float* style_embedding,
                            float* prompt_embedding, float* semantic_score, void* stream);
int lo_teacher_full_backward(LoTeacher* h, const float* images_nchw, float* flat_state, void* ws, void* bws, const float* expert_weights,
                             float coef, float gscale, float* rows, float* flat_grads, void* stream);
/* The same backward for arbitrary upstream gradients d_quality [B][4] / d_weights [B][E] (either may be NULL) with the head inputs
 * (lo_teacher_heads_saved), dropout_p and call seed of the forward being differentiated passed explicitly: what the module's autograd
 * node calls (LunarMoETeacher(full_backward=True), so that teacher_loss.backward() of a foreign training loop fills every .grad).
 * Upstream gradients should be of order 1: a foreign loss scale is divided out first (lo_grad_scale_pick / lo_scale_copy_dev). */
int lo_teacher_full_backward_ex(LoTeacher* h, const float* images_nchw, float* flat_state, void* ws, void* bws, const float* pooled_f,
                                const float* pooled_e, const float* raw_q, const float* expert_weights, const float* d_quality,
                                const float* d_weights, float dropout_p, uint64_t drop_seed, float gscale, float* rows, float* flat_grads,
                                void* stream);
/* the same, and the gradient wrt the images: dx fp32 NCHW [B,3,128,128] (NULL = not wanted; lo_teacher_full_backward_ex is this with NULL).
 * The autograd node of a train-mode LunarMoETeacher whose input requires grad calls it. */
int lo_teacher_full_backward_dx(LoTeacher* h, const float* images_nchw, float* flat_state, void* ws, void* bws, const float* pooled_f,
                                const float* pooled_e, const float* raw_q, const float* expert_weights, const float* d_quality,
                                const float* d_weights, float dropout_p, uint64_t drop_seed, float gscale, float* rows, float* flat_grads,
                                float* dx, void* stream);
/* LunarMoETeacher.forward in eval mode (lunar_evaluator.py:408-462 under module.eval(): every BatchNorm2d with its running statistics,
 * lunar_evaluator.py:61-89, 240-257; every Dropout / Dropout2d the identity), plain form, every tensor the backward reads left in bws
 * (lo_teacher_full_backward_bytes): the forward of the eval-mode teacher used as a differentiable reward.  Not one byte of flat_state
 * changes; the pooled features and pre-weighting logits are where lo_teacher_heads_saved says; lo_teacher_last_path reports 1.  The
 * outputs differ from lo_teacher_forward(training = 0) (folded form at feature_dim 128) at the fp16 rounding level. */
int lo_teacher_forward_keep_eval(LoTeacher* h, const float* images_nchw, const float* flat_state, void* ws, void* bws,
                                 float* quality_scores, float* expert_weights, float* style_embedding,
                                 float* prompt_embedding, float* semantic_score, void* stream);
/* Its backward for upstream gradients d_quality [B][4] / d_weights [B][E] (either may be NULL): the chain of
 * lo_teacher_full_backward_dx with frozen BatchNorm -- y = (r - running_mean) rstd gamma + beta has dr = gamma rstd ls g, no batch
 * statistic term couples the samples -- and no dropout.  Parameter gradients keep their form (dbeta = ls sum g, dgamma = ls sum g xhat,
 * dls = gamma S2 + beta S1); running statistics get none.  flat_grads NULL: parameter gradients are not computed at all (no
 * weight-gradient GEMM, no column sums, no BatchNorm reduce; one streaming pass per BatchNorm) -- the frozen-reward case; dx has the
 * same bits with and without flat_grads.  dx NULL: frozen-BatchNorm fine-tuning.  After lo_teacher_forward_keep_eval on the same bws
 * nothing is recomputed; after anything else (a train-mode kept forward included) the trunk is recomputed in eval mode from
 * images_nchw.  gscale as for lo_teacher_full_backward (eval-mode gradients are smaller than train-mode ones). */
int lo_teacher_eval_backward(LoTeacher* h, const float* images_nchw, const float* flat_state, void* ws, void* bws,
                             const float* pooled_f, const float* pooled_e, const float* raw_q, const float* expert_weights,
                             const float* d_quality, const float* d_weights, float gscale, float* rows,
                             float* flat_grads /* NULL: parameter gradients not wanted */,
                             float* dx /* fp32 NCHW [B,3,128,128]; NULL: not wanted */, void* stream);
/* lo_teacher_eval_backward with flat_grads = NULL whose last kernel (the image data gradient of conv1) stores the SEEDED form
 *   dx = scale_factor * (d / d images) + seed_coef[0] * (images - target)
 * seed_coef: one float on the device (lo_vae_reward_term writes it), target: fp32 NCHW [B,3,128,128].  The hybrid step's reward-gradient
 * objective: the teacher's input IS the VAE's reconstruction, so dx is the complete d vae_loss / d recon (reward term + MSE term) with no
 * add pass.  scale_factor multiplies the fp32 result, not the fp16 activation gradients: pass upstream rows of order 1 (the step passes
 * constant rows of -2) and fold the objective's small coefficient in here.  seed_coef[0] == 0 and scale_factor == 1: the bits of
 * lo_teacher_eval_backward. */
int lo_teacher_eval_backward_seed(LoTeacher* h, const float* images_nchw, const float* flat_state, void* ws, void* bws,
                                  const float* pooled_f, const float* pooled_e, const float* raw_q, const float* expert_weights,
                                  const float* d_quality, const float* d_weights, float gscale, float* rows, const float* target,
                                  const float* seed_coef, float scale_factor, float* dx, void* stream);
/* clip_grad_norm_(teacher.parameters()) + AdamW (train_hybrid.py:914, 922) with every teacher parameter live: the norm over the whole
 * flat gradient of lo_teacher_full_backward, the update over exactly the tensors that have a .grad in the reference (not the
 * BatchNorm buffers, not the style / prompt / semantic heads, whose .grad is None there).  m, v: lo_teacher_flat_elems floats each,
 * scratch: 1028 floats ([1024..1027] = norm, clip coefficient, finite flag, skipped count as for lo_clip_adamw_step).  The fp16 operand
 * copies are stale afterwards: lo_teacher_pack before the next forward. */
int lo_teacher_clip_adamw_full(LoTeacher* h, float* flat_state, const float* flat_grads, float* m, float* v, float max_norm, float lr,
                               float beta1, float beta2, float eps, float weight_decay, int step, float* scratch, void* stream);
int lo_teacher_full_param_count(const LoTeacher* h, size_t* tensors, size_t* elems);
/* reward / baseline / advantage bookkeeping of _process_batch (train_hybrid.py:870-892) on the device; state2 =
 * {baseline, initialised}; out7 = quality_loss, semantic_reward, quality_reward, baseline, advantage, teacher_loss,
 * mean(quality_scores); adv_dev = mean advantage (input of lo_vae_loss). */
int lo_hybrid_reward(const float* quality_scores, const float* semantic_score, int B, float semantic_weight,
                     float reward_scale, float momentum, float quality_weight, float accum, float* state2, float* out7,
                     float* adv_dev, void* stream);

/* The same backward in two calls, for data-parallel overlap: phase 1 = final conv, decoder, decoder.fc, latent, encoder
 * heads (afterwards the gradients of the three Linear layers — 82 % of the bytes, one contiguous range of the flat
 * buffer, see lo_vae_linear_grad_range — are final and can be all-reduced while phase 2 runs); phase 2 = encoder. */
int lo_vae_backward_phase(LoVae* h, int phase, const float* x, const float* flat_params, void* ws, const float* recon,
                          const float* target, int fused, const float* drecon, const float* gmu, const float* glv,
                          float loss_scale, float* flat_grads, void* stream);
int lo_vae_linear_grad_range(const LoVae* h, size_t* begin_elem, size_t* end_elem);
/* [begin, end) of the flat gradient buffer that is complete after lo_vae_backward_phase(.., phase = 1): fc_mu.weight up to
 * the end of the buffer (Linear layers, decoder convs, final conv).  The rest (encoder convs) is complete after phase 2. */
int lo_vae_phase1_grad_range(const LoVae* h, size_t* begin_elem, size_t* end_elem);
/* Three-call form for the data-parallel exchange: phase 1, then phase 3 (encoder stage 4 = down4, 94 % of the encoder's
 * gradient bytes; its range below is complete afterwards), then phase 4 (stages 3..1; [0, stage-4 begin) complete).  Phase 2
 * = 3 + 4 in one call. */
int lo_vae_stage4_grad_range(const LoVae* h, size_t* begin_elem, size_t* end_elem);

/* ---- data-parallel gradient exchange helpers (lunaris_orion_amd/parallel.py; the reference has no distributed code) ---------
 * One streaming pass each around the RCCL calls of the direct (all-to-all reduce-scatter + all-gather) exchange:
 * wire[i] = fp16(g[i] * scale);  share[i] = mean over the `world` received chunks recv[r * chunk + i] (fp32 accumulation, ranks in
 * order; fp16 or fp32 elements);  g[i] = float(wire[i]) * inv_scale. */
int lo_dp_pack_f16(const float* g, void* wire, size_t n, float scale, void* stream);
int lo_dp_unpack_f16(const void* wire, float* g, size_t n, float inv_scale, void* stream);
/* ... and, in the same pass, the sum of squares of the unpacked range into scratch[512..1024) (lo_gradnorm_early_range's result) */
int lo_dp_unpack_f16_sumsq(const void* wire, float* g, size_t n, float inv_scale, float* scratch, void* stream);
int lo_dp_sum_shares(const void* recv, void* share, int world, size_t chunk, int is_f16, void* stream);

/* ---- held-out validation (lunaris_orion_amd/evaluate.py) ---------------------------------------------------------------------
 * The reference sets a tenth of the dataset aside (train_hybrid.py:552-573 builds a val_loader) and names the early-stopping
 * argument validation_loss (:216), then feeds it the training loss (:1049) and never reads the loader.  These three entries are what
 * a pass over those sprites needs on the device, so that a whole pass ends in ONE device-to-host copy.  All three sum in a fixed
 * order without atomics: the same inputs give the same bits.  Samples b >= n_valid are padding (the short last batch of a pass,
 * filled up to the engine's batch size): their output rows are written as 0 and their inputs are NOT READ -- NaN there is invisible.
 *
 * lo_eval_image_metrics: recon, target fp32 NCHW [B][3][128][128] in [-1, 1] (what lo_vae_forward writes and reads) ->
 *   per_sample [B][2] = (sum over the sample's 49 152 elements of (recon - target)^2 -- the per-sample numerator of F.mse_loss,
 *   train_hybrid.py:859 --, mean SSIM).  SSIM as Wang et al. 2004: 11 x 11 Gaussian window, sigma 1.5 (weights in double on the host,
 *   normalised to sum 1), "valid" window positions only (a 118 x 118 map per channel), C1 = (0.01 * 2)^2, C2 = (0.03 * 2)^2 (data
 *   range 2), variances as E[x^2] - mu^2, mean over the map and the three channels.  fp32 throughout, separable filter out of LDS,
 *   one workgroup per sample.  An identical pair gives exactly (0, 1).
 * lo_eval_latent_kl: mu, logvar [B][L] (L a multiple of 64) -> per_sample_kl [B] = -0.5 * mean_l(1 + logvar - mu^2 - exp(logvar)),
 *   the per-sample form of train_hybrid.py:661-662; its mean over b is the batch's kl_loss.
 * lo_eval_accumulate: adds one batch to acc, 8 doubles on the device: [0] samples counted, [1..5] sums of the per-sample MSE
 *   (per_sample_img[b][0] / 49 152), KL, PSNR = 10 log10(4 / max(MSE, 1e-12)), SSIM and mean quality score (quality: NULL, or the
 *   teacher's quality_scores [B][4], lunar_evaluator.py:431-432; NULL leaves [5] alone), [6] / [7] the smallest / largest PSNR.  A
 *   call that finds acc[0] == 0 starts a pass (the caller zeroes acc once).  One workgroup. */
int lo_eval_image_metrics(const float* recon, const float* target, int B, int n_valid, float* per_sample, void* stream);
int lo_eval_latent_kl(const float* mu, const float* logvar, int B, int L, int n_valid, float* per_sample_kl, void* stream);
int lo_eval_accumulate(const float* per_sample_img, const float* per_sample_kl, const float* quality, int n_valid, double* acc,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif
