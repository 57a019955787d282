// feature_dim 128: the three forms an ExpertBlock takes inside lo_teacher_forward, and the kernels only they use.
//   sparse   (default) folded attention, proj and conv2 on the 8 image rows per sample that are not a constant field; with the fused
//            tail the full-resolution block output is never written
//   dense    (LO_T_DENSE=1) every convolution in full, the chunk-local attention with the reference's write-offset quirk
//   dropout  (train mode, dropout_p > 0) both 3x3 convs in full (optionally e4m3), the attention still folded
#include "lo_teacher.h"
#include "lo_conv.h"

// ---------------------------------------------------------------------------------------------
// chunk-local attention with the reference's offset quirk (lunar_evaluator.py:203-216): one wave per written position.
//   position p <  512 : query = token 32p        (row 0 of chunk p),      keys/values = chunk p
//   position p >= 512 : query = token 32*511+r,  r = p - 511 (rows 1..31), keys/values = chunk 511
// qkv: [B][16384][384] fp16, channel = t*128 + head*16 + d.  att: [B][16384][128] fp16 (positions >= 543 stay zero).
// lane = (head = lane>>3, part = lane&7: keys 4*part..4*part+3)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lo_t_attn_kernel(const f16* __restrict__ qkv, f16* __restrict__ att, int B) {
  const int wave_g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int per_b = 512 + 31;
  if (wave_g >= B * per_b) return;
  const int b = wave_g / per_b, p = wave_g - b * per_b;
  const int chunk = p < 512 ? p : 511;
  const int qtok = p < 512 ? 32 * p : 32 * 511 + (p - 511);
  const int head = lane >> 3, part = lane & 7;
  const f16* base = qkv + (size_t)b * T_HW * 384;
  f16x8 q0 = *reinterpret_cast<const f16x8*>(base + (size_t)qtok * 384 + head * 16);
  f16x8 q1 = *reinterpret_cast<const f16x8*>(base + (size_t)qtok * 384 + head * 16 + 8);
  float sc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const f16* kp = base + (size_t)(32 * chunk + part * 4 + k) * 384 + 128 + head * 16;
    f16x8 k0 = *reinterpret_cast<const f16x8*>(kp), k1 = *reinterpret_cast<const f16x8*>(kp + 8);
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < 8; ++d) s += (float)q0[d] * (float)k0[d] + (float)q1[d] * (float)k1[d];
    sc[k] = s * 0.25f;   // head_dim ** -0.5 = 16 ** -0.5; the relative-position term is constant along keys: no effect
  }
  float m = fmaxf(fmaxf(sc[0], sc[1]), fmaxf(sc[2], sc[3]));
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  float e[4], l = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) { e[k] = __expf(sc[k] - m); l += e[k]; }
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) l += __shfl_xor(l, o, 64);
  float acc[16];
#pragma unroll
  for (int d = 0; d < 16; ++d) acc[d] = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const f16* vp = base + (size_t)(32 * chunk + part * 4 + k) * 384 + 256 + head * 16;
    f16x8 v0 = *reinterpret_cast<const f16x8*>(vp), v1 = *reinterpret_cast<const f16x8*>(vp + 8);
    float pw = e[k] / l;
#pragma unroll
    for (int d = 0; d < 8; ++d) { acc[d] += pw * (float)v0[d]; acc[8 + d] += pw * (float)v1[d]; }
  }
#pragma unroll
  for (int d = 0; d < 16; ++d)
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) acc[d] += __shfl_xor(acc[d], o, 64);
  if (part == 0) {
    f16x8 o0, o1;
#pragma unroll
    for (int d = 0; d < 8; ++d) { o0[d] = (f16)acc[d]; o1[d] = (f16)acc[8 + d]; }
    f16* dst = att + ((size_t)b * T_HW + p) * 128 + head * 16;
    *reinterpret_cast<f16x8*>(dst) = o0;
    *reinterpret_cast<f16x8*>(dst + 8) = o1;
  }
}

// ---------------------------------------------------------------------------------------------
// Sparse expert path.  The attention output is zero outside positions 0..542 (image rows 0..4), so proj(att) equals
// fp16(proj.bias) there and conv2 of that constant field is one of six vectors, depending only on which taps fall into
// the zero padding.  cvec[k][co] = fp16(lrelu(fp16(bias2[co] + sum_{valid taps} sum_ci Wp[co][tap][ci] * fp16(pb[ci])))),
// exactly the value the dense igemm epilogue stores.  k: 0 interior, 1 left column, 2 right column, 3 bottom row,
// 4 bottom-left, 5 bottom-right.  grid = 6, block = 128 (one output channel per thread).  Weights only: runs at pack time.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void lo_t_cvec_kernel(const f16* __restrict__ wp, const float* __restrict__ bias2,
                                                        const float* __restrict__ proj_bias, float* __restrict__ cvec) {
  __shared__ float pb[128];
  const int k = blockIdx.x, co = threadIdx.x;
  pb[co] = (float)(f16)proj_bias[co];
  __syncthreads();
  const bool left = (k == 1 || k == 4), right = (k == 2 || k == 5), bottom = k >= 3;
  float acc = 0.f;
  for (int t = 0; t < 9; ++t) {
    const int r = t / 3, sx = t % 3;
    if ((left && sx == 0) || (right && sx == 2) || (bottom && r == 2)) continue;
    const f16* w = wp + ((size_t)co * 9 + t) * 128;
    float a = 0.f;
    for (int ci = 0; ci < 128; ci += 8) {
      f16x8 h = *reinterpret_cast<const f16x8*>(w + ci);
#pragma unroll
      for (int j = 0; j < 8; ++j) a += (float)h[j] * pb[ci + j];
    }
    acc += a;
  }
  float v = (float)(f16)(acc + bias2[co]);
  v = v > 0.f ? v : 0.2f * v;
  cvec[k * 128 + co] = (float)(f16)v;
}

// ---- folded attention ------------------------------------------------------------------------------------------
// With x = BN(conv1 output) (fp16), q = Wq x_q + bq, k_j = Wk x_j + bk, v_j = Wv x_j + bv and a softmax over the 32 keys
// of one chunk, the q.bk term is constant along the keys and drops out, so per head h
//     score_j = (0.25 Wk_h^T (Wq_h x_q + bq_h)) . x_j  =: u_h . x_j          (0.25 = head_dim^-0.5)
//     proj(att)  = sum_h (Wp[:,h] Wv_h) (sum_j p_hj x_j) + Wp bv + bp       (sum_j p_hj = 1)
// i.e. k and v are never materialised: U = Xq WU^T + ub (one GEMM over the 543 query rows per sample, WU = the 8
// stacked 128x128 matrices 0.25 Wk_h^T Wq_h), the kernel below turns (U row, 32 x rows) into z_h = sum_j p_hj x_j, and
// proj = [z_1..z_8, 1] WZ^T + bp (one GEMM, K = 1024 + 64).  Weight-only products WU / ub / WZ are built at pack time.

// WU[(h,c)][c'] = 0.25 sum_d Wk[h16+d][c] Wq[h16+d][c'];  ub[(h,c)] = 0.25 sum_d Wk[h16+d][c] bq[h16+d].  grid 1024, block 128
__global__ __launch_bounds__(128) void lo_t_fold_qk_kernel(const float* __restrict__ wqkv, const float* __restrict__ bqkv,
                                                           f16* __restrict__ wu, float* __restrict__ ub) {
  const int r = blockIdx.x, h = r >> 7, c = r & 127, cp = threadIdx.x;
  float acc = 0.f, accb = 0.f;
#pragma unroll
  for (int d = 0; d < 16; ++d) {
    float wk = wqkv[(size_t)(128 + h * 16 + d) * 128 + c];
    acc += wk * wqkv[(size_t)(h * 16 + d) * 128 + cp];
    accb += wk * bqkv[h * 16 + d];
  }
  wu[(size_t)r * 128 + cp] = (f16)(0.25f * acc);
  if (cp == 0) ub[r] = 0.25f * accb;
}
// WZ[o][(h,c)] = sum_d Wp[o][h16+d] Wv[h16+d][c];  WZ[o][1024] = sum_hd Wp[o][hd] bv[hd];  WZ[o][1025 + h] = sum_d Wp[o][h16+d]
// bv[h16+d] (the same term per head: with attn_drop the probabilities of head h sum to s_h != 1 and the Z row carries s_h in
// column 1025 + h and 0 in column 1024);  WZ[o][1033..1087] = 0.  grid 128, block 256
__global__ __launch_bounds__(256) void lo_t_fold_pv_kernel(const float* __restrict__ wqkv, const float* __restrict__ bqkv,
                                                           const float* __restrict__ wp, f16* __restrict__ wz) {
  const int o = blockIdx.x;
  for (int col = threadIdx.x; col < 1088; col += 256) {
    float acc = 0.f;
    if (col < 1024) {
      const int h = col >> 7, c = col & 127;
#pragma unroll
      for (int d = 0; d < 16; ++d) acc += wp[o * 128 + h * 16 + d] * wqkv[(size_t)(256 + h * 16 + d) * 128 + c];
    } else if (col == 1024) {
      for (int k = 0; k < 128; ++k) acc += wp[o * 128 + k] * bqkv[256 + k];
    } else if (col < 1033) {
      const int h = col - 1025;
#pragma unroll
      for (int d = 0; d < 16; ++d) acc += wp[o * 128 + h * 16 + d] * bqkv[256 + h * 16 + d];
    }
    wz[(size_t)o * 1088 + col] = (f16)acc;
  }
}

// query rows: qin[b*543 + p][128] = fp16(BN(raw[b][qtok(p)]))  (16-byte chunks; thread = (row, chunk))
__global__ __launch_bounds__(256) void lo_t_gather_q_kernel(const f16* __restrict__ raw, const float* __restrict__ ss,
                                                            f16* __restrict__ qin, int B, int ss_stride) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  const int chunk = gid & 15, row = gid >> 4;
  if (row >= B * 543) return;
  const int b = row / 543, p = row - b * 543;
  const int qtok = p < 512 ? 32 * p : 32 * 511 + (p - 511);
  f16x8 v = *reinterpret_cast<const f16x8*>(raw + ((size_t)b * T_HW + qtok) * 128 + chunk * 8), o;
  ss += (size_t)b * ss_stride;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (f16)((float)v[j] * ss[(chunk * 8 + j) * 2] + ss[(chunk * 8 + j) * 2 + 1]);
  *reinterpret_cast<f16x8*>(qin + (size_t)row * 128 + chunk * 8) = o;
}

// byte offset of 16-byte chunk ch (0..15) of row `row` in a [rows][128 x fp16] LDS image that serves row reads
// (ds_read_b128) and transposed reads (ds_read_b64_tr_b16) alike
__device__ __forceinline__ int t_off(int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }

// one wave per written position p of sample b (chunk = min(p, 511)): x = BN(raw rows of the chunk) -> LDS (fp16),
// S^T[key][head] = X U^T on MFMA (the key order of the M index is chosen so that the accumulators ARE the A operand of
// the second product), softmax over the 32 keys (8 in-lane values x 4 lane groups), Z[head][c] = P X on MFMA with X
// fragments by transposed LDS reads; Z row (8 x 128 fp16 + the constant-one column 1024) -> Z[b*1024 + p][1088].
// DROP: x = Dropout2d(BN(raw)) through the per-sample (scale, shift) table (ss_stride = 256), attn_drop on the probabilities
// (element index ((b*543 + p)*8 + head)*32 + key of site `ds`), the per-head sums s_h of the dropped probabilities in
// columns 1025.. of the Z row (see lo_t_fold_pv_kernel).
template <bool DROP>
__global__ __launch_bounds__(256) void lo_t_attn_folded_kernel(const f16* __restrict__ raw, const float* __restrict__ ss,
                                                               const f16* __restrict__ U, f16* __restrict__ Z, int B, int ss_stride,
                                                               LoDropSite ds, uint32_t thr, float inv_keep) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[4][12288];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wave_g = blockIdx.x * 4 + wave;
  if (wave_g >= B * 543) return;                        // wave-uniform: EXEC stays all ones for the transposed reads
  const int b = wave_g / 543, p = wave_g - b * 543;
  const int chunk = p < 512 ? p : 511;
  unsigned char* sx = smem[wave];
  unsigned char* su = sx + 8192;
  unsigned char* sz = su + 2048;
  {
    const int c0 = (lane & 15) * 8;
    float sc[8], sh[8];
    ss += (size_t)b * ss_stride;
#pragma unroll
    for (int j = 0; j < 8; ++j) { sc[j] = ss[(c0 + j) * 2]; sh[j] = ss[(c0 + j) * 2 + 1]; }
    const f16* src = raw + ((size_t)b * T_HW + 32 * chunk) * 128;
    f16x8 v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = *reinterpret_cast<const f16x8*>(src + (size_t)(i * 64 + lane) * 8);
    const f16* usrc = U + (size_t)(b * 543 + p) * 1024;
    f16x8 u0 = *reinterpret_cast<const f16x8*>(usrc + lane * 8), u1 = *reinterpret_cast<const f16x8*>(usrc + (64 + lane) * 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      f16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (f16)((float)v[i][j] * sc[j] + sh[j]);
      *reinterpret_cast<f16x8*>(sx + t_off(i * 4 + (lane >> 4), lane & 15)) = o;
    }
    *reinterpret_cast<f16x8*>(su + t_off(lane >> 4, lane & 15)) = u0;
    *reinterpret_cast<f16x8*>(su + t_off(4 + (lane >> 4), lane & 15)) = u1;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const int m = lane & 15, g = lane >> 4;
  // M index m = 4q + i  <->  key 8(q&1) + 4(q>>1) + i (+16 for the second tile): lane group g then owns keys
  // r0..r0+3 and 16+r0..16+r0+3, r0 = 8(g&1) + 4(g>>1), which makes the transposed reads below conflict-free
  const int keyrow = 8 * ((m >> 2) & 1) + 4 * (m >> 3) + (m & 3);
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const int ch = 4 * ks + g;
    f16x8 bu = *reinterpret_cast<const f16x8*>(su + t_off(m & 7, ch));
    if (m >= 8) bu = (f16x8){0, 0, 0, 0, 0, 0, 0, 0};
    f16x8 a0 = *reinterpret_cast<const f16x8*>(sx + t_off(keyrow, ch));
    f16x8 a1 = *reinterpret_cast<const f16x8*>(sx + t_off(16 + keyrow, ch));
    s0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, bu, s0, 0, 0, 0);
    s1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, bu, s1, 0, 0, 0);
  }
  // softmax over the 32 keys of head m: 8 values here, the rest in lanes m+16, m+32, m+48
  float mx = fmaxf(fmaxf(fmaxf(s0[0], s0[1]), fmaxf(s0[2], s0[3])), fmaxf(fmaxf(s1[0], s1[1]), fmaxf(s1[2], s1[3])));
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  float e[8], l = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) { e[r] = __expf(s0[r] - mx); e[4 + r] = __expf(s1[r] - mx); }
#pragma unroll
  for (int r = 0; r < 8; ++r) l += e[r];
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  const float inv = 1.0f / l;
  f16x8 pf;
  const int r0 = 8 * (g & 1) + 4 * (g >> 1), tq = m >> 2, tp = m & 3;
  float hsum = 0.f;
  if (DROP) {
    // this lane's keys: r0 .. r0+3 (e[0..3]) and 16+r0 .. 16+r0+3 (e[4..7]) of head m (lanes with m >= 8 hold padding)
    const uint32_t base = ((uint32_t)(b * 543 + p) * 8u + (uint32_t)(m & 7)) * 32u;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const uint32_t i0 = base + hf * 16 + r0;
      const uint32_t w0 = lo_drop_word(ds, i0 >> 1), w1 = lo_drop_word(ds, (i0 >> 1) + 1);
      const bool k0 = (w0 & 0xFFFFu) >= thr, k1 = (w0 >> 16) >= thr, k2 = (w1 & 0xFFFFu) >= thr, k3 = (w1 >> 16) >= thr;
      e[hf * 4 + 0] = k0 ? e[hf * 4 + 0] * inv_keep : 0.f;
      e[hf * 4 + 1] = k1 ? e[hf * 4 + 1] * inv_keep : 0.f;
      e[hf * 4 + 2] = k2 ? e[hf * 4 + 2] * inv_keep : 0.f;
      e[hf * 4 + 3] = k3 ? e[hf * 4 + 3] * inv_keep : 0.f;
    }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) { pf[r] = (f16)(e[r] * inv); if (DROP) hsum += (float)pf[r]; }
  if (DROP) {
    hsum += __shfl_xor(hsum, 16, 64);
    hsum += __shfl_xor(hsum, 32, 64);
  }
#pragma unroll
  for (int ct = 0; ct < 8; ++ct) {
    h16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((h16x4 __attribute__((address_space(3)))*)(sx + t_off(r0 + tq, 2 * ct + (tp >> 1)) + 8 * (tp & 1)));
    h16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((h16x4 __attribute__((address_space(3)))*)(sx + t_off(16 + r0 + tq, 2 * ct + (tp >> 1)) + 8 * (tp & 1)));
    f16x8 bf = (f16x8){(f16)lo[0], (f16)lo[1], (f16)lo[2], (f16)lo[3], (f16)hi[0], (f16)hi[1], (f16)hi[2], (f16)hi[3]};
    f32x4 z = __builtin_amdgcn_mfma_f32_16x16x32_f16(pf, bf, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    if (g < 2) {
#pragma unroll
      for (int r = 0; r < 4; ++r) *reinterpret_cast<f16*>(sz + ((4 * g + r) * 128 + ct * 16 + m) * 2) = (f16)z[r];
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  f16* dst = Z + (size_t)(b * 1024 + p) * 1088;
  *reinterpret_cast<f16x8*>(dst + lane * 8) = *reinterpret_cast<const f16x8*>(sz + lane * 16);
  *reinterpret_cast<f16x8*>(dst + (64 + lane) * 8) = *reinterpret_cast<const f16x8*>(sz + (64 + lane) * 16);
  // columns 1024 .. 1039: [1, 0 x 15] without attn_drop, [0, s_0 .. s_7, 0 x 7] with it
  float sh8[8];
#pragma unroll
  for (int hh = 0; hh < 8; ++hh) sh8[hh] = DROP ? __shfl(hsum, hh, 64) : 0.f;
  if (lane == 0) {
    *reinterpret_cast<f16x8*>(dst + 1024) = DROP ? (f16x8){(f16)0.f, (f16)sh8[0], (f16)sh8[1], (f16)sh8[2], (f16)sh8[3], (f16)sh8[4], (f16)sh8[5], (f16)sh8[6]}
                                                 : (f16x8){(f16)1.0f, 0, 0, 0, 0, 0, 0, 0};
    *reinterpret_cast<f16x8*>(dst + 1032) = (f16x8){(f16)sh8[7], 0, 0, 0, 0, 0, 0, 0};
  }
}

// ---- fused block tail -------------------------------------------------------------------------------------------
// ExpertBlock tail  x_l = lrelu(BN2(conv2) * layer_scale + x_{l-1})  (lunar_evaluator.py:273-275).  Outside image rows
// 0..5 conv2 is one of six constant vectors, so there  x_l = lrelu(x_{l-1} + K_l[class]),  K_l[class][c] =
// (cvec[class][c] * scale2[c] + shift2[c]) * layer_scale[c].  The full-resolution x_l is never written: the next block's
// conv1 (lo_conv3x3_pp, transform on load) reads the expert's input `feat` and applies T_l .. T_1 to its LDS patch; only
// image rows 0..7 exist as tensors (xc_l, [B][8][128][128]), and the global average pool of x_3 is one pass over feat.
__device__ __forceinline__ int t_pos_class(int y, int x) { return (y == 127 ? 3 : 0) + (x == 0 ? 1 : (x == 127 ? 2 : 0)); }

// rows 0..7 of x_l, and the level's transform constants kx[class][c] (written by workgroup 0).  Block = 16 positions x 16
// chunks of 8 channels; the per-channel scale / shift / layer-scale live in registers.  idt: x_{l-1} rows (feat for l = 0,
// pitch 16384 pixels per sample; else the previous compact buffer, pitch 1024)
__global__ __launch_bounds__(256) void lo_t_tail_compact_kernel(const f16* __restrict__ rawc, const float* __restrict__ ss,
                                                                const float* __restrict__ ls, const float* __restrict__ cvec,
                                                                const f16* __restrict__ idt, int idt_pitch, f16* __restrict__ xc,
                                                                f16* __restrict__ kx, int B) {
  const int tid = threadIdx.x, chunk = tid & 15, c0 = chunk * 8;
  float sc[8], sh[8], lsv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { sc[j] = ss[(c0 + j) * 2]; sh[j] = ss[(c0 + j) * 2 + 1]; lsv[j] = ls[c0 + j]; }
  if (blockIdx.x == 0) {
    for (int i = tid; i < 6 * 128; i += 256) {
      const int c = i & 127;
      kx[i] = (f16)((cvec[i] * ss[c * 2] + ss[c * 2 + 1]) * ls[c]);
    }
  }
  // 16 positions per pass, 4 passes per block
  for (int r = 0; r < 4; ++r) {
    const int gp = (blockIdx.x * 4 + r) * 16 + (tid >> 4);
    const int p = gp & 1023, b = gp >> 10;
    if (b >= B) return;
    const int y = p >> 7, x = p & 127;
    f16x8 id = *reinterpret_cast<const f16x8*>(idt + ((size_t)b * idt_pitch + p) * 128 + c0), o, rw;
    if (y < 6) rw = *reinterpret_cast<const f16x8*>(rawc + ((size_t)b * 1024 + p) * 128 + c0);
    else {
      const float* cv = cvec + t_pos_class(y, x) * 128 + c0;
#pragma unroll
      for (int j = 0; j < 8; ++j) rw[j] = (f16)cv[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = ((float)rw[j] * sc[j] + sh[j]) * lsv[j] + (float)id[j];
      o[j] = (f16)(v > 0.f ? v : 0.2f * v);
    }
    *reinterpret_cast<f16x8*>(xc + ((size_t)b * 1024 + p) * 128 + c0) = o;
  }
}

// pooled partial sums of x_3 = T_3(T_2(T_1(feat))) (rows >= 8) / xc (rows 0..7) for ALL experts in one pass over feat:
// pool_partial[e][n][blk][c], 64 blocks of 256 positions per sample (the layout lo_pool_finalize_kernel reads).
// kx: [E][3][6][128] fp16, xc: [E][B][1024][128] (compact x_3 rows of every expert).
template <int E>
__global__ __launch_bounds__(256) void lo_t_pool_xf_kernel(const f16* __restrict__ feat, const f16* __restrict__ xc,
                                                           const f16* __restrict__ kx, float* __restrict__ pool_partial, int B) {
  __shared__ float s_red[256 * 8];
  const int tid = threadIdx.x, n = blockIdx.y, blk = blockIdx.x;
  const int cc = tid & 15, slot = tid >> 4, c0 = cc * 8;
  float acc[E][8];
#pragma unroll
  for (int e = 0; e < E; ++e)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[e][j] = 0.f;
  for (int r = slot; r < 256; r += 16) {
    const int p = blk * 256 + r, y = p >> 7, x = p & 127;
    if (y < 8) {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        f16x8 h = *reinterpret_cast<const f16x8*>(xc + (((size_t)e * B + n) * 1024 + p) * 128 + c0);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[e][j] += (float)h[j];
      }
    } else {
      const f16x8 f = *reinterpret_cast<const f16x8*>(feat + ((size_t)n * T_HW + p) * 128 + c0);
      const int cls = t_pos_class(y, x);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        f16x8 h = f;
        // the levels are applied in fp16 exactly as the conv kernels do it
#pragma unroll
        for (int lev = 0; lev < 3; ++lev) {
          const f16x8 k = *reinterpret_cast<const f16x8*>(kx + ((e * 3 + lev) * 6 + cls) * 128 + c0);
          h = h + k;
          h = __builtin_elementwise_max(h, h * (f16)0.2f);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[e][j] += (float)h[j];
      }
    }
  }
#pragma unroll
  for (int e = 0; e < E; ++e) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) s_red[tid * 8 + j] = acc[e][j];
    __syncthreads();
    for (int c = tid; c < 128; c += 256) {
      const int ccx = c >> 3, j = c & 7;
      float tot = 0.f;
      for (int s = 0; s < 16; ++s) tot += s_red[(s * 16 + ccx) * 8 + j];
      pool_partial[(((size_t)e * B + n) * gridDim.x + blk) * 128 + c] = tot;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
int t_pack_f128(LoTeacher* h, const float* P, void* ws, int e, int l, hipStream_t st) {
  const TBlockOff& k = h->blk[e][l];
  hipLaunchKernelGGL(lo_t_cvec_kernel, dim3(6), dim3(128), 0, st, TW(f16, h->o_wp3[e][l][1]), TP(k.conv2_b), TP(k.proj_b), TW(float, h->o_cvec[e][l]));
  LO_LAUNCH_CHECK("t_cvec");
  hipLaunchKernelGGL(lo_t_fold_qk_kernel, dim3(1024), dim3(128), 0, st, TP(k.qkv_w), TP(k.qkv_b), TW(f16, h->o_wu[e][l]), TW(float, h->o_ub[e][l]));
  LO_LAUNCH_CHECK("t_fold_qk");
  hipLaunchKernelGGL(lo_t_fold_pv_kernel, dim3(128), dim3(256), 0, st, TP(k.qkv_w), TP(k.qkv_b), TP(k.proj_w), TW(f16, h->o_wz[e][l]));
  LO_LAUNCH_CHECK("t_fold_pv");
  return LO_OK;
}

// full-resolution output of block l (ping-pong; l = -1: the expert's input), and its e4m3 copy in fp8 mode
static f16* t_x(const TFwd& c, int l) { void* ws = c.ws; return l < 0 ? TW(f16, c.h->o_feat) : TW(f16, (l & 1) ? c.h->o_x1 : c.h->o_x0); }
static uint8_t* t_x8(const TFwd& c, int l) {
  void* ws = c.ws;
  return !c.f8 ? nullptr : (l < 0 ? TW(uint8_t, c.h->o_feat8) : TW(uint8_t, c.h->o_x8[l & 1]));
}

// folded attention up to proj on the compact rows: BN(conv1) (through the (scale, shift) table ss) is applied on the fly, k / v never
// exist (see lo_t_attn_folded_kernel).  DROP: per-sample table (Dropout2d) and attn_drop on the probabilities
template <bool DROP>
static int t_attn_folded(const TFwd& c, int e, int l, const float* ss) {
  LoTeacher* h = c.h; float* P = c.P; void* ws = c.ws; hipStream_t st = c.st;
  const int B = h->B;
  const size_t px = (size_t)B * T_HW;
  {
    LoProfScope _p("lo_t_gather_q", 0, 0, st);
    hipLaunchKernelGGL(lo_t_gather_q_kernel, dim3((B * 543 * 16 + 255) / 256), dim3(256), 0, st, TW(f16, h->o_rawA), ss, TW(f16, h->o_qin), B, DROP ? 256 : 0);
  }
  LO_LAUNCH_CHECK("t_gather_q");
  LO_TAGGED("t_U (igemm)", lo_conv_run(h->gU, {.in = TW(f16, h->o_qin), .w = TW(f16, h->o_wu[e][l]), .bias = TW(float, h->o_ub[e][l]), .out = TW(f16, h->o_U)}, st));
  {
    LoProfScope _p("lo_t_attn_folded", 2.0 * B * 543 * 2 * 8 * 32 * 128, 2.0 * px * 128 + 2.0 * B * 543 * 2112, st);
    if (DROP)
      hipLaunchKernelGGL((lo_t_attn_folded_kernel<true>), dim3((B * 543 + 3) / 4), dim3(256), 0, st, TW(f16, h->o_rawA), ss, TW(f16, h->o_U),
                         TW(f16, h->o_Z), B, 256, c.d.site(LO_DS_BLOCK(e, l, 1)), c.d.thr, c.d.inv_keep);
    else
      hipLaunchKernelGGL((lo_t_attn_folded_kernel<false>), dim3((B * 543 + 3) / 4), dim3(256), 0, st, TW(f16, h->o_rawA), ss, TW(f16, h->o_U), TW(f16, h->o_Z), B,
                         0, LoDropSite{0u, 0u}, 0u, 1.0f);
  }
  LO_LAUNCH_CHECK("t_attn_folded");
  LO_TAGGED("t_proj (igemm)", lo_conv_run(h->gZ, {.in = TW(f16, h->o_Z), .w = TW(f16, h->o_wz[e][l]), .bias = TP(h->blk[e][l].proj_b), .out = TW(f16, h->o_projc)}, st));
  return LO_OK;
}

// one full-resolution 3x3 conv of the dropout path: e4m3 operands, the fused-tap kernel, or the igemm; *rows: BatchNorm partial rows it wrote
static int t_conv3_full(const TFwd& c, const char* tag, int e, int l, int which, const f16* in, const uint8_t* in8, const float* bias, f16* out, int* rows) {
  LoTeacher* h = c.h; void* ws = c.ws; hipStream_t st = c.st;
  LoConvExtra ex{1, TW(float, h->o_bnp)};
  const f16* w = TW(f16, h->o_wp3[e][l][which]);
  const LoConvOp op{.in = in, .w = w, .bias = bias, .out = out, .ex = &ex};
  const bool pp = c.f8 || lo_conv3_pp_applies(h->g3);
  LoConvChoice ch;
  *rows = lo_conv3_pp_rows(h->g3);
  if (c.f8) { LO_TAGGED(tag, lo_conv3_run_pp_f8(h->g3, in8, TW(uint8_t, h->o_w8[e][l][which]), TW(float, h->o_ws8[e][l][which]), bias, out, st, &ex)); }
  else if (pp) { LO_TAGGED(tag, lo_conv3_run_pp_xf(h->g3, in, nullptr, nullptr, 0, w, bias, out, st, &ex)); }
  else { LO_TAGGED(tag, lo_conv_run(h->g3, op, st, &ch)); *rows = ch.rows; }
  return LO_OK;
}

// dropout path: both 3x3 convs in full, the attention still folded (only 543 positions of its output are ever non-zero BEFORE
// proj_drop; Dropout2d is a per-sample channel scale that rides on the BatchNorm table)
int t_block_dropout(const TFwd& c, int e, int l) {
  LoTeacher* h = c.h; float* P = c.P; void* ws = c.ws; hipStream_t st = c.st;
  const TBlockOff& k = h->blk[e][l];
  const int B = h->B;
  const size_t px = (size_t)B * T_HW;
  float* bnp = TW(float, h->o_bnp);
  const bool f8 = c.f8;
  int rows3 = 0;
  LO_TRYT(t_conv3_full(c, f8 ? "t_conv1 (dense, dropout path, e4m3)" : "t_conv1 (dense, dropout path)", e, l, 0, t_x(c, l - 1), t_x8(c, l - 1), TP(k.conv1_b),
                       TW(f16, h->o_rawA), &rows3));
  LO_TRYT(t_bn_finalize(h, P, ws, {.partial = bnp, .nrow = rows3, .C = 128, .bn = k.bn1, .training = c.training}, st));
  LO_TRYT(t_drop2d(h, ws, 128, c.d, LO_DS_BLOCK(e, l, 0), st));
  LO_TRYT(t_attn_folded<true>(c, e, l, TW(float, h->o_ssb)));
  {
    LoProfScope _p("lo_t_projdrop", 0, 2.0 * px * 128, st);
    LO_TRYT(t_projdrop(128, TW(f16, h->o_projc), TP(k.proj_b), TW(f16, h->o_proj), f8 ? TW(uint8_t, h->o_proj8) : nullptr, px * 16,
                       c.d.site(LO_DS_BLOCK(e, l, 2)), c.d.thr, c.d.inv_keep, st));
  }
  LO_TRYT(t_conv3_full(c, f8 ? "t_conv2 (dense, dropout path, e4m3)" : "t_conv2 (dense, dropout path)", e, l, 1, TW(f16, h->o_proj),
                       f8 ? TW(uint8_t, h->o_proj8) : nullptr, TP(k.conv2_b), TW(f16, h->o_rawB), &rows3));
  LO_TRYT(t_bn_finalize(h, P, ws, {.partial = bnp, .nrow = rows3, .C = 128, .bn = k.bn2, .training = c.training}, st));
  LO_TRYT(t_drop2d(h, ws, 128, c.d, LO_DS_BLOCK(e, l, 3), st));
  // the last block's output feeds nothing but the global average pool: a statistics-only call skips its tail, a full call
  // only sums it (no 268 MB store)
  if (l < 2 || !c.stats_only)
    LO_TRYT(t_bn_apply(h, ws, {.raw = TW(f16, h->o_rawB), .ls = TP(k.layer_scale), .identity = t_x(c, l - 1), .y = l < 2 ? t_x(c, l) : nullptr,
                               .C = 128, .mode = T_BN_TAIL, .pool_partial = (l == 2 && !c.stats_only) ? TW(float, h->o_poolp) : nullptr,
                               .per_sample = true, .y8 = l < 2 ? t_x8(c, l) : nullptr}, st));
  return LO_OK;
}

// sparse path; with the fused tail conv1 reads the expert's input and applies the l previous block tails to its LDS patch (rows 0..7: xc)
int t_block_sparse(const TFwd& c, int e, int l) {
  LoTeacher* h = c.h; float* P = c.P; void* ws = c.ws; hipStream_t st = c.st;
  const TBlockOff& k = h->blk[e][l];
  const int B = h->B;
  float* bnp = TW(float, h->o_bnp);
  LoConvExtra ex{1, bnp};
  if (h->fuse_tail) {
    LO_TAGGED(l ? "t_conv1 (fused tap, tail on load)" : "t_conv1 (fused tap)",
              lo_conv3_run_pp_xf(h->g3, TW(f16, h->o_feat), l ? TW(f16, h->o_xc[(l - 1) & 1]) : nullptr, TW(f16, h->o_kx[e]), l,
                                 TW(f16, h->o_wp3[e][l][0]), TP(k.conv1_b), TW(f16, h->o_rawA), st, &ex));
    LO_TRYT(t_bn_finalize(h, P, ws, {.partial = bnp, .nrow = lo_conv3_pp_rows(h->g3), .C = 128, .bn = k.bn1, .training = c.training}, st));
  } else {
    const LoConvOp c1{.in = t_x(c, l - 1), .w = TW(f16, h->o_wp3[e][l][0]), .bias = TP(k.conv1_b), .out = TW(f16, h->o_rawA), .ex = &ex};
    LoConvChoice ch;
    LO_TAGGED("t_conv1 (igemm)", lo_conv_run(h->g3, c1, st, &ch));
    LO_TRYT(t_bn_finalize(h, P, ws, {.partial = bnp, .nrow = ch.rows, .C = 128, .bn = k.bn1, .training = c.training}, st));
  }
  LO_TRYT(t_attn_folded<false>(c, e, l, TW(float, h->o_ss)));
  const LoConvOp c2{.in = TW(f16, h->o_projc), .w = TW(f16, h->o_wp3[e][l][1]), .bias = TP(k.conv2_b), .out = TW(f16, h->o_rawBc), .ex = &ex};
  LoConvChoice ch2;
  LO_TAGGED("t_conv2c (igemm)", lo_conv_run(h->g3c, c2, st, &ch2));
  const int tm = ch2.bm;     // the compact rows below are counted in lo_igemm_nt's M tiles
  LO_REQUIRE(ch2.kernel == LO_CK_IGEMM && (tm == 64 || tm == 128), "teacher sparse path: unexpected conv kernel %d / tile height %d", ch2.kernel, tm);
  const float* cv = TW(float, h->o_cvec[e][l]);
  LO_TRYT(t_bn_finalize(h, P, ws, {.partial = bnp, .nrow = B * 1024 / tm, .C = 128, .bn = k.bn2, .training = c.training, .tps = 1024 / tm,
                                   .vtps = 6 * 128 / tm, .cvec = cv}, st));
  if (!h->fuse_tail)
    return t_bn_apply(h, ws, {.raw = TW(f16, h->o_rawBc), .ls = TP(k.layer_scale), .identity = t_x(c, l - 1), .y = t_x(c, l), .C = 128,
                              .mode = T_BN_TAIL_SPARSE, .pool_partial = l == 2 ? TW(float, h->o_poolp) : nullptr, .cvec = cv}, st);
  f16* kx = TW(f16, h->o_kx[e]) + l * 6 * 128;
  {
    LoProfScope _p("lo_t_tail (rows 0..7 + constants)", 0, 0, st);
    hipLaunchKernelGGL(lo_t_tail_compact_kernel, dim3(B * 16), dim3(256), 0, st, TW(f16, h->o_rawBc), TW(float, h->o_ss), TP(k.layer_scale), cv,
                       l ? TW(f16, h->o_xc[(l - 1) & 1]) : TW(f16, h->o_feat), l ? 1024 : T_HW,
                       l == 2 ? TW(f16, h->o_xc3) + (size_t)e * B * 1024 * 128 : TW(f16, h->o_xc[l & 1]), kx, B);
  }
  LO_LAUNCH_CHECK("t_tail_compact");
  return LO_OK;
}

int t_block_dense(const TFwd& c, int e, int l) {
  LoTeacher* h = c.h; float* P = c.P; void* ws = c.ws; hipStream_t st = c.st;
  const TBlockOff& k = h->blk[e][l];
  const int B = h->B;
  float* bnp = TW(float, h->o_bnp);
  LoConvExtra ex{1, bnp};
  const LoConvOp c1{.in = t_x(c, l - 1), .w = TW(f16, h->o_wp3[e][l][0]), .bias = TP(k.conv1_b), .out = TW(f16, h->o_rawA), .ex = &ex};
  LoConvChoice ch;     // of the launch that just ran: BatchNorm partial rows of its epilogue (igemm: M tiles)
  LO_TAGGED("t_conv1 (igemm)", lo_conv_run(h->g3, c1, st, &ch));
  LO_TRYT(t_bn_finalize(h, P, ws, {.partial = bnp, .nrow = ch.rows, .C = 128, .bn = k.bn1, .training = c.training}, st));
  LO_TRYT(t_bn_apply(h, ws, {.raw = TW(f16, h->o_rawA), .y = TW(f16, h->o_bnA), .C = 128}, st));
  LO_TRYT(lo_conv_run(h->gq, {.in = TW(f16, h->o_bnA), .w = TW(f16, h->o_wqkv[e][l]), .bias = TP(k.qkv_b), .out = TW(f16, h->o_qkv)}, st));
  {
    LoProfScope _p("lo_t_attn", 0, 0, st);
    int nw = B * 543;
    hipLaunchKernelGGL(lo_t_attn_kernel, dim3((nw + 3) / 4), dim3(256), 0, st, TW(f16, h->o_qkv), TW(f16, h->o_att), B);
  }
  LO_LAUNCH_CHECK("t_attn");
  LO_TRYT(lo_conv_run(h->gp, {.in = TW(f16, h->o_att), .w = TW(f16, h->o_wproj[e][l]), .bias = TP(k.proj_b), .out = TW(f16, h->o_proj)}, st));
  LO_TRYT(lo_conv_run(h->g3, {.in = TW(f16, h->o_proj), .w = TW(f16, h->o_wp3[e][l][1]), .bias = TP(k.conv2_b), .out = TW(f16, h->o_rawB), .ex = &ex}, st, &ch));
  LO_TRYT(t_bn_finalize(h, P, ws, {.partial = bnp, .nrow = ch.rows, .C = 128, .bn = k.bn2, .training = c.training}, st));
  return t_bn_apply(h, ws, {.raw = TW(f16, h->o_rawB), .ls = TP(k.layer_scale), .identity = t_x(c, l - 1), .y = t_x(c, l), .C = 128,
                            .mode = T_BN_TAIL, .pool_partial = l == 2 ? TW(float, h->o_poolp) : nullptr}, st);
}

// x_3 of every expert is pooled in ONE pass over feat (the full-resolution x_l were never written)
int t_pool_fused(const TFwd& c) {
  LoTeacher* h = c.h; void* ws = c.ws; hipStream_t st = c.st;
  const int B = h->B;
  {
    LoProfScope _p("lo_t_pool (tail on load)", 0, 2.0 * (size_t)B * T_HW * 128, st);
#define LO_POOL(EE) hipLaunchKernelGGL((lo_t_pool_xf_kernel<EE>), dim3(64, B), dim3(256), 0, st, TW(f16, h->o_feat), TW(f16, h->o_xc3), \
                                       TW(f16, h->o_kx[0]), TW(float, h->o_poolpe), B)
    switch (h->E) {
      case 1: LO_POOL(1); break; case 2: LO_POOL(2); break; case 3: LO_POOL(3); break; case 4: LO_POOL(4); break;
      case 5: LO_POOL(5); break; case 6: LO_POOL(6); break; case 7: LO_POOL(7); break; default: LO_POOL(8); break;
    }
#undef LO_POOL
  }
  LO_LAUNCH_CHECK("t_pool_xf");
  return t_pool_finalize(TW(float, h->o_poolpe), TW(float, h->o_pool_e), 64, 128, h->E * B * 128, st);
}
