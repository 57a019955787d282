// Bottleneck self-attention of the VAE (SelfAttention2d, lunar_generate.py:56-78, at the 8 x 8 x 512 stage): the two core kernels.
//   qkv [B][64][640] fp16: per position the 64 query, 64 key and 512 value channels (one 1x1-conv GEMM, x Wqkv^T + b)
//   S[i][j] = sum_c q[i][c] k[j][c],  P = softmax_j S,  O[i][c] = sum_j P[i][j] v[j][c],  y = gamma O + x      (fp16 NHWC)
// One workgroup (4 waves) per sample; every product runs on v_mfma_f32_16x16x32_f16, no N x N tensor goes to global memory, every sum
// has a fixed order (no atomics).  Operand maps of the instruction (lane l: l16 = l & 15, g = l >> 4):
//   A[m = l16][k = 8g + e], B[k = 8g + e][n = l16] (e = 0..7), D[m = 4g + r][n = l16] (r = 0..3).
// The kernels compute S TRANSPOSED: tile jt of S^T has the key position j = 16 jt + 4g + r in its rows and the query position i on the
// lane.  A product that sums over j then takes two such tiles as ONE B fragment with no lane movement: slot e < 4 = tile 2ks row
// 4g + e, slot e >= 4 = tile 2ks + 1 row 4g + e - 4.  The sum over k does not care about the order of its terms, so the A fragment
// is gathered with the same map (j = 16 (2ks + (e >> 2)) + 4g + (e & 3)), which costs nothing where A is read with a stride anyway.
#include "lo_internal.h"
#include "../../include/lunaris_hip.h"

namespace {
constexpr int AN = 64;       // positions
constexpr int AC = 512;      // channels
constexpr int AW = 640;      // row of qkv: q | k | v
constexpr int AQ = 0, AK = 64, AV = 128;
constexpr int LDP = 72;      // row pitch (fp16) of the 64 x 64 LDS images: 144 B, keeps the 16-byte fragment reads aligned

__device__ __forceinline__ f32x4 mfma(const f16x8 a, const f16x8 b, const f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
// key / query position of slot e of k-step ks under the permuted map above
__device__ __forceinline__ int perm_pos(int ks, int g, int e) { return 16 * (2 * ks + (e >> 2)) + 4 * g + (e & 3); }

// S^T of query tile `it`: st[jt][r] = S[i = 16 it + l16][j = 16 jt + 4g + r]
__device__ __forceinline__ void attn8_scores(const f16* __restrict__ qkv, int it, int l16, int g, f32x4 st[4]) {
  f16x8 qf[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) qf[ks] = *reinterpret_cast<const f16x8*>(qkv + (size_t)(16 * it + l16) * AW + AQ + 32 * ks + 8 * g);
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const f16x8 kf = *reinterpret_cast<const f16x8*>(qkv + (size_t)(16 * jt + l16) * AW + AK + 32 * ks + 8 * g);
      acc = mfma(kf, qf[ks], acc);
    }
    st[jt] = acc;
  }
}
// softmax over j of the lane's column: st becomes exp(s - max) (not normalised); returns 1 / sum.  The 16 values of a lane, then the
// four lanes of the column (xor 16, 32): the same order in every run
__device__ __forceinline__ float attn8_softmax(f32x4 st[4]) {
  float m = st[0][0];
#pragma unroll
  for (int jt = 0; jt < 4; ++jt)
#pragma unroll
    for (int r = 0; r < 4; ++r) m = fmaxf(m, st[jt][r]);
  m = fmaxf(m, __shfl_xor(m, 16));
  m = fmaxf(m, __shfl_xor(m, 32));
  float s = 0.f;
#pragma unroll
  for (int jt = 0; jt < 4; ++jt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float e = __expf(st[jt][r] - m);
      st[jt][r] = e;
      s += e;
    }
  s += __shfl_xor(s, 16);
  s += __shfl_xor(s, 32);
  return 1.0f / s;
}
__device__ __forceinline__ f16x8 pack_tiles(const f32x4 a, const f32x4 b, float sc) {
  return f16x8{(f16)(a[0] * sc), (f16)(a[1] * sc), (f16)(a[2] * sc), (f16)(a[3] * sc), (f16)(b[0] * sc), (f16)(b[1] * sc), (f16)(b[2] * sc), (f16)(b[3] * sc)};
}
// A fragment of a product over positions whose rows are channels: src[pos][ch] read with the stride of a row, positions by perm_pos
// (perm) or in natural order
template <bool PERM>
__device__ __forceinline__ f16x8 gather_pos(const f16* __restrict__ src, int pitch, int ch, int ks, int g) {
  f16x8 a;
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] = src[(size_t)(PERM ? perm_pos(ks, g, e) : 32 * ks + 8 * g + e) * pitch + ch];
  return a;
}

// ---- forward: wave w owns channels [128 w, 128 w + 128) of all 64 positions; every wave forms the whole P (32 MFMAs) in registers
__global__ __launch_bounds__(256) void lo_attn8_fwd_kernel(const f16* __restrict__ x, const f16* __restrict__ qkv, const float* __restrict__ gamma,
                                                           f16* __restrict__ y) {
  const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6, l16 = lane & 15, g = lane >> 4;
  const f16* qb = qkv + (size_t)b * AN * AW;
  const float gam = gamma[0];
  f16x8 pf[4][2];
  float inv[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    f32x4 st[4];
    attn8_scores(qb, it, l16, g, st);
    inv[it] = attn8_softmax(st);
    pf[it][0] = pack_tiles(st[0], st[1], 1.0f);       // exp(s - max) <= 1: the 1 / sum is applied to the fp32 result
    pf[it][1] = pack_tiles(st[2], st[3], 1.0f);
  }
#pragma unroll 2
  for (int ct = 0; ct < 8; ++ct) {
    const int c0 = 128 * w + 16 * ct;
    f32x4 acc[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) acc[it] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const f16x8 vf = gather_pos<true>(qb + AV, AW, c0 + l16, ks, g);      // A[m = c][k = j] = v[j][c]
#pragma unroll
      for (int it = 0; it < 4; ++it) acc[it] = mfma(vf, pf[it][ks], acc[it]);
    }
    // D[m = channel c0 + 4g + r][n = position 16 it + l16]
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const size_t o = ((size_t)b * AN + 16 * it + l16) * AC + c0 + 4 * g;
      const f16x4 xv = *reinterpret_cast<const f16x4*>(x + o);
      f16x4 yv;
#pragma unroll
      for (int r = 0; r < 4; ++r) yv[r] = (f16)(gam * (acc[it][r] * inv[it]) + (float)xv[r]);
      *reinterpret_cast<f16x4*>(y + o) = yv;
    }
  }
}

// ---- backward: wave w owns query tile w for S, P, dA, dS and dQ, key tile w for dK, channels [128 w, 128 w + 128) for dV
__global__ __launch_bounds__(256) void lo_attn8_bwd_kernel(const f16* __restrict__ qkv, const float* __restrict__ gamma, const f16* __restrict__ dy,
                                                           f16* __restrict__ dqkv, float* __restrict__ dgamma_part) {
  __shared__ __attribute__((aligned(16))) f16 s_p[AN * LDP];       // P^T  [j][i]
  __shared__ __attribute__((aligned(16))) f16 s_ds[AN * LDP];      // dS^T [j][i], times the power of two `sc`
  __shared__ float s_red[4], s_max[4];
  const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6, l16 = lane & 15, g = lane >> 4;
  const f16* qb = qkv + (size_t)b * AN * AW;
  const f16* dyb = dy + (size_t)b * AN * AC;
  f16* dqb = dqkv + (size_t)b * AN * AW;
  const float gam = gamma[0];
  // P of query tile w
  f32x4 p[4];
  attn8_scores(qb, w, l16, g, p);
  {
    const float inv = attn8_softmax(p);
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) p[jt] *= inv;
  }
  // dA^T[j][i] = sum_c v[j][c] dy[i][c]  (without gamma; carries the loss scale of dy)
  f32x4 da[4];
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) da[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int kc = 0; kc < AC / 32; ++kc) {
    const f16x8 df = *reinterpret_cast<const f16x8*>(dyb + (size_t)(16 * w + l16) * AC + 32 * kc + 8 * g);
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      const f16x8 vf = *reinterpret_cast<const f16x8*>(qb + (size_t)(16 * jt + l16) * AW + AV + 32 * kc + 8 * g);
      da[jt] = mfma(vf, df, da[jt]);
    }
  }
  // t_i = sum_j P dA: the softmax backward's row term, and sum_i t_i = sum dy . O = this sample's share of dgamma
  float t = 0.f;
#pragma unroll
  for (int jt = 0; jt < 4; ++jt)
#pragma unroll
    for (int r = 0; r < 4; ++r) t += p[jt][r] * da[jt][r];
  t += __shfl_xor(t, 16);
  t += __shfl_xor(t, 32);
  float tg = t;
#pragma unroll
  for (int d = 1; d < 16; d <<= 1) tg += __shfl_xor(tg, d);
  // dS = gamma P (dA - t), fp32; its largest magnitude over the sample picks the power of two under which it becomes an fp16 operand
  float mx = 0.f;
#pragma unroll
  for (int jt = 0; jt < 4; ++jt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      da[jt][r] = gam * p[jt][r] * (da[jt][r] - t);
      mx = fmaxf(mx, fabsf(da[jt][r]));
    }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
  if (lane == 0) { s_red[w] = tg; s_max[w] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) dgamma_part[b] = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
  const float m = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
  float sc = 1.f, isc = 1.f;
  if (m > 0.f && m < 3.0e38f) {      // largest |dS| * sc in [2^13, 2^14): far from fp16's 65 504, 24 binades above its subnormals
    int e;
    (void)frexpf(m, &e);
    e = e < -100 ? -100 : e;
    sc = ldexpf(1.f, 14 - e);
    isc = ldexpf(1.f, e - 14);
  }
#pragma unroll
  for (int jt = 0; jt < 4; ++jt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = 16 * jt + 4 * g + r, i = 16 * w + l16;
      s_p[j * LDP + i] = (f16)p[jt][r];
      s_ds[j * LDP + i] = (f16)(da[jt][r] * sc);
    }
  // dQ^T[c][i] = sum_j k[j][c] dS[i][j]: dS^T of this wave's query tile is the B operand as it stands
  {
    const f16x8 sf[2] = {pack_tiles(da[0], da[1], sc), pack_tiles(da[2], da[3], sc)};
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) acc = mfma(gather_pos<true>(qb + AK, AW, 16 * ct + l16, ks, g), sf[ks], acc);
      f16x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = (f16)(acc[r] * isc);
      *reinterpret_cast<f16x4*>(dqb + (size_t)(16 * w + l16) * AW + AQ + 16 * ct + 4 * g) = o;
    }
  }
  __syncthreads();
  // dK^T[c][j] = sum_i q[i][c] dS[i][j], key tile w
  {
    f16x8 sf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) sf[ks] = *reinterpret_cast<const f16x8*>(s_ds + (16 * w + l16) * LDP + 32 * ks + 8 * g);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) acc = mfma(gather_pos<false>(qb + AQ, AW, 16 * ct + l16, ks, g), sf[ks], acc);
      f16x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = (f16)(acc[r] * isc);
      *reinterpret_cast<f16x4*>(dqb + (size_t)(16 * w + l16) * AW + AK + 16 * ct + 4 * g) = o;
    }
  }
  // dV^T[c][j] = gamma sum_i dy[i][c] P[i][j], channels [128 w, 128 w + 128)
  {
    f16x8 pf[4][2];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) pf[jt][ks] = *reinterpret_cast<const f16x8*>(s_p + (16 * jt + l16) * LDP + 32 * ks + 8 * g);
#pragma unroll 2
    for (int ct = 0; ct < 8; ++ct) {
      const int c0 = 128 * w + 16 * ct;
      f32x4 acc[4];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) acc[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const f16x8 df = gather_pos<false>(dyb, AC, c0 + l16, ks, g);
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) acc[jt] = mfma(df, pf[jt][ks], acc[jt]);
      }
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        f16x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (f16)(gam * acc[jt][r]);
        *reinterpret_cast<f16x4*>(dqb + (size_t)(16 * jt + l16) * AW + AV + c0 + 4 * g) = o;
      }
    }
  }
}

// dgamma = scale * (the B per-sample shares, added in a fixed order: each lane its stride-256 subsequence, then a fixed tree)
__global__ __launch_bounds__(256) void lo_attn8_dgamma_kernel(const float* __restrict__ part, int B, float scale, float* __restrict__ out) {
  __shared__ float red[256];
  float s = 0.f;
  for (int k = threadIdx.x; k < B; k += 256) s += part[k];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) red[threadIdx.x] += red[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0] * scale;
}
}  // namespace

int lo_attn8_fwd(const f16* x, const f16* qkv, const float* gamma, f16* y, int B, hipStream_t st) {
  LO_REQUIRE(x && qkv && gamma && y && B >= 1, "lo_attn8_fwd: bad argument");
  LoProfScope prof("lo_attn8_fwd", 2.0 * B * AN * AN * (64 + AC), 2.0 * B * AN * (AW + 2 * AC), st);
  LO_LAUNCH_STOP(lo_attn8_fwd_kernel, dim3(B), dim3(256), 0, st, x, qkv, gamma, y);
  LO_LAUNCH_CHECK("lo_attn8_fwd");
  return LO_OK;
}
int lo_attn8_bwd(const f16* qkv, const float* gamma, const f16* dy, f16* dqkv, float* dgamma_part, int B, hipStream_t st) {
  LO_REQUIRE(qkv && gamma && dy && dqkv && dgamma_part && B >= 1, "lo_attn8_bwd: bad argument");
  LoProfScope prof("lo_attn8_bwd", 2.0 * B * AN * AN * (3 * 64 + 2 * AC), 2.0 * B * AN * (2 * AW + AC), st);
  LO_LAUNCH_STOP(lo_attn8_bwd_kernel, dim3(B), dim3(256), 0, st, qkv, gamma, dy, dqkv, dgamma_part);
  LO_LAUNCH_CHECK("lo_attn8_bwd");
  return LO_OK;
}
int lo_attn8_dgamma(const float* part, int B, float scale, float* out, hipStream_t st) {
  LO_REQUIRE(part && out && B >= 1, "lo_attn8_dgamma: bad argument");
  hipLaunchKernelGGL(lo_attn8_dgamma_kernel, dim3(1), dim3(256), 0, st, part, B, scale, out);
  LO_LAUNCH_CHECK("lo_attn8_dgamma");
  return LO_OK;
}

// op level (include/lunaris_hip.h): plain device pointers, fp16 tensors; x of the backward is not read (the residual's gradient is
// added where dx is formed) and may be NULL
extern "C" int lo_attn8_forward(const void* x, const void* qkv, const float* gamma, void* y, int B, void* stream) {
  return lo_attn8_fwd((const f16*)x, (const f16*)qkv, gamma, (f16*)y, B, S(stream));
}
extern "C" int lo_attn8_backward(const void* x, const void* qkv, const float* gamma, const void* dy, void* dqkv, float* dgamma_part, int B,
                                 void* stream) {
  (void)x;
  return lo_attn8_bwd((const f16*)qkv, gamma, (const f16*)dy, (f16*)dqkv, dgamma_part, B, S(stream));
}
