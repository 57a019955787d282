// Full backward of LunarMoETeacher, part 1 (see lo_teacher_bwd.hip for the shape of the computation): the BatchNorm backward every layer
// uses and the backward of one ExpertBlock -- tail, BatchNorm2, conv2, proj_drop, proj, the chunk attention as executed (543 live rows),
// qkv, Dropout2d, BatchNorm1, conv1 (+ shortcut conv / BatchNorm when feature_dim != 128).
// Heavy contractions reuse the VAE path's kernels: lo_conv_run (3x3 data gradients as LO_CONV3_S1_DGRAD, 1x1 data gradients as
// LO_LINEAR on transposed weights) and lo_wgrad_run (weight gradients).  Everything else is below: simple, HBM-bound passes.
#include "lo_teacher.h"
#include "lo_conv.h"

// ---------------------------------------------------------------------------------------------
// BatchNorm(train) backward, per channel over (N, H, W):   y = (r - mean) * rstd * gamma + beta,  r = LeakyReLU(conv) (or conv)
//   upstream:  g(pix, c) = din(pix, c) * keep(...)            (Dropout2d: per (sample, channel); Dropout: per element; none)
//   dn = ls[c] * g          (ls = the block's layer_scale on the tail, else 1)
//   S1 = sum g, S2 = sum g * xhat                              (reduce kernel: partial rows, fixed order)
//   dbeta = ls S1, dgamma = ls S2, dls = gamma S2 + beta S1    (finalize)
//   dr = gamma rstd (dn - ls S1 / N - xhat ls S2 / N);  dconv = dr * (r > 0 ? 1 : 0.2)   (apply)
// BatchNorm(eval) backward (`frozen`): mean / rstd are the running statistics, constants of the graph, and there is no dropout:
//   dr = gamma rstd ls g;  dconv = dr * (r > 0 ? 1 : 0.2);  dbeta, dgamma, dls as above (reduce + finalize run for them only)
// A call that wants no parameter gradient runs lo_tb_bn_frozen_kernel alone: one streaming pass per layer.
// ---------------------------------------------------------------------------------------------
struct TbBnArgs {
  const f16* din; int din_pitch, din_off;       // upstream gradient [pix][din_pitch] (+ channel offset)
  const f16* raw; int raw_pitch, raw_off;       // BatchNorm input as stored by the forward
  const float* mr;                              // [C][2] mean, rstd
  const float* gamma; const float* ls;          // ls may be null
  const float* coef;                            // apply: [C][2] = ls S1 / N, ls S2 / N
  float* partial;                               // reduce: [B * 64][C][2]
  float* bpartial;                              // apply (may be null): [B * 64][C] column sums of `out` per block = the conv's bias gradient
  f16* out; int out_pitch, out_off;             // apply: gradient wrt the conv output
  int C, act;                                   // act 1: the stored tensor is LeakyReLU(conv): multiply by its slope
  int dmode; LoDropSite ds; uint32_t thr; float inv_keep; int didx_pitch, didx_off;   // 0 none, 1 Dropout2d (idx b*C+c), 2 Dropout (idx pix*pitch+off+c)
  // lo_tb_bn_frozen_kernel<true>: the ExpertBlock tail in front of the BatchNorm, y / tds dense [pix][C]; din null = tdpool broadcast
  const f16* ty; const float* tdpool; float tbscale; f16* tds;
};
// the frozen data path of one element, shared by the apply kernel (with parameters) and the fused pass (without): products only, so
// both give the same bits
__device__ __forceinline__ float tb_frozen_d(float gr, float ls, float g, float rv, int act) {
  float d = gr * (ls * g);
  if (act && !(rv > 0.f)) d *= 0.2f;
  return d;
}
__device__ __forceinline__ float tb_keep(const TbBnArgs& a, int n, size_t pix, int c) {
  if (a.dmode == 0 || a.thr == 0) return 1.f;
  const uint32_t idx = a.dmode == 1 ? (uint32_t)(n * a.C + c) : (uint32_t)(pix * (size_t)a.didx_pitch + a.didx_off + c);
  return lo_drop_keep(a.ds, idx, a.thr) ? a.inv_keep : 0.f;
}
__global__ __launch_bounds__(256) void lo_tb_bn_reduce_kernel(TbBnArgs a) {
  __shared__ float s_red[256 * 16];
  const int tid = threadIdx.x, n = blockIdx.y, blk = blockIdx.x;
  const int C = a.C, CC = C >> 3;
  const int cc = tid % CC, slot = tid / CC, nslot = 256 / CC, c0 = cc * 8;
  float mean[8], rstd[8], kc[8], s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    mean[j] = a.mr[(c0 + j) * 2]; rstd[j] = a.mr[(c0 + j) * 2 + 1]; s1[j] = 0.f; s2[j] = 0.f;
    kc[j] = a.dmode == 1 ? tb_keep(a, n, 0, c0 + j) : 1.f;
  }
  const size_t row0 = (size_t)n * T_HW + (size_t)blk * 256;
  for (int r = slot; r < 256; r += nslot) {
    const size_t pix = row0 + r;
    const f16x8 g = *reinterpret_cast<const f16x8*>(a.din + pix * a.din_pitch + a.din_off + c0);
    const f16x8 v = *reinterpret_cast<const f16x8*>(a.raw + pix * a.raw_pitch + a.raw_off + c0);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float k = a.dmode == 2 ? tb_keep(a, n, pix, c0 + j) : kc[j];
      const float gv = (float)g[j] * k, xh = ((float)v[j] - mean[j]) * rstd[j];
      s1[j] += gv; s2[j] += gv * xh;
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) { s_red[tid * 16 + j * 2] = s1[j]; s_red[tid * 16 + j * 2 + 1] = s2[j]; }
  __syncthreads();
  for (int o = tid; o < C * 2; o += 256) {
    const int c = o >> 1, w = o & 1, ccx = c >> 3, j = c & 7;
    float tot = 0.f;
    for (int s = 0; s < nslot; ++s) tot += s_red[(s * CC + ccx) * 16 + j * 2 + w];
    a.partial[(((size_t)n * 64 + blk) * C + c) * 2 + w] = tot;
  }
}
// block = 16 channels x 16 row lanes: lane r adds rows r, r + 16, ... (eight loads in flight), then the 16 lane sums in a fixed
// order (double throughout).  (One thread per channel walking all B * 64 rows was 1.2 ms per launch, 35 ms per step at batch 64.)
__global__ __launch_bounds__(256) void lo_tb_bn_finalize_kernel(const float* __restrict__ partial, int nrow, int C, float count, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, const float* __restrict__ ls, float* __restrict__ coef,
                                                                float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ dls, float inv_gscale) {
  __shared__ double red[2][16][17];
  const int cl = threadIdx.x & 15, r = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  double s1 = 0.0, s2 = 0.0;
  if (c < C) {
    int k = r;
    for (; k + 16 * 7 < nrow; k += 16 * 8) {
      f32x2 p[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) p[u] = *reinterpret_cast<const f32x2*>(partial + ((size_t)(k + 16 * u) * C + c) * 2);
#pragma unroll
      for (int u = 0; u < 8; ++u) { s1 += (double)p[u][0]; s2 += (double)p[u][1]; }
    }
    for (; k < nrow; k += 16) {
      const f32x2 p = *reinterpret_cast<const f32x2*>(partial + ((size_t)k * C + c) * 2);
      s1 += (double)p[0]; s2 += (double)p[1];
    }
  }
  red[0][r][cl] = s1; red[1][r][cl] = s2;
  __syncthreads();
  if (r != 0 || c >= C) return;
  s1 = 0.0; s2 = 0.0;
  for (int k = 0; k < 16; ++k) { s1 += red[0][k][cl]; s2 += red[1][k][cl]; }
  const double l = ls ? (double)ls[c] : 1.0;
  coef[c * 2] = (float)(l * s1 / (double)count);
  coef[c * 2 + 1] = (float)(l * s2 / (double)count);
  dbeta[c] = (float)(l * s1 * (double)inv_gscale);
  dgamma[c] = (float)(l * s2 * (double)inv_gscale);
  if (dls) dls[c] = (float)(((double)gamma[c] * s2 + (double)beta[c] * s1) * (double)inv_gscale);
}
// FROZEN: no statistic terms, coef is not read (the instantiation without it is the train-mode kernel, untouched)
template <bool FROZEN>
__global__ __launch_bounds__(256) void lo_tb_bn_apply_kernel(TbBnArgs a) {
  __shared__ float s_red[256 * 8];
  const int tid = threadIdx.x, n = blockIdx.y, blk = blockIdx.x;
  const int C = a.C, CC = C >> 3;
  const int cc = tid % CC, slot = tid / CC, nslot = 256 / CC, c0 = cc * 8;
  float mean[8], rstd[8], kc[8], k1[8], k2[8], gr[8], lsv[8], acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    acc[j] = 0.f;
    mean[j] = a.mr[(c0 + j) * 2]; rstd[j] = a.mr[(c0 + j) * 2 + 1];
    k1[j] = FROZEN ? 0.f : a.coef[(c0 + j) * 2]; k2[j] = FROZEN ? 0.f : a.coef[(c0 + j) * 2 + 1];
    gr[j] = a.gamma[c0 + j] * rstd[j];
    lsv[j] = a.ls ? a.ls[c0 + j] : 1.f;
    kc[j] = a.dmode == 1 ? tb_keep(a, n, 0, c0 + j) : 1.f;
  }
  const size_t row0 = (size_t)n * T_HW + (size_t)blk * 256;
  for (int r = slot; r < 256; r += nslot) {
    const size_t pix = row0 + r;
    const f16x8 g = *reinterpret_cast<const f16x8*>(a.din + pix * a.din_pitch + a.din_off + c0);
    const f16x8 v = *reinterpret_cast<const f16x8*>(a.raw + pix * a.raw_pitch + a.raw_off + c0);
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float k = a.dmode == 2 ? tb_keep(a, n, pix, c0 + j) : kc[j];
      const float rv = (float)v[j], xh = (rv - mean[j]) * rstd[j];
      float d;
      if (FROZEN) d = tb_frozen_d(gr[j], lsv[j], (float)g[j], rv, a.act);
      else {
        d = gr[j] * (lsv[j] * ((float)g[j] * k) - k1[j] - xh * k2[j]);
        if (a.act && !(rv > 0.f)) d *= 0.2f;
      }
      o[j] = (f16)d;
      acc[j] += (float)o[j];            // the bias gradient sums the values the weight-gradient GEMM will also see
    }
    *reinterpret_cast<f16x8*>(a.out + pix * a.out_pitch + a.out_off + c0) = o;
  }
  if (!a.bpartial) return;
#pragma unroll
  for (int j = 0; j < 8; ++j) s_red[tid * 8 + j] = acc[j];
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    const int ccx = c >> 3, j = c & 7;
    float tot = 0.f;
    for (int s = 0; s < nslot; ++s) tot += s_red[(s * CC + ccx) * 8 + j];
    a.bpartial[((size_t)n * 64 + blk) * C + c] = tot;
  }
}

// Frozen BatchNorm backward without parameter gradients, one pass: out = f16(gamma rstd ls g slope(raw)).  TAIL: also the ExpertBlock
// tail in front of BatchNorm2 -- g = dS = f16(dy slope(y)) (dy a tensor or the broadcast pooled gradient, as in lo_tb_tail_kernel) is
// written for the identity branch and the BatchNorm reads the ROUNDED value, so the bits are those of the two-kernel form.
// 3 reads + 2 writes per element (TAIL), 2 + 1 otherwise.  Thread = (8-channel chunk, row slot) like lo_tb_bn_apply_kernel; per-channel
// constants in registers, U rows' 16-byte loads issued before the first use.
template <bool TAIL>
__global__ __launch_bounds__(256) void lo_tb_bn_frozen_kernel(TbBnArgs a) {
  const int tid = threadIdx.x, n = blockIdx.y, blk = blockIdx.x;
  const int C = a.C, CC = C >> 3;
  const int cc = tid % CC, slot = tid / CC, nslot = 256 / CC, c0 = cc * 8;
  float gr[8], lsv[8], dpb[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    gr[j] = a.gamma[c0 + j] * a.mr[(c0 + j) * 2 + 1];
    lsv[j] = a.ls ? a.ls[c0 + j] : 1.f;
    dpb[j] = (TAIL && !a.din) ? a.tdpool[(size_t)n * C + c0 + j] * a.tbscale : 0.f;
  }
  const size_t row0 = (size_t)n * T_HW + (size_t)blk * 256;
  constexpr int U = 4;                     // 256 / nslot = C / 8 rows per thread: a multiple of 4 for every C >= 32
  for (int r = slot; r < 256; r += U * nslot) {
    f16x8 g[U], v[U], yv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t pix = row0 + r + u * nslot;
      v[u] = *reinterpret_cast<const f16x8*>(a.raw + pix * a.raw_pitch + a.raw_off + c0);
      if (TAIL) {
        yv[u] = *reinterpret_cast<const f16x8*>(a.ty + pix * C + c0);
        if (a.din) g[u] = *reinterpret_cast<const f16x8*>(a.din + pix * C + c0);
      } else {
        g[u] = *reinterpret_cast<const f16x8*>(a.din + pix * a.din_pitch + a.din_off + c0);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t pix = row0 + r + u * nslot;
      f16x8 o;
      if (TAIL) {
        f16x8 s;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float sl = (float)yv[u][j] > 0.f ? 1.f : 0.2f;
          s[j] = a.din ? (f16)((float)g[u][j] * sl) : (f16)(dpb[j] * sl);
        }
        *reinterpret_cast<f16x8*>(a.tds + pix * C + c0) = s;
        g[u] = s;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (f16)tb_frozen_d(gr[j], lsv[j], (float)g[u][j], (float)v[u][j], a.act);
      *reinterpret_cast<f16x8*>(a.out + pix * a.out_pitch + a.out_off + c0) = o;
    }
  }
}

// ExpertBlock tail  y = lrelu(s):  ds = dy * (y > 0 ? 1 : 0.2).  dy is a tensor, or (last block) the broadcast of the pooled
// gradient: dy(pix, c) = dpool[n][c] * bscale   (bscale = gscale / HW: the mean over positions)
__global__ __launch_bounds__(256) void lo_tb_tail_kernel(const f16* __restrict__ y, const f16* __restrict__ dy, const float* __restrict__ dpool,
                                                         float bscale, f16* __restrict__ ds, int lgc8, size_t nchunk) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;       // 8-channel chunk
  if (i >= nchunk) return;
  const int C = 8 << lgc8, c0 = (int)(i & ((1u << lgc8) - 1)) * 8;
  const size_t n = (i >> lgc8) >> 14;
  const f16x8 yv = *reinterpret_cast<const f16x8*>(y + i * 8);
  f16x8 o;
  if (dy) {
    const f16x8 d = *reinterpret_cast<const f16x8*>(dy + i * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (f16)((float)d[j] * ((float)yv[j] > 0.f ? 1.f : 0.2f));
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (f16)(dpool[n * C + c0 + j] * bscale * ((float)yv[j] > 0.f ? 1.f : 0.2f));
  }
  *reinterpret_cast<f16x8*>(ds + i * 8) = o;
}

// proj_drop backward: dpf = d_a2 * keep (element index (b*HW + pix)*C + c); the rows of image rows 0..7 go to the compact tensor
// dprojc [B][1024][C] (what the proj conv on the compact rows produced); per-block column sums of dpf over ALL positions -> the
// proj bias gradient (every position of proj's output carries the bias)
__global__ __launch_bounds__(256) void lo_tb_projdrop_bwd_kernel(const f16* __restrict__ da2, f16* __restrict__ dprojc, float* __restrict__ partial,
                                                                 int C, LoDropSite ds, uint32_t thr, float inv_keep) {
  __shared__ float s_red[256 * 8];
  const int tid = threadIdx.x, n = blockIdx.y, blk = blockIdx.x;
  const int CC = C >> 3, cc = tid % CC, slot = tid / CC, nslot = 256 / CC, c0 = cc * 8;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  for (int r = slot; r < 256; r += nslot) {
    const int p = blk * 256 + r;
    const size_t pix = (size_t)n * T_HW + p;
    const f16x8 g = *reinterpret_cast<const f16x8*>(da2 + pix * C + c0);
    const uint32_t keep = thr ? lo_drop_keep8(ds, (uint32_t)(pix * (size_t)C + c0), thr) : 0xFFu;
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = ((keep >> j) & 1u) ? (float)g[j] * inv_keep : 0.f;
      o[j] = (f16)v;
      acc[j] += v;
    }
    if (p < 1024) *reinterpret_cast<f16x8*>(dprojc + ((size_t)n * 1024 + p) * C + c0) = o;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) s_red[tid * 8 + j] = acc[j];
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    const int ccx = c >> 3, j = c & 7;
    float tot = 0.f;
    for (int s = 0; s < nslot; ++s) tot += s_red[(s * CC + ccx) * 8 + j];
    partial[((size_t)n * 64 + blk) * C + c] = tot;
  }
}

// Chunk attention as executed (lo_t_attn_generic_kernel), backward.  One workgroup per (sample, chunk): chunks 0..510 have ONE live query
// (token 32*chunk, output row = chunk), chunk 511 has 32 (rows 511..542) -- looped, so every k / v row has one writer.
// thread = (head = tid / 32, key = tid % 32).  The chunk's k | v rows (32 x 2F halves) come in through LDS with 16-byte coalesced loads
// (row pitch + 8 halves: the 32 key lanes of a head read 32 different rows), the gradients dk | dv go back through the same buffer and
// the q gradients through a second one (zero for the tokens that are nobody's query), then the 32 x 3F output rows leave in 16-byte
// coalesced stores.  dO = dattc rows (fp16, scaled like every activation gradient).  (First form: one wave per chunk, a lane owning four
// keys and fetching them with strided global loads, 256 registers: 0.88 ms per launch at batch 64 for 1.6 GB of traffic.)
template <int HD>
__global__ __launch_bounds__(256) void lo_tb_attn_bwd_kernel(const f16* __restrict__ qkv, const f16* __restrict__ dattc, f16* __restrict__ dqkv,
                                                             int B, LoDropSite ds, uint32_t thr, float inv_keep) {
  constexpr int F = 8 * HD, KP = 2 * F + 8, QP = F + 8;
  extern __shared__ __attribute__((aligned(16))) unsigned char tb_smem[];
  f16* skv = reinterpret_cast<f16*>(tb_smem);            // [32][KP]
  f16* sdq = skv + 32 * KP;                              // [32][QP]
  const int tid = threadIdx.x, b = blockIdx.x >> 9, chunk = blockIdx.x & 511;
  const int head = tid >> 5, key = tid & 31;
  const float scale = HD == 16 ? 0.25f : (HD == 32 ? 0.17677669529663687f : 0.125f);
  const f16* base = qkv + ((size_t)b * T_HW + 32 * chunk) * (3 * F);
  f16* dbase = dqkv + ((size_t)b * T_HW + 32 * chunk) * (3 * F);
  constexpr int CK = 2 * F / 8;                          // 16-byte chunks of the k | v part of a row
  for (int i = tid; i < 32 * CK; i += 256) {
    const int r = i / CK, c = i - r * CK;
    *reinterpret_cast<f16x8*>(skv + r * KP + c * 8) = *reinterpret_cast<const f16x8*>(base + (size_t)r * (3 * F) + F + c * 8);
  }
  for (int i = tid; i < 32 * (F / 8); i += 256) {
    const int r = i / (F / 8), c = i - r * (F / 8);
    *reinterpret_cast<f16x8*>(sdq + r * QP + c * 8) = (f16x8){0, 0, 0, 0, 0, 0, 0, 0};
  }
  __syncthreads();
  float kk[HD], vv[HD], dk[HD], dv[HD];
#pragma unroll
  for (int i = 0; i < HD / 8; ++i) {
    const f16x8 k8 = *reinterpret_cast<const f16x8*>(skv + key * KP + head * HD + 8 * i);
    const f16x8 v8 = *reinterpret_cast<const f16x8*>(skv + key * KP + F + head * HD + 8 * i);
#pragma unroll
    for (int d = 0; d < 8; ++d) { kk[8 * i + d] = (float)k8[d]; vv[8 * i + d] = (float)v8[d]; dk[8 * i + d] = 0.f; dv[8 * i + d] = 0.f; }
  }
  const int nq = chunk < 511 ? 1 : 32;
  for (int qi = 0; qi < nq; ++qi) {
    const int p = chunk + qi;                            // output row of this query (token 32 * chunk + qi)
    float q[HD], dO[HD];
#pragma unroll
    for (int i = 0; i < HD / 8; ++i) {
      const f16x8 q8 = *reinterpret_cast<const f16x8*>(base + (size_t)qi * (3 * F) + head * HD + 8 * i);
      const f16x8 o8 = *reinterpret_cast<const f16x8*>(dattc + ((size_t)b * 1024 + p) * F + head * HD + 8 * i);
#pragma unroll
      for (int d = 0; d < 8; ++d) { q[8 * i + d] = (float)q8[d]; dO[8 * i + d] = (float)o8[d]; }
    }
    float sc = 0.f;
#pragma unroll
    for (int d = 0; d < HD; ++d) sc += q[d] * kk[d];
    sc *= scale;                                         // the relative-position term is constant along the keys: no effect on the softmax
    float m = sc;
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    const float e = __expf(sc - m);
    float l = e;
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) l += __shfl_xor(l, o, 64);
    const float pw = e / l;
    float km = 1.f;
    if (thr) {
      const uint32_t idx = ((uint32_t)(b * 543 + p) * 8u + (uint32_t)head) * 32u + (uint32_t)key;
      km = lo_drop_keep(ds, idx, thr) ? inv_keep : 0.f;
    }
    // out = sum_keys (pw km) v:  dv += pw km dO;  dpw = km (dO . v);  softmax backward;  dq = sum_keys dsc k;  dk += dsc q
    float t = 0.f;
    const float w = pw * km;
#pragma unroll
    for (int d = 0; d < HD; ++d) { t += dO[d] * vv[d]; dv[d] += w * dO[d]; }
    const float dpw = t * km;
    float dot = pw * dpw;
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) dot += __shfl_xor(dot, o, 64);
    const float dsc = pw * (dpw - dot) * scale;
#pragma unroll
    for (int d = 0; d < HD; ++d) {
      dk[d] += dsc * q[d];
      float x = dsc * kk[d];
#pragma unroll
      for (int o = 1; o < 32; o <<= 1) x += __shfl_xor(x, o, 64);
      if (key == 0) sdq[qi * QP + head * HD + d] = (f16)x;
    }
  }
  // this thread's k | v slots become dk | dv (nobody else reads or writes them)
#pragma unroll
  for (int i = 0; i < HD / 8; ++i) {
    f16x8 k8, v8;
#pragma unroll
    for (int d = 0; d < 8; ++d) { k8[d] = (f16)dk[8 * i + d]; v8[d] = (f16)dv[8 * i + d]; }
    *reinterpret_cast<f16x8*>(skv + key * KP + head * HD + 8 * i) = k8;
    *reinterpret_cast<f16x8*>(skv + key * KP + F + head * HD + 8 * i) = v8;
  }
  __syncthreads();
  constexpr int CR = 3 * F / 8;                          // 16-byte chunks of an output row
  for (int i = tid; i < 32 * CR; i += 256) {
    const int r = i / CR, c = i - r * CR;
    const f16x8 v = c < F / 8 ? *reinterpret_cast<const f16x8*>(sdq + r * QP + c * 8) : *reinterpret_cast<const f16x8*>(skv + r * KP + (c - F / 8) * 8);
    *reinterpret_cast<f16x8*>(dbase + (size_t)r * (3 * F) + c * 8) = v;
  }
}

// column sums of a [B * HW][C] fp16 tensor (bias gradients), stage 1: partial[(n, blk)][C] over the block's 256 rows; thread =
// (8-channel chunk, row slot) with as many slots as fit 256 threads.  Stage 2: lo_colsum over the B * 64 partial rows.
__global__ __launch_bounds__(256) void lo_tb_colsum_kernel(const f16* __restrict__ x, float* __restrict__ partial, int C) {
  __shared__ float s_red[256 * 8];
  const int tid = threadIdx.x, n = blockIdx.y, blk = blockIdx.x;
  const int CC = C >> 3, nslot = 256 / CC;
  const bool on = tid < nslot * CC;
  const int cc = tid % CC, slot = tid / CC, c0 = cc * 8;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  if (on)
    for (int r = slot; r < 256; r += nslot) {
      const f16x8 g = *reinterpret_cast<const f16x8*>(x + ((size_t)n * T_HW + (size_t)blk * 256 + r) * C + c0);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += (float)g[j];
    }
#pragma unroll
  for (int j = 0; j < 8; ++j) s_red[tid * 8 + j] = acc[j];
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    const int ccx = c >> 3, j = c & 7;
    float tot = 0.f;
    for (int s = 0; s < nslot; ++s) tot += s_red[(s * CC + ccx) * 8 + j];
    partial[((size_t)n * 64 + blk) * C + c] = tot;
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
int tb_bn_backward(TbCtx& c, const TbBnBwd& op) {
  LoTeacher* h = c.h; float* P = c.P; float* G = c.G; void* bws = c.bws;
  const TBnOff& bn = op.bn;
  const float* ls = op.ls; float* dls = op.dls; float* dbias = op.dbias;
  const int C = op.C;
  TbBnArgs a;
  memset(&a, 0, sizeof(a));
  a.din = op.din.p; a.din_pitch = op.din.pitch; a.din_off = op.din.off; a.raw = op.raw.p; a.raw_pitch = op.raw.pitch; a.raw_off = op.raw.off;
  a.mr = op.mr; a.gamma = TP(bn.weight); a.ls = ls; a.coef = TB(float, c.pl.o_coef); a.partial = TB(float, c.pl.o_part);
  a.bpartial = dbias ? TB(float, c.pl.o_part) : nullptr;       // the reduce pass's rows have been consumed by the finalize launch by then
  a.out = op.out.p; a.out_pitch = op.out.pitch; a.out_off = op.out.off; a.C = C; a.act = op.act;
  a.dmode = c.d.on ? op.drop.mode : TB_DROP_NONE; a.ds = c.d.site(op.drop.site); a.thr = c.d.thr; a.inv_keep = c.d.inv_keep;
  a.didx_pitch = op.drop.idx_pitch; a.didx_off = op.drop.idx_off;
  a.ty = op.tail_y; a.tdpool = op.tail_dpool; a.tbscale = c.gscale / (float)T_HW; a.tds = op.tail_ds;
  LO_REQUIRE(C % 8 == 0 && 256 % (C / 8) == 0, "tb_bn_backward: C = %d", C);
  if (!G) {
    // no parameter gradient wanted (frozen only): the layer is one streaming pass
    const bool tail = op.tail_y != nullptr;
    LO_REQUIRE(c.frozen && a.dmode == TB_DROP_NONE && C >= 32, "tb_bn_backward: the pass without parameter gradients is the frozen one (C = %d)", C);
    LO_REQUIRE(!tail || (op.tail_ds && (op.din.p || op.tail_dpool) && op.out.pitch == C && op.raw.pitch == C), "tb_bn_backward: tail arguments");
    LoProfScope _p(tail ? "lo_tb_bn_frozen<tail>" : "lo_tb_bn_frozen", 0, (tail ? 10.0 : 6.0) * h->B * T_HW * C, c.st);
    if (tail) hipLaunchKernelGGL(lo_tb_bn_frozen_kernel<true>, dim3(64, h->B), dim3(256), 0, c.st, a);
    else hipLaunchKernelGGL(lo_tb_bn_frozen_kernel<false>, dim3(64, h->B), dim3(256), 0, c.st, a);
    LO_LAUNCH_CHECK("tb_bn_frozen");
    return LO_OK;
  }
  LO_REQUIRE(!op.tail_y, "tb_bn_backward: the fused tail belongs to the pass without parameter gradients");
  {
    LoProfScope _p("lo_tb_bn_reduce", 0, 4.0 * h->B * T_HW * C, c.st);
    hipLaunchKernelGGL(lo_tb_bn_reduce_kernel, dim3(64, h->B), dim3(256), 0, c.st, a);
  }
  LO_LAUNCH_CHECK("tb_bn_reduce");
  hipLaunchKernelGGL(lo_tb_bn_finalize_kernel, dim3((C + 15) / 16), dim3(256), 0, c.st, a.partial, h->B * 64, C, (float)((size_t)h->B * T_HW),
                     a.gamma, TP(bn.bias), ls, TB(float, c.pl.o_coef), TG(bn.weight), TG(bn.bias), dls, c.inv_g);
  LO_LAUNCH_CHECK("tb_bn_finalize");
  {
    LoProfScope _p("lo_tb_bn_apply", 0, 6.0 * h->B * T_HW * C, c.st);
    if (c.frozen) hipLaunchKernelGGL(lo_tb_bn_apply_kernel<true>, dim3(64, h->B), dim3(256), 0, c.st, a);
    else hipLaunchKernelGGL(lo_tb_bn_apply_kernel<false>, dim3(64, h->B), dim3(256), 0, c.st, a);
  }
  LO_LAUNCH_CHECK("tb_bn_apply");
  if (dbias) LO_TRYT(lo_colsum(TB(float, c.pl.o_part), dbias, h->B * 64, C, C, c.inv_g, c.st));      // bias gradient of the conv in front of the BatchNorm
  return LO_OK;
}

static int tb_colsum16(TbCtx& c, const f16* x, float* out, size_t M, int N) {
  void* bws = c.bws;
  LO_REQUIRE(M == (size_t)c.h->B * T_HW && N % 8 == 0 && N / 8 <= 256, "tb_colsum16: shape");
  {
    LoProfScope _p("lo_tb_colsum", 0, 2.0 * M * N, c.st);
    hipLaunchKernelGGL(lo_tb_colsum_kernel, dim3(64, c.h->B), dim3(256), 0, c.st, x, TB(float, c.pl.o_part), N);
  }
  LO_LAUNCH_CHECK("tb_colsum");
  return lo_colsum(TB(float, c.pl.o_part), out, c.h->B * 64, N, N, c.inv_g, c.st);
}

// the chunk attention's backward: dattc (gradient of the compact attention rows) -> dqkv
static int tb_attn_backward(TbCtx& c, int e, int l, const f16* qkv) {
  void* bws = c.bws; hipStream_t st = c.st;
  const int B = c.h->B, F = c.h->F;
  const dim3 grid(B * 512);
  const LoDropSite dsa = c.d.site(LO_DS_BLOCK(e, l, 1));
  const int lds = (32 * (2 * F + 8) + 32 * (F + 8)) * 2;          // k | v rows + q-gradient rows (feature_dim 512: 98 KB)
  if (lds > 64 * 1024) {
    static bool raised = false;
    if (!raised) { LO_HIP(hipFuncSetAttribute((const void*)lo_tb_attn_bwd_kernel<64>, hipFuncAttributeMaxDynamicSharedMemorySize, lds)); raised = true; }
  }
  {
    LoProfScope _p("lo_tb_attn_bwd", 0, 4.0 * (size_t)B * T_HW * 3 * F, st);
    f16* dattc = TB(f16, c.pl.o_dattc); f16* dqkv = TB(f16, c.pl.o_dqkv);
    if (F == 128) hipLaunchKernelGGL((lo_tb_attn_bwd_kernel<16>), grid, dim3(256), lds, st, qkv, dattc, dqkv, B, dsa, c.d.thr, c.d.inv_keep);
    else if (F == 256) hipLaunchKernelGGL((lo_tb_attn_bwd_kernel<32>), grid, dim3(256), lds, st, qkv, dattc, dqkv, B, dsa, c.d.thr, c.d.inv_keep);
    else hipLaunchKernelGGL((lo_tb_attn_bwd_kernel<64>), grid, dim3(256), lds, st, qkv, dattc, dqkv, B, dsa, c.d.thr, c.d.inv_keep);
  }
  LO_LAUNCH_CHECK("tb_attn_bwd");
  return LO_OK;
}

int tb_block_backward(TbCtx& c, int e, int l, const f16* xin, const f16* y, const f16* dy, const float* dpool, f16* dx_out) {
  LoTeacher* h = c.h; float* P = c.P; float* G = c.G; void* bws = c.bws; hipStream_t st = c.st;
  const TbBlk& b = c.pl.blk[e][l];
  const TBlockOff& k = h->blk[e][l];
  const int B = h->B, F = h->F;
  const size_t px = (size_t)B * T_HW;
  const int lgc8 = F == 128 ? 4 : (F == 256 ? 5 : 6);
  const size_t nchunk = px * (F / 8);
  const bool sc = F != 128 && l == 0;
  f16* dS = TB(f16, c.pl.o_dA);      // ds: gradient of the pre-activation sum = gradient of the identity branch
  f16* dT = TB(f16, c.pl.o_dB);
  f16* dU = TB(f16, c.pl.o_dC);
  // G null (the eval backward for the images' gradient alone): no weight gradient, no bias column sum, and the tail rides in
  // BatchNorm2's single pass
  const bool wg = G != nullptr;
  if (wg) {
    hipLaunchKernelGGL(lo_tb_tail_kernel, dim3((unsigned)((nchunk + 255) / 256)), dim3(256), 0, st, y, dy, dpool, c.gscale / (float)T_HW, dS, lgc8, nchunk);
    LO_LAUNCH_CHECK("tb_tail");
  }
  // BatchNorm2 (+ layer_scale, Dropout2d): dS -> dT = gradient wrt conv2's output
  LO_TRYT(tb_bn_backward(c, {.din = {wg ? dS : dy, F}, .raw = {TB(f16, b.rawB), F}, .mr = TB(float, b.mrB), .bn = k.bn2, .ls = TP(k.layer_scale),
                             .dls = wg ? TG(k.layer_scale) : nullptr, .out = {dT, F}, .C = F, .act = TB_ACT_LRELU,
                             .drop = {TB_DROP_2D, LO_DS_BLOCK(e, l, 3)}, .dbias = wg ? TG(k.conv2_b) : nullptr,
                             .tail_y = wg ? nullptr : y, .tail_dpool = dpool, .tail_ds = dS}));
  if (wg) LO_TAGGED("tb conv2 wgrad", lo_wgrad_run(h->g3b, TB(f16, b.a2), dT, TB(float, c.pl.o_wslab), TG(k.conv2_w), c.inv_g, st));
  LO_TRYT(lo_pack_weight(TP(k.conv2_w), TB(f16, c.pl.o_wd), c.d1b, st));
  LO_TAGGED("tb conv2 dgrad", lo_conv_run(c.d1b, {.in = dT, .w = TB(f16, c.pl.o_wd), .out = dU}, st));     // dU = d a2
  // proj_drop, proj (compact rows)
  if (wg) {
    hipLaunchKernelGGL(lo_tb_projdrop_bwd_kernel, dim3(64, B), dim3(256), 0, st, dU, TB(f16, c.pl.o_dprojc), TB(float, c.pl.o_part), F,
                       c.d.site(LO_DS_BLOCK(e, l, 2)), c.d.thr, c.d.inv_keep);
    LO_LAUNCH_CHECK("tb_projdrop_bwd");
    LO_TRYT(lo_colsum(TB(float, c.pl.o_part), TG(k.proj_b), B * 64, F, F, c.inv_g, st));
    LO_TAGGED("tb proj wgrad", lo_wgrad_run(h->gpc, TB(f16, b.attc), TB(f16, c.pl.o_dprojc), TB(float, c.pl.o_wslab), TG(k.proj_w), c.inv_g, st));
  } else {
    // no bias gradient and (frozen) no mask: what is left of the pass is the copy of each sample's first 1024 rows to the compact tensor
    LO_REQUIRE(!c.d.on, "tb_block_backward: the backward without parameter gradients has no dropout");
    LO_HIP(hipMemcpy2DAsync(TB(f16, c.pl.o_dprojc), (size_t)1024 * F * 2, dU, (size_t)T_HW * F * 2, (size_t)1024 * F * 2, B, hipMemcpyDeviceToDevice, st));
  }
  LO_TRYT(lo_transpose_cast(TP(k.proj_w), TB(f16, c.pl.o_wt), F, F, st));
  LO_TAGGED("tb proj dgrad", lo_conv_run(c.dpc, {.in = TB(f16, c.pl.o_dprojc), .w = TB(f16, c.pl.o_wt), .out = TB(f16, c.pl.o_dattc)}, st));
  LO_TRYT(tb_attn_backward(c, e, l, TB(f16, b.qkv)));
  // qkv conv
  if (wg) {
    LO_TRYT(tb_colsum16(c, TB(f16, c.pl.o_dqkv), TG(k.qkv_b), px, 3 * F));
    LO_TAGGED("tb qkv wgrad", lo_wgrad_run(h->gqF, TB(f16, b.bnA), TB(f16, c.pl.o_dqkv), TB(float, c.pl.o_wslab), TG(k.qkv_w), c.inv_g, st));
  }
  LO_TRYT(lo_transpose_cast(TP(k.qkv_w), TB(f16, c.pl.o_wt), 3 * F, F, st));
  LO_TAGGED("tb qkv dgrad", lo_conv_run(c.dq, {.in = TB(f16, c.pl.o_dqkv), .w = TB(f16, c.pl.o_wt), .out = dU}, st));      // dU = d a1
  // Dropout2d, BatchNorm1: dU -> dT = gradient wrt conv1's output
  LO_TRYT(tb_bn_backward(c, {.din = {dU, F}, .raw = {TB(f16, b.rawA), F}, .mr = TB(float, b.mrA), .bn = k.bn1, .out = {dT, F}, .C = F,
                             .act = TB_ACT_LRELU, .drop = {TB_DROP_2D, LO_DS_BLOCK(e, l, 0)}, .dbias = wg ? TG(k.conv1_b) : nullptr}));
  const LoGeom& g1 = l == 0 ? h->g3a : h->g3b;
  const LoGeom& d1 = l == 0 ? c.d1a : c.d1b;
  if (wg) LO_TAGGED("tb conv1 wgrad", lo_wgrad_run(g1, xin, dT, TB(float, c.pl.o_wslab), TG(k.conv1_w), c.inv_g, st));
  LO_TRYT(lo_pack_weight(TP(k.conv1_w), TB(f16, c.pl.o_wd), d1, st));
  if (!sc) {
    LO_TAGGED("tb conv1 dgrad", lo_conv_run(d1, {.in = dT, .w = TB(f16, c.pl.o_wd), .add_src = dS, .out = dx_out}, st));    // + the identity branch
  } else {
    // shortcut = BatchNorm(Conv1x1(x)): dS -> gradient wrt the shortcut conv's output (no activation), its parameters, then both data gradients
    LO_TAGGED("tb conv1 dgrad", lo_conv_run(d1, {.in = dT, .w = TB(f16, c.pl.o_wd), .out = dU}, st));
    LO_TRYT(tb_bn_backward(c, {.din = {dS, F}, .raw = {TB(f16, b.scraw), F}, .mr = TB(float, b.mrS), .bn = k.bn_sc, .out = {dT, F}, .C = F,
                               .dbias = wg ? TG(k.sc_b) : nullptr}));
    if (wg) LO_TAGGED("tb shortcut wgrad", lo_wgrad_run(h->gsc, xin, dT, TB(float, c.pl.o_wslab), TG(k.sc_w), c.inv_g, st));
    LO_TRYT(lo_transpose_cast(TP(k.sc_w), TB(f16, c.pl.o_wt), F, 128, st));
    LO_TAGGED("tb shortcut dgrad", lo_conv_run(c.dsc, {.in = dT, .w = TB(f16, c.pl.o_wt), .add_src = dU, .out = dx_out}, st));
  }
  return LO_OK;
}
