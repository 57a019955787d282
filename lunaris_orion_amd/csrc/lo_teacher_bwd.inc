// Full backward of LunarMoETeacher (SURVEY §8 row F2, second half): gradients for the experts and the feature extractor as well,
// i.e. what the reference's teacher loss produces when its three `torch.utils.checkpoint.checkpoint` calls
// (lunar_evaluator.py:194-197, 266-275, 411-414) are non-reentrant.  Textually included at the end of lo_teacher.hip (same
// translation unit: LoTeacher, the forward kernels and the launch helpers are file-local there).
//
// Shape of the computation = the reference's own under checkpointing: the trunk is RECOMPUTED block by block from the block inputs
// (plain form: every tensor of the block exists, nothing folded), then differentiated.
//   pass 1  feature extractor and the 12 ExpertBlocks again, BatchNorm with batch statistics but WITHOUT touching the running
//           statistics (lo_bn_finalize training = 2; the forward of the same step has moved them), keeping x_{e,l} for every block;
//   pass 2  heads backward (existing kernel, now also d loss / d pooled features), then per expert, blocks 2..0: recompute the
//           block from x_{e,l} into scratch, backward through tail, BatchNorm2, conv2, proj_drop, proj, the chunk attention as
//           executed (543 live rows), qkv, Dropout2d, BatchNorm1, conv1 (+ shortcut conv / BatchNorm when feature_dim != 128);
//   pass 3  feature extractor backward (fusion, Dropout, three depthwise + pointwise branches, conv1).
// Activation gradients are fp16 multiplied by `gscale` (a power of two chosen by the host: the gradient of a mean over 16384
// positions of a loss of order 1/B underflows fp16 otherwise); parameter gradients are fp32, unscaled, written to their slots of
// the teacher's flat gradient buffer (layout = the state table, like lo_teacher_heads_backward).
// Heavy contractions reuse the VAE path's kernels: lo_conv_run (3x3 data gradients as LO_CONV3_S1_DGRAD, 1x1 data gradients as
// LO_LINEAR on transposed weights) and lo_wgrad_run (weight gradients).  Everything else is below: simple, HBM-bound passes.

// ---------------------------------------------------------------------------------------------
// BatchNorm(train) backward, per channel over (N, H, W):   y = (r - mean) * rstd * gamma + beta,  r = LeakyReLU(conv) (or conv)
//   upstream:  g(pix, c) = din(pix, c) * keep(...)            (Dropout2d: per (sample, channel); Dropout: per element; none)
//   dn = ls[c] * g          (ls = the block's layer_scale on the tail, else 1)
//   S1 = sum g, S2 = sum g * xhat                              (reduce kernel: partial rows, fixed order)
//   dbeta = ls S1, dgamma = ls S2, dls = gamma S2 + beta S1    (finalize)
//   dr = gamma rstd (dn - ls S1 / N - xhat ls S2 / N);  dconv = dr * (r > 0 ? 1 : 0.2)   (apply)
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
};
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
    k1[j] = a.coef[(c0 + j) * 2]; k2[j] = a.coef[(c0 + j) * 2 + 1];
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
      float d = gr[j] * (lsv[j] * ((float)g[j] * k) - k1[j] - xh * k2[j]);
      if (a.act && !(rv > 0.f)) d *= 0.2f;
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
// out = a + b (+ dpool broadcast): fp16 tensors of n8 8-element chunks
__global__ __launch_bounds__(256) void lo_tb_add_kernel(const f16* __restrict__ a, const f16* __restrict__ b, const float* __restrict__ dpool,
                                                        float bscale, f16* __restrict__ out, int lgc8, size_t nchunk) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nchunk) return;
  const int C = 8 << lgc8, c0 = (int)(i & ((1u << lgc8) - 1)) * 8;
  const size_t n = (i >> lgc8) >> 14;
  const f16x8 av = *reinterpret_cast<const f16x8*>(a + i * 8);
  f16x8 bv = {0, 0, 0, 0, 0, 0, 0, 0};
  if (b) bv = *reinterpret_cast<const f16x8*>(b + i * 8);
  f16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float v = (float)av[j] + (float)bv[j];
    if (dpool) v += dpool[n * C + c0 + j] * bscale;
    o[j] = (f16)v;
  }
  *reinterpret_cast<f16x8*>(out + i * 8) = o;
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

// ---- feature extractor pieces ---------------------------------------------------------------------------------
// pointwise conv 32 -> 64 backward (Cin = 32 is below the GEMM kernels' tile): thread = (pixel, 8 input channels) for the data
// gradient; the weight gradient as per-block partial sums [blk][64][32] (then lo_colsum)
__global__ __launch_bounds__(256) void lo_tb_pw_dgrad_kernel(const f16* __restrict__ dy, int dy_pitch, int dy_off, const float* __restrict__ w,
                                                             f16* __restrict__ dx, size_t npix) {
  __shared__ float ws[64][32];
  for (int i = threadIdx.x; i < 64 * 32; i += 256) ws[i >> 5][i & 31] = w[i];
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t pix = i >> 2;
  if (pix >= npix) return;
  const int c0 = (int)(i & 3) * 8;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  for (int o = 0; o < 64; o += 8) {
    const f16x8 g = *reinterpret_cast<const f16x8*>(dy + pix * dy_pitch + dy_off + o);
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += (float)g[u] * ws[o + u][c0 + j];
  }
  f16x8 out;
#pragma unroll
  for (int j = 0; j < 8; ++j) out[j] = (f16)acc[j];
  *reinterpret_cast<f16x8*>(dx + pix * 32 + c0) = out;
}
// partial[blk][co][ci] = sum over the block's 1024 pixels of dy[pix][co] * x[pix][ci];  thread = (co, 8 ci)
__global__ __launch_bounds__(256) void lo_tb_pw_wgrad_kernel(const f16* __restrict__ dy, int dy_pitch, int dy_off, const f16* __restrict__ x,
                                                             float* __restrict__ partial) {
  __shared__ float sx[64][32], sd[64][64];
  const int tid = threadIdx.x, co = tid >> 2, c0 = (tid & 3) * 8;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  const size_t p0 = (size_t)blockIdx.x * 1024;
  for (int t = 0; t < 16; ++t) {
    __syncthreads();
    for (int i = tid; i < 64 * 32; i += 256) sx[i >> 5][i & 31] = (float)x[(p0 + t * 64 + (i >> 5)) * 32 + (i & 31)];
    for (int i = tid; i < 64 * 64; i += 256) sd[i >> 6][i & 63] = (float)dy[(p0 + t * 64 + (i >> 6)) * dy_pitch + dy_off + (i & 63)];
    __syncthreads();
    for (int r = 0; r < 64; ++r) {
      const float g = sd[r][co];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += g * sx[r][c0 + j];
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) partial[(size_t)blockIdx.x * 2048 + co * 32 + c0 + j] = acc[j];
}
// depthwise KxK backward.  Forward: out[p][c] = bias[c] + sum_t w[c][t] n0[p + t][c] (zero padding of n0 = BN(raw32)).
//   data gradient (accumulated over the three branches by the caller: add != null): dn0[p][c] = sum_t w[c][t] dout[p - t][c]
//   weight gradient: partial[blk = image row][c][t] = sum over the row's pixels of dout[p][c] * n0[p + t][c]
template <int K>
__global__ __launch_bounds__(256) void lo_tb_dw_dgrad_kernel(const f16* __restrict__ dout, const float* __restrict__ w, const f16* __restrict__ add,
                                                             f16* __restrict__ dn0) {
  __shared__ float ws[K * K][32];
  for (int i = threadIdx.x; i < K * K * 32; i += 256) ws[i / 32][i % 32] = w[(i % 32) * K * K + i / 32];
  __syncthreads();
  constexpr int P = K / 2;
  const int n = blockIdx.y, yy = blockIdx.x;
  for (int i = threadIdx.x; i < 128 * 4; i += 256) {
    const int xx = i >> 2, c0 = (i & 3) * 8;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int r = 0; r < K; ++r) {
      const int oy = yy - (r - P);
      if ((unsigned)oy >= 128u) continue;
      for (int s = 0; s < K; ++s) {
        const int ox = xx - (s - P);
        if ((unsigned)ox >= 128u) continue;
        const f16x8 g = *reinterpret_cast<const f16x8*>(dout + (((size_t)n * 128 + oy) * 128 + ox) * 32 + c0);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += (float)g[j] * ws[r * K + s][c0 + j];
      }
    }
    const size_t o = (((size_t)n * 128 + yy) * 128 + xx) * 32 + c0;
    f16x8 out;
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = (f16)(acc[j] + (add ? (float)add[o + j] : 0.f));
    *reinterpret_cast<f16x8*>(dn0 + o) = out;
  }
}
template <int K>
__global__ __launch_bounds__(256) void lo_tb_dw_wgrad_kernel(const f16* __restrict__ dout, const f16* __restrict__ raw, const float* __restrict__ ss,
                                                             float* __restrict__ partial, float* __restrict__ bpartial) {
  // block = (image row, sample); thread = (channel c = tid & 31, tap group); n0 = raw * scale + shift inside the image, 0 outside
  __shared__ float red[8][32];
  constexpr int P = K / 2;
  const int n = blockIdx.y, yy = blockIdx.x, c = threadIdx.x & 31, tg = threadIdx.x >> 5;      // 8 tap groups
  const float sc = ss[c * 2], sh = ss[c * 2 + 1];
  float* dst = partial + ((size_t)n * 128 + yy) * 32 * K * K;
  for (int t = tg; t < K * K; t += 8) {
    const int r = t / K, s = t - r * K;
    const int iy = yy + r - P;
    float acc = 0.f;
    if ((unsigned)iy < 128u)
      for (int xx = 0; xx < 128; ++xx) {
        const int ix = xx + s - P;
        if ((unsigned)ix >= 128u) continue;
        acc += (float)dout[(((size_t)n * 128 + yy) * 128 + xx) * 32 + c] * ((float)raw[(((size_t)n * 128 + iy) * 128 + ix) * 32 + c] * sc + sh);
      }
    dst[c * K * K + t] = acc;
  }
  // bias gradient: sum of dout over the row
  float b = 0.f;
  for (int xx = tg; xx < 128; xx += 8) b += (float)dout[(((size_t)n * 128 + yy) * 128 + xx) * 32 + c];
  red[tg][c] = b;
  __syncthreads();
  if (tg == 0) {
    float t = 0.f;
    for (int k = 0; k < 8; ++k) t += red[k][c];
    bpartial[((size_t)n * 128 + yy) * 32 + c] = t;
  }
}
// conv1 (3 -> 32, 3x3) weight gradient: partial[(n, row)][co][27] = sum over the row of dconv[p][co] * x[ci][p + tap]; bias likewise
__global__ __launch_bounds__(256) void lo_tb_conv1_wgrad_kernel(const float* __restrict__ x, const f16* __restrict__ dc, float* __restrict__ partial,
                                                                float* __restrict__ bpartial) {
  __shared__ float xs[3][3][130];
  __shared__ float ds[128][33];
  const int tid = threadIdx.x, yy = blockIdx.x, n = blockIdx.y;
  for (int i = tid; i < 3 * 3 * 130; i += 256) {
    const int col = i % 130, r = (i / 130) % 3, ci = i / (3 * 130);
    const int iy = yy - 1 + r, ix = col - 1;
    xs[ci][r][col] = ((unsigned)iy < 128u && (unsigned)ix < 128u) ? x[(((size_t)n * 3 + ci) * 128 + iy) * 128 + ix] : 0.f;
  }
  for (int i = tid; i < 128 * 32; i += 256) ds[i >> 5][i & 31] = (float)dc[(((size_t)n * 128 + yy) * 128 + (i >> 5)) * 32 + (i & 31)];
  __syncthreads();
  for (int o = tid; o < 32 * 27; o += 256) {
    const int co = o / 27, t = o - co * 27, ci = t / 9, r = (t % 9) / 3, s = t % 3;
    float acc = 0.f;
    for (int xx = 0; xx < 128; ++xx) acc += ds[xx][co] * xs[ci][r][xx + s];
    partial[((size_t)n * 128 + yy) * 864 + o] = acc;
  }
  if (tid < 32) {
    float b = 0.f;
    for (int xx = 0; xx < 128; ++xx) b += ds[xx][tid];
    bpartial[((size_t)n * 128 + yy) * 32 + tid] = b;
  }
}
// The Dropout between the branch BatchNorms and the fusion conv needs no pass of its own, nor does the 192-channel gradient have to be
// split: the BatchNorm backward kernels read the pitch-192 tensor with a channel offset and replay the element-wise mask (dmode 2).
// dst[pix][64] = src[pix][192 pitch][off..off+64): dense copies of the fusion conv's INPUT for its three weight-gradient GEMMs
__global__ __launch_bounds__(256) void lo_tb_slice64_kernel(const f16* __restrict__ src, int off, f16* __restrict__ dst, size_t nchunk) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nchunk) return;
  *reinterpret_cast<f16x8*>(dst + i * 8) = *reinterpret_cast<const f16x8*>(src + (i >> 3) * 192 + off + (i & 7) * 8);
}
// W[128][192] columns [off, off+64) <- tmp[128][64]
__global__ void lo_tb_scatter_cols_kernel(const float* __restrict__ tmp, float* __restrict__ w, int off) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 128 * 64) w[(i >> 6) * 192 + off + (i & 63)] = tmp[i];
}
// transposed fp16 slice of a weight: dst[r][c] = (f16) src[c * ld + roff + r]   (R x Ccols)  -- operand of a 1x1 data gradient
__global__ void lo_tb_wt_kernel(const float* __restrict__ src, f16* __restrict__ dst, int R, int Ccols, int ld, int roff) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < R * Ccols) { const int r = i / Ccols, c = i - r * Ccols; dst[i] = (f16)src[(size_t)c * ld + roff + r]; }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// the tensors of one ExpertBlock that its backward reads (plain form).  saved plan: one set per block, filled once by the forward
// (lo_teacher_forward_keep) or by the backward's own first pass; otherwise ONE shared set, refilled in front of every block's backward
struct TbBlk { size_t rawA, bnA, qkv, attc, projc, a2, rawB, scraw, mrA, mrB, mrS, ssS; };
struct TbPlan {
  size_t o_raw32, o_dwb[3], o_cat, o_catd, o_rawF, o_feat, o_xs[8][3];
  bool saved;
  TbBlk blk[8][3];
  size_t o_mr[8], o_ssx[4];                  // feature extractor: (mean, rstd) tables 3 conv1, 4..6 branches, 7 fusion; o_ssx[3] = conv1's (scale, shift)
  size_t o_dA, o_dB, o_dC, o_dqkv, o_dattc, o_dprojc, o_dfeat, o_dcat, o_d32a, o_d32b;
  size_t o_part, o_bpart, o_coef, o_wslab, o_wd, o_wt, o_tmpw, o_dpool_f, o_dpool_e, o_cat64;
  size_t bytes;
};
static void tb_plan(const LoTeacher* h, TbPlan* p) {
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t r = off; off += (bytes + 255) & ~(size_t)255; return r; };
  const size_t px = (size_t)h->B * T_HW, F = (size_t)h->F;
  // every block's tensors kept (nothing is ever recomputed) while that fits comfortably: 8 F-channel tensors per block, 12 blocks --
  // 26 GB at batch 64 / feature_dim 128, 103 GB at 512; above 160 GB one shared set and a recomputation per block
  p->saved = (double)px * (double)F * 2.0 * 8.0 * 3.0 * (double)h->E <= 160.0e9;
  p->o_raw32 = take(px * 32 * 2);
  for (int b = 0; b < 3; ++b) p->o_dwb[b] = take(px * 32 * 2);
  p->o_cat = take(px * 192 * 2); p->o_catd = take(px * 192 * 2);
  p->o_rawF = take(px * 128 * 2); p->o_feat = take(px * 128 * 2);
  for (int e = 0; e < h->E; ++e) for (int l = 0; l < 3; ++l) p->o_xs[e][l] = take(px * F * 2);
  auto take_blk = [&](int l) {
    TbBlk b;
    b.rawA = take(px * F * 2); b.bnA = take(px * F * 2); b.qkv = take(px * 3 * F * 2);
    b.attc = take((size_t)h->B * 1024 * F * 2); b.projc = take((size_t)h->B * 1024 * F * 2);
    b.a2 = take(px * F * 2); b.rawB = take(px * F * 2); b.scraw = take((F != 128 && l == 0) ? px * F * 2 : 256);
    b.mrA = take(512 * 2 * 4); b.mrB = take(512 * 2 * 4); b.mrS = take(512 * 2 * 4); b.ssS = take(512 * 2 * 4);
    return b;
  };
  if (p->saved) {
    for (int e = 0; e < h->E; ++e) for (int l = 0; l < 3; ++l) p->blk[e][l] = take_blk(l);
  } else {
    const TbBlk shared = take_blk(0);
    for (int e = 0; e < h->E; ++e) for (int l = 0; l < 3; ++l) p->blk[e][l] = shared;
  }
  for (int k = 0; k < 8; ++k) p->o_mr[k] = take(512 * 2 * 4);
  for (int k = 0; k < 4; ++k) p->o_ssx[k] = take(512 * 2 * 4);
  p->o_dA = take(px * F * 2); p->o_dB = take(px * F * 2); p->o_dC = take(px * F * 2);
  p->o_dqkv = take(px * 3 * F * 2);
  p->o_dattc = take((size_t)h->B * 1024 * F * 2); p->o_dprojc = take((size_t)h->B * 1024 * F * 2);
  p->o_dfeat = take(px * 128 * 2); p->o_dcat = take(px * 192 * 2); p->o_d32a = take(px * 32 * 2); p->o_d32b = take(px * 32 * 2);
  p->o_cat64 = take(px * 64 * 2);
  p->o_part = take((size_t)h->B * 128 * 864 * 4 > (size_t)h->B * 64 * F * 2 * 4 ? (size_t)h->B * 128 * 864 * 4 : (size_t)h->B * 64 * F * 2 * 4);
  p->o_bpart = take((size_t)h->B * 128 * 32 * 4);
  p->o_coef = take(512 * 2 * 4);
  size_t slab = 0;
  auto ws_of = [&](int kind, int H, int W, int ci, int co) {
    LoGeom g;
    if (lo_make_geom(&g, kind, h->B, H, W, ci, co) == LO_OK) { const size_t b = lo_wgrad_slab_bytes(g); if (b > slab) slab = b; }
  };
  ws_of(LO_CONV3_S1, 128, 128, 128, (int)F); ws_of(LO_CONV3_S1, 128, 128, (int)F, (int)F);
  ws_of(LO_LINEAR, 128, 128, (int)F, 3 * (int)F); ws_of(LO_LINEAR, 8, 128, (int)F, (int)F); ws_of(LO_LINEAR, 128, 128, 128, (int)F);
  ws_of(LO_LINEAR, 128, 128, 64, 128);
  p->o_wslab = take(slab + 256);
  p->o_wd = take(F * 9 * F * 2);                 // packed data-gradient weights of a 3x3 conv
  p->o_wt = take(3 * F * F * 2);                 // transposed 1x1 weights
  p->o_tmpw = take(128 * 64 * 4);
  p->o_dpool_f = take((size_t)h->B * 128 * 4); p->o_dpool_e = take((size_t)h->E * h->B * F * 4);
  p->bytes = off;
}
extern "C" size_t lo_teacher_full_backward_bytes(const LoTeacher* h) {
  if (!h) return 0;
  TbPlan p;
  tb_plan(h, &p);
  return p.bytes;
}

#define TB(T, o) reinterpret_cast<T*>(reinterpret_cast<unsigned char*>(bws) + (o))
#define TG(name) (G + h->off[t_idx(h, name)])

struct TbCtx {
  LoTeacher* h; float* P; void* ws; void* bws; float* G; hipStream_t st; TbPlan pl;
  bool drop; uint32_t thr; float inv_keep; uint64_t seed; float gscale, inv_g;
  LoGeom g1a, g1b, gq, gpc, gsc;          // forward geometries of a block: conv 128->F, conv F->F, qkv, proj on the compact rows, shortcut
  LoGeom d1a, d1b, dq, dpc, dsc;          // their data gradients
};
static LoDropSite tb_site(const TbCtx& c, uint32_t s) { return lo_drop_site_keys(c.seed, s); }

// BatchNorm backward of one layer: upstream din -> gradient wrt the conv output (out), parameter gradients into G
static int tb_bn_backward(TbCtx& c, const f16* din, int din_pitch, int din_off, const f16* raw, int raw_pitch, int raw_off, const float* mr,
                          const std::string& bn, const float* ls, float* dls, f16* out, int out_pitch, int out_off, int C, int act, int dmode,
                          uint32_t site, int didx_pitch, int didx_off, float* dbias = nullptr) {
  LoTeacher* h = c.h; float* P = c.P; float* G = c.G; void* bws = c.bws;
  TbBnArgs a;
  memset(&a, 0, sizeof(a));
  a.din = din; a.din_pitch = din_pitch; a.din_off = din_off; a.raw = raw; a.raw_pitch = raw_pitch; a.raw_off = raw_off; a.mr = mr;
  a.gamma = TP(bn + ".weight"); a.ls = ls; a.coef = TB(float, c.pl.o_coef); a.partial = TB(float, c.pl.o_part);
  a.bpartial = dbias ? TB(float, c.pl.o_part) : nullptr;       // the reduce pass's rows have been consumed by the finalize launch by then
  a.out = out; a.out_pitch = out_pitch; a.out_off = out_off; a.C = C; a.act = act;
  a.dmode = (c.drop && dmode) ? dmode : 0; a.ds = tb_site(c, site); a.thr = c.drop ? c.thr : 0; a.inv_keep = c.inv_keep;
  a.didx_pitch = didx_pitch; a.didx_off = didx_off;
  LO_REQUIRE(C % 8 == 0 && 256 % (C / 8) == 0, "tb_bn_backward: C = %d", C);
  {
    LoProfScope _p("lo_tb_bn_reduce", 0, 4.0 * h->B * T_HW * C, c.st);
    hipLaunchKernelGGL(lo_tb_bn_reduce_kernel, dim3(64, h->B), dim3(256), 0, c.st, a);
  }
  LO_LAUNCH_CHECK("tb_bn_reduce");
  hipLaunchKernelGGL(lo_tb_bn_finalize_kernel, dim3((C + 15) / 16), dim3(256), 0, c.st, a.partial, h->B * 64, C, (float)((size_t)h->B * T_HW),
                     a.gamma, TP(bn + ".bias"), ls, TB(float, c.pl.o_coef), TG(bn + ".weight"), TG(bn + ".bias"), dls, c.inv_g);
  LO_LAUNCH_CHECK("tb_bn_finalize");
  {
    LoProfScope _p("lo_tb_bn_apply", 0, 6.0 * h->B * T_HW * C, c.st);
    hipLaunchKernelGGL(lo_tb_bn_apply_kernel, dim3(64, h->B), dim3(256), 0, c.st, a);
  }
  LO_LAUNCH_CHECK("tb_bn_apply");
  if (dbias) LO_TRYT(lo_colsum(TB(float, c.pl.o_part), dbias, h->B * 64, C, C, c.inv_g, c.st));      // bias gradient of the conv in front of the BatchNorm
  return LO_OK;
}

// ExpertBlock (e, l) in plain form from xin into the block's tensor set; xout = the block output (null: not wanted).
// train: 1 = the step's forward (running statistics move), 2 = a recomputation (they do not).  pool_partial: column sums of xout
static int tb_block_forward(TbCtx& c, int e, int l, const f16* xin, f16* xout, int train, float* pool_partial) {
  LoTeacher* h = c.h; float* P = c.P; void* ws = c.ws; void* bws = c.bws; hipStream_t st = c.st;
  const TbBlk& b = c.pl.blk[e][l];
  const int B = h->B, F = h->F;
  const size_t px = (size_t)B * T_HW;
  std::string p = "experts." + std::to_string(e) + "." + std::to_string(l);
  float* bnp = TW(float, h->o_bnp);
  LoConvExtra ex{1, bnp};
  const LoGeom& g1 = (l == 0) ? c.g1a : c.g1b;
  const bool sc = F != 128 && l == 0;
  if (sc) {
    LoConvExtra exs{0, bnp};
    LO_TAGGED("tb shortcut (igemm)", lo_conv_run(c.gsc, xin, TW(f16, h->o_wsc[e]), TP(p + ".shortcut.0.bias"), nullptr, TB(f16, b.scraw), nullptr, nullptr, 1, st, nullptr, &exs));
    LO_TRYT(t_bn_finalize(h, bnp, lo_conv_bn_rows(c.gsc), F, p + ".shortcut.1", P, ws, train, st, 1, 1, nullptr, TB(float, b.ssS), TB(float, b.mrS)));
  }
  LO_TAGGED("tb conv1 (recompute)", lo_conv_run(g1, xin, TW(f16, h->o_wp3[e][l][0]), TP(p + ".conv1.0.bias"), nullptr, TB(f16, b.rawA), nullptr, nullptr, 1, st, nullptr, &ex));
  LO_TRYT(t_bn_finalize(h, bnp, lo_conv_bn_rows(g1), F, p + ".conv1.2", P, ws, train, st, 1, 1, nullptr, nullptr, TB(float, b.mrA)));
  if (c.drop) {
    hipLaunchKernelGGL(lo_t_drop2d_ss_kernel, dim3((B * F + 255) / 256), dim3(256), 0, st, TW(float, h->o_ss), TW(float, h->o_ssb), B, F,
                       tb_site(c, LO_DS_BLOCK(e, l, 0)), c.thr, c.inv_keep);
    LO_LAUNCH_CHECK("t_drop2d_ss");
  }
  LO_TRYT(t_bn_apply(h, TB(f16, b.rawA), nullptr, nullptr, TB(f16, b.bnA), F, F, 0, 0, nullptr, ws, st, nullptr, c.drop));
  LO_TAGGED("tb qkv (recompute)", lo_conv_run(c.gq, TB(f16, b.bnA), TW(f16, h->o_wqkv[e][l]), TP(p + ".attention.qkv.bias"), nullptr, TB(f16, b.qkv), nullptr, nullptr, 1, st));
  {
    const dim3 grid((B * 543 + 3) / 4);
    const LoDropSite dsa = tb_site(c, LO_DS_BLOCK(e, l, 1));
    const uint32_t thr = c.drop ? c.thr : 0u;
    if (F == 128) hipLaunchKernelGGL((lo_t_attn_generic_kernel<16>), grid, dim3(256), 0, st, TB(f16, b.qkv), TB(f16, b.attc), B, dsa, thr, c.inv_keep);
    else if (F == 256) hipLaunchKernelGGL((lo_t_attn_generic_kernel<32>), grid, dim3(256), 0, st, TB(f16, b.qkv), TB(f16, b.attc), B, dsa, thr, c.inv_keep);
    else hipLaunchKernelGGL((lo_t_attn_generic_kernel<64>), grid, dim3(256), 0, st, TB(f16, b.qkv), TB(f16, b.attc), B, dsa, thr, c.inv_keep);
  }
  LO_LAUNCH_CHECK("t_attn_generic");
  LO_TAGGED("tb proj (recompute)", lo_conv_run(c.gpc, TB(f16, b.attc), TW(f16, h->o_wproj[e][l]), TP(p + ".attention.proj.bias"), nullptr, TB(f16, b.projc), nullptr, nullptr, 1, st));
  {
    const size_t nchunk = px * (F / 8);
    const LoDropSite dsp = tb_site(c, LO_DS_BLOCK(e, l, 2));
    const uint32_t thr = c.drop ? c.thr : 0u;
    const dim3 grid((unsigned)((nchunk + 255) / 256));
#define LO_TB_PD(LG) hipLaunchKernelGGL((lo_t_projdrop_kernel<LG>), grid, dim3(256), 0, st, TB(f16, b.projc), TP(p + ".attention.proj.bias"), \
                                        TB(f16, b.a2), (uint8_t*)nullptr, nchunk, dsp, thr, c.inv_keep)
    if (F == 128) LO_TB_PD(4); else if (F == 256) LO_TB_PD(5); else LO_TB_PD(6);
#undef LO_TB_PD
  }
  LO_LAUNCH_CHECK("t_projdrop");
  LO_TAGGED("tb conv2 (recompute)", lo_conv_run(c.g1b, TB(f16, b.a2), TW(f16, h->o_wp3[e][l][1]), TP(p + ".conv2.0.bias"), nullptr, TB(f16, b.rawB), nullptr, nullptr, 1, st, nullptr, &ex));
  LO_TRYT(t_bn_finalize(h, bnp, lo_conv_bn_rows(c.g1b), F, p + ".conv2.2", P, ws, train, st, 1, 1, nullptr, nullptr, TB(float, b.mrB)));
  if (c.drop) {
    hipLaunchKernelGGL(lo_t_drop2d_ss_kernel, dim3((B * F + 255) / 256), dim3(256), 0, st, TW(float, h->o_ss), TW(float, h->o_ssb), B, F,
                       tb_site(c, LO_DS_BLOCK(e, l, 3)), c.thr, c.inv_keep);
    LO_LAUNCH_CHECK("t_drop2d_ss");
  }
  if (xout || pool_partial)
    LO_TRYT(t_bn_apply(h, TB(f16, b.rawB), TP(p + ".layer_scale"), sc ? TB(f16, b.scraw) : xin, xout, F, F, 0, 1, pool_partial, ws, st, nullptr, c.drop,
                       nullptr, sc ? TB(float, b.ssS) : nullptr));
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

// backward of ExpertBlock (e, l): scratch holds its recomputation; y = the block output, dy / dpool = its gradient.
// dx_out = gradient wrt the block input (conv1's data gradient + the identity branch's)
static int tb_block_backward(TbCtx& c, int e, int l, const f16* xin, const f16* y, const f16* dy, const float* dpool, f16* dx_out) {
  LoTeacher* h = c.h; float* P = c.P; float* G = c.G; void* bws = c.bws; hipStream_t st = c.st;
  const TbBlk& b = c.pl.blk[e][l];
  const int B = h->B, F = h->F;
  const size_t px = (size_t)B * T_HW;
  const int lgc8 = F == 128 ? 4 : (F == 256 ? 5 : 6);
  const size_t nchunk = px * (F / 8);
  std::string p = "experts." + std::to_string(e) + "." + std::to_string(l);
  const bool sc = F != 128 && l == 0;
  f16* dS = TB(f16, c.pl.o_dA);      // ds: gradient of the pre-activation sum = gradient of the identity branch
  f16* dT = TB(f16, c.pl.o_dB);
  f16* dU = TB(f16, c.pl.o_dC);
  hipLaunchKernelGGL(lo_tb_tail_kernel, dim3((unsigned)((nchunk + 255) / 256)), dim3(256), 0, st, y, dy, dpool, c.gscale / (float)T_HW, dS, lgc8, nchunk);
  LO_LAUNCH_CHECK("tb_tail");
  // BatchNorm2 (+ layer_scale, Dropout2d): dS -> dT = gradient wrt conv2's output
  LO_TRYT(tb_bn_backward(c, dS, F, 0, TB(f16, b.rawB), F, 0, TB(float, b.mrB), p + ".conv2.2", TP(p + ".layer_scale"), TG(p + ".layer_scale"),
                         dT, F, 0, F, 1, 1, LO_DS_BLOCK(e, l, 3), 0, 0, TG(p + ".conv2.0.bias")));
  LO_TAGGED("tb conv2 wgrad", lo_wgrad_run(c.g1b, TB(f16, b.a2), dT, TB(float, c.pl.o_wslab), TG(p + ".conv2.0.weight"), c.inv_g, st));
  LO_TRYT(lo_pack_weight(TP(p + ".conv2.0.weight"), TB(f16, c.pl.o_wd), c.d1b, st));
  LO_TAGGED("tb conv2 dgrad", lo_conv_run(c.d1b, dT, TB(f16, c.pl.o_wd), nullptr, nullptr, dU, nullptr, nullptr, 1, st));     // dU = d a2
  // proj_drop, proj (compact rows)
  {
    const LoDropSite dsp = tb_site(c, LO_DS_BLOCK(e, l, 2));
    hipLaunchKernelGGL(lo_tb_projdrop_bwd_kernel, dim3(64, B), dim3(256), 0, st, dU, TB(f16, c.pl.o_dprojc), TB(float, c.pl.o_part), F, dsp,
                       c.drop ? c.thr : 0u, c.inv_keep);
    LO_LAUNCH_CHECK("tb_projdrop_bwd");
    LO_TRYT(lo_colsum(TB(float, c.pl.o_part), TG(p + ".attention.proj.bias"), B * 64, F, F, c.inv_g, st));
  }
  LO_TAGGED("tb proj wgrad", lo_wgrad_run(c.gpc, TB(f16, b.attc), TB(f16, c.pl.o_dprojc), TB(float, c.pl.o_wslab), TG(p + ".attention.proj.weight"), c.inv_g, st));
  LO_TRYT(lo_transpose_cast(TP(p + ".attention.proj.weight"), TB(f16, c.pl.o_wt), F, F, st));
  LO_TAGGED("tb proj dgrad", lo_conv_run(c.dpc, TB(f16, c.pl.o_dprojc), TB(f16, c.pl.o_wt), nullptr, nullptr, TB(f16, c.pl.o_dattc), nullptr, nullptr, 1, st));
  // attention
  {
    const dim3 grid(B * 512);
    const LoDropSite dsa = tb_site(c, LO_DS_BLOCK(e, l, 1));
    const uint32_t thr = c.drop ? c.thr : 0u;
    const int lds = (32 * (2 * F + 8) + 32 * (F + 8)) * 2;          // k | v rows + q-gradient rows (feature_dim 512: 98 KB)
    if (lds > 64 * 1024) {
      static bool raised = false;
      if (!raised) { LO_HIP(hipFuncSetAttribute((const void*)lo_tb_attn_bwd_kernel<64>, hipFuncAttributeMaxDynamicSharedMemorySize, lds)); raised = true; }
    }
    LoProfScope _p("lo_tb_attn_bwd", 0, 4.0 * px * 3 * F, st);
    if (F == 128) hipLaunchKernelGGL((lo_tb_attn_bwd_kernel<16>), grid, dim3(256), lds, st, TB(f16, b.qkv), TB(f16, c.pl.o_dattc), TB(f16, c.pl.o_dqkv), B, dsa, thr, c.inv_keep);
    else if (F == 256) hipLaunchKernelGGL((lo_tb_attn_bwd_kernel<32>), grid, dim3(256), lds, st, TB(f16, b.qkv), TB(f16, c.pl.o_dattc), TB(f16, c.pl.o_dqkv), B, dsa, thr, c.inv_keep);
    else hipLaunchKernelGGL((lo_tb_attn_bwd_kernel<64>), grid, dim3(256), lds, st, TB(f16, b.qkv), TB(f16, c.pl.o_dattc), TB(f16, c.pl.o_dqkv), B, dsa, thr, c.inv_keep);
  }
  LO_LAUNCH_CHECK("tb_attn_bwd");
  // qkv conv
  LO_TRYT(tb_colsum16(c, TB(f16, c.pl.o_dqkv), TG(p + ".attention.qkv.bias"), px, 3 * F));
  LO_TAGGED("tb qkv wgrad", lo_wgrad_run(c.gq, TB(f16, b.bnA), TB(f16, c.pl.o_dqkv), TB(float, c.pl.o_wslab), TG(p + ".attention.qkv.weight"), c.inv_g, st));
  LO_TRYT(lo_transpose_cast(TP(p + ".attention.qkv.weight"), TB(f16, c.pl.o_wt), 3 * F, F, st));
  LO_TAGGED("tb qkv dgrad", lo_conv_run(c.dq, TB(f16, c.pl.o_dqkv), TB(f16, c.pl.o_wt), nullptr, nullptr, dU, nullptr, nullptr, 1, st));      // dU = d a1
  // Dropout2d, BatchNorm1: dU -> dT = gradient wrt conv1's output
  LO_TRYT(tb_bn_backward(c, dU, F, 0, TB(f16, b.rawA), F, 0, TB(float, b.mrA), p + ".conv1.2", nullptr, nullptr, dT, F, 0, F, 1, 1,
                         LO_DS_BLOCK(e, l, 0), 0, 0, TG(p + ".conv1.0.bias")));
  const LoGeom& g1 = l == 0 ? c.g1a : c.g1b;
  const LoGeom& d1 = l == 0 ? c.d1a : c.d1b;
  LO_TAGGED("tb conv1 wgrad", lo_wgrad_run(g1, xin, dT, TB(float, c.pl.o_wslab), TG(p + ".conv1.0.weight"), c.inv_g, st));
  LO_TRYT(lo_pack_weight(TP(p + ".conv1.0.weight"), TB(f16, c.pl.o_wd), d1, st));
  if (!sc) {
    LO_TAGGED("tb conv1 dgrad", lo_conv_run(d1, dT, TB(f16, c.pl.o_wd), nullptr, dS, dx_out, nullptr, nullptr, 1, st));    // + the identity branch
  } else {
    // shortcut = BatchNorm(Conv1x1(x)): dS -> gradient wrt the shortcut conv's output (no activation), its parameters, then both data gradients
    LO_TAGGED("tb conv1 dgrad", lo_conv_run(d1, dT, TB(f16, c.pl.o_wd), nullptr, nullptr, dU, nullptr, nullptr, 1, st));
    LO_TRYT(tb_bn_backward(c, dS, F, 0, TB(f16, b.scraw), F, 0, TB(float, b.mrS), p + ".shortcut.1", nullptr, nullptr, dT, F, 0, F, 0, 0, 0, 0, 0,
                           TG(p + ".shortcut.0.bias")));
    LO_TAGGED("tb shortcut wgrad", lo_wgrad_run(c.gsc, xin, dT, TB(float, c.pl.o_wslab), TG(p + ".shortcut.0.weight"), c.inv_g, st));
    LO_TRYT(lo_transpose_cast(TP(p + ".shortcut.0.weight"), TB(f16, c.pl.o_wt), F, 128, st));
    LO_TAGGED("tb shortcut dgrad", lo_conv_run(c.dsc, dT, TB(f16, c.pl.o_wt), nullptr, dU, dx_out, nullptr, nullptr, 1, st));
  }
  return LO_OK;
}

// feature extractor: recomputation (keeps every tensor its backward reads) ...
static int tb_fe_forward(TbCtx& c, const float* x, int train, float* pool_partial) {
  LoTeacher* h = c.h; float* P = c.P; void* ws = c.ws; void* bws = c.bws; hipStream_t st = c.st;
  const int B = h->B;
  const size_t px = (size_t)B * T_HW;
  float* bnp = TW(float, h->o_bnp);
  LoConvExtra ex{1, bnp};
  std::string fe = "feature_extractor";
  hipLaunchKernelGGL(lo_t_conv1_kernel, dim3(128, B), dim3(256), 0, st, x, TP(fe + ".conv1.0.weight"), TP(fe + ".conv1.0.bias"), TB(f16, c.pl.o_raw32), bnp);
  LO_LAUNCH_CHECK("t_conv1");
  float* ss32 = TB(float, c.pl.o_ssx[3]);
  LO_TRYT(t_bn_finalize(h, bnp, B * 128, 32, fe + ".conv1.2", P, ws, train, st, 1, 1, nullptr, ss32, TB(float, c.pl.o_mr[3])));
  const char* brs[3] = {"edge_branch", "color_branch", "detail_branch"};
  for (int b = 0; b < 3; ++b) {
    std::string q = fe + "." + brs[b];
    if (b == 1) hipLaunchKernelGGL((lo_t_dwconv_kernel<5>), dim3(32, B), dim3(256), 0, st, TB(f16, c.pl.o_raw32), ss32, TP(q + ".0.weight"), TP(q + ".0.bias"), TB(f16, c.pl.o_dwb[b]), B);
    else hipLaunchKernelGGL((lo_t_dwconv_kernel<3>), dim3(32, B), dim3(256), 0, st, TB(f16, c.pl.o_raw32), ss32, TP(q + ".0.weight"), TP(q + ".0.bias"), TB(f16, c.pl.o_dwb[b]), B);
    LO_LAUNCH_CHECK("t_dwconv");
    LoConvExtra exb{1, bnp, 192, 64 * b};
    LO_TRYT(lo_conv_run(h->gpw, TB(f16, c.pl.o_dwb[b]), TW(f16, h->o_wpw[b]), TP(q + ".1.bias"), nullptr, TB(f16, c.pl.o_cat), nullptr, nullptr, 1, st, nullptr, &exb));
    const int mt = (int)(px / lo_conv_tile_m(h->gpw));
    LO_TRYT(t_bn_finalize(h, bnp, mt, 64, q + ".3", P, ws, train, st, 1, 1, nullptr, TW(float, h->o_ss_cat) + 128 * b, TB(float, c.pl.o_mr[4 + b])));
  }
  // catd = Dropout(BN(cat)) (thr 0: BatchNorm only); the kernel works in place: copy first
  LO_HIP(hipMemcpyAsync(TB(void, c.pl.o_catd), TB(void, c.pl.o_cat), px * 192 * 2, hipMemcpyDeviceToDevice, st));
  {
    const size_t nchunk = px * 24;
    hipLaunchKernelGGL(lo_t_cat_bn_drop_kernel, dim3((unsigned)((nchunk + 255) / 256)), dim3(256), 0, st, TB(f16, c.pl.o_catd), TW(float, h->o_ss_cat),
                       nchunk, tb_site(c, LO_DS_FE), c.drop ? c.thr : 0u, c.inv_keep);
  }
  LO_LAUNCH_CHECK("t_cat_bn_drop");
  LO_TRYT(lo_conv_run(h->gfus, TB(f16, c.pl.o_catd), TW(f16, h->o_wfus), TP(fe + ".fusion.0.bias"), nullptr, TB(f16, c.pl.o_rawF), nullptr, nullptr, 1, st, nullptr, &ex));
  LO_TRYT(t_bn_finalize(h, bnp, (int)(px / lo_conv_tile_m(h->gfus)), 128, fe + ".fusion.2", P, ws, train, st, 1, 1, nullptr, nullptr, TB(float, c.pl.o_mr[7])));
  LO_TRYT(t_bn_apply(h, TB(f16, c.pl.o_rawF), nullptr, nullptr, TB(f16, c.pl.o_feat), 128, 128, 0, 0, pool_partial, ws, st));
  return LO_OK;
}
// ... and backward, from dfeat (gradient wrt the features, scaled); dx (NULL = not wanted): the gradient wrt the images
static int tb_fe_backward(TbCtx& c, const float* x, float* dx) {
  LoTeacher* h = c.h; float* P = c.P; float* G = c.G; void* bws = c.bws; hipStream_t st = c.st;
  const int B = h->B;
  const size_t px = (size_t)B * T_HW;
  std::string fe = "feature_extractor";
  f16* dcf = TB(f16, c.pl.o_dA);                   // gradient wrt the fusion conv's output [pix][128]
  LO_TRYT(tb_bn_backward(c, TB(f16, c.pl.o_dfeat), 128, 0, TB(f16, c.pl.o_rawF), 128, 0, TB(float, c.pl.o_mr[7]), fe + ".fusion.2", nullptr, nullptr,
                         dcf, 128, 0, 128, 1, 0, 0, 0, 0, TG(fe + ".fusion.0.bias")));
  // fusion conv 192 -> 128 as three 64-channel slices (the GEMM kernels want power-of-two channel counts)
  LoGeom g64, d64;
  LO_TRYT(lo_make_geom(&g64, LO_LINEAR, B, 128, 128, 64, 128));
  LO_TRYT(lo_make_geom(&d64, LO_LINEAR, B, 128, 128, 128, 64));
  for (int b = 0; b < 3; ++b) {
    const size_t nchunk = px * 8;
    hipLaunchKernelGGL(lo_tb_slice64_kernel, dim3((unsigned)((nchunk + 255) / 256)), dim3(256), 0, st, TB(f16, c.pl.o_catd), 64 * b, TB(f16, c.pl.o_cat64), nchunk);
    LO_LAUNCH_CHECK("tb_slice64");
    LO_TAGGED("tb fusion wgrad", lo_wgrad_run(g64, TB(f16, c.pl.o_cat64), dcf, TB(float, c.pl.o_wslab), TB(float, c.pl.o_tmpw), c.inv_g, st));
    hipLaunchKernelGGL(lo_tb_scatter_cols_kernel, dim3(32), dim3(256), 0, st, TB(float, c.pl.o_tmpw), TG(fe + ".fusion.0.weight"), 64 * b);
    LO_LAUNCH_CHECK("tb_scatter_cols");
    // data gradient of the slice: dcat[pix][64 b + ci] = sum_co dcf[pix][co] W[co][64 b + ci]  (operand [ci][co], written at its channel offset)
    hipLaunchKernelGGL(lo_tb_wt_kernel, dim3((64 * 128 + 255) / 256), dim3(256), 0, st, TP(fe + ".fusion.0.weight"), TB(f16, c.pl.o_wt), 64, 128, 192, 64 * b);
    LO_LAUNCH_CHECK("tb_wt");
    LoConvExtra exd{0, nullptr, 192, 64 * b};
    LO_TAGGED("tb fusion dgrad", lo_conv_run(d64, dcf, TB(f16, c.pl.o_wt), nullptr, nullptr, TB(f16, c.pl.o_dcat), nullptr, nullptr, 1, st, nullptr, &exd));
  }
  const char* brs[3] = {"edge_branch", "color_branch", "detail_branch"};
  f16* dpw = TB(f16, c.pl.o_cat64);               // gradient wrt a pointwise conv's output [pix][64]
  f16* ddw = TB(f16, c.pl.o_d32a);                // gradient wrt a depthwise conv's output [pix][32]
  f16* dn0 = TB(f16, c.pl.o_d32b);                // gradient wrt BN(conv1) [pix][32], summed over the branches
  const float* ss32 = TB(float, c.pl.o_ssx[3]);
  for (int b = 0; b < 3; ++b) {
    std::string q = fe + "." + brs[b];
    const int K = b == 1 ? 5 : 3;
    // Dropout (element index pix * 192 + 64 b + c), BatchNorm of the branch, LeakyReLU
    LO_TRYT(tb_bn_backward(c, TB(f16, c.pl.o_dcat), 192, 64 * b, TB(f16, c.pl.o_cat), 192, 64 * b, TB(float, c.pl.o_mr[4 + b]), q + ".3", nullptr, nullptr,
                           dpw, 64, 0, 64, 1, 2, LO_DS_FE, 192, 64 * b, TG(q + ".1.bias")));
    hipLaunchKernelGGL(lo_tb_pw_wgrad_kernel, dim3((unsigned)(px / 1024)), dim3(256), 0, st, dpw, 64, 0, TB(f16, c.pl.o_dwb[b]), TB(float, c.pl.o_part));
    LO_LAUNCH_CHECK("tb_pw_wgrad");
    LO_TRYT(lo_colsum(TB(float, c.pl.o_part), TG(q + ".1.weight"), (int)(px / 1024), 2048, 2048, c.inv_g, st));
    hipLaunchKernelGGL(lo_tb_pw_dgrad_kernel, dim3((unsigned)((px * 4 + 255) / 256)), dim3(256), 0, st, dpw, 64, 0, TP(q + ".1.weight"), ddw, px);
    LO_LAUNCH_CHECK("tb_pw_dgrad");
    if (K == 5) {
      hipLaunchKernelGGL((lo_tb_dw_wgrad_kernel<5>), dim3(128, B), dim3(256), 0, st, ddw, TB(f16, c.pl.o_raw32), ss32, TB(float, c.pl.o_part), TB(float, c.pl.o_bpart));
      LO_LAUNCH_CHECK("tb_dw_wgrad");
      hipLaunchKernelGGL((lo_tb_dw_dgrad_kernel<5>), dim3(128, B), dim3(256), 0, st, ddw, TP(q + ".0.weight"), b ? dn0 : (const f16*)nullptr, dn0);
    } else {
      hipLaunchKernelGGL((lo_tb_dw_wgrad_kernel<3>), dim3(128, B), dim3(256), 0, st, ddw, TB(f16, c.pl.o_raw32), ss32, TB(float, c.pl.o_part), TB(float, c.pl.o_bpart));
      LO_LAUNCH_CHECK("tb_dw_wgrad");
      hipLaunchKernelGGL((lo_tb_dw_dgrad_kernel<3>), dim3(128, B), dim3(256), 0, st, ddw, TP(q + ".0.weight"), b ? dn0 : (const f16*)nullptr, dn0);
    }
    LO_LAUNCH_CHECK("tb_dw_dgrad");
    LO_TRYT(lo_colsum(TB(float, c.pl.o_part), TG(q + ".0.weight"), B * 128, 32 * K * K, 32 * K * K, c.inv_g, st));
    LO_TRYT(lo_colsum(TB(float, c.pl.o_bpart), TG(q + ".0.bias"), B * 128, 32, 32, c.inv_g, st));
  }
  // BatchNorm + LeakyReLU of conv1, then its weight gradient and -- for a caller whose images require grad -- its data gradient
  LO_TRYT(tb_bn_backward(c, dn0, 32, 0, TB(f16, c.pl.o_raw32), 32, 0, TB(float, c.pl.o_mr[3]), fe + ".conv1.2", nullptr, nullptr, ddw, 32, 0, 32, 1, 0, 0, 0, 0));
  hipLaunchKernelGGL(lo_tb_conv1_wgrad_kernel, dim3(128, B), dim3(256), 0, st, x, ddw, TB(float, c.pl.o_part), TB(float, c.pl.o_bpart));
  LO_LAUNCH_CHECK("tb_conv1_wgrad");
  LO_TRYT(lo_colsum(TB(float, c.pl.o_part), TG(fe + ".conv1.0.weight"), B * 128, 864, 864, c.inv_g, st));
  LO_TRYT(lo_colsum(TB(float, c.pl.o_bpart), TG(fe + ".conv1.0.bias"), B * 128, 32, 32, c.inv_g, st));
  if (dx) LO_TRYT(lo_image_dgrad(ddw, 32, 1, TP(fe + ".conv1.0.weight"), B, c.inv_g, dx, st));
  return LO_OK;
}

static int tb_ctx_init(TbCtx& c, LoTeacher* h, float* P, void* ws, void* bws, float* grads, float drop_p, uint64_t drop_seed, float gscale, void* stream) {
  c.h = h; c.P = P; c.ws = ws; c.bws = bws; c.G = grads; c.st = reinterpret_cast<hipStream_t>(stream);
  tb_plan(h, &c.pl);
  c.drop = drop_p > 0.f; c.seed = drop_seed;
  c.thr = c.drop ? (uint32_t)lrintf(drop_p * 65536.f) : 0u;
  if (c.drop && c.thr == 0) c.thr = 1;
  c.inv_keep = c.drop ? 1.0f / (1.0f - drop_p) : 1.0f;
  c.gscale = gscale; c.inv_g = 1.0f / gscale;
  const int B = h->B, F = h->F;
  LO_TRYT(lo_make_geom(&c.g1a, LO_CONV3_S1, B, 128, 128, 128, F));
  LO_TRYT(lo_make_geom(&c.g1b, LO_CONV3_S1, B, 128, 128, F, F));
  LO_TRYT(lo_make_geom(&c.gq, LO_LINEAR, B, 128, 128, F, 3 * F));
  LO_TRYT(lo_make_geom(&c.gpc, LO_LINEAR, B, 8, 128, F, F));
  LO_TRYT(lo_make_geom(&c.gsc, LO_LINEAR, B, 128, 128, 128, F));
  LO_TRYT(lo_make_geom(&c.d1a, LO_CONV3_S1_DGRAD, B, 128, 128, F, 128));
  LO_TRYT(lo_make_geom(&c.d1b, LO_CONV3_S1_DGRAD, B, 128, 128, F, F));
  LO_TRYT(lo_make_geom(&c.dq, LO_LINEAR, B, 128, 128, 3 * F, F));
  LO_TRYT(lo_make_geom(&c.dpc, LO_LINEAR, B, 8, 128, F, F));
  LO_TRYT(lo_make_geom(&c.dsc, LO_LINEAR, B, 128, 128, F, 128));
  return LO_OK;
}
// the compact attention rows >= 543 of every sample are never written: zero them once per call
static int tb_zero_attc(TbCtx& c) {
  void* bws = c.bws;
  const size_t bytes = (size_t)c.h->B * 1024 * c.h->F * 2;
  for (int e = 0; e < (c.pl.saved ? c.h->E : 1); ++e)
    for (int l = 0; l < (c.pl.saved ? 3 : 1); ++l) LO_HIP(hipMemsetAsync(TB(void, c.pl.blk[e][l].attc), 0, bytes, c.st));
  return LO_OK;
}
// the trunk in plain form: feature extractor and the 12 blocks, every block's output (and, with a saved plan, every tensor its backward
// reads) left inside bws.  train 1: the step's forward (pooled features for the heads, running statistics move); 2: the backward's own pass
static int tb_trunk_forward(TbCtx& c, const float* x, int train) {
  LoTeacher* h = c.h; void* ws = c.ws; void* bws = c.bws;
  const int B = h->B, F = h->F;
  float* poolp = train == 1 ? TW(float, h->o_poolp) : nullptr;
  LO_TRYT(tb_fe_forward(c, x, train, poolp));
  if (train == 1) LO_TRYT(t_pool(h, TW(float, h->o_pool_f), 128, ws, c.st));
  const f16* feat = TB(f16, c.pl.o_feat);
  for (int e = 0; e < h->E; ++e) {
    for (int l = 0; l < 3; ++l)
      LO_TRYT(tb_block_forward(c, e, l, l ? TB(f16, c.pl.o_xs[e][l - 1]) : feat, TB(f16, c.pl.o_xs[e][l]), train, l == 2 ? poolp : nullptr));
    if (train == 1) LO_TRYT(t_pool(h, TW(float, h->o_pool_e) + (size_t)e * B * F, F, ws, c.st));
  }
  return LO_OK;
}

// The forward of a step that ends in lo_teacher_full_backward(..., the same bws): LunarMoETeacher.forward in train mode (same outputs and
// side effects as lo_teacher_forward(training = 1): BatchNorm running statistics, pooled features and logits for the heads' backward) in
// plain form, every tensor the backward reads left inside bws -- the backward then recomputes nothing.  (Values differ from the folded
// feature_dim-128 paths of lo_teacher_forward at the fp16 rounding level, like any two of that function's paths.)
extern "C" int lo_teacher_forward_keep(LoTeacher* h, const float* x, float* P, void* ws, void* bws, float dropout_p, uint64_t drop_seed,
                                       float* quality, float* weights, float* style, float* prompt, float* semantic, void* stream) {
  LO_REQUIRE(h && x && P && ws && bws && quality && weights && style && prompt && semantic, "lo_teacher_forward_keep: null argument");
  LO_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "lo_teacher_forward_keep: dropout_p %g outside [0, 1)", (double)dropout_p);
  TbCtx c;
  LO_TRYT(tb_ctx_init(c, h, P, ws, bws, nullptr, dropout_p, drop_seed, 1.0f, stream));
  h->kept = false; h->kept_bws = nullptr;
  h->last_p = c.drop ? dropout_p : 0.f; h->last_seed = drop_seed; h->last_path = c.drop ? 2 : 1;
  LO_TRYT(tb_zero_attc(c));
  LO_TRYT(tb_trunk_forward(c, x, 1));
  LO_TRYT(t_run_heads(h, P, ws, quality, weights, style, prompt, semantic, c.drop ? c.thr : 0u, c.inv_keep, drop_seed, c.st));
  h->kept = true; h->kept_bws = bws;
  return LO_OK;
}

// coef = quality_weight / accum (like lo_teacher_heads_backward).  Must follow lo_teacher_forward(training = 1) on the same batch
// with the same dropout_p / drop_seed (h->last_*): the heads' backward reads that call's pooled features.  gscale: power of two by
// which the fp16 activation gradients are multiplied (parameter gradients come out unscaled).  rows: [B][head range] scratch of
// lo_teacher_heads_backward.  grads: the teacher's flat gradient buffer (state-table layout); every parameter on the loss path is
// written, everything else is zeroed.
static int tb_full_backward_impl(LoTeacher* h, const float* x, float* P, void* ws, void* bws, const float* pooled_f, const float* pooled_e,
                                 const float* raw_q, const float* expert_weights, const float* dq_up, const float* dw_up, float coef,
                                 float drop_p, uint64_t drop_seed, float gscale, float* rows, float* grads, float* dx, void* stream) {
  LO_REQUIRE(h && x && P && ws && bws && expert_weights && rows && grads, "lo_teacher_full_backward: null argument");
  LO_REQUIRE(gscale > 0.f, "lo_teacher_full_backward: gscale must be positive");
  LO_REQUIRE(h->last_path >= 0, "lo_teacher_full_backward: no forward has run on this engine");
  TbCtx c;
  LO_TRYT(tb_ctx_init(c, h, P, ws, bws, grads, drop_p, drop_seed, gscale, stream));
  hipStream_t st = c.st;
  float* G = grads;
  const int B = h->B, F = h->F, E = h->E;
  const size_t px = (size_t)B * T_HW;
  LO_HIP(hipMemsetAsync(G, 0, h->flat_elems * sizeof(float), st));
  // heads: their own parameter gradients + d loss / d pooled features
  LO_TRYT(t_heads_backward(h, P, pooled_f, pooled_e, raw_q, expert_weights, dq_up, dw_up, coef, drop_p, drop_seed, rows, grads, st,
                           TB(float, c.pl.o_dpool_f), TB(float, c.pl.o_dpool_e)));
  // pass 1: the trunk again in plain form -- unless the forward of this step was lo_teacher_forward_keep on this bws
  const bool kept = h->kept && h->kept_bws == bws && h->last_seed == drop_seed && h->last_p == drop_p;
  h->kept = false; h->kept_bws = nullptr;
  if (!kept) {
    LO_TRYT(tb_zero_attc(c));
    LO_TRYT(tb_trunk_forward(c, x, 2));
  }
  const bool recompute = !c.pl.saved;          // one shared tensor set: every block is recomputed in front of its backward
  const f16* feat = TB(f16, c.pl.o_feat);
  // pass 2: experts, last block first
  const size_t nchunk128 = px * 16;
  for (int e = 0; e < E; ++e) {
    for (int l = 2; l >= 0; --l) {
      const f16* xin = l ? TB(f16, c.pl.o_xs[e][l - 1]) : feat;
      if (recompute) LO_TRYT(tb_block_forward(c, e, l, xin, nullptr, 2, nullptr));
      f16* dx = l ? TB(f16, c.pl.o_dC) : (e == 0 ? TB(f16, c.pl.o_dfeat) : TB(f16, c.pl.o_dqkv));
      LO_TRYT(tb_block_backward(c, e, l, xin, TB(f16, c.pl.o_xs[e][l]), l == 2 ? (const f16*)nullptr : TB(f16, c.pl.o_dC),
                                l == 2 ? TB(float, c.pl.o_dpool_e) + (size_t)e * B * F : (const float*)nullptr, dx));
    }
    if (e > 0 || e == E - 1) {
      // dfeat += this expert's share (e > 0); the last pass also adds the gate's pooled gradient, spread over the positions
      hipLaunchKernelGGL(lo_tb_add_kernel, dim3((unsigned)((nchunk128 + 255) / 256)), dim3(256), 0, st, TB(f16, c.pl.o_dfeat),
                         e > 0 ? TB(f16, c.pl.o_dqkv) : (const f16*)nullptr, e == E - 1 ? TB(float, c.pl.o_dpool_f) : (const float*)nullptr,
                         c.gscale / (float)T_HW, TB(f16, c.pl.o_dfeat), 4, nchunk128);
      LO_LAUNCH_CHECK("tb_add");
    }
  }
  // pass 3: feature extractor
  return tb_fe_backward(c, x, dx);
}

// clip_grad_norm_ + AdamW over the teacher's parameters in the full-backward mode (train_hybrid.py:914, 922 with every parameter
// live).  The norm is taken over the whole flat gradient buffer (lo_teacher_full_backward zeroes what is not a gradient); the
// update runs over the contiguous runs of tensors that HAVE a gradient in the reference -- not over BatchNorm buffers (weight
// decay would shrink the running statistics) and not over the three heads the loss does not read (their .grad is None in the
// reference, so its optimizer skips them, decay included).  m / v: flat_elems floats each.  scratch: 1028 floats.
static bool tb_has_grad(const std::string& k) {
  auto ends = [&](const char* s) { const size_t n = strlen(s); return k.size() >= n && k.compare(k.size() - n, n, s) == 0; };
  if (ends("running_mean") || ends("running_var") || ends("num_batches_tracked") || ends("last_spatial_shapes") || ends("rel_pos_cache")) return false;
  return k.compare(0, 14, "semantic_head.") != 0 && k.compare(0, 10, "style_net.") != 0 && k.compare(0, 11, "prompt_net.") != 0;
}
extern "C" int lo_teacher_clip_adamw_full(LoTeacher* h, float* P, const float* G, float* M, float* V, float max_norm, float lr, float beta1,
                                          float beta2, float eps, float weight_decay, int step, float* scratch, void* stream) {
  LO_REQUIRE(h && P && G && M && V && scratch, "lo_teacher_clip_adamw_full: null argument");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LO_TRYT(lo_gradnorm(G, h->flat_elems, max_norm, scratch, scratch + 1024, st));
  size_t run_b = 0, run_e = 0;
  auto flush = [&]() -> int {
    if (run_e > run_b) return lo_adamw(P + run_b, G + run_b, M + run_b, V + run_b, run_e - run_b, scratch + 1024, lr, beta1, beta2, eps, weight_decay, step, st);
    return LO_OK;
  };
  for (size_t i = 0; i < h->names.size(); ++i) {
    if (!h->is_float[i] || !tb_has_grad(h->names[i])) continue;
    const size_t b = h->off[i], e = b + h->numel[i];
    // tensors start on aligned offsets: a gap between two live tensors is padding (zero gradient, zero parameter) and may ride along
    bool adjacent = run_e > run_b && b >= run_e && b - run_e < 64;
    if (adjacent) {
      for (size_t j = 0; j < h->names.size() && adjacent; ++j)
        if (h->is_float[j] && h->off[j] >= run_e && h->off[j] < b) adjacent = false;     // another tensor sits in between
    }
    if (adjacent) { run_e = e; continue; }
    LO_TRYT(flush());
    run_b = b; run_e = e;
  }
  return flush();
}
// how many parameter tensors / elements lo_teacher_clip_adamw_full updates (tests, logging)
extern "C" int lo_teacher_full_param_count(const LoTeacher* h, size_t* tensors, size_t* elems) {
  LO_REQUIRE(h && tensors && elems, "lo_teacher_full_param_count: null argument");
  *tensors = 0; *elems = 0;
  for (size_t i = 0; i < h->names.size(); ++i)
    if (h->is_float[i] && tb_has_grad(h->names[i])) { ++*tensors; *elems += h->numel[i]; }
  return LO_OK;
}

extern "C" int lo_teacher_full_backward(LoTeacher* h, const float* x, float* P, void* ws, void* bws, const float* expert_weights, float coef,
                                        float gscale, float* rows, float* grads, void* stream) {
  LO_REQUIRE(h && ws, "lo_teacher_full_backward: null argument");
  return tb_full_backward_impl(h, x, P, ws, bws, TW(float, h->o_pool_f), TW(float, h->o_pool_e), TW(float, h->o_rawq), expert_weights, nullptr, nullptr,
                               coef, h->last_p, h->last_seed, gscale, rows, grads, nullptr, stream);
}
// The same backward for arbitrary upstream gradients of quality_scores [B][4] / expert_weights [B][E] (either may be NULL), with the
// head inputs, dropout_p and call seed of the forward being differentiated passed explicitly (lo_teacher_heads_saved: a caller may
// have run other forwards since) -- what the module's autograd node calls (LunarMoETeacher(full_backward=True)).  The images must be
// the ones of that forward.  Upstream gradients should be of order 1 (the caller normalises a foreign loss scale: lo_grad_scale_pick).
// lo_teacher_full_backward_dx also writes the gradient wrt the images, fp32 NCHW [B,3,128,128] (NULL = not wanted), from the same pass.
extern "C" int lo_teacher_full_backward_dx(LoTeacher* h, const float* x, float* P, void* ws, void* bws, const float* pooled_f, const float* pooled_e,
                                           const float* raw_q, const float* expert_weights, const float* d_quality, const float* d_weights,
                                           float dropout_p, uint64_t drop_seed, float gscale, float* rows, float* grads, float* dx, void* stream) {
  LO_REQUIRE(pooled_f && pooled_e && raw_q && (d_quality || d_weights), "lo_teacher_full_backward_ex: null argument");
  return tb_full_backward_impl(h, x, P, ws, bws, pooled_f, pooled_e, raw_q, expert_weights, d_quality, d_weights, 0.f, dropout_p, drop_seed, gscale,
                               rows, grads, dx, stream);
}
extern "C" int lo_teacher_full_backward_ex(LoTeacher* h, const float* x, float* P, void* ws, void* bws, const float* pooled_f, const float* pooled_e,
                                           const float* raw_q, const float* expert_weights, const float* d_quality, const float* d_weights,
                                           float dropout_p, uint64_t drop_seed, float gscale, float* rows, float* grads, void* stream) {
  return lo_teacher_full_backward_dx(h, x, P, ws, bws, pooled_f, pooled_e, raw_q, expert_weights, d_quality, d_weights, dropout_p, drop_seed,
                                     gscale, rows, grads, nullptr, stream);
}
