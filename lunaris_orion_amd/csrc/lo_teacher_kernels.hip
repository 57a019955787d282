// Teacher kernels that every path shares, and their host launchers (lo_teacher.h): the first conv 3->32 (direct), BatchNorm finalize
// (batch or running statistics, running-stat update) and apply (+ concat / + layer-scale, identity, LeakyReLU block tail), global average
// pooling, the depthwise 3x3 / 5x5 convs with BatchNorm-on-load, the chunk-local attention for any feature_dim, the dropout glue and
// the fold of the branch BatchNorms into the fusion conv.  The 3x3 and 1x1 convolutions run on lo_igemm_nt with the teacher epilogue
// (bias + LeakyReLU + per-channel BatchNorm partial sums).
#include "lo_teacher.h"

// ---------------------------------------------------------------------------------------------
// first conv: x fp32 NCHW [B,3,128,128] -> lrelu(conv3x3 s1 p1 + bias) fp16 NHWC [B,128,128,32]; BN partials per image row
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lo_t_conv1_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bias, f16* __restrict__ out,
                                                         float* __restrict__ bn_partial) {
  __shared__ float xs[3][3][T_W + 2];
  __shared__ float ws[27][32];
  __shared__ float red[256][2];
  const int tid = threadIdx.x, oy = blockIdx.x, n = blockIdx.y;
  for (int i = tid; i < 3 * 3 * (T_W + 2); i += 256) {
    int col = i % (T_W + 2), r = (i / (T_W + 2)) % 3, ci = i / (3 * (T_W + 2));
    int iy = oy - 1 + r, ix = col - 1;
    float v = 0.f;
    if ((unsigned)iy < 128u && (unsigned)ix < 128u) v = x[(((size_t)n * 3 + ci) * 128 + iy) * 128 + ix];
    xs[ci][r][col] = v;
  }
  for (int i = tid; i < 27 * 32; i += 256) ws[i / 32][i % 32] = w[(i % 32) * 27 + i / 32];
  __syncthreads();
  const int px = tid >> 1, cg = tid & 1;
  float acc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = bias[cg * 16 + j];
#pragma unroll
  for (int ci = 0; ci < 3; ++ci)
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        float xv = xs[ci][r][px + s];
        const float* wr = &ws[ci * 9 + r * 3 + s][cg * 16];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] += xv * wr[j];
      }
  f16x8 h0, h1;
  float vals[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    float a = acc[j] > 0.f ? acc[j] : 0.2f * acc[j];
    f16 hh = (f16)a;
    if (j < 8) h0[j] = hh; else h1[j - 8] = hh;
    vals[j] = (float)hh;
  }
  f16* dst = out + (((size_t)n * 128 + oy) * 128 + px) * 32 + cg * 16;
  *reinterpret_cast<f16x8*>(dst) = h0;
  *reinterpret_cast<f16x8*>(dst + 8) = h1;
  // per-channel sums over the 128 pixels of this row: butterfly over the 32 pixels of a wave (lanes of equal channel half),
  // then the four waves in a fixed order (was: 16 block-wide rounds with 4 active threads each)
  float* dstp = bn_partial + ((size_t)n * 128 + oy) * 32 * 2;
  float (*red2)[2][16][2] = reinterpret_cast<float (*)[2][16][2]>(&red[0][0]);   // [wave][half][channel][sum, sumsq]
  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    float s1 = vals[j], s2 = vals[j] * vals[j];
#pragma unroll
    for (int o = 2; o < 64; o <<= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
    if (lane < 2) { red2[wave][lane][j][0] = s1; red2[wave][lane][j][1] = s2; }
  }
  __syncthreads();
  if (tid < 64) {
    const int c2 = tid >> 5, j = (tid >> 1) & 15, which = tid & 1;
    dstp[(c2 * 16 + j) * 2 + which] = ((red2[0][c2][j][which] + red2[1][c2][j][which]) + red2[2][c2][j][which]) + red2[3][c2][j][which];
  }
}

// ---------------------------------------------------------------------------------------------
// BatchNorm finalize: partial [nrow][C][2] -> ss[C][2] = (scale, shift);  training: batch statistics + running-stat
// update (momentum 0.1, unbiased variance); eval: running statistics.  Optionally pooled[n][c] = mean over the sample of
// the NORMALISED tensor (= scale * mean_n(raw) + shift), from the same partials (rows_per_sample rows per sample).
// Row mask: partial row k counts iff (k % tps) < vtps (tps = partial rows per sample; the compact conv2 of the sparse
// expert path computes 8 image rows per sample of which 6 are real).  cvec != null adds, analytically, the positions
// the compact path does not compute: per sample T_CNT[k] positions of value cvec[k][c] (see lo_t_cvec_kernel).
// ---------------------------------------------------------------------------------------------
__constant__ float T_CNT[6] = {121.f * 126.f, 121.f, 121.f, 126.f, 1.f, 1.f};   // interior, left, right, bottom, bottom-left, bottom-right
__global__ __launch_bounds__(256) void lo_bn_finalize_kernel(const float* __restrict__ partial, int nrow, int C, float count,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             float* __restrict__ rmean, float* __restrict__ rvar, int training,
                                                             float* __restrict__ ss, int tps, int vtps,
                                                             const float* __restrict__ cvec, float nsample, float* __restrict__ mr) {
  // training: 1 = batch statistics + running-statistics update; 2 = batch statistics only (the recomputation of a block inside
  // lo_teacher_full_backward: the forward of the same step has already moved the running statistics); 0 = running statistics.
  // mr != null: (mean, 1/sqrt(var + eps)) per channel for the BatchNorm backward.
  __shared__ double red[2][16][17];
  const int cl = threadIdx.x & 15, r = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  double s = 0.0, q = 0.0;
  if (c < C && training)
    for (int k = r; k < nrow; k += 16) {
      if ((k % tps) >= vtps) continue;
      f32x2 p = *reinterpret_cast<const f32x2*>(partial + ((size_t)k * C + c) * 2);
      s += (double)p[0];
      q += (double)p[1];
    }
  red[0][r][cl] = s; red[1][r][cl] = q;
  __syncthreads();
  if (r == 0 && c < C) {
    float mean, var;
    if (training) {
      double ts = 0.0, tq = 0.0;
      for (int k = 0; k < 16; ++k) { ts += red[0][k][cl]; tq += red[1][k][cl]; }
      if (cvec)
        for (int k = 0; k < 6; ++k) {
          double v = (double)cvec[k * C + c], n = (double)nsample * (double)T_CNT[k];
          ts += n * v;
          tq += n * v * v;
        }
      double m = ts / (double)count;
      double v = tq / (double)count - m * m;
      if (v < 0.0) v = 0.0;
      mean = (float)m; var = (float)v;
      if (training == 1) {
        rmean[c] = 0.9f * rmean[c] + 0.1f * mean;
        rvar[c] = 0.9f * rvar[c] + 0.1f * (float)(v * (double)count / ((double)count - 1.0));
      }
    } else {
      mean = rmean[c]; var = rvar[c];
    }
    if (mr) { mr[c * 2] = mean; mr[c * 2 + 1] = 1.0f / sqrtf(var + BN_EPS); }
    float sc = gamma[c] / sqrtf(var + BN_EPS);
    ss[c * 2] = sc;
    ss[c * 2 + 1] = beta[c] - mean * sc;
  }
}

// stage 1 of the finalize for many partial rows: out[split][C][2] = sum of the rows of that split (fixed order)
__global__ __launch_bounds__(256) void lo_bn_presum_kernel(const float* __restrict__ partial, int nrow, int C, float* __restrict__ out,
                                                           int tps, int vtps) {
  __shared__ float red[2][16][17];
  const int cl = threadIdx.x & 15, r = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  const int per = (nrow + gridDim.y - 1) / gridDim.y;
  const int k0 = blockIdx.y * per, k1 = min(nrow, k0 + per);
  float s = 0.f, q = 0.f;
  if (c < C)
    for (int k = k0 + r; k < k1; k += 16) {
      if ((k % tps) >= vtps) continue;
      f32x2 p = *reinterpret_cast<const f32x2*>(partial + ((size_t)k * C + c) * 2);
      s += p[0];
      q += p[1];
    }
  red[0][r][cl] = s; red[1][r][cl] = q;
  __syncthreads();
  if (r < 2 && c < C) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[r][k][cl];
    out[((size_t)blockIdx.y * C + c) * 2 + r] = t;
  }
}

// ---------------------------------------------------------------------------------------------
// BatchNorm apply (elementwise, 16-byte vectors over channels)
//   y[pix][dst_off + c] = raw[pix][c]*scale[c] + shift[c]                                   (mode 0; dst pitch for concat)
//   y = lrelu( (raw*scale + shift) * ls[c] + identity , 0.2 )                               (mode 1: ExpertBlock tail)
//   mode 2 = mode 1 with the SPARSE raw tensor: image rows 0..5 come from the compact buffer [n][8][128][C], every other
//   position is one of the six constant vectors cvec[k][C] (interior / left / right / bottom / two bottom corners)
// optional pool_partial[n][chunk][C] = per-sample, per-channel sums of y (global average pooling)
// ---------------------------------------------------------------------------------------------
struct BnApplyArgs {
  const f16* raw; const float* ss; const float* ls; const f16* identity; f16* y; float* pool_partial;
  int C, dst_pitch, dst_off, mode, rows_per_block;
  const float* cvec;
  int ss_stride;   // floats between the (scale, shift) tables of consecutive samples: 0 = one table (BatchNorm), 2*C = per sample (BatchNorm + Dropout2d)
  uint8_t* y8;     // fp8 mode: e4m3(y * LO_F8_ACT_SCALE) copy of y ([pix][C], no pitch), the operand of the next 3x3 convolution; or null
  const float* id_ss;   // mode 1: the identity branch is BatchNorm(identity) with this (scale, shift) table [C][2] (ExpertBlock.shortcut
                        // = Conv1x1 + BatchNorm when in_channels != out_channels, lunar_evaluator.py:254-257); null: identity as stored
};
__global__ __launch_bounds__(256) void lo_bn_apply_kernel(BnApplyArgs a) {
  __shared__ float s_red[256 * 8];
  const int tid = threadIdx.x, n = blockIdx.y, blk = blockIdx.x;
  const int C = a.C, CC = C >> 3;
  const int cc = tid % CC, slot = tid / CC, nslot = 256 / CC;
  const int c0 = cc * 8;
  float sc[8], sh[8], lsv[8], acc[8], isc[8], ish[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sc[j] = a.ss[(size_t)n * a.ss_stride + (c0 + j) * 2];
    sh[j] = a.ss[(size_t)n * a.ss_stride + (c0 + j) * 2 + 1];
    lsv[j] = a.mode >= 1 ? a.ls[c0 + j] : 1.f;
    isc[j] = a.id_ss ? a.id_ss[(c0 + j) * 2] : 1.f;
    ish[j] = a.id_ss ? a.id_ss[(c0 + j) * 2 + 1] : 0.f;
    acc[j] = 0.f;
  }
  const size_t row0 = (size_t)n * T_HW + (size_t)blk * a.rows_per_block;
  f16x8 hint;
  if (a.mode == 2) {
#pragma unroll
    for (int j = 0; j < 8; ++j) hint[j] = (f16)a.cvec[c0 + j];
  }
  constexpr int U = 4;
  for (int r = slot; r < a.rows_per_block; r += U * nslot) {
    f16x8 h[U], idv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int rr = r + u * nslot;
      if (rr < a.rows_per_block) {
        if (a.mode == 2) {
          const int p = blk * a.rows_per_block + rr, py = p >> 7, px = p & 127;
          if (py < 6) {
            h[u] = *reinterpret_cast<const f16x8*>(a.raw + ((size_t)n * 1024 + p) * C + c0);
          } else {
            const int k = (py == 127 ? 3 : 0) + (px == 0 ? 1 : px == 127 ? 2 : 0);
            h[u] = hint;
            if (k) {
#pragma unroll
              for (int j = 0; j < 8; ++j) h[u][j] = (f16)a.cvec[k * C + c0 + j];
            }
          }
        } else {
          h[u] = *reinterpret_cast<const f16x8*>(a.raw + (row0 + rr) * C + c0);
        }
        if (a.mode >= 1) idv[u] = *reinterpret_cast<const f16x8*>(a.identity + (row0 + rr) * C + c0);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int rr = r + u * nslot;
      if (rr < a.rows_per_block) {
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float v = (float)h[u][j] * sc[j] + sh[j];
          if (a.mode >= 1) {
            v = v * lsv[j] + ((float)idv[u][j] * isc[j] + ish[j]);
            v = v > 0.f ? v : 0.2f * v;
          }
          o[j] = (f16)v;
          acc[j] += (float)o[j];
        }
        if (a.y) *reinterpret_cast<f16x8*>(a.y + (row0 + rr) * a.dst_pitch + a.dst_off + c0) = o;   // y == null: pooling sums only
        if (a.y8) {
          const u32x2 q = {lo_pack4_fp8((float)o[0] * LO_F8_ACT_SCALE, (float)o[1] * LO_F8_ACT_SCALE, (float)o[2] * LO_F8_ACT_SCALE, (float)o[3] * LO_F8_ACT_SCALE),
                           lo_pack4_fp8((float)o[4] * LO_F8_ACT_SCALE, (float)o[5] * LO_F8_ACT_SCALE, (float)o[6] * LO_F8_ACT_SCALE, (float)o[7] * LO_F8_ACT_SCALE)};
          *reinterpret_cast<u32x2*>(a.y8 + (row0 + rr) * C + c0) = q;
        }
      }
    }
  }
  if (a.pool_partial) {
#pragma unroll
    for (int j = 0; j < 8; ++j) s_red[tid * 8 + j] = acc[j];
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
      int ccx = c >> 3, j = c & 7;
      float tot = 0.f;
      for (int s = 0; s < nslot; ++s) tot += s_red[(s * CC + ccx) * 8 + j];
      a.pool_partial[((size_t)n * gridDim.x + blk) * C + c] = tot;
    }
  }
}

// pooled[n][c] = sum_blk partial[n][blk][c] / HW
__global__ void lo_pool_finalize_kernel(const float* __restrict__ partial, float* __restrict__ pooled, int nblk, int C, int total) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int n = i / C, c = i - n * C;
  // eight loads in flight (the plain loop chained nblk dependent loads: 25 us for 8192 outputs); fixed order, so reproducible
  const float* p = partial + (size_t)n * nblk * C + c;
  float t = 0.f;
  int k = 0;
  for (; k + 8 <= nblk; k += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(k + u) * C];
#pragma unroll
    for (int u = 0; u < 8; ++u) t += v[u];
  }
  for (; k < nblk; ++k) t += p[(size_t)k * C];
  pooled[i] = t * (1.0f / (float)T_HW);
}

// ---------------------------------------------------------------------------------------------
// depthwise KxK conv (groups = 32) on BN(raw1): out[pix][c] = bias[c] + sum_taps w[c][tap] * (raw1[pix+tap][c]*scale[c]+shift[c])
// (zero padding applies to the normalised tensor).  thread = (pixel, 8-channel chunk)
// ---------------------------------------------------------------------------------------------
// Workgroup = a 16 x 32 pixel tile of one image, all 32 channels.  The normalised input tile with its halo is staged ONCE in
// LDS as fp16 ([row][col][32 ch], BatchNorm applied while staging, zeros outside the image: the padding of the normalised
// tensor), so a tap costs one fma instead of convert + normalise + fma.  Thread = (column, 8-channel chunk, 8-row half): a
// wave's 16-byte LDS reads are 1 KiB contiguous (16 pixels x 4 chunks), each loaded input value feeds up to K output rows
// from registers.  fp32 accumulation.  (Was: thread = pixel x chunk reading every tap from global: 87 us per launch.)
template <int K>
__global__ __launch_bounds__(256) void lo_t_dwconv_kernel(const f16* __restrict__ raw, const float* __restrict__ ss,
                                                          const float* __restrict__ w, const float* __restrict__ bias,
                                                          f16* __restrict__ out, int B) {
  constexpr int TR = 16, TC = 32, HR = TR + K - 1, HC = TC + K - 1, P = K / 2;
  __shared__ __attribute__((aligned(16))) f16 tile[HR * HC * 32];
  __shared__ __attribute__((aligned(16))) float ws[K * K][32];
  const int tid = threadIdx.x;
  const int n = blockIdx.y;
  const int ty0 = (blockIdx.x >> 2) * TR, tx0 = (blockIdx.x & 3) * TC;   // 8 x 4 tiles per 128 x 128 image
  for (int i = tid; i < K * K * 32; i += 256) ws[i / 32][i % 32] = w[(i % 32) * K * K + i / 32];
  {
    const int cc = tid & 3;
    float sc[8], sh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { sc[j] = ss[(cc * 8 + j) * 2]; sh[j] = ss[(cc * 8 + j) * 2 + 1]; }
    for (int q = tid >> 2; q < HR * HC; q += 64) {
      const int r = q / HC, c = q - r * HC;
      const int iy = ty0 + r - P, ix = tx0 + c - P;
      f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if ((unsigned)iy < 128u && (unsigned)ix < 128u) {
        const f16x8 h = *reinterpret_cast<const f16x8*>(raw + (((size_t)n * 128 + iy) * 128 + ix) * 32 + cc * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (f16)((float)h[j] * sc[j] + sh[j]);
      }
      *reinterpret_cast<f16x8*>(tile + q * 32 + cc * 8) = v;
    }
  }
  __syncthreads();
  const int cc = tid & 3, col = (tid >> 2) & 31, half = tid >> 7;   // rows half*8 .. half*8+7 of the tile
  const int c0 = cc * 8;
  float acc[8][8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float b = bias[c0 + j];
#pragma unroll
    for (int r = 0; r < 8; ++r) acc[r][j] = b;
  }
#pragma unroll 1
  for (int s = 0; s < K; ++s) {   // one tap column at a time (not unrolled: 64 accumulators + K x 8 weights already fill the budget)
    float wv[K][8];
#pragma unroll
    for (int r = 0; r < K; ++r) {
      const f32x4 w0 = *reinterpret_cast<const f32x4*>(&ws[r * K + s][c0]), w1 = *reinterpret_cast<const f32x4*>(&ws[r * K + s][c0 + 4]);
#pragma unroll
      for (int j = 0; j < 4; ++j) { wv[r][j] = w0[j]; wv[r][4 + j] = w1[j]; }
    }
#pragma unroll
    for (int ir = 0; ir < 8 + K - 1; ++ir) {        // input row of the halo tile (relative to this thread's first output row)
      const f16x8 h = *reinterpret_cast<const f16x8*>(tile + ((half * 8 + ir) * HC + col + s) * 32 + c0);
      float hv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) hv[j] = (float)h[j];
#pragma unroll
      for (int r = 0; r < K; ++r) {                 // tap row r of output row ir - r
        const int orow = ir - r;
        if (orow >= 0 && orow < 8) {
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[orow][j] += wv[r][j] * hv[j];
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (f16)acc[r][j];
    *reinterpret_cast<f16x8*>(out + (((size_t)n * 128 + ty0 + half * 8 + r) * 128 + tx0 + col) * 32 + c0) = o;
  }
}

// The same attention for any feature_dim F = 8 * HD (generic path, feature_dim != 128): qkv [B][16384][3F] fp16 (channel =
// t*F + head*HD + d), output on the compact rows attc [B][1024][F] (positions >= 543 are never written and stay zero).
// thr != 0: attn_drop on the probabilities, element index ((b*543 + p)*8 + head)*32 + key of site ds (lunar_evaluator.py:212).
template <int HD>
__global__ __launch_bounds__(256) void lo_t_attn_generic_kernel(const f16* __restrict__ qkv, f16* __restrict__ attc, int B, LoDropSite ds,
                                                                uint32_t thr, float inv_keep) {
  constexpr int F = 8 * HD, NV = HD / 8;
  const int wave_g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int per_b = 512 + 31;
  if (wave_g >= B * per_b) return;
  const int b = wave_g / per_b, p = wave_g - b * per_b;
  const int chunk = p < 512 ? p : 511;
  const int qtok = p < 512 ? 32 * p : 32 * 511 + (p - 511);
  const int head = lane >> 3, part = lane & 7;
  const f16* base = qkv + (size_t)b * T_HW * (3 * F);
  f16x8 qv[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) qv[i] = *reinterpret_cast<const f16x8*>(base + (size_t)qtok * (3 * F) + head * HD + 8 * i);
  float sc[4];
  const float scale = HD == 16 ? 0.25f : (HD == 32 ? 0.17677669529663687f : 0.125f);   // head_dim ** -0.5
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const f16* kp = base + (size_t)(32 * chunk + part * 4 + k) * (3 * F) + F + head * HD;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const f16x8 kv = *reinterpret_cast<const f16x8*>(kp + 8 * i);
#pragma unroll
      for (int d = 0; d < 8; ++d) s += (float)qv[i][d] * (float)kv[d];
    }
    sc[k] = s * scale;                // the relative-position term is constant along the keys: no effect on the softmax
  }
  float m = fmaxf(fmaxf(sc[0], sc[1]), fmaxf(sc[2], sc[3]));
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  float e[4], l = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) { e[k] = __expf(sc[k] - m); l += e[k]; }
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) l += __shfl_xor(l, o, 64);
  float pw[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) pw[k] = e[k] / l;
  if (thr) {
    const uint32_t i0 = ((uint32_t)(b * 543 + p) * 8u + (uint32_t)head) * 32u + (uint32_t)part * 4u;
    const uint32_t w0 = lo_drop_word(ds, i0 >> 1), w1 = lo_drop_word(ds, (i0 >> 1) + 1);
    pw[0] = (w0 & 0xFFFFu) >= thr ? pw[0] * inv_keep : 0.f;
    pw[1] = (w0 >> 16) >= thr ? pw[1] * inv_keep : 0.f;
    pw[2] = (w1 & 0xFFFFu) >= thr ? pw[2] * inv_keep : 0.f;
    pw[3] = (w1 >> 16) >= thr ? pw[3] * inv_keep : 0.f;
  }
  float acc[HD];
#pragma unroll
  for (int d = 0; d < HD; ++d) acc[d] = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const f16* vp = base + (size_t)(32 * chunk + part * 4 + k) * (3 * F) + 2 * F + head * HD;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const f16x8 vv = *reinterpret_cast<const f16x8*>(vp + 8 * i);
#pragma unroll
      for (int d = 0; d < 8; ++d) acc[8 * i + d] += pw[k] * (float)vv[d];
    }
  }
#pragma unroll
  for (int d = 0; d < HD; ++d)
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) acc[d] += __shfl_xor(acc[d], o, 64);
  if (part == 0) {
    f16* dst = attc + ((size_t)b * 1024 + p) * F + head * HD;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      f16x8 o8;
#pragma unroll
      for (int d = 0; d < 8; ++d) o8[d] = (f16)acc[8 * i + d];
      *reinterpret_cast<f16x8*>(dst + 8 * i) = o8;
    }
  }
}

// ---- dropout glue (train mode with dropout_rate > 0: the sparse shortcuts above do not hold, see lo_teacher_forward) ----------
// Dropout2d after a BatchNorm: ssb[b][c] = (scale, shift)[c] * (keep(b*C + c) ? 1/(1-p) : 0)   (lunar_evaluator.py:245-246,252-253)
__global__ void lo_t_drop2d_ss_kernel(const float* __restrict__ ss, float* __restrict__ ssb, int B, int C, LoDropSite ds, uint32_t thr,
                                      float inv_keep) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * C) return;
  const int c = i % C;
  const float f = lo_drop_keep(ds, (uint32_t)i, thr) ? inv_keep : 0.f;
  ssb[i * 2] = ss[c * 2] * f;
  ssb[i * 2 + 1] = ss[c * 2 + 1] * f;
}
// feature extractor: cat[pix][192] <- Dropout(BN(cat)) in place (lunar_evaluator.py:108-111); element index pix*192 + c
__global__ __launch_bounds__(256) void lo_t_cat_bn_drop_kernel(f16* __restrict__ cat, const float* __restrict__ ss, size_t nchunk,
                                                               LoDropSite ds, uint32_t thr, float inv_keep) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;       // 8-channel chunk
  if (i >= nchunk) return;
  const int c0 = (int)(i % 24) * 8;
  f16x8 v = *reinterpret_cast<const f16x8*>(cat + i * 8), o;
  const uint32_t keep = lo_drop_keep8(ds, (uint32_t)(i * 8), thr);
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = ((keep >> j) & 1u) ? (f16)(((float)v[j] * ss[(c0 + j) * 2] + ss[(c0 + j) * 2 + 1]) * inv_keep) : (f16)0.f;
  *reinterpret_cast<f16x8*>(cat + i * 8) = o;
}
// proj_drop: full-resolution conv2 input = Dropout(proj(att)) (lunar_evaluator.py:224-225).  proj(att) is the compact tensor
// projc [B][1024][128] on image rows 0..7 and fp16(proj.bias) everywhere else (what the dense 1x1 conv stores for a zero
// attention row).  Element index (b*HW + pix)*128 + c.
// out8 != null (fp8 mode): the tensor is written as e4m3(value * LO_F8_ACT_SCALE) bytes instead of fp16 (conv2 is its only reader).
// lgc8 = log2(C / 8): C = 128 / 256 / 512 channels per pixel.  thr = 0: no dropout (every element kept, inv_keep = 1): the plain
// expansion of the compact tensor that the generic (feature_dim != 128) path uses in eval mode.
template <int lgc8>
__global__ __launch_bounds__(256) void lo_t_projdrop_kernel(const f16* __restrict__ projc, const float* __restrict__ pbias,
                                                            f16* __restrict__ out, uint8_t* __restrict__ out8, size_t nchunk, LoDropSite ds,
                                                            uint32_t thr, float inv_keep) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;       // 8-channel chunk i & (C/8 - 1) of pixel i >> lgc8
  if (i >= nchunk) return;
  const int c0 = (int)(i & ((1u << lgc8) - 1)) * 8;
  const size_t gp = i >> lgc8;
  const int pix = (int)(gp & (T_HW - 1));
  const size_t b = gp >> 14;
  f16x8 v, o;
  if (pix < 1024) v = *reinterpret_cast<const f16x8*>(projc + ((b * 1024 + pix) << (lgc8 + 3)) + c0);
  else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (f16)pbias[c0 + j];
  }
  const uint32_t keep = thr ? lo_drop_keep8(ds, (uint32_t)(i * 8), thr) : 0xFFu;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = ((keep >> j) & 1u) ? (f16)((float)v[j] * inv_keep) : (f16)0.f;
  if (out8) {
    const u32x2 q = {lo_pack4_fp8((float)o[0] * LO_F8_ACT_SCALE, (float)o[1] * LO_F8_ACT_SCALE, (float)o[2] * LO_F8_ACT_SCALE, (float)o[3] * LO_F8_ACT_SCALE),
                     lo_pack4_fp8((float)o[4] * LO_F8_ACT_SCALE, (float)o[5] * LO_F8_ACT_SCALE, (float)o[6] * LO_F8_ACT_SCALE, (float)o[7] * LO_F8_ACT_SCALE)};
    *reinterpret_cast<u32x2*>(out8 + i * 8) = q;
  } else {
    *reinterpret_cast<f16x8*>(out + i * 8) = o;
  }
}

// The three branches end in BatchNorm and the fusion conv is linear in its input, so the branch BatchNorms fold into it:
//   fusion(BN(x)) = (W diag(scale)) x + (b + W shift).  ss: [192][2] (scale, shift) of the concatenated channels (this
// call's batch statistics in train mode).  The branches then write their raw outputs straight into the concatenated tensor
// and the three normalise passes over it (0.14 ms and 0.8 GB per forward) disappear.  One workgroup per output channel.
__global__ __launch_bounds__(256) void lo_t_fold_fusion_kernel(const float* __restrict__ w, const float* __restrict__ bias,
                                                               const float* __restrict__ ss, f16* __restrict__ w16,
                                                               float* __restrict__ bias_out) {
  __shared__ float red[256];
  const int n = blockIdx.x, k = threadIdx.x;
  float part = 0.f;
  if (k < 192) {
    const float wv = w[n * 192 + k];
    w16[n * 192 + k] = (f16)(wv * ss[k * 2]);
    part = wv * ss[k * 2 + 1];
  }
  red[k] = part;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (k < o) red[k] += red[k + o];
    __syncthreads();
  }
  if (k == 0) bias_out[n] = bias[n] + red[0];
}

// ---------------------------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------------------------
int t_bn_finalize(LoTeacher* h, float* P, void* ws, const TBnFinalize& op, hipStream_t st) {
  const float* partial = op.partial;
  int nrow = op.nrow, tps = op.tps, vtps = op.vtps;
  const int C = op.C, training = op.training;
  const TBnOff& bn = op.bn;
  LoProfScope _p("lo_bn_finalize", 0, 0, st);
  if (training && nrow > 256) {
    // two stages: 64 row splits in parallel, then the 64 split sums
    float* pre = TW(float, h->o_bnpre);
    hipLaunchKernelGGL(lo_bn_presum_kernel, dim3((C + 15) / 16, 64), dim3(256), 0, st, partial, nrow, C, pre, tps, vtps);
    LO_LAUNCH_CHECK("bn_presum");
    partial = pre;
    nrow = 64; tps = 1; vtps = 1;
  }
  hipLaunchKernelGGL(lo_bn_finalize_kernel, dim3((C + 15) / 16), dim3(256), 0, st, partial, nrow, C, (float)((size_t)h->B * T_HW),
                     TP(bn.weight), TP(bn.bias), TP(bn.running_mean), TP(bn.running_var), training,
                     op.ss_dst ? op.ss_dst : TW(float, h->o_ss), tps, vtps, op.cvec, (float)h->B, op.mr);   // ss_dst: (scale, shift) kept elsewhere than the shared slot
  LO_LAUNCH_CHECK("bn_finalize");
  return LO_OK;
}
int t_bn_apply(LoTeacher* h, void* ws, const TBnApply& op, hipStream_t st) {
  const int C = op.C, mode = op.mode;
  BnApplyArgs a{op.raw, op.per_sample ? TW(float, h->o_ssb) : TW(float, h->o_ss), op.ls, op.identity, op.y, op.pool_partial, C,
                op.dst_pitch, op.dst_off, mode, T_HW / 64, op.cvec, op.per_sample ? 2 * C : 0, op.y8, op.id_ss};
  LoProfScope _p(mode ? "lo_bn_apply (block tail)" : "lo_bn_apply", 0, 2.0 * h->B * T_HW * C * (mode == 1 ? 3 : 2), st);
  hipLaunchKernelGGL(lo_bn_apply_kernel, dim3(64, h->B), dim3(256), 0, st, a);
  LO_LAUNCH_CHECK("bn_apply");
  return LO_OK;
}
int t_pool_finalize(const float* partial, float* pooled, int nblk, int C, int total, hipStream_t st) {
  hipLaunchKernelGGL(lo_pool_finalize_kernel, dim3((total + 255) / 256), dim3(256), 0, st, partial, pooled, nblk, C, total);
  LO_LAUNCH_CHECK("pool_finalize");
  return LO_OK;
}
int t_pool(LoTeacher* h, float* pooled, int C, void* ws, hipStream_t st) {
  return t_pool_finalize(TW(float, h->o_poolp), pooled, 64, C, h->B * C, st);
}
int t_conv1(const float* x, const float* w, const float* bias, f16* out, float* bn_partial, int B, hipStream_t st) {
  hipLaunchKernelGGL(lo_t_conv1_kernel, dim3(128, B), dim3(256), 0, st, x, w, bias, out, bn_partial);
  LO_LAUNCH_CHECK("t_conv1");
  return LO_OK;
}
int t_dwconv(int K, const f16* raw, const float* ss, const float* w, const float* bias, f16* out, int B, hipStream_t st) {
  if (K == 5) hipLaunchKernelGGL((lo_t_dwconv_kernel<5>), dim3(32, B), dim3(256), 0, st, raw, ss, w, bias, out, B);
  else hipLaunchKernelGGL((lo_t_dwconv_kernel<3>), dim3(32, B), dim3(256), 0, st, raw, ss, w, bias, out, B);
  LO_LAUNCH_CHECK("t_dwconv");
  return LO_OK;
}
int t_attn_generic(int F, const f16* qkv, f16* attc, int B, LoDropSite ds, uint32_t thr, float inv_keep, hipStream_t st) {
  const dim3 grid((B * 543 + 3) / 4);
  if (F == 128) hipLaunchKernelGGL((lo_t_attn_generic_kernel<16>), grid, dim3(256), 0, st, qkv, attc, B, ds, thr, inv_keep);
  else if (F == 256) hipLaunchKernelGGL((lo_t_attn_generic_kernel<32>), grid, dim3(256), 0, st, qkv, attc, B, ds, thr, inv_keep);
  else hipLaunchKernelGGL((lo_t_attn_generic_kernel<64>), grid, dim3(256), 0, st, qkv, attc, B, ds, thr, inv_keep);
  LO_LAUNCH_CHECK("t_attn_generic");
  return LO_OK;
}
int t_projdrop(int C, const f16* projc, const float* pbias, f16* out, uint8_t* out8, size_t nchunk, LoDropSite ds, uint32_t thr,
               float inv_keep, hipStream_t st) {
  const dim3 grid((unsigned)((nchunk + 255) / 256));
  if (C == 128) hipLaunchKernelGGL((lo_t_projdrop_kernel<4>), grid, dim3(256), 0, st, projc, pbias, out, out8, nchunk, ds, thr, inv_keep);
  else if (C == 256) hipLaunchKernelGGL((lo_t_projdrop_kernel<5>), grid, dim3(256), 0, st, projc, pbias, out, out8, nchunk, ds, thr, inv_keep);
  else hipLaunchKernelGGL((lo_t_projdrop_kernel<6>), grid, dim3(256), 0, st, projc, pbias, out, out8, nchunk, ds, thr, inv_keep);
  LO_LAUNCH_CHECK("t_projdrop");
  return LO_OK;
}
int t_cat_bn_drop(f16* cat, const float* ss, size_t nchunk, LoDropSite ds, uint32_t thr, float inv_keep, hipStream_t st) {
  hipLaunchKernelGGL(lo_t_cat_bn_drop_kernel, dim3((unsigned)((nchunk + 255) / 256)), dim3(256), 0, st, cat, ss, nchunk, ds, thr, inv_keep);
  LO_LAUNCH_CHECK("t_cat_bn_drop");
  return LO_OK;
}
int t_fold_fusion(const float* w, const float* bias, const float* ss, f16* w16, float* bias_out, hipStream_t st) {
  hipLaunchKernelGGL(lo_t_fold_fusion_kernel, dim3(128), dim3(256), 0, st, w, bias, ss, w16, bias_out);
  LO_LAUNCH_CHECK("t_fold_fusion");
  return LO_OK;
}
int t_drop2d(LoTeacher* h, void* ws, int C, const LoDropCfg& d, uint32_t site, hipStream_t st) {
  hipLaunchKernelGGL(lo_t_drop2d_ss_kernel, dim3((h->B * C + 255) / 256), dim3(256), 0, st, TW(float, h->o_ss), TW(float, h->o_ssb), h->B, C,
                     d.site(site), d.thr, d.inv_keep);
  LO_LAUNCH_CHECK("t_drop2d_ss");
  return LO_OK;
}
