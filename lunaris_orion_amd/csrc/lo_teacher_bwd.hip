// Full backward of LunarMoETeacher (second half): gradients for the experts and the feature extractor as well,
// i.e. what the reference's teacher loss produces when its three `torch.utils.checkpoint.checkpoint` calls
// (lunar_evaluator.py:194-197, 266-275, 411-414) are non-reentrant.  This unit: scratch plan, the trunk in plain form, the feature
// extractor's backward, the executor and clip + AdamW; lo_teacher_bwd_block.hip: the BatchNorm and ExpertBlock backward.
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
#include "lo_teacher.h"
#include "lo_conv.h"
#include <algorithm>

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
// every geometry the full backward passes to lo_wgrad_run (through o_wslab): tb_plan sizes the slab from this list and the executor
// launches from the same objects.  (gsc runs at feature_dim 256 / 512 only.)
struct TbWgradGeoms { const LoGeom* g[6]; };
static TbWgradGeoms tb_wgrad_geoms(const LoTeacher* h) { return {{&h->g3a, &h->g3b, &h->gqF, &h->gpc, &h->gsc, &h->gfw}}; }

static void tb_plan(const LoTeacher* h, TbPlan* p) {
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t r = off; off += (bytes + 255) & ~(size_t)255; return r; };
  const size_t px = (size_t)h->B * T_HW, F = (size_t)h->F;
  // every block's tensors kept (nothing is ever recomputed) while that fits comfortably: 8 F-channel tensors per block, 12 blocks --
  // 26 GB at batch 64 / feature_dim 128, 103 GB at 512; above 160 GB one shared set and a recomputation per block
  // (LO_T_BWD_SHARED=1 takes the shared set at any size: how the tests reach that plan)
  p->saved = !h->bwd_shared && (double)px * (double)F * 2.0 * 8.0 * 3.0 * (double)h->E <= 160.0e9;
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
  for (const LoGeom* g : tb_wgrad_geoms(h).g) slab = std::max(slab, lo_wgrad_slab_bytes(*g));
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

// Where a teacher tensor lives (include/lunaris_hip.h has the table of kinds): space 1 = the scratch of lo_teacher_forward_keep /
// _keep_eval, straight from tb_plan; space 0 = the workspace of lo_teacher_forward.  Launches nothing, changes nothing.
extern "C" int lo_teacher_debug_tensor(const LoTeacher* h, int space, int which, int e, int l, size_t* byte_offset, int* dims4, int* elem_bytes) {
  LO_REQUIRE(h && byte_offset && dims4 && elem_bytes, "lo_teacher_debug_tensor: null argument");
  LO_REQUIRE(space == 0 || space == 1, "lo_teacher_debug_tensor: unknown space %d (0 = forward workspace, 1 = kept-forward scratch)", space);
  const int B = h->B, F = h->F;
  auto put = [&](size_t off, int d0, int d1, int d2, int d3, int eb) {
    *byte_offset = off; dims4[0] = d0; dims4[1] = d1; dims4[2] = d2; dims4[3] = d3; *elem_bytes = eb;
    return LO_OK;
  };
  if (space == 0) {
    LO_REQUIRE(e == 0 && l == 0, "lo_teacher_debug_tensor: the forward workspace holds one tensor per kind (e = l = 0), asked for (%d, %d)", e, l);
    switch (which) {
      case 0: return put(h->o_raw32, B, 128, 128, 32, 2);
      case 1: return put(h->o_cat, B, 128, 128, 192, 2);
      case 2: return put(h->o_feat, B, 128, 128, 128, 2);
      case 3: return put(h->o_x0, B, 128, 128, F, 2);
      case 4: return put(h->o_x1, B, 128, 128, F, 2);
      case 5: return put(h->o_rawA, B, 128, 128, F, 2);
      case 6: return put(h->o_projc, B, 8, 128, F, 2);
      case 7: return put(h->o_proj, B, 128, 128, F, 2);
      case 8: return put(h->o_rawB, B, 128, 128, F, 2);
      case 9: return put(h->o_ss, 1, 1, F, 2, 4);
      case 10: return put(h->o_ssb, B, 1, F, 2, 4);
      case 11: return put(h->o_ss_cat, 1, 1, 192, 2, 4);
      case 12: return put(h->o_wfus_fold, 1, 1, 128, 192, 2);
      case 13: return put(h->o_bfus_fold, 1, 1, 1, 128, 4);
      default: break;
    }
    LO_REQUIRE(false, "lo_teacher_debug_tensor: unknown tensor kind %d of the forward workspace (0 .. 13)", which);
  }
  TbPlan p;
  tb_plan(h, &p);
  const bool per_block = which >= 6 && which <= 18;
  if (per_block) {
    LO_REQUIRE(e >= 0 && e < h->E && l >= 0 && l < 3, "lo_teacher_debug_tensor: block (%d, %d) out of range (%d experts, 3 layers)", e, l, h->E);
    LO_REQUIRE(which == 6 || p.saved, "lo_teacher_debug_tensor: tensor kind %d is per block, and this plan keeps one shared set (LO_T_BWD_SHARED)", which);
  } else if (which == 1) {
    LO_REQUIRE(e == 0 && l >= 0 && l < 3, "lo_teacher_debug_tensor: depthwise branch %d out of range (e = 0, l = 0 .. 2)", l);
  } else if (which == 19) {
    LO_REQUIRE(e == 0 && l >= 3 && l <= 7, "lo_teacher_debug_tensor: (mean, rstd) table %d out of range (e = 0, l = 3 .. 7)", l);
  } else {
    LO_REQUIRE(e == 0 && l == 0, "lo_teacher_debug_tensor: tensor kind %d takes e = l = 0, asked for (%d, %d)", which, e, l);
  }
  const TbBlk& b = p.blk[per_block ? e : 0][per_block ? l : 0];
  switch (which) {
    case 0: return put(p.o_raw32, B, 128, 128, 32, 2);
    case 1: return put(p.o_dwb[l], B, 128, 128, 32, 2);
    case 2: return put(p.o_cat, B, 128, 128, 192, 2);
    case 3: return put(p.o_catd, B, 128, 128, 192, 2);
    case 4: return put(p.o_rawF, B, 128, 128, 128, 2);
    case 5: return put(p.o_feat, B, 128, 128, 128, 2);
    case 6: return put(p.o_xs[e][l], B, 128, 128, F, 2);
    case 7: return put(b.rawA, B, 128, 128, F, 2);
    case 8: return put(b.bnA, B, 128, 128, F, 2);
    case 9: return put(b.qkv, B, 128, 128, 3 * F, 2);
    case 10: return put(b.attc, B, 8, 128, F, 2);
    case 11: return put(b.projc, B, 8, 128, F, 2);
    case 12: return put(b.a2, B, 128, 128, F, 2);
    case 13: return put(b.rawB, B, 128, 128, F, 2);
    case 14:
      LO_REQUIRE(F != 128 && l == 0, "lo_teacher_debug_tensor: block (%d, %d) at feature_dim %d has no shortcut conv", e, l, F);
      return put(b.scraw, B, 128, 128, F, 2);
    case 15: return put(b.mrA, 1, 1, F, 2, 4);
    case 16: return put(b.mrB, 1, 1, F, 2, 4);
    case 17:
    case 18:
      LO_REQUIRE(F != 128 && l == 0, "lo_teacher_debug_tensor: block (%d, %d) at feature_dim %d has no shortcut BatchNorm", e, l, F);
      return put(which == 17 ? b.mrS : b.ssS, 1, 1, F, 2, 4);
    case 19: return put(p.o_mr[l], 1, 1, l == 3 ? 32 : (l == 7 ? 128 : 64), 2, 4);
    case 20: return put(p.o_ssx[3], 1, 1, 32, 2, 4);
    default: break;
  }
  LO_REQUIRE(false, "lo_teacher_debug_tensor: unknown tensor kind %d of the kept-forward scratch (0 .. 20)", which);
  return LO_OK;
}

static int tb_ctx_init(TbCtx& c, LoTeacher* h, float* P, void* ws, void* bws, float* grads, float drop_p, uint64_t drop_seed, float gscale, void* stream) {
  c.h = h; c.P = P; c.ws = ws; c.bws = bws; c.G = grads; c.st = reinterpret_cast<hipStream_t>(stream);
  tb_plan(h, &c.pl);
  c.d = lo_drop_cfg(drop_p, drop_seed);
  c.gscale = gscale; c.inv_g = 1.0f / gscale;
  const int B = h->B, F = h->F;
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
// ExpertBlock (e, l) in plain form into its tensor set inside bws (t_block_plain, under this mode's profiler names)
static int tb_block_forward(TbCtx& c, int e, int l, const f16* xin, f16* xout, int train, float* pool_partial) {
  void* bws = c.bws;
  const TbBlk& b = c.pl.blk[e][l];
  const TBlkT t{TB(f16, b.rawA), TB(f16, b.bnA), TB(f16, b.qkv), TB(f16, b.attc), TB(f16, b.projc), TB(f16, b.a2), TB(f16, b.rawB), TB(f16, b.scraw),
                TB(float, b.mrA), TB(float, b.mrB), TB(float, b.mrS), TB(float, b.ssS)};
  static const TBlkNames nm{"tb shortcut (igemm)", "tb conv1 (recompute)", "tb qkv (recompute)", "tb proj (recompute)", "tb conv2 (recompute)", nullptr, nullptr};
  return t_block_plain(c.h, c.P, c.ws, e, l, c.d, t, xin, xout, train, pool_partial, nm, c.st);
}
// the trunk in plain form: feature extractor and the 12 blocks, every block's output (and, with a saved plan, every tensor its backward
// reads) left inside bws.  train 1: the step's forward (pooled features for the heads, running statistics move); 2: the backward's own pass;
// 0: eval mode (running statistics, read only; the (mean, rstd) tables hold them).  pool: the pooled features for the heads as well
static int tb_trunk_forward(TbCtx& c, const float* x, int train, bool pool) {
  LoTeacher* h = c.h; void* ws = c.ws; void* bws = c.bws;
  const int B = h->B, F = h->F;
  float* poolp = pool ? TW(float, h->o_poolp) : nullptr;
  // the feature extractor keeps every tensor its backward reads: the raw concatenation next to catd = Dropout(BN(cat))
  const TFeDst fd{TB(f16, c.pl.o_raw32), {TB(f16, c.pl.o_dwb[0]), TB(f16, c.pl.o_dwb[1]), TB(f16, c.pl.o_dwb[2])}, TB(f16, c.pl.o_cat), TB(f16, c.pl.o_catd),
                  TB(f16, c.pl.o_rawF), TB(f16, c.pl.o_feat), nullptr, TB(float, c.pl.o_ssx[3]), TB(float, c.pl.o_mr[3]),
                  {TB(float, c.pl.o_mr[4]), TB(float, c.pl.o_mr[5]), TB(float, c.pl.o_mr[6])}, TB(float, c.pl.o_mr[7]), poolp};
  static const TFeNames fe_names{nullptr, nullptr, nullptr, nullptr};
  LO_TRYT(t_fe_forward(h, x, c.P, ws, train, c.d, false, fd, fe_names, c.st));
  if (pool) LO_TRYT(t_pool(h, TW(float, h->o_pool_f), 128, ws, c.st));
  const f16* feat = TB(f16, c.pl.o_feat);
  for (int e = 0; e < h->E; ++e) {
    for (int l = 0; l < 3; ++l)
      LO_TRYT(tb_block_forward(c, e, l, l ? TB(f16, c.pl.o_xs[e][l - 1]) : feat, TB(f16, c.pl.o_xs[e][l]), train, l == 2 ? poolp : nullptr));
    if (pool) LO_TRYT(t_pool(h, TW(float, h->o_pool_e) + (size_t)e * B * F, F, ws, c.st));
  }
  return LO_OK;
}

// feature extractor backward, from dfeat (gradient wrt the features, scaled); dx (NULL = not wanted): the gradient wrt the images.
// Without a gradient buffer (c.G null) the weight-gradient kernels and their column sums are skipped
static int tb_fe_backward(TbCtx& c, const float* x, float* dx) {
  LoTeacher* h = c.h; float* P = c.P; float* G = c.G; void* bws = c.bws; hipStream_t st = c.st;
  const bool wg = G != nullptr;
  const TFeOff& fe = h->fe;
  const int B = h->B;
  const size_t px = (size_t)B * T_HW;
  f16* dcf = TB(f16, c.pl.o_dA);                   // gradient wrt the fusion conv's output [pix][128]
  LO_TRYT(tb_bn_backward(c, {.din = {TB(f16, c.pl.o_dfeat), 128}, .raw = {TB(f16, c.pl.o_rawF), 128}, .mr = TB(float, c.pl.o_mr[7]),
                             .bn = fe.bn_fus, .out = {dcf, 128}, .C = 128, .act = TB_ACT_LRELU, .dbias = wg ? TG(fe.fus_b) : nullptr}));
  // fusion conv 192 -> 128 as three 64-channel slices (the GEMM kernels want power-of-two channel counts)
  LoGeom d64;
  LO_TRYT(lo_make_geom(&d64, LO_LINEAR, B, 128, 128, 128, 64));
  for (int b = 0; b < 3; ++b) {
    if (wg) {
      const size_t nchunk = px * 8;
      hipLaunchKernelGGL(lo_tb_slice64_kernel, dim3((unsigned)((nchunk + 255) / 256)), dim3(256), 0, st, TB(f16, c.pl.o_catd), 64 * b, TB(f16, c.pl.o_cat64), nchunk);
      LO_LAUNCH_CHECK("tb_slice64");
      LO_TAGGED("tb fusion wgrad", lo_wgrad_run(h->gfw, TB(f16, c.pl.o_cat64), dcf, TB(float, c.pl.o_wslab), TB(float, c.pl.o_tmpw), c.inv_g, st));
      hipLaunchKernelGGL(lo_tb_scatter_cols_kernel, dim3(32), dim3(256), 0, st, TB(float, c.pl.o_tmpw), TG(fe.fus_w), 64 * b);
      LO_LAUNCH_CHECK("tb_scatter_cols");
    }
    // data gradient of the slice: dcat[pix][64 b + ci] = sum_co dcf[pix][co] W[co][64 b + ci]  (operand [ci][co], written at its channel offset)
    hipLaunchKernelGGL(lo_tb_wt_kernel, dim3((64 * 128 + 255) / 256), dim3(256), 0, st, TP(fe.fus_w), TB(f16, c.pl.o_wt), 64, 128, 192, 64 * b);
    LO_LAUNCH_CHECK("tb_wt");
    LoConvExtra exd{0, nullptr, 192, 64 * b};
    LO_TAGGED("tb fusion dgrad", lo_conv_run(d64, {.in = dcf, .w = TB(f16, c.pl.o_wt), .out = TB(f16, c.pl.o_dcat), .ex = &exd}, st));
  }
  f16* dpw = TB(f16, c.pl.o_cat64);               // gradient wrt a pointwise conv's output [pix][64]
  f16* ddw = TB(f16, c.pl.o_d32a);                // gradient wrt a depthwise conv's output [pix][32]
  f16* dn0 = TB(f16, c.pl.o_d32b);                // gradient wrt BN(conv1) [pix][32], summed over the branches
  const float* ss32 = TB(float, c.pl.o_ssx[3]);
  for (int b = 0; b < 3; ++b) {
    const TBranchOff& br = fe.br[b];
    const int K = b == 1 ? 5 : 3;
    // Dropout (element index pix * 192 + 64 b + c), BatchNorm of the branch, LeakyReLU
    LO_TRYT(tb_bn_backward(c, {.din = {TB(f16, c.pl.o_dcat), 192, 64 * b}, .raw = {TB(f16, c.pl.o_cat), 192, 64 * b},
                               .mr = TB(float, c.pl.o_mr[4 + b]), .bn = br.bn, .out = {dpw, 64}, .C = 64, .act = TB_ACT_LRELU,
                               .drop = {TB_DROP_ELEM, LO_DS_FE, 192, 64 * b}, .dbias = wg ? TG(br.pw_b) : nullptr}));
    if (wg) {
      hipLaunchKernelGGL(lo_tb_pw_wgrad_kernel, dim3((unsigned)(px / 1024)), dim3(256), 0, st, dpw, 64, 0, TB(f16, c.pl.o_dwb[b]), TB(float, c.pl.o_part));
      LO_LAUNCH_CHECK("tb_pw_wgrad");
      LO_TRYT(lo_colsum(TB(float, c.pl.o_part), TG(br.pw_w), (int)(px / 1024), 2048, 2048, c.inv_g, st));
    }
    hipLaunchKernelGGL(lo_tb_pw_dgrad_kernel, dim3((unsigned)((px * 4 + 255) / 256)), dim3(256), 0, st, dpw, 64, 0, TP(br.pw_w), ddw, px);
    LO_LAUNCH_CHECK("tb_pw_dgrad");
    if (K == 5) {
      if (wg) hipLaunchKernelGGL((lo_tb_dw_wgrad_kernel<5>), dim3(128, B), dim3(256), 0, st, ddw, TB(f16, c.pl.o_raw32), ss32, TB(float, c.pl.o_part), TB(float, c.pl.o_bpart));
      LO_LAUNCH_CHECK("tb_dw_wgrad");
      hipLaunchKernelGGL((lo_tb_dw_dgrad_kernel<5>), dim3(128, B), dim3(256), 0, st, ddw, TP(br.dw_w), b ? dn0 : (const f16*)nullptr, dn0);
    } else {
      if (wg) hipLaunchKernelGGL((lo_tb_dw_wgrad_kernel<3>), dim3(128, B), dim3(256), 0, st, ddw, TB(f16, c.pl.o_raw32), ss32, TB(float, c.pl.o_part), TB(float, c.pl.o_bpart));
      LO_LAUNCH_CHECK("tb_dw_wgrad");
      hipLaunchKernelGGL((lo_tb_dw_dgrad_kernel<3>), dim3(128, B), dim3(256), 0, st, ddw, TP(br.dw_w), b ? dn0 : (const f16*)nullptr, dn0);
    }
    LO_LAUNCH_CHECK("tb_dw_dgrad");
    if (wg) {
      LO_TRYT(lo_colsum(TB(float, c.pl.o_part), TG(br.dw_w), B * 128, 32 * K * K, 32 * K * K, c.inv_g, st));
      LO_TRYT(lo_colsum(TB(float, c.pl.o_bpart), TG(br.dw_b), B * 128, 32, 32, c.inv_g, st));
    }
  }
  // BatchNorm + LeakyReLU of conv1, then its weight gradient and -- for a caller whose images require grad -- its data gradient
  LO_TRYT(tb_bn_backward(c, {.din = {dn0, 32}, .raw = {TB(f16, c.pl.o_raw32), 32}, .mr = TB(float, c.pl.o_mr[3]), .bn = fe.bn1,
                             .out = {ddw, 32}, .C = 32, .act = TB_ACT_LRELU}));
  if (wg) {
    hipLaunchKernelGGL(lo_tb_conv1_wgrad_kernel, dim3(128, B), dim3(256), 0, st, x, ddw, TB(float, c.pl.o_part), TB(float, c.pl.o_bpart));
    LO_LAUNCH_CHECK("tb_conv1_wgrad");
    LO_TRYT(lo_colsum(TB(float, c.pl.o_part), TG(fe.conv1_w), B * 128, 864, 864, c.inv_g, st));
    LO_TRYT(lo_colsum(TB(float, c.pl.o_bpart), TG(fe.conv1_b), B * 128, 32, 32, c.inv_g, st));
  }
  if (dx) LO_TRYT(lo_image_dgrad(ddw, 32, 1, TP(fe.conv1_w), B, c.seed ? c.inv_g * c.dx_factor : c.inv_g, dx, st, c.seed));
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
  h->last_p = c.d.on ? dropout_p : 0.f; h->last_seed = drop_seed; h->last_path = c.d.on ? 2 : 1;
  LO_TRYT(tb_zero_attc(c));
  LO_TRYT(tb_trunk_forward(c, x, 1, true));
  LO_TRYT(t_run_heads(h, P, ws, quality, weights, style, prompt, semantic, c.d, c.st));
  h->kept = true; h->kept_eval = false; h->kept_bws = bws;
  return LO_OK;
}
// The same in eval mode (lunar_evaluator.py:408-462 under module.eval()): BatchNorm with the running statistics, no dropout, nothing of
// the state written (training = 0 of the plain-form code; P is const for the caller); the (mean, rstd) tables hold (running_mean,
// 1 / sqrt(running_var + eps)) for lo_teacher_eval_backward
extern "C" int lo_teacher_forward_keep_eval(LoTeacher* h, const float* x, const float* P, void* ws, void* bws, float* quality, float* weights,
                                            float* style, float* prompt, float* semantic, void* stream) {
  LO_REQUIRE(h && x && P && ws && bws && quality && weights && style && prompt && semantic, "lo_teacher_forward_keep_eval: null argument");
  TbCtx c;
  LO_TRYT(tb_ctx_init(c, h, const_cast<float*>(P), ws, bws, nullptr, 0.f, 0, 1.0f, stream));
  h->kept = false; h->kept_bws = nullptr;
  h->last_p = 0.f; h->last_seed = 0; h->last_path = 1;
  LO_TRYT(tb_zero_attc(c));
  LO_TRYT(tb_trunk_forward(c, x, 0, true));
  LO_TRYT(t_run_heads(h, c.P, ws, quality, weights, style, prompt, semantic, c.d, c.st));
  h->kept = true; h->kept_eval = true; h->kept_bws = bws;
  return LO_OK;
}

// coef = quality_weight / accum (like lo_teacher_heads_backward).  Must follow lo_teacher_forward(training = 1) on the same batch
// with the same dropout_p / drop_seed (h->last_*): the heads' backward reads that call's pooled features.  gscale: power of two by
// which the fp16 activation gradients are multiplied (parameter gradients come out unscaled).  rows: [B][head range] scratch of
// lo_teacher_heads_backward.  grads: the teacher's flat gradient buffer (state-table layout); every parameter on the loss path is
// written, everything else is zeroed.
// frozen (lo_teacher_eval_backward): the eval-mode function -- running statistics as constants, no dropout; grads may then be null (no
// parameter gradient is computed: no weight-gradient GEMM, no column sum, no BatchNorm reduce) and dx alone is produced.
static int tb_full_backward_impl(LoTeacher* h, const float* x, float* P, void* ws, void* bws, const float* pooled_f, const float* pooled_e,
                                 const float* raw_q, const float* expert_weights, const float* dq_up, const float* dw_up, float coef,
                                 float drop_p, uint64_t drop_seed, float gscale, float* rows, float* grads, float* dx, void* stream, int frozen = 0,
                                 const LoImgSeed* seed = nullptr, float dx_factor = 1.0f) {
  LO_REQUIRE(h && x && P && ws && bws && expert_weights && rows && (grads || (frozen && dx)), "lo_teacher_full_backward: null argument");
  LO_REQUIRE(gscale > 0.f, "lo_teacher_full_backward: gscale must be positive");
  LO_REQUIRE(h->last_path >= 0, "lo_teacher_full_backward: no forward has run on this engine");
  TbCtx c;
  LO_TRYT(tb_ctx_init(c, h, P, ws, bws, grads, drop_p, drop_seed, gscale, stream));
  c.frozen = frozen; c.seed = seed; c.dx_factor = dx_factor;
  hipStream_t st = c.st;
  float* G = grads;
  const int B = h->B, F = h->F, E = h->E;
  const size_t px = (size_t)B * T_HW;
  if (G) LO_HIP(hipMemsetAsync(G, 0, h->flat_elems * sizeof(float), st));
  // heads: their own parameter gradients + d loss / d pooled features
  LO_TRYT(t_heads_backward(h, P, pooled_f, pooled_e, raw_q, expert_weights, dq_up, dw_up, coef, c.d, rows, grads, st,
                           TB(float, c.pl.o_dpool_f), TB(float, c.pl.o_dpool_e)));
  // pass 1: the trunk again in plain form -- unless the forward of this step was lo_teacher_forward_keep on this bws
  // (kept by the forward of the same mode: eval tensors are not train tensors)
  const bool kept = h->kept && h->kept_eval == (frozen != 0) && h->kept_bws == bws && h->last_seed == drop_seed && h->last_p == drop_p;
  h->kept = false; h->kept_bws = nullptr;
  if (!kept) {
    LO_TRYT(tb_zero_attc(c));
    LO_TRYT(tb_trunk_forward(c, x, frozen ? 0 : 2, false));
  }
  const bool recompute = !c.pl.saved;          // one shared tensor set: every block is recomputed in front of its backward
  const f16* feat = TB(f16, c.pl.o_feat);
  // pass 2: experts, last block first
  const size_t nchunk128 = px * 16;
  for (int e = 0; e < E; ++e) {
    for (int l = 2; l >= 0; --l) {
      const f16* xin = l ? TB(f16, c.pl.o_xs[e][l - 1]) : feat;
      if (recompute) LO_TRYT(tb_block_forward(c, e, l, xin, nullptr, frozen ? 0 : 2, nullptr));      // in the call's mode: frozen = running statistics
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

// Backward of lo_teacher_forward_keep_eval (the eval-mode teacher as a differentiable reward, or fine-tuned with frozen BatchNorm): the
// chain of lo_teacher_full_backward_dx with every BatchNorm differentiated at its running statistics and no dropout.  flat_grads NULL:
// parameter gradients not wanted -- one streaming pass per BatchNorm (the block tail fused into BatchNorm2's), no weight-gradient
// GEMM, no column sum, no reduce / finalize, no memset of a flat buffer; dx has the same bits either way.  Does not find its own kept
// tensors in bws: recomputes the trunk with training = 0 from the images.
extern "C" int lo_teacher_eval_backward(LoTeacher* h, const float* x, const float* P, void* ws, void* bws, const float* pooled_f,
                                        const float* pooled_e, const float* raw_q, const float* expert_weights, const float* d_quality,
                                        const float* d_weights, float gscale, float* rows, float* grads, float* dx, void* stream) {
  LO_REQUIRE(pooled_f && pooled_e && raw_q && (d_quality || d_weights) && (grads || dx), "lo_teacher_eval_backward: null argument");
  return tb_full_backward_impl(h, x, const_cast<float*>(P), ws, bws, pooled_f, pooled_e, raw_q, expert_weights, d_quality, d_weights, 0.f, 0.f, 0,
                               gscale, rows, grads, dx, stream, 1);
}
// The same with flat_grads = NULL and the SEEDED image data gradient as its last kernel: dx = scale_factor * (d / d images) +
// seed_coef[0] * (images - target) -- the whole d vae_loss / d recon of the hybrid step's reward-gradient objective (the teacher's
// input is the reconstruction), with no add pass.  The chain above with one more field in its context
extern "C" int lo_teacher_eval_backward_seed(LoTeacher* h, const float* x, const float* P, void* ws, void* bws, const float* pooled_f,
                                             const float* pooled_e, const float* raw_q, const float* expert_weights, const float* d_quality,
                                             const float* d_weights, float gscale, float* rows, const float* target, const float* seed_coef,
                                             float scale_factor, float* dx, void* stream) {
  LO_REQUIRE(pooled_f && pooled_e && raw_q && (d_quality || d_weights) && dx && x && target && seed_coef, "lo_teacher_eval_backward_seed: null argument");
  LO_REQUIRE(scale_factor > 0.f, "lo_teacher_eval_backward_seed: scale_factor must be positive");
  const LoImgSeed seed{seed_coef, x, target};
  return tb_full_backward_impl(h, x, const_cast<float*>(P), ws, bws, pooled_f, pooled_e, raw_q, expert_weights, d_quality, d_weights, 0.f, 0.f, 0,
                               gscale, rows, nullptr, dx, stream, 1, &seed, scale_factor);
}
