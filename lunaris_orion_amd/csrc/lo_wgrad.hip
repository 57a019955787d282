// Weight gradients: the per-tap TN GEMM lo_wgrad_tn (both operands are reduced over the pixel index, the slow axis of NHWC, so their
// MFMA fragments are read with ds_read_b64_tr_b16), the slab reduce kernels, and the choice among the three weight-gradient kernels.
#include "lo_conv.h"
#include "lo_conv_dev.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>

// ---------------------------------------------------------------------------------------------
// TN weight-gradient GEMM:  dWp[p][n][t*Cin + c] = sum_m dy[m][n] * Xtap[m][c]
//   dy rows are the op's OUTPUT pixels (forward geometry), Xtap rows the input pixels a tap reads.
//   Tile: BMW output channels (n) x BNW input channels (c) for one (phase, tap); K loop over pixels in
//   steps of 32; grid.z splits the pixel range; fp32 partial slabs, reduced by lo_wgrad_reduce_kernel.
// ---------------------------------------------------------------------------------------------
struct WgradArgs {
  const f16* x;     // forward input  [B,Hin,Win,Cin]
  const f16* dy;    // grad of forward output [B,Hout,Wout,Cout]
  float* slab;      // [nsplit][packed elems]
  float* grad;      // canonical fp32 gradient, written directly when nsplit == 1 (direct mode)
  float scale;
  int direct;
  int taps;         // total taps over all phases
  int M;            // pixels per phase = B*GH*GW
  int nsplit;
  int msteps_per_split;  // 32-pixel steps per split
  int packed_elems;
  LoGeom g;         // FORWARD geometry
};

// LDS-DMA staged like lo_igemm_nt.  Tiles are [32 pixel rows][BMW or BNW channels] fp16, unpadded; the transposed
// fragment reads (ds_read_b64_tr_b16) are kept conflict-free by the block swizzle lo_tr_swz (lo_conv_dev.h).
// Output channels n >= Cout (a 32-channel layer run with the 64-wide tile) read the zero page and are not stored.
template <int BMW, int BNW, int NSTAGE, int BKP>
__global__ __launch_bounds__(256) void lo_wgrad_tn(WgradArgs a) {
  static_assert(BKP == 32 || BKP == 64, "pixels per K step");
  constexpr int RBA = BMW * 2, RBB = BNW * 2;    // row bytes
  static_assert((RBA == 128 || RBA == 256) && (RBB == 128 || RBB == 256), "tile rows must be 128 or 256 bytes");
  constexpr int A_BYTES = BKP * RBA, B_BYTES = BKP * RBB;
  constexpr int STAGE = A_BYTES + B_BYTES;
  constexpr int IA = A_BYTES / 1024 / 4, IB = B_BYTES / 1024 / 4;   // LDS-DMA instructions per wave and K step
  constexpr int CPA = RBA / 16, CPB = RBB / 16;  // 16-byte chunks per row
  constexpr int RPA = 64 / CPA, RPB = 64 / CPB;  // rows per wave-instruction
  constexpr int LPT = IA + IB, D = NSTAGE - 1;
  constexpr int WM = BMW / 2, WN = BNW / 2, MI = WM / 16, NI = WN / 16;
  __shared__ __attribute__((aligned(1024))) unsigned char smem[NSTAGE * STAGE];

  const LoGeom& g = a.g;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1;
  const int ntile_n = (g.Cout + BMW - 1) / BMW, ntile_c = g.Cin / BNW;
  // logical id -> (tap fastest, then channel tiles, then pixel split): workgroups that read the same pixels are adjacent
  const int wid = lo_xcd_remap(blockIdx.x, gridDim.x);
  int t = wid % a.taps;
  const int tile = (wid / a.taps) % (ntile_n * ntile_c);
  const int tn = tile % ntile_n, tc = tile / ntile_n;
  const int n0 = tn * BMW, c0 = tc * BNW;
  int phase = 0;                   // t enumerates (phase, tap)
  while (t >= g.T[phase]) { t -= g.T[phase]; ++phase; }
  const int dyo = g.dy[phase][t], dxo = g.dx[phase][t];
  const int ooy = g.out_oy[phase], oox = g.out_ox[phase];
  const int split = wid / (a.taps * ntile_n * ntile_c);
  const int ms_begin = split * a.msteps_per_split;
  const int ms_total = (a.M + BKP - 1) / BKP;
  const int ms_end = min(ms_total, ms_begin + a.msteps_per_split);
  const int nk = ms_end - ms_begin;
  const f16* zpage = reinterpret_cast<const f16*>(lo_zero_page);

  // per-lane constants of the DMA instructions
  int a_row[IA], a_col[IA], b_row[IB], b_col[IB];
#pragma unroll
  for (int i = 0; i < IA; ++i) {
    int row = (wave * IA + i) * RPA + lane / CPA, pos = lane % CPA;
    int chunk = (((pos >> 1) ^ lo_tr_swz<RBA>(row)) << 1) | (pos & 1);
    a_row[i] = row;
    a_col[i] = n0 + chunk * 8;
  }
#pragma unroll
  for (int i = 0; i < IB; ++i) {
    int row = (wave * IB + i) * RPB + lane / CPB, pos = lane % CPB;
    int chunk = (((pos >> 1) ^ lo_tr_swz<RBB>(row)) << 1) | (pos & 1);
    b_row[i] = row;
    b_col[i] = c0 + chunk * 8;
  }
  const int pmask_w = g.GW - 1, pmask_h = g.GH - 1;
  // all tensor dims on this path are powers of two (checked by the launcher): multiplies become shifts
  const int sh_hin = g.lg_hin, sh_win = g.lg_win, sh_cin = g.lg_cin, sh_hout = g.lg_hout, sh_wout = g.lg_wout;
  const bool cout_pow2 = g.lg_cout >= 0;

  auto issue = [&](int stage, int ms) __attribute__((always_inline)) {
    unsigned char* sa = smem + stage * STAGE;
    unsigned char* sb = sa + A_BYTES;
    const bool live = ms < ms_end;
#pragma unroll
    for (int i = 0; i < IA; ++i) {
      int m = ms * BKP + a_row[i];
      int gx = m & pmask_w, gy = (m >> g.lgw) & pmask_h, n_img = m >> (g.lgw + g.lgh);
      int oy = gy * g.out_stride + ooy, ox = gx * g.out_stride + oox;
      bool ok = live && m < a.M && a_col[i] < g.Cout;
      const int pix = (((n_img << sh_hout) + oy) << sh_wout) + ox;
      const f16* src = ok ? a.dy + (cout_pow2 ? ((size_t)pix << g.lg_cout) : (size_t)pix * g.Cout) + a_col[i] : zpage;
      lo_dma16(src, (unsigned int)(size_t)(sa + (wave * IA + i) * 1024));
    }
#pragma unroll
    for (int i = 0; i < IB; ++i) {
      int m = ms * BKP + b_row[i];
      int gx = m & pmask_w, gy = (m >> g.lgw) & pmask_h, n_img = m >> (g.lgw + g.lgh);
      int iy = gy * g.in_stride + dyo, ix = gx * g.in_stride + dxo;
      bool ok = live && m < a.M && (unsigned)iy < (unsigned)g.Hin && (unsigned)ix < (unsigned)g.Win;
      const f16* src = ok ? a.x + ((size_t)((((n_img << sh_hin) + iy) << sh_win) + ix) << sh_cin) + b_col[i] : zpage;
      lo_dma16(src, (unsigned int)(size_t)(sb + (wave * IB + i) * 1024));
    }
  };

  f32x4 acc[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // transposed fragment reads.  Each group of 32 pixel rows is assigned to the MFMA k positions by the SAME
  // permutation for both operands (lane group q reads rows 4q..4q+3 and 16+4q..16+4q+3); any consistent k
  // permutation leaves the sum unchanged.
  const int q16 = lane >> 4, i16 = lane & 15;
  const int trow = 4 * q16 + (i16 >> 2);   // row supplied by this lane (first read); +16 for the second
  const int tsub = (i16 & 3) * 8;          // byte offset inside the 32-byte block
  constexpr int KS = BKP / 32;
  int aoff[MI][2 * KS], boff[NI][2 * KS];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int h = 0; h < 2 * KS; ++h) {
      int R = trow + 16 * h, blk = (wm * WM + mi * 16) / 16;
      aoff[mi][h] = R * RBA + ((blk ^ lo_tr_swz<RBA>(R)) * 32) + tsub;
    }
#pragma unroll
  for (int ni = 0; ni < NI; ++ni)
#pragma unroll
    for (int h = 0; h < 2 * KS; ++h) {
      int R = trow + 16 * h, blk = (wn * WN + ni * 16) / 16;
      boff[ni][h] = A_BYTES + R * RBB + ((blk ^ lo_tr_swz<RBB>(R)) * 32) + tsub;
    }

  if (nk > 0) {
#pragma unroll
    for (int s = 0; s < D; ++s) issue(s, ms_begin + s);
    int rs = 0, ws = D % NSTAGE;
    for (int it = 0; it < nk; ++it) {
      LO_VMCNT(LPT * (D - 1));
      __builtin_amdgcn_s_barrier();
      issue(ws, ms_begin + it + D);
      const unsigned char* sbase = smem + rs * STAGE;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        f16x8 af[MI], bf[NI];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          h16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((h16x4 __attribute__((address_space(3)))*)(sbase + aoff[mi][2 * ks]));
          h16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((h16x4 __attribute__((address_space(3)))*)(sbase + aoff[mi][2 * ks + 1]));
          af[mi] = (f16x8){(f16)lo[0], (f16)lo[1], (f16)lo[2], (f16)lo[3], (f16)hi[0], (f16)hi[1], (f16)hi[2], (f16)hi[3]};
        }
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
          h16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((h16x4 __attribute__((address_space(3)))*)(sbase + boff[ni][2 * ks]));
          h16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((h16x4 __attribute__((address_space(3)))*)(sbase + boff[ni][2 * ks + 1]));
          bf[ni] = (f16x8){(f16)lo[0], (f16)lo[1], (f16)lo[2], (f16)lo[3], (f16)hi[0], (f16)hi[1], (f16)hi[2], (f16)hi[3]};
        }
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int ni = 0; ni < NI; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[mi], bf[ni], acc[mi][ni], 0, 0, 0);
      }
      rs = (rs + 1 == NSTAGE) ? 0 : rs + 1;
      ws = (ws + 1 == NSTAGE) ? 0 : ws + 1;
    }
    LO_VMCNT(0);
  }
  // D[n][c] block (mi, ni): lane holds column c = ni*16 + (lane&15), rows n = mi*16 + (lane>>4)*4 + j
  float* slab = a.slab + (size_t)split * a.packed_elems + g.wofs[phase];
  const int Ktot = g.T[phase] * g.Cin;
  const int rs_w = g.rs[phase][t];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      int c = c0 + wn * WN + ni * 16 + (lane & 15);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int n = n0 + wm * WM + mi * 16 + (lane >> 4) * 4 + j;
        if (n < g.Cout) {
          if (a.direct) a.grad[(size_t)n * g.sn + (size_t)c * g.sc + rs_w] = acc[mi][ni][j] * a.scale;
          else slab[(size_t)n * Ktot + t * g.Cin + c] = acc[mi][ni][j];
        }
      }
    }
}

// sum the split slabs and scatter to the canonical fp32 gradient:  grad[n*sn + c*sc + rs] = scale * sum_s slab
// block = 64 column threads x 4 split groups; a column = 4 consecutive packed elements (same n and tap, consecutive c:
// 16-byte slab loads); group sg sums splits sg, sg+4, ... (4 loads in flight), the four partial sums are added in a fixed
// order through LDS (bitwise reproducible).  Small weight tensors (36 k elements, up to 256 splits) get 4x the
// workgroups and 4x the loads in flight of a one-thread-per-column loop.
__device__ __forceinline__ void lo_wgrad_reduce_block(const float* __restrict__ slab, float* __restrict__ grad, const LoGeom& g,
                                                      int total, int nsplit, float scale, int bid) {
  __shared__ f32x4 part[4][64];
  const int col = threadIdx.x & 63, sg = threadIdx.x >> 6;
  const int i = (bid * 64 + col) * 4;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (i < total) {
    const float* src = slab + i;
    int s = sg;
    for (; s + 12 < nsplit; s += 16) {
      f32x4 a0 = *reinterpret_cast<const f32x4*>(src + (size_t)s * total);
      f32x4 a1 = *reinterpret_cast<const f32x4*>(src + (size_t)(s + 4) * total);
      f32x4 a2 = *reinterpret_cast<const f32x4*>(src + (size_t)(s + 8) * total);
      f32x4 a3 = *reinterpret_cast<const f32x4*>(src + (size_t)(s + 12) * total);
      v += a0; v += a1; v += a2; v += a3;
    }
    for (; s < nsplit; s += 4) v += *reinterpret_cast<const f32x4*>(src + (size_t)s * total);
  }
  part[sg][col] = v;
  __syncthreads();
  if (sg != 0 || i >= total) return;
  v = part[0][col] + part[1][col] + part[2][col] + part[3][col];
  int p = 0;
#pragma unroll
  for (int q = 1; q < LO_MAX_PHASE; ++q) if (q < g.n_phase && i >= g.wofs[q]) p = q;
  int j = i - g.wofs[p];
  int K = g.T[p] * g.Cin;
  int n = j / K, k = j - n * K;
  int t = k / g.Cin, c = k - t * g.Cin;
  float* dst = grad + (size_t)n * g.sn + (size_t)c * g.sc + g.rs[p][t];
#pragma unroll
  for (int e = 0; e < 4; ++e) dst[(size_t)e * g.sc] = v[e] * scale;
}
__global__ __launch_bounds__(256) void lo_wgrad_reduce_kernel(const float* __restrict__ slab, float* __restrict__ grad, LoGeom g,
                                                              int total, int nsplit, float scale) {
  lo_wgrad_reduce_block(slab, grad, g, total, nsplit, scale, (int)blockIdx.x);
}
// The same reduction for the 3x3 convolutions (one phase, nine taps, canonical weight W[co][ci][3][3]: sc == 9) with COALESCED
// stores.  The kernel above walks the packed layout [n][tap][c] and scatters every value to n*sn + c*9 + rs: 4-byte stores 36 bytes
// apart, neighbouring lanes 144 bytes apart -- for the 512 x 512 layers (2.4 M elements from two slabs) that was 39 us per launch,
// against 6 us for the small layers whose time is the slab reads (rocprofv3, round 4: 176 us per step over the 15 launches).  Here a
// workgroup owns (output channel n, 64 input channels): its nine tap segments are summed over the splits (thread = (16-byte column,
// tap, split group)), staged in LDS, and leave as ONE contiguous run of 64 x 9 floats in 16-byte stores.  Same split-group order
// as above: the same bits.
__global__ __launch_bounds__(576) void lo_wgrad_reduce_rows_kernel(const float* __restrict__ slab, float* __restrict__ grad, LoGeom g,
                                                                   int total, int nsplit, float scale) {
  __shared__ float part[4][9][64];
  __shared__ int tap_of_rs[9];
  const int x = threadIdx.x, t = threadIdx.y, sg = threadIdx.z, G = blockDim.z;
  const int cblocks = g.Cin >> 6;
  const int n = blockIdx.x / cblocks, c0 = (blockIdx.x - n * cblocks) << 6;
  if (sg == 0 && x == 0) tap_of_rs[g.rs[0][t]] = t;
  const size_t i = (size_t)n * 9 * g.Cin + (size_t)t * g.Cin + c0 + 4 * x;
  const float* src = slab + i;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  int s = sg;
  for (; s + 3 * G < nsplit; s += 4 * G) {
    f32x4 a0 = *reinterpret_cast<const f32x4*>(src + (size_t)s * total);
    f32x4 a1 = *reinterpret_cast<const f32x4*>(src + (size_t)(s + G) * total);
    f32x4 a2 = *reinterpret_cast<const f32x4*>(src + (size_t)(s + 2 * G) * total);
    f32x4 a3 = *reinterpret_cast<const f32x4*>(src + (size_t)(s + 3 * G) * total);
    v += a0; v += a1; v += a2; v += a3;
  }
  for (; s < nsplit; s += G) v += *reinterpret_cast<const f32x4*>(src + (size_t)s * total);
  *reinterpret_cast<f32x4*>(&part[sg][t][4 * x]) = v;
  __syncthreads();
  const int w = x + 16 * (t + 9 * sg);
  if (w >= 144) return;
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int f = 4 * w + e, cc = f / 9, rs = f - cc * 9, tt = tap_of_rs[rs];
    float acc = part[0][tt][cc];
    for (int q = 1; q < G; ++q) acc += part[q][tt][cc];
    o[e] = acc * scale;
  }
  *reinterpret_cast<f32x4*>(grad + (size_t)n * g.sn + (size_t)c0 * 9 + 4 * w) = o;
}
// ... and for the 4x4 stride-2 transposed convolutions (four phases of four taps, canonical weight W[ci][co][4][4]: sn == 16,
// sc == Cout * 16, so the contiguous runs of the gradient are (co, rs) for a fixed ci).  A workgroup owns 16 reduced channels c
// (one 64-byte run of every packed segment) x 4 output channels n: thread = (16-byte column, n, phase, tap) sums its column over the
// splits in split order, the 16 x (4 x 16) block is staged in LDS and leaves as sixteen 256-byte runs in 16-byte stores (the
// scattering kernel needed 15 - 35 us for these four layers).
__global__ __launch_bounds__(256) void lo_wgrad_reduce_convt_kernel(const float* __restrict__ slab, float* __restrict__ grad, LoGeom g,
                                                                    int total, int nsplit, float scale) {
  __shared__ float outb[16][4][16];
  const int tid = threadIdx.x, x = tid & 3, seg = tid >> 2, nl = seg >> 4, p = (seg >> 2) & 3, t = seg & 3;
  const int cblocks = g.Cin >> 4;
  const int nb = blockIdx.x / cblocks, c0 = (blockIdx.x - nb * cblocks) << 4, n0 = nb << 2;
  const size_t i = (size_t)g.wofs[p] + (size_t)(n0 + nl) * 4 * g.Cin + (size_t)t * g.Cin + c0 + 4 * x;
  const float* src = slab + i;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  int s = 0;
  for (; s + 4 <= nsplit; s += 4) {
    f32x4 a0 = *reinterpret_cast<const f32x4*>(src + (size_t)s * total);
    f32x4 a1 = *reinterpret_cast<const f32x4*>(src + (size_t)(s + 1) * total);
    f32x4 a2 = *reinterpret_cast<const f32x4*>(src + (size_t)(s + 2) * total);
    f32x4 a3 = *reinterpret_cast<const f32x4*>(src + (size_t)(s + 3) * total);
    v += a0; v += a1; v += a2; v += a3;
  }
  for (; s < nsplit; ++s) v += *reinterpret_cast<const f32x4*>(src + (size_t)s * total);
  const int rs = g.rs[p][t];
#pragma unroll
  for (int e = 0; e < 4; ++e) outb[4 * x + e][nl][rs] = v[e] * scale;
  __syncthreads();
  const int cc = tid >> 4, q = tid & 15;
  *reinterpret_cast<f32x4*>(grad + (size_t)(c0 + cc) * g.sc + (size_t)n0 * 16 + 4 * q) =
      *reinterpret_cast<const f32x4*>(&outb[cc][q >> 2][(q & 3) * 4]);
}
static bool lo_wgrad_reduce_convt_applies(const LoGeom& g) {
  if (g.n_phase != 4 || g.sn != 16 || g.sc != g.Cout * 16 || g.Cin % 16 != 0 || g.Cout % 4 != 0) return false;
  for (int p = 0; p < 4; ++p)
    if (g.T[p] != 4 || g.wofs[p] != p * 4 * g.Cin * g.Cout) return false;
  return true;
}
static bool lo_wgrad_reduce_rows_applies(const LoGeom& g) {
  return g.n_phase == 1 && g.T[0] == 9 && g.sc == 9 && g.sn == 9 * g.Cin && g.wofs[0] == 0 && g.Cin % 64 == 0;
}

// ---------------------------------------------------------------------------------------------
// The plan (LoWgradChoice, lo_conv.h): kernel, tile, K split, both launches.  Nothing below or in the launchers recomputes any of it.
// ---------------------------------------------------------------------------------------------
// lo_wgrad3x3_mt: 3x3 stride 1, 64-channel tiles, maps cut into 2 x 16 or 4 x 8 chunks
static bool wgrad3_applies(const LoGeom& g) {
  if (g.n_phase != 1 || g.T[0] != 9 || g.in_stride != 1 || g.out_stride != 1) return false;
  if (g.Cin % 64 || g.Cout % 64 || g.Hin != g.Hout || g.Win != g.Wout) return false;
  if (g.Win % 16 == 0) return g.Hin % 2 == 0;
  return g.Win == 8 && g.Hin % 4 == 0;
}
// lo_wgrad_s2_mt: a coarse tensor (64-channel tiles, 4 x 8 chunks) against a fine one of twice the resolution
struct Wgrad2Shape { bool convt; int Hc, Wc, Ca, Cf; };
static bool wgrad2_applies(const LoGeom& g, Wgrad2Shape* s) {
  const bool s2 = g.n_phase == 1 && g.T[0] == 9 && g.in_stride == 2 && g.out_stride == 1;                  // Conv2d k3 s2 p1 forward geometry
  const bool ct = g.n_phase == 4 && g.in_stride == 1 && g.out_stride == 2 && g.T[0] == 4 && g.T[3] == 4;   // ConvTranspose2d k4 s2 p1
  if (!s2 && !ct) return false;
  *s = {ct, s2 ? g.Hout : g.Hin, s2 ? g.Wout : g.Win, s2 ? g.Cout : g.Cin, s2 ? g.Cin : g.Cout};
  return s->Hc % 4 == 0 && s->Wc % 8 == 0 && s->Ca % 64 == 0 && (s->Cf % 64 == 0 || s->Cf == 32);
}
// LO_WGRAD_S2=0: the stride-2 layers' weight gradients through the per-tap kernel lo_wgrad_tn (the round-2 path; A/B)
static bool lo_wgrad_s2_enabled() {
  static const bool on = [] { const char* e = getenv("LO_WGRAD_S2"); return !(e && atoi(e) == 0); }();
  return on;
}

// The split policy: as many K splits as bring the launch to `target` workgroups, but
//   - every split writes (and the reduce pass re-reads) one fp32 slab: the slab traffic stays under ~24 MB per launch ...
//   - ... unless that leaves fewer than `floor` workgroups;
//   - at least `min_units` K units per split, at most `max_splits` splits.
struct WgradPolicy { int target, floor, min_units, max_splits; };
// Per-tap kernel: target 512 / 768 / 1024 swept in round 2, inside +-0.5 %; never below one workgroup per CU; 8 K steps per split.
static constexpr WgradPolicy kPolicyTn = {768, 256, 8, 256};
// Multi-tap kernels: they run on the side stream BESIDE the dependent chain, and every CU one of their 512-thread workgroups holds is
// lost to the chain.  Round 3, sprites/s on the step (interleaved on one box) | serial time of the 8 lo_wgrad3x3_mt launches:
//   target 256 / floor 256 (one workgroup per CU at least)   21 854-21 994 | 0.240 ms
//   192 / 192                                                22 375-22 499 | 0.269 ms
//   256 / 128                                                22 513-22 706 | 0.303 ms   <- shipped
//   128 / 64                                                 22 544-22 747 | 0.340 ms
// fewer, longer workgroups (and less slab traffic) win on the step although the launch alone takes longer.  The same for
// lo_wgrad_s2_mt: with the per-tap policy (>= 256 workgroups) it LOST 1 % on the step against the kernel it replaces (21 014-21 067
// against 21 215-21 251) although alone it is faster: a multi-tap tile has 9 / 16 times fewer tiles per layer, so filling 256 CUs
// took up to 32 position splits and 64 MB of slab per layer.  With a floor of 128: 22 262-22 317 against 21 955-22 019 for the
// per-tap kernel on the same box (+1.3 %).  (max_splits cannot bind below a target of 256.)
static constexpr WgradPolicy kPolicyMt = {256, 128, 4, 256};

static int wgrad_wanted_splits(long tiles, long units, long packed_bytes, const WgradPolicy& p) {
  long want = (p.target + tiles - 1) / tiles;
  long cap = (24L << 20) / (packed_bytes > 0 ? packed_bytes : 1);
  const long floor_wgs = (p.floor + tiles - 1) / tiles;
  if (cap < floor_wgs) cap = floor_wgs;
  if (want > cap) want = cap;
  if (want > units / p.min_units) want = units / p.min_units;
  if (want > p.max_splits) want = p.max_splits;
  return want < 1 ? 1 : (int)want;
}

LoWgradChoice lo_wgrad_choose(const LoGeom& g) {
  LoWgradChoice c{};
  const WgradPolicy* pol = &kPolicyMt;
  Wgrad2Shape s2;
  if (wgrad3_applies(g)) {
    c.kernel = LO_WK_WGRAD3;
    c.tw = g.Win % 16 == 0 ? 16 : 8;
    c.tiles = (g.Cout / 64) * (g.Cin / 64);
    c.units = g.B * g.Hin * g.Win / 32;
    c.block = dim3(512);
  } else if (lo_wgrad_s2_enabled() && wgrad2_applies(g, &s2)) {
    c.kernel = LO_WK_WGRAD2;
    c.convt = s2.convt;
    c.tiles = (s2.Ca / 64) * ((s2.Cf + 63) / 64);
    c.units = g.B * s2.Hc * s2.Wc / 32;
    c.block = dim3(512);
  } else {
    c.kernel = LO_WK_TN;
    pol = &kPolicyTn;
    const long M = (long)g.B * g.GH * g.GW;
    c.bmw = g.Cout % 128 == 0 ? 128 : 64;
    c.bnw = g.Cin % 128 == 0 ? 128 : 64;
    c.bkp = M % 64 == 0 && M >= 1024 ? 64 : 32;
    c.stages = c.bkp == 64 && c.bmw + c.bnw > 192 ? 2 : 3;   // 64-pixel steps: 3 LDS stages where the tile fits (+0.9 % on the step over 2)
    for (int p = 0; p < g.n_phase; ++p) c.taps += g.T[p];
    c.tiles = ((g.Cout + c.bmw - 1) / c.bmw) * (g.Cin / c.bnw) * c.taps;
    c.units = (int)((M + c.bkp - 1) / c.bkp);
    c.block = dim3(256);
  }
  const int total = lo_geom_packed_elems(g);
  const int want = wgrad_wanted_splits(c.tiles, c.units, (long)total * 4, *pol);
  c.units_per_split = (c.units + want - 1) / want;
  c.nsplit = (c.units + c.units_per_split - 1) / c.units_per_split;   // the one "no empty split" rule: trailing splits past the last unit go
  // Exported sizes (lo_wgrad_slab_bytes_for, the workspace sizes) keep the counts they have always had: the wanted count for
  // lo_wgrad_tn and lo_wgrad3x3_mt -- there slabs > nsplit wherever the rule above dropped a split, and the slabs past nsplit are
  // neither written nor read -- and the written count for lo_wgrad_s2_mt.
  c.slabs = c.kernel == LO_WK_WGRAD2 ? c.nsplit : want;
  c.grid = dim3(c.tiles * c.nsplit);
  c.direct = c.kernel == LO_WK_TN && c.nsplit == 1 && g.sc == 1;      // one split of a Linear layer
  // the reduce: the coalescing form where the geometry allows it
  if (c.direct) {
    c.reduce = LO_WR_NONE;
  } else if (lo_wgrad_reduce_rows_applies(g)) {
    c.reduce = LO_WR_ROWS;
    c.rgrid = dim3(g.Cout * (g.Cin / 64));
    c.rblock = dim3(16, 9, c.nsplit >= 4 ? 4 : c.nsplit);             // z: split groups
  } else if (lo_wgrad_reduce_convt_applies(g)) {
    c.reduce = LO_WR_CONVT;
    c.rgrid = dim3((g.Cout / 4) * (g.Cin / 16));
    c.rblock = dim3(256);
  } else {
    c.reduce = LO_WR_SCATTER;
    c.rgrid = dim3((total / 4 + 63) / 64);
    c.rblock = dim3(256);
  }
  return c;
}

size_t lo_wgrad_slab_bytes(const LoGeom& g) { return (size_t)lo_wgrad_choose(g).slabs * lo_geom_packed_elems(g) * sizeof(float); }

// ---------------------------------------------------------------------------------------------
// launchers: arguments from (g, plan)
// ---------------------------------------------------------------------------------------------
static int wgrad_tn_run(const LoGeom& g, const LoWgradChoice& p, const f16* x, const f16* dy, float* slab, float* grad, float scale, hipStream_t st) {
  LO_REQUIRE(g.Cin % 64 == 0 && g.Cout % 32 == 0, "lo_wgrad_run: need Cin %% 64 == 0 and Cout %% 32 == 0 (Cin=%d Cout=%d)", g.Cin, g.Cout);
  LO_REQUIRE(g.lg_hin >= 0 && g.lg_win >= 0 && g.lg_cin >= 0 && g.lg_hout >= 0 && g.lg_wout >= 0,
             "lo_wgrad_run: tensor dims must be powers of two");
  WgradArgs a;
  a.x = x; a.dy = dy; a.slab = slab; a.g = g; a.grad = grad; a.scale = scale;
  a.M = g.B * g.GH * g.GW;
  a.packed_elems = lo_geom_packed_elems(g);
  a.taps = p.taps; a.nsplit = p.nsplit; a.msteps_per_split = p.units_per_split;
  a.direct = p.direct ? 1 : 0;
#define LO_WG(BMW, BNW)                                                                                                          \
  do {                                                                                                                           \
    if (p.bkp == 64 && p.stages == 3) hipLaunchKernelGGL((lo_wgrad_tn<BMW, BNW, 3, 64>), p.grid, p.block, 0, st, a);             \
    else if (p.bkp == 64) hipLaunchKernelGGL((lo_wgrad_tn<BMW, BNW, 2, 64>), p.grid, p.block, 0, st, a);                         \
    else hipLaunchKernelGGL((lo_wgrad_tn<BMW, BNW, 3, 32>), p.grid, p.block, 0, st, a);                                          \
  } while (0)
  if (p.bmw == 128 && p.bnw == 128) LO_WG(128, 128);
  else if (p.bmw == 128 && p.bnw == 64) LO_WG(128, 64);
  else if (p.bmw == 64 && p.bnw == 128) LO_WG(64, 128);
  else LO_WG(64, 64);
#undef LO_WG
  LO_LAUNCH_CHECK("wgrad_tn");
  return LO_OK;
}

// slab [nsplit][packed] -> canonical fp32 gradient (scaled)
static int lo_wgrad_reduce_launch(const LoGeom& g, const LoWgradChoice& p, const float* slab, float* grad, float scale, hipStream_t st) {
  auto* const kernel = p.reduce == LO_WR_ROWS ? lo_wgrad_reduce_rows_kernel : p.reduce == LO_WR_CONVT ? lo_wgrad_reduce_convt_kernel : lo_wgrad_reduce_kernel;
  hipLaunchKernelGGL(kernel, p.rgrid, p.rblock, 0, st, slab, grad, g, lo_geom_packed_elems(g), p.nsplit, scale);
  LO_LAUNCH_CHECK("wgrad_reduce");
  return LO_OK;
}

// (one reduction launch for several layers -- a slab per layer, job table in the workspace -- was built in round 3 and measured 1 %
// SLOWER on the step in both forms tried, all layers at the end of the backward and one launch per stage: the per-layer launch
// right behind its GEMM finds the slab in the Infinity Cache, the merged one re-reads up to 0.2 GB from HBM in front of the join)
int lo_wgrad_run(const LoGeom& g, const f16* x, const f16* dy, float* slab, float* grad, float scale, hipStream_t st) {
  static const char* const scope[3] = {"lo_wgrad3x3_mt", "lo_wgrad_s2_mt", "lo_wgrad_tn"};   // indexed by LoWgradKernel
  const LoWgradChoice p = lo_wgrad_choose(g);
  {
    LoProfScope _p(lo_prof_geom_name(scope[p.kernel], g), lo_geom_flops(g), lo_geom_bytes(g), st);
    int r = p.kernel == LO_WK_WGRAD3   ? lo_wgrad3_run(g, p, x, dy, slab, st)
            : p.kernel == LO_WK_WGRAD2 ? lo_wgrad2_run(g, p, x, dy, slab, st)
                                       : wgrad_tn_run(g, p, x, dy, slab, grad, scale, st);
    if (r != LO_OK) return r;
  }
  if (p.reduce == LO_WR_NONE) return LO_OK;
  LoProfScope _p2(lo_prof_geom_name("lo_wgrad_reduce", g), 0, 4.0 * lo_geom_packed_elems(g) * (p.nsplit + 1), st);
  return lo_wgrad_reduce_launch(g, p, slab, grad, scale, st);
}
