// Implicit-GEMM convolution kernels for gfx950 (MI355X): fp16 NHWC activations, fp32 accumulation on
// v_mfma_f32_16x16x32_f16, LDS-staged operand tiles (register prefetch, two LDS stages, one barrier
// per K step), LDS-staged coalesced epilogue with fused bias / residual-add / GroupNorm partial sums.
//
// One kernel template covers every forward conv, transposed conv (as 4 sub-pixel phases) and every
// data-gradient of the VAE (LoGeom in lo_common.h), plus the Linear layers (1 tap, optional split-K).
// The weight gradients are in lo_wgrad.hip; which kernel runs an op is decided in lo_conv_select.hip.
//
// Reference ops replaced (PyTorch ATen, dispatched from /root/reference/lunar_generate.py):
//   conv2d            :36,41,95,102,109,116   conv_transpose2d :169,175,181,187   linear :124,125,165
#include "lo_conv.h"
#include "lo_conv_dev.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>

// ---------------------------------------------------------------------------------------------
// NT implicit GEMM
// ---------------------------------------------------------------------------------------------
struct IgemmArgs {
  const f16* in;
  const f16* w;        // packed fp16 weights
  const float* bias;   // [Cout] or null
  const f16* add_src;  // same layout as out, or null
  f16* out;
  float* gn_partial;   // [B][MT][8][2] or null
  float* slab;         // split-K fp32 partials [nsplit][M][Cout] (SPLITK only)
  // fused GroupNorm-backward reduction (data-gradient ops): the output of this op is dL/da of a conv+GN+Mish layer
  // whose raw conv output is gb_v; the epilogue also emits P1[n][mtile][c] = (sum du, sum du*xhat), du = da*mish'(u)
  // teacher path: LeakyReLU(0.2) on (conv + bias) and per-channel BatchNorm partial sums of the stored values
  int act;                 // 0 none, 1 LeakyReLU(0.2)
  float* bn_partial;       // [M tiles][Cout][2] (sum, sumsq) or null
  const f16* gb_v;
  const float* gb_stats;   // [B][8][2] mean, rstd
  const float* gb_gamma;
  const float* gb_beta;
  float* gb_P1;
  f16* gb_dv;              // != null: the GroupNorm-backward apply runs here too (LoGnBwdFuse in lo_internal.h)
  float* gb_P2;
  unsigned int* gb_counter;
  unsigned int gb_target;
  unsigned int* gb_fail;
  int gb_keep_out;
  const float* f8_scale;   // fp8 operand path: [n_phase][Cout] dequantisation factor (weight row scale / activation scale)
  int out_pitch, out_choff;   // out_pitch > 0: `out` has out_pitch channels per pixel, this op's channels start at out_choff
  LoGnFuse gf;         // gf.y != null: GroupNorm + Mish of this output in the epilogue (sample rendezvous, lo_common.h)
  int M;               // rows per phase = B*GH*GW
  int nsplit;          // >= 1
  int ksteps_per_split;
  LoGeom g;
};

// Operand tiles go HBM -> LDS by LDS-DMA (global_load_lds_dwordx4): no staging VGPRs and no ds_write pass (the
// ds_write_b128 path sustains only ~80 B/clk/CU, which made the register-staged version LDS-bound).  One
// wave-instruction fills 1 KiB of LDS linearly, so tiles are unpadded [rows][BK] and bank conflicts are removed by an
// XOR swizzle applied on the per-lane SOURCE chunk and again on the fragment read: chunk' = chunk ^ ((row >> 1) & (CPR-1)).
// NSTAGE LDS stages, NSTAGE-1 K steps in flight behind a counted s_waitcnt vmcnt + one raw s_barrier per K step.
// F8: both operands are OCP e4m3 bytes (in / w point at bytes, every element offset below is scaled by ES), BK = 128 elements
// so a tile row is the same 128 bytes as the fp16 BK = 64 row, and one K step is ONE v_mfma_scale_f32_16x16x128_f8f6f4 per
// 16x16 block (lane holds row lane&15 and 32 bytes of k: chunks fq and fq + 4 of the row; unit block scales) - twice the
// K per byte moved and per MFMA cycle.  The epilogue multiplies by f8_scale[phase][n] before the bias.
template <int BM, int BN, int BK, int NSTAGE, bool F8>
constexpr int igemm_lds_bytes() {   // the K-loop ring, or the epilogue's staging tile + reduction scratch, whichever is larger
  constexpr int ring = NSTAGE * (BM + BN) * BK * (F8 ? 1 : 2);
  constexpr int epi = BM * (BN * 2 + 16) + 16384 + 1024;
  return ring > epi ? ring : epi;
}

template <int BM, int BN, int BK, int NSTAGE, bool SPLITK, bool F8 = false>
__global__ __launch_bounds__(256) void lo_igemm_nt(IgemmArgs a) {
  constexpr int ES = F8 ? 1 : 2;          // bytes per operand element
  constexpr int CE = 16 / ES;             // elements per 16-byte chunk
  constexpr int CPR = BK / CE;            // 16-byte chunks per tile row
  constexpr int RPI = 64 / CPR;           // tile rows filled by one wave-instruction
  constexpr int ROWB = BK * ES;           // bytes per tile row
  static_assert(!(F8 && SPLITK) && (!F8 || BK == 128), "fp8 path: BK = 128, no split-K");
  constexpr int IA = BM / RPI / 4, IB = BN / RPI / 4;   // LDS-DMA instructions per wave and K step (A, B)
  static_assert(IA >= 1 && IB >= 1 && IA * RPI * 4 == BM && IB * RPI * 4 == BN, "tile / wave-instruction mismatch");
  constexpr int LPT = IA + IB;
  constexpr int D = NSTAGE - 1;           // K steps in flight
  static_assert(LPT * D <= 63, "vmcnt range");
  constexpr int A_BYTES = BM * ROWB, B_BYTES = BN * ROWB;
  constexpr int STAGE = A_BYTES + B_BYTES;
  constexpr int WM = BM / 2, WN = BN / 2; // wave tile (2 x 2 waves)
  constexpr int MI = WM / 16, NI = WN / 16;
  constexpr int OPITCH = BN * 2 + 16;     // epilogue staging pitch (bytes)
  // the epilogue's reduction scratch `red` ([256][16] floats behind the staging tile) lies inside the allocation whatever the ring size
  static_assert(BM * OPITCH + 16384 <= igemm_lds_bytes<BM, BN, BK, NSTAGE, F8>(), "epilogue scratch outside the LDS allocation");
  // dynamic LDS (igemm_lds_bytes<...>() bytes, passed by the launcher): the deep-pipeline instantiations exceed the 64 KB a static
  // array may have; it is the kernel's only LDS object, so it starts at offset 0 (1 KB-aligned DMA destinations)
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];

  const LoGeom& g = a.g;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1;
  // logical tile id -> (n tile fastest, then m tile, then phase / K split)
  const int NT = g.Cout / BN, MT = (a.M + BM - 1) / BM;
  const int tile_id = lo_xcd_remap(blockIdx.x, gridDim.x);
  int nt_i = tile_id % NT, mt_i = (tile_id / NT) % MT, z_i = tile_id / (NT * MT);
  if (!SPLITK && a.gf.y) {
    // fused GroupNorm: the tiles of one sample wait for each other, so they get adjacent ids (sample, phase, m tile, n tile) --
    // the default order puts the phase outermost, i.e. a sample's tiles a whole grid quarter apart
    const int rows_ps = (g.GH * g.GW) / BM, tiles_ps = rows_ps * g.n_phase * NT;
    const int n_s = tile_id / tiles_ps, r = tile_id - n_s * tiles_ps;
    const int row = r / NT;
    nt_i = r - row * NT;
    z_i = row / rows_ps;
    mt_i = n_s * rows_ps + (row - z_i * rows_ps);
  }
  const int m0 = mt_i * BM, n0 = nt_i * BN;
  const int phase = SPLITK ? 0 : z_i;
  const int split = SPLITK ? z_i : 0;
  const int T = g.T[phase];
  const int KCB = g.Cin / BK;
  const int ksteps_total = T * KCB;
  int ks_begin = 0, ks_end = ksteps_total;
  if (SPLITK) {
    ks_begin = split * a.ksteps_per_split;
    ks_end = min(ksteps_total, ks_begin + a.ksteps_per_split);
  }
  const int nk = ks_end - ks_begin;
  const int Ktot = T * g.Cin;
  const unsigned char* inb = reinterpret_cast<const unsigned char*>(a.in);
  const unsigned char* wbase = reinterpret_cast<const unsigned char*>(a.w) + (size_t)g.wofs[phase] * ES;
  const unsigned char* zpage = reinterpret_cast<const unsigned char*>(lo_zero_page);
  const uint32_t dyc = g.dyc[phase], dxc = g.dxc[phase];   // tap offsets in registers: no memory load inside the K loop

  // per-lane source coordinates of the LDS-DMA instructions this wave issues.  Everything that depends only on the
  // tap is recomputed when the tap changes; a K step then costs one add + one select per instruction.
  const int lrow = lane / CPR, lpos = lane % CPR;
  int a_base[IA], a_iy0[IA], a_ix0[IA];   // element offset of (n, iy0, ix0, chunk); -1 = row out of range
#pragma unroll
  for (int i = 0; i < IA; ++i) {
    int row = (wave * IA + i) * RPI + lrow;
    int m = m0 + row;
    bool ok = m < a.M;
    int mm = ok ? m : 0;
    int gx = mm & (g.GW - 1), gy = (mm >> g.lgw) & (g.GH - 1), n_img = mm >> (g.lgw + g.lgh);
    a_iy0[i] = ok ? gy * g.in_stride : -100000;       // makes every tap invalid for an out-of-range row
    a_ix0[i] = gx * g.in_stride;
    a_base[i] = ((n_img * g.Hin + gy * g.in_stride) * g.Win + gx * g.in_stride) * g.Cin +
                (lpos ^ ((row >> 1) & (CPR - 1))) * CE;  // logical chunk stored at this lane's LDS slot
  }
  int b_base[IB];
#pragma unroll
  for (int i = 0; i < IB; ++i) {
    int row = (wave * IB + i) * RPI + lrow;
    b_base[i] = (n0 + row) * Ktot + (lpos ^ ((row >> 1) & (CPR - 1))) * CE;
  }
  // issue-side K position (tap, channel block) and the per-tap source offsets
  int i_t = ks_begin / KCB, i_cb = ks_begin - i_t * KCB, i_ks = ks_begin;
  int a_tap[IA];
  auto set_tap = [&](int t) __attribute__((always_inline)) {
    int dy = (int)((dyc >> (2 * t)) & 3u) - 1, dx = (int)((dxc >> (2 * t)) & 3u) - 1;
    int delta = (dy * g.Win + dx) * g.Cin;
#pragma unroll
    for (int i = 0; i < IA; ++i) {
      bool ok = (unsigned)(a_iy0[i] + dy) < (unsigned)g.Hin && (unsigned)(a_ix0[i] + dx) < (unsigned)g.Win;
      a_tap[i] = ok ? a_base[i] + delta : -1;
    }
  };
  set_tap(i_t < T ? i_t : 0);

  auto issue = [&](int stage) __attribute__((always_inline)) {
    unsigned char* sa = smem + stage * STAGE;
    unsigned char* sb = sa + A_BYTES;
    const bool live = i_ks < ks_end;
    const int coff = i_cb * BK;
#pragma unroll
    for (int i = 0; i < IA; ++i) {
      const unsigned char* src = (live && a_tap[i] >= 0) ? inb + (size_t)(a_tap[i] + coff) * ES : zpage;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)(sa + (wave * IA + i) * 1024), 16, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < IB; ++i) {
      const unsigned char* src = live ? wbase + (size_t)(b_base[i] + i_ks * BK) * ES : zpage;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)(sb + (wave * IB + i) * 1024), 16, 0, 0);
    }
    ++i_ks;
    if (++i_cb == KCB) {
      i_cb = 0;
      ++i_t;
      if (i_t < T) set_tap(i_t);
    }
  };

  f32x4 acc[NI][MI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni)
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) acc[ni][mi] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fq = lane >> 4;
  // fragment read offsets (bytes inside a stage), swizzled like the DMA sources
  constexpr int NKK = F8 ? BK / 128 : BK / 32;   // MFMA k sub-steps per K step
  constexpr int CPF = F8 ? 2 : 1;                // 16-byte chunks per lane fragment
  int xoff[MI][NKK][CPF], woff[NI][NKK][CPF];
#pragma unroll
  for (int kk = 0; kk < NKK; ++kk)
#pragma unroll
    for (int cf = 0; cf < CPF; ++cf) {
      // F8: the lane's 32-byte fragment = chunks (fq, fq + 4) of the 128-byte row, the same two reads as the fp16 k sub-steps (the
      // adjacent pair (2 fq, 2 fq + 1) would touch only every other 16-byte slot per read: 2-way bank conflicts); both operands
      // go through this chunk -> k map, so the product is unchanged
      const int chunk = F8 ? kk * 8 + cf * 4 + fq : kk * 4 + fq;
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        int R = wm * WM + mi * 16 + fr;
        xoff[mi][kk][cf] = R * ROWB + ((chunk ^ ((R >> 1) & (CPR - 1))) * 16);
      }
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        int R = wn * WN + ni * 16 + fr;
        woff[ni][kk][cf] = A_BYTES + R * ROWB + ((chunk ^ ((R >> 1) & (CPR - 1))) * 16);
      }
    }

  if (nk > 0) {
#pragma unroll
    for (int s = 0; s < D; ++s) issue(s);
    int rs = 0;            // stage being read
    int ws = D % NSTAGE;   // stage being refilled
    for (int it = 0; it < nk; ++it) {
      LO_VMCNT(LPT * (D - 1));          // this wave's DMA for K step `it` has landed ...
      __builtin_amdgcn_s_barrier();     // ... and so has every other wave's; stage `ws` is no longer being read
      issue(ws);
      const unsigned char* sbase = smem + rs * STAGE;
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) {
        if constexpr (F8) {
          i32x8 wf[NI], xf[MI];
#pragma unroll
          for (int ni = 0; ni < NI; ++ni) {
            const i32x4 lo = *reinterpret_cast<const i32x4*>(sbase + woff[ni][kk][0]), hi = *reinterpret_cast<const i32x4*>(sbase + woff[ni][kk][1]);
            wf[ni] = (i32x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          }
#pragma unroll
          for (int mi = 0; mi < MI; ++mi) {
            const i32x4 lo = *reinterpret_cast<const i32x4*>(sbase + xoff[mi][kk][0]), hi = *reinterpret_cast<const i32x4*>(sbase + xoff[mi][kk][1]);
            xf[mi] = (i32x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          }
#pragma unroll
          for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)   // formats 0 / 0 = e4m3 x e4m3; block scales 0x7f = 2^0
              acc[ni][mi] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[ni], xf[mi], acc[ni][mi], 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
        } else {
          f16x8 wf[NI], xf[MI];
#pragma unroll
          for (int ni = 0; ni < NI; ++ni) wf[ni] = *reinterpret_cast<const f16x8*>(sbase + woff[ni][kk][0]);
#pragma unroll
          for (int mi = 0; mi < MI; ++mi) xf[mi] = *reinterpret_cast<const f16x8*>(sbase + xoff[mi][kk][0]);
#pragma unroll
          for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
              acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[ni], xf[mi], acc[ni][mi], 0, 0, 0);
        }
      }
      rs = (rs + 1 == NSTAGE) ? 0 : rs + 1;
      ws = (ws + 1 == NSTAGE) ? 0 : ws + 1;
    }
    LO_VMCNT(0);                        // drain the (dummy) tail DMAs before LDS is reused by the epilogue
  }
  __syncthreads();

  // D^T block (ni, mi): lane holds pixel m = mi*16 + fr, channels n = ni*16 + fq*4 + {0..3}
  if (SPLITK) {
    float* slab = a.slab + (size_t)split * a.M * g.Cout;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      int m = m0 + wm * WM + mi * 16 + fr;
      if (m < a.M) {
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
          int n = n0 + wn * WN + ni * 16 + fq * 4;
          *reinterpret_cast<f32x4*>(slab + (size_t)m * g.Cout + n) = acc[ni][mi];
        }
      }
    }
    return;
  }

  // ---- epilogue: bias, stage fp16 tile in LDS, then coalesced 16-byte stores (+ residual add, GN partials)
  unsigned char* so = smem;  // all waves are past the last barrier of the K loop
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    int nl = wn * WN + ni * 16 + fq * 4;
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (a.bias) bv = *reinterpret_cast<const f32x4*>(a.bias + n0 + nl);
    f32x4 sv = {1.f, 1.f, 1.f, 1.f};
    if constexpr (F8) sv = *reinterpret_cast<const f32x4*>(a.f8_scale + (size_t)phase * g.Cout + n0 + nl);
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      int ml = wm * WM + mi * 16 + fr;
      f32x4 v = F8 ? acc[ni][mi] * sv + bv : acc[ni][mi] + bv;
      f16x4 h = {(f16)v[0], (f16)v[1], (f16)v[2], (f16)v[3]};
      *reinterpret_cast<f16x4*>(so + ml * OPITCH + nl * 2) = h;
    }
  }
  __syncthreads();
  constexpr int OCPR = BN / 8, ORPP = 256 / OCPR, OP = BM / ORPP;
  const int orow = tid / OCPR, ochunk = tid % OCPR;
  const int G = g.Cout >> 3;          // channels per GroupNorm group (8 groups)
  float s0 = 0.f, q0 = 0.f, s1 = 0.f, q1 = 0.f;
  // fused GN-backward reduction: per-thread constants of its 8 channels (the tile lies inside one sample)
  float gsc[8], gsh[8], ga1[8], ga2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { ga1[j] = 0.f; ga2[j] = 0.f; }
  if (a.gb_v) {
    const int n_img_t = m0 >> (g.lgw + g.lgh);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int c = n0 + ochunk * 8 + j;
      int grp = c / G;
      float mean = a.gb_stats[n_img_t * 16 + grp * 2], rstd = a.gb_stats[n_img_t * 16 + grp * 2 + 1];
      gsc[j] = a.gb_gamma[c] * rstd;
      gsh[j] = a.gb_beta[c] - mean * gsc[j];
    }
  }
#pragma unroll
  for (int i = 0; i < OP; ++i) {
    int ml = orow + i * ORPP;
    int m = m0 + ml;
    if (m >= a.M) continue;
    f16x8 h = *reinterpret_cast<const f16x8*>(so + ml * OPITCH + ochunk * 16);
    // the output grid is a power of two in both directions (lo_make_geom checks): shifts, not divisions
    int n_img = m >> (g.lgw + g.lgh);
    int gy = (m >> g.lgw) & (g.GH - 1), gx = m & (g.GW - 1);
    int oy = gy * g.out_stride + g.out_oy[phase], ox = gx * g.out_stride + g.out_ox[phase];
    size_t off = ((size_t)(n_img * g.Hout + oy) * g.Wout + ox) * g.Cout + n0 + ochunk * 8;
    if (a.add_src) {
      f16x8 r = *reinterpret_cast<const f16x8*>(a.add_src + off);
#pragma unroll
      for (int j = 0; j < 8; ++j) h[j] = (f16)((float)h[j] + (float)r[j]);
    }
    if (a.act == 1) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { float x = (float)h[j]; h[j] = (f16)(x > 0.f ? x : 0.2f * x); }
    }
    if (a.out_pitch > 0)   // concatenated output tensor (teacher feature extractor); add_src / gb_v are not used with it
      *reinterpret_cast<f16x8*>(a.out + ((size_t)(n_img * g.Hout + oy) * g.Wout + ox) * a.out_pitch + a.out_choff + n0 + ochunk * 8) = h;
    else if (a.gb_dv) {    // fused GroupNorm-backward apply: the activation gradient lives on in this tile (LDS); stored only if somebody else reads it
      *reinterpret_cast<f16x8*>(so + ml * OPITCH + ochunk * 16) = h;
      if (a.gb_keep_out) *reinterpret_cast<f16x8*>(a.out + off) = h;
    } else
      *reinterpret_cast<f16x8*>(a.out + off) = h;
    if (a.bn_partial) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { float x = (float)h[j]; ga1[j] += x; ga2[j] += x * x; }
    }
    if (a.gb_v) {
      f16x8 vv = *reinterpret_cast<const f16x8*>(a.gb_v + off);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float hv = (float)vv[j];
        float du = (float)h[j] * lo_mish_grad(hv * gsc[j] + gsh[j]);
        ga1[j] += du;
        ga2[j] += du * hv;          // sum du*xhat = rstd * (sum du*v - mean * sum du): finished after the loop
      }
    }
    if (a.gn_partial || a.gf.y) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { float x = (float)h[j]; s0 += x; q0 += x * x; }
#pragma unroll
      for (int j = 4; j < 8; ++j) { float x = (float)h[j]; s1 += x; q1 += x * x; }
    }
  }
  if (a.bn_partial) {
    // per-channel (sum, sumsq) of this tile, fixed summation order -> bn_partial[m tile][channel][2]
    float* red = reinterpret_cast<float*>(smem + BM * OPITCH);   // [256][16] floats
#pragma unroll
    for (int j = 0; j < 8; ++j) { red[tid * 16 + j * 2] = ga1[j]; red[tid * 16 + j * 2 + 1] = ga2[j]; }
    __syncthreads();
    float* dst = a.bn_partial + ((size_t)(phase * MT + mt_i) * g.Cout + n0) * 2;
    for (int o = tid; o < BN * 2; o += 256) {
      int cl = o >> 1, w = o & 1;
      int ccx = cl >> 3, j = cl & 7;
      float tot = 0.f;
      for (int r = 0; r < ORPP; ++r) tot += red[(r * OCPR + ccx) * 16 + j * 2 + w];
      dst[o] = tot;
    }
    __syncthreads();
  }
  if (a.gb_v) {
    // the saved mean / rstd are read here, after the store loop, not held in registers across it
    const int n_img_t = m0 >> (g.lgw + g.lgh);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int grp = (n0 + ochunk * 8 + j) / G;
      float mean = a.gb_stats[n_img_t * 16 + grp * 2], rstd = a.gb_stats[n_img_t * 16 + grp * 2 + 1];
      ga2[j] = rstd * (ga2[j] - mean * ga1[j]);
    }
    // reduce (ga1, ga2) over the row slots in a fixed order: BN*2 outputs, one per thread (looped)
    float* red = reinterpret_cast<float*>(smem + BM * OPITCH);   // [256][16] floats
#pragma unroll
    for (int j = 0; j < 8; ++j) { red[tid * 16 + j * 2] = ga1[j]; red[tid * 16 + j * 2 + 1] = ga2[j]; }
    __syncthreads();
    const int per_sample = g.GH * g.GW;
    const int n_img = m0 / per_sample;
    const int mt = (m0 - n_img * per_sample) / BM;
    const int MTs = (per_sample / BM) * g.n_phase;
    float* dst = a.gb_P1 + (((size_t)n_img * MTs + phase * (per_sample / BM) + mt) * g.Cout + n0) * 2;
    for (int o = tid; o < BN * 2; o += 256) {
      int cl = o >> 1, w = o & 1;
      int ccx = cl >> 3, j = cl & 7;
      float tot = 0.f;
      for (int r = 0; r < ORPP; ++r) tot += red[(r * OCPR + ccx) * 16 + j * 2 + w];
      if (a.gb_dv) __hip_atomic_store(reinterpret_cast<unsigned int*>(dst) + o, __float_as_uint(tot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else dst[o] = tot;
    }
    if (a.gb_dv) {
      // ---- GroupNorm-backward APPLY of the producing layer, here: wait until every m tile of this sample (same n tile) has
      //      published its P1 row, form the gamma-weighted group sums in lo_gn_bwd_apply's order, turn the tile's activation
      //      gradient (still in LDS) into dv.  Single phase ops only (the launcher checks).
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      lo_arrive_and_wait(a.gb_counter + n_img * NT + nt_i, a.gb_target, a.gb_fail, tid);
      float* s_g = red;                   // [BN][2] gamma-weighted per-channel totals
      float* s_c = red + 2 * BN;          // [BN / G][2] group means of (gamma du, gamma du xhat)
      for (int c = tid; c < BN; c += 256) {
        float t1 = 0.f, t2 = 0.f;
        const unsigned int* p = reinterpret_cast<const unsigned int*>(a.gb_P1) + ((size_t)n_img * MTs * g.Cout + n0 + c) * 2;
        for (int k = 0; k < MTs; ++k) {
          t1 += __uint_as_float(__hip_atomic_load(p + (size_t)k * g.Cout * 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
          t2 += __uint_as_float(__hip_atomic_load(p + (size_t)k * g.Cout * 2 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        }
        const float gm = a.gb_gamma[n0 + c];
        s_g[c * 2] = gm * t1;
        s_g[c * 2 + 1] = gm * t2;
      }
      __syncthreads();
      if (tid < (BN / G) * 2) {
        const int gl = tid >> 1, w = tid & 1;
        float tot = 0.f;
        for (int c = gl * G; c < (gl + 1) * G; ++c) tot += s_g[c * 2 + w];
        s_c[tid] = tot / ((float)per_sample * (float)G);
      }
      __syncthreads();
      // this thread's 8 channels lie in ONE group (G >= 8: checked by the launcher)
      const int gl = (ochunk * 8) / G, grp = n0 / G + gl;
      const float mean = a.gb_stats[n_img * 16 + grp * 2], rstd = a.gb_stats[n_img * 16 + grp * 2 + 1];
      const float nmr = -mean * rstd, kb = rstd * s_c[gl * 2], kc = rstd * s_c[gl * 2 + 1];
      float sc[8], sh[8], acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float gm = a.gb_gamma[n0 + ochunk * 8 + j];
        sc[j] = gm * rstd;
        sh[j] = __builtin_fmaf(nmr, gm, a.gb_beta[n0 + ochunk * 8 + j]);
        acc[j] = 0.f;
      }
#pragma unroll
      for (int i = 0; i < OP; ++i) {
        const int ml = orow + i * ORPP;
        const int m = m0 + ml;
        if (m >= a.M) continue;
        const f16x8 d = *reinterpret_cast<const f16x8*>(so + ml * OPITCH + ochunk * 16);
        const int gy = (m >> g.lgw) & (g.GH - 1), gx = m & (g.GW - 1);
        const size_t off = ((size_t)(n_img * g.Hout + gy) * g.Wout + gx) * g.Cout + n0 + ochunk * 8;
        const f16x8 vv = *reinterpret_cast<const f16x8*>(a.gb_v + off);
        f16x8 outv;
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
          lo_f2 du, xh;
          lo_gn_du2_plain((lo_f2){(float)vv[j], (float)vv[j + 1]}, (lo_f2){(float)d[j], (float)d[j + 1]}, (lo_f2){sc[j], sc[j + 1]},
                          (lo_f2){sh[j], sh[j + 1]}, (lo_f2){rstd, rstd}, (lo_f2){nmr, nmr}, du, xh);
          const lo_f2 dv = lo_gn_dv2(du, xh, (lo_f2){sc[j], sc[j + 1]}, kb, kc);
          const f16 d0 = (f16)dv[0], d1 = (f16)dv[1];
          outv[j] = d0; outv[j + 1] = d1;
          acc[j] += (float)d0; acc[j + 1] += (float)d1;
        }
        *reinterpret_cast<f16x8*>(a.gb_dv + off) = outv;
      }
      // per-channel sums of dv of this tile (conv bias gradient partials), fixed order over the row slots
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 8; ++j) red[tid * 8 + j] = acc[j];
      __syncthreads();
      for (int c = tid; c < BN; c += 256) {
        const int ccx = c >> 3, j = c & 7;
        float tot = 0.f;
        for (int r = 0; r < ORPP; ++r) tot += red[(r * OCPR + ccx) * 8 + j];
        a.gb_P2[((size_t)n_img * MTs + mt) * g.Cout + n0 + c] = tot;
      }
    }
    if (a.gn_partial) __syncthreads();   // the section below reuses `red` (no caller sets both today; the barrier keeps that legal)
  }
  if (a.gn_partial || a.gf.y) {
    // deterministic block reduction of the per-thread (sum, sumsq) of the two 4-channel halves of each chunk:
    //   level 1: 256 threads, each adds ORPP/P row slots of one (chunk, value)   level 2: P partials -> chunk sums
    //   level 3: half-chunks of a group (<= 16) -> group sums
    float* red = reinterpret_cast<float*>(smem + BM * OPITCH);  // [256][4] floats, then [P][NV], then [NV]
    red[tid * 4 + 0] = s0; red[tid * 4 + 1] = q0; red[tid * 4 + 2] = s1; red[tid * 4 + 3] = q1;
    constexpr int NV = OCPR * 4;          // values per row slot
    constexpr int P = 256 / NV;           // parts
    constexpr int RPP2 = ORPP / P;        // row slots per part
    static_assert(P >= 1 && RPP2 * P == ORPP, "epilogue reduction shape");
    float* red2 = red + 1024;
    float* red3 = red2 + 256;
    float* s_x = red3 + 64;               // fused GroupNorm: this tile's exchange line (32 floats), then the sample's statistics (16)
    float* s_stat = s_x + 32;
    if (tid < 32) s_x[tid] = 0.f;
    __syncthreads();
    {
      const int o = tid % NV, part = tid / NV;
      float t = 0.f;
#pragma unroll
      for (int r = 0; r < RPP2; ++r) t += red[((part * RPP2 + r) * OCPR) * 4 + o];
      red2[part * NV + o] = t;
    }
    __syncthreads();
    if (tid < NV) {
      float t = 0.f;
#pragma unroll
      for (int q = 0; q < P; ++q) t += red2[q * NV + tid];
      red3[tid] = t;                      // index = chunk*4 + half*2 + which
    }
    __syncthreads();
    const int ngroups = BN / G;           // BN >= G is checked by the launcher
    const int per_sample = g.GH * g.GW;
    const int n_img = m0 / per_sample;
    const int mt = (m0 - n_img * per_sample) / BM;
    const int MTs = (per_sample / BM) * g.n_phase;
    const int row = phase * (per_sample / BM) + mt;
    if (tid < ngroups * 2) {
      int gl = tid >> 1, which = tid & 1;
      int hc_begin = gl * G / 4, hc_end = (gl + 1) * G / 4;
      float tot = 0.f;
      for (int hc = hc_begin; hc < hc_end; ++hc) tot += red3[(hc >> 1) * 4 + (hc & 1) * 2 + which];
      int grp = (n0 / G) + gl;
      if (a.gn_partial) a.gn_partial[(((size_t)n_img * MTs + row) * 8 + grp) * 2 + which] = tot;
      s_x[grp * 2 + which] = tot;
    }
    if (a.gf.y) {
      // ---- GroupNorm + Mish of this tile, once the whole sample's sums are known (lo_common.h: LoGnFuse)
      __syncthreads();
      lo_gn_rendezvous(a.gf, n_img, row, nt_i, G, BN, 1.0f / ((float)(per_sample * g.n_phase) * (float)G), s_x, s_stat, tid);
      if (row == 0 && nt_i == 0 && tid < 16 && a.gf.stats) a.gf.stats[n_img * 16 + tid] = s_stat[tid];
      float sc[8], sh[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = n0 + ochunk * 8 + j, grp = c / G;
        const float mean = s_stat[grp * 2], rstd = s_stat[grp * 2 + 1];
        lo_gn_scale_shift(a.gf.gamma[c], a.gf.beta[c], mean, rstd, sc[j], sh[j]);
      }
#pragma unroll
      for (int i = 0; i < OP; ++i) {
        const int ml = orow + i * ORPP;
        const int m = m0 + ml;
        if (m >= a.M) continue;
        const f16x8 h = *reinterpret_cast<const f16x8*>(so + ml * OPITCH + ochunk * 16);
        const int gy = (m >> g.lgw) & (g.GH - 1), gx = m & (g.GW - 1);
        const int oy = gy * g.out_stride + g.out_oy[phase], ox = gx * g.out_stride + g.out_ox[phase];
        const size_t off = ((size_t)(n_img * g.Hout + oy) * g.Wout + ox) * g.Cout + n0 + ochunk * 8;
        f16x8 o = h;
        if (a.gf.mode != 0) o = *reinterpret_cast<const f16x8*>(a.gf.other + off);
        *reinterpret_cast<f16x8*>(a.gf.y + off) = lo_gn_apply8(h, sc, sh, a.gf.mode, o);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// split-K slab reduction: out[m][n] = bias[n] + sum_s slab[s][m][n]   (fp32 and/or fp16 outputs)
// ---------------------------------------------------------------------------------------------
__global__ void lo_splitk_reduce_kernel(const float* __restrict__ slab, const float* __restrict__ bias,
                                        float* __restrict__ out32, f16* __restrict__ out16, int M, int N, int nsplit) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * N) return;
  int n = i % N;
  float v = bias ? bias[n] : 0.f;
  int s = 0;
  for (; s + 8 <= nsplit; s += 8) {              // eight loads in flight, added in split order
    float t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = slab[(size_t)(s + u) * M * N + i];
#pragma unroll
    for (int u = 0; u < 8; ++u) v += t[u];
  }
  for (; s < nsplit; ++s) v += slab[(size_t)s * M * N + i];
  if (out32) out32[i] = v;
  if (out16) out16[i] = (f16)v;
}

template <int BM, int BN, int BK, int NS, bool SK, bool F8 = false>
static int igemm_launch(dim3 grid, const IgemmArgs& a, hipStream_t st) {
  constexpr int lds = igemm_lds_bytes<BM, BN, BK, NS, F8>();
  static_assert(lds <= 160 * 1024, "LDS");
  if constexpr (lds > 65536) {
    static bool attr = false;
    if (!attr) {
      LO_HIP(hipFuncSetAttribute((const void*)lo_igemm_nt<BM, BN, BK, NS, SK, F8>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      attr = true;
    }
  }
  LO_LAUNCH_STOP((lo_igemm_nt<BM, BN, BK, NS, SK, F8>), grid, dim3(256), lds, st, a);   // may carry the hand-over event of the dv it writes
  return LO_OK;
}

template <int BM, int BN, int BK>
static int launch_igemm(const IgemmArgs& a, int nwg, hipStream_t st) {
  const LoGeom& g = a.g;
  static char name[64];
  snprintf(name, sizeof(name), "lo_igemm_nt<%d,%d,%d>%s", BM, BN, BK, a.nsplit > 1 ? "/splitK" : "");  // same text for every call of this instantiation
  // algorithmic bytes of the FUSED op: operands + output once, plus what its epilogue must read by definition: the residual
  // / skip gradient it adds (add_src) and the producing layer's raw conv output for the fused GroupNorm-backward reduction
  // (gb_v), each the size of the output
  const double out_bytes = 2.0 * (double)g.B * g.Hout * g.Wout * g.Cout;
  LoProfScope _p(lo_prof_geom_name(name, g), lo_geom_flops(g), lo_geom_bytes(g) + (a.add_src ? out_bytes : 0.0) + (a.gb_v ? out_bytes : 0.0), st);
  dim3 grid(nwg);     // LoConvChoice::grid: m tiles x n tiles x (phases, or K splits)
  constexpr int STAGE_BYTES = (BM + BN) * BK * 2;
  constexpr int NSTAGE = STAGE_BYTES >= 32768 ? 2 : (STAGE_BYTES >= 16384 ? 3 : 4);
  // short K loops (<= 9 steps: the 64-channel 3x3 layers) are prologue / epilogue bound: one LDS stage less puts a third
  // workgroup on the CU (measured 46.9 -> 39.8 us at 64 channels, 64x64; no gain on the longer loops; more stages where the grid
  // leaves LDS unused did not make any launch faster either: these launches sit at the L2 -> LDS rate)
  int ksteps_max = 0;
  for (int p = 0; p < g.n_phase; ++p) ksteps_max = g.T[p] * (g.Cin / BK) > ksteps_max ? g.T[p] * (g.Cin / BK) : ksteps_max;
  const bool shallow = ksteps_max <= 9;
  if (a.nsplit > 1)
    LO_CHECK(igemm_launch<BM, BN, BK, NSTAGE, true>(grid, a, st));
  else if (shallow && NSTAGE > 2)
    LO_CHECK(igemm_launch<BM, BN, BK, (NSTAGE > 2 ? NSTAGE - 1 : 2), false>(grid, a, st));
  else
    LO_CHECK(igemm_launch<BM, BN, BK, NSTAGE, false>(grid, a, st));
  LO_LAUNCH_CHECK("igemm");
  return LO_OK;
}

// ---- fp8 operand path -------------------------------------------------------------------------------------------------
template <int BM, int BN>
static int launch_igemm_f8(const IgemmArgs& a, int nwg, hipStream_t st) {
  const LoGeom& g = a.g;
  static char name[64];
  snprintf(name, sizeof(name), "lo_igemm_nt<%d,%d,128>/fp8", BM, BN);
  LoProfScope _p(lo_prof_geom_name(name, g), lo_geom_flops(g), 0.5 * lo_geom_bytes(g) + (double)g.B * g.Hout * g.Wout * g.Cout, st);
  dim3 grid(nwg);
  constexpr int STAGE_BYTES = (BM + BN) * 128;
  constexpr int NSTAGE = STAGE_BYTES >= 32768 ? 2 : (STAGE_BYTES >= 16384 ? 3 : 4);
  LO_CHECK((igemm_launch<BM, BN, 128, NSTAGE, false, true>(grid, a, st)));
  LO_LAUNCH_CHECK("igemm_f8");
  return LO_OK;
}

// ---------------------------------------------------------------------------------------------
// argument packing and tile dispatch (the tile comes from lo_conv_choose)
// ---------------------------------------------------------------------------------------------
int lo_igemm_run(const LoGeom& g, const LoConvOp& op, const LoConvChoice& c, hipStream_t st) {
  const LoGnBwdFuse* gb = op.gb;
  const LoConvExtra* ex = op.ex;
  IgemmArgs a;
  memset(&a.gf, 0, sizeof(a.gf));
  if (op.gf) a.gf = *op.gf;
  a.in = op.in; a.w = op.w; a.bias = op.bias; a.add_src = op.add_src; a.out = op.out; a.gn_partial = op.gn_partial; a.slab = op.slab;
  a.gb_v = gb ? gb->v : nullptr; a.gb_stats = gb ? gb->stats : nullptr; a.gb_gamma = gb ? gb->gamma : nullptr;
  a.gb_beta = gb ? gb->beta : nullptr; a.gb_P1 = gb ? gb->P1 : nullptr;
  a.gb_dv = gb ? gb->dv : nullptr; a.gb_P2 = gb ? gb->P2 : nullptr; a.gb_counter = gb ? gb->counter : nullptr;
  a.gb_target = gb ? gb->target : 0u; a.gb_fail = gb ? gb->fail : nullptr; a.gb_keep_out = gb && gb->keep_out ? 1 : 0;
  a.act = ex ? ex->act : 0; a.bn_partial = ex ? ex->bn_partial : nullptr;
  a.out_pitch = ex ? ex->out_pitch : 0; a.out_choff = ex ? ex->out_choff : 0;
  a.f8_scale = nullptr;
  a.g = g;
  a.M = g.B * g.GH * g.GW;
  a.nsplit = op.nsplit < 1 ? 1 : op.nsplit;
  int ksteps = 0;
  for (int p = 0; p < g.n_phase; ++p) ksteps = g.T[p] * (g.Cin / c.bk) > ksteps ? g.T[p] * (g.Cin / c.bk) : ksteps;
  a.ksteps_per_split = (ksteps + a.nsplit - 1) / a.nsplit;
  if (c.kernel == LO_CK_IGEMM_SPLITK) {
    LO_REQUIRE(g.n_phase == 1 && op.slab, "lo_conv_run: split-K needs a single phase and a slab");
    LO_REQUIRE(c.bk == 64 && g.Cout % 64 == 0, "lo_conv_run: split-K path needs Cin%%64==0 and Cout%%64==0");
  } else {
    if (op.gn_partial || gb || op.gf) {
      LO_REQUIRE((g.GH * g.GW) % c.bm == 0 && a.M % c.bm == 0, "lo_conv_run: GN partials need whole tiles per sample");
      LO_REQUIRE((g.Cout >> 3) <= c.bn, "lo_conv_run: GroupNorm group wider than the N tile");
    }
    if (c.bk == 32) LO_REQUIRE(g.Cout % 64 == 0, "lo_conv_run: BK=32 path needs Cout%%64==0");
  }
#define LO_IG(BM, BN, BK) if (c.bm == BM && c.bn == BN && c.bk == BK) return launch_igemm<BM, BN, BK>(a, c.grid, st)
  LO_IG(128, 128, 64); LO_IG(128, 64, 64); LO_IG(64, 128, 64); LO_IG(64, 64, 64); LO_IG(128, 32, 64); LO_IG(64, 32, 64);
  LO_IG(128, 64, 32); LO_IG(64, 64, 32);
#undef LO_IG
  lo_set_error("lo_conv_run: no kernel for tile %dx%dx%d", c.bm, c.bn, c.bk);
  return LO_ERR_ARG;
}

int lo_igemm_run_f8(const LoGeom& g, const uint8_t* in8, const uint8_t* w8, const float* wscale, const LoConvOp& op, const LoConvChoice& c,
                    hipStream_t st) {
  IgemmArgs a;
  memset(&a, 0, sizeof(a));       // (a.gf.y = null: no fused GroupNorm on the fp8 path)
  a.in = reinterpret_cast<const f16*>(in8); a.w = reinterpret_cast<const f16*>(w8); a.f8_scale = wscale;
  a.bias = op.bias; a.add_src = op.add_src; a.out = op.out; a.gn_partial = op.gn_partial;
  if (op.ex) { a.act = op.ex->act; a.bn_partial = op.ex->bn_partial; }   // teacher epilogue; the pitched output is not taken (lo_conv_run_f8)
  a.g = g;
  a.M = g.B * g.GH * g.GW;
  a.nsplit = 1;
  int ksteps = 0;
  for (int p = 0; p < g.n_phase; ++p) ksteps = g.T[p] * (g.Cin / 128) > ksteps ? g.T[p] * (g.Cin / 128) : ksteps;
  a.ksteps_per_split = ksteps;
  if (op.gn_partial) {
    LO_REQUIRE((g.GH * g.GW) % c.bm == 0 && a.M % c.bm == 0, "lo_conv_run_f8: GN partials need whole tiles per sample");
    LO_REQUIRE((g.Cout >> 3) <= c.bn, "lo_conv_run_f8: GroupNorm group wider than the N tile");
  }
  if (c.bm == 128 && c.bn == 128) return launch_igemm_f8<128, 128>(a, c.grid, st);
  if (c.bm == 128 && c.bn == 64) return launch_igemm_f8<128, 64>(a, c.grid, st);
  if (c.bm == 64 && c.bn == 128) return launch_igemm_f8<64, 128>(a, c.grid, st);
  if (c.bm == 64 && c.bn == 64) return launch_igemm_f8<64, 64>(a, c.grid, st);
  lo_set_error("lo_conv_run_f8: no kernel for tile %dx%d", c.bm, c.bn);
  return LO_ERR_ARG;
}

int lo_splitk_reduce(const float* slab, const float* bias, float* out32, f16* out16, int M, int N, int nsplit,
                     hipStream_t st) {
  int total = M * N;
  LoProfScope _p("lo_splitk_reduce", 0, 4.0 * total * (nsplit + 1), st);
  hipLaunchKernelGGL(lo_splitk_reduce_kernel, dim3((total + 255) / 256), dim3(256), 0, st, slab, bias, out32, out16, M, N, nsplit);
  LO_LAUNCH_CHECK("splitk_reduce");
  return LO_OK;
}
