// Convolution geometry (LoGeom, lo_common.h) and the fp16 weight packing of the implicit-GEMM operand layout.
#include "lo_conv.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>

// ---------------------------------------------------------------------------------------------
// geometry builder (host)
// ---------------------------------------------------------------------------------------------
int lo_make_geom(LoGeom* g, int kind, int B, int H, int W, int Cin, int Cout) {
  memset(g, 0, sizeof(*g));
  g->B = B; g->Hin = H; g->Win = W; g->Cin = Cin; g->Cout = Cout;
  auto tap = [&](int p, int dy, int dx, int r, int s, int S) {
    int t = g->T[p]++;
    g->dy[p][t] = (int8_t)dy; g->dx[p][t] = (int8_t)dx; g->rs[p][t] = (int8_t)(r * S + s);
  };
  switch (kind) {
    case LO_CONV3_S1:
    case LO_CONV3_S2: {
      int st = kind == LO_CONV3_S1 ? 1 : 2;
      g->Hout = H / st; g->Wout = W / st; g->GH = g->Hout; g->GW = g->Wout;
      g->in_stride = st; g->out_stride = 1; g->n_phase = 1;
      for (int r = 0; r < 3; ++r) for (int s = 0; s < 3; ++s) tap(0, r - 1, s - 1, r, s, 3);
      g->sn = Cin * 9; g->sc = 9;   // Conv2d weight [Cout][Cin][3][3]
      break;
    }
    case LO_CONV3_S1_DGRAD: {
      // dx[ih] = sum_r dy[ih + 1 - r] W[co][ci][r]; this op's output channel n = ci_fwd, reduced c = co_fwd
      g->Hout = H; g->Wout = W; g->GH = H; g->GW = W; g->in_stride = 1; g->out_stride = 1; g->n_phase = 1;
      for (int r = 0; r < 3; ++r) for (int s = 0; s < 3; ++s) tap(0, 1 - r, 1 - s, r, s, 3);
      g->sn = 9; g->sc = Cout * 9;  // W[co_fwd = c][ci_fwd = n][3][3], Cin_fwd = Cout of this op
      break;
    }
    case LO_CONV3_S2_DGRAD: {
      // forward: oh = (ih + 1 - r)/2.  Reads dy [B,H,W,Cin=Cout_fwd], writes dx [B,2H,2W,Cout=Cin_fwd].
      g->Hout = 2 * H; g->Wout = 2 * W; g->GH = H; g->GW = W; g->in_stride = 1; g->out_stride = 2; g->n_phase = 4;
      for (int ph = 0; ph < 2; ++ph) for (int pw = 0; pw < 2; ++pw) {
        int p = ph * 2 + pw; g->out_oy[p] = ph; g->out_ox[p] = pw;
        int nr = ph ? 2 : 1, ns = pw ? 2 : 1;
        int rr[2], dyy[2], ss[2], dxx[2];
        if (!ph) { rr[0] = 1; dyy[0] = 0; } else { rr[0] = 0; dyy[0] = 1; rr[1] = 2; dyy[1] = 0; }
        if (!pw) { ss[0] = 1; dxx[0] = 0; } else { ss[0] = 0; dxx[0] = 1; ss[1] = 2; dxx[1] = 0; }
        for (int a = 0; a < nr; ++a) for (int b = 0; b < ns; ++b) tap(p, dyy[a], dxx[b], rr[a], ss[b], 3);
      }
      g->sn = 9; g->sc = Cout * 9;
      break;
    }
    case LO_CONVT4_S2: {
      // oh = 2 ih - 1 + r.  ConvTranspose2d weight [Cin][Cout][4][4]
      g->Hout = 2 * H; g->Wout = 2 * W; g->GH = H; g->GW = W; g->in_stride = 1; g->out_stride = 2; g->n_phase = 4;
      for (int ph = 0; ph < 2; ++ph) for (int pw = 0; pw < 2; ++pw) {
        int p = ph * 2 + pw; g->out_oy[p] = ph; g->out_ox[p] = pw;
        int rr[2], dyy[2], ss[2], dxx[2];
        if (!ph) { rr[0] = 1; dyy[0] = 0; rr[1] = 3; dyy[1] = -1; } else { rr[0] = 0; dyy[0] = 1; rr[1] = 2; dyy[1] = 0; }
        if (!pw) { ss[0] = 1; dxx[0] = 0; ss[1] = 3; dxx[1] = -1; } else { ss[0] = 0; dxx[0] = 1; ss[1] = 2; dxx[1] = 0; }
        for (int a = 0; a < 2; ++a) for (int b = 0; b < 2; ++b) tap(p, dyy[a], dxx[b], rr[a], ss[b], 4);
      }
      g->sn = 16; g->sc = Cout * 16;  // W[ci = c][co = n][4][4]
      break;
    }
    case LO_CONVT4_S2_DGRAD: {
      // din[ih] = sum_r dout[2 ih - 1 + r] W[ci][co][r]: a k4 s2 p1 convolution of dout.
      g->Hout = H / 2; g->Wout = W / 2; g->GH = g->Hout; g->GW = g->Wout; g->in_stride = 2; g->out_stride = 1; g->n_phase = 1;
      for (int r = 0; r < 4; ++r) for (int s = 0; s < 4; ++s) tap(0, r - 1, s - 1, r, s, 4);
      g->sn = Cin * 16; g->sc = 16;   // W[ci_fwd = n][co_fwd = c][4][4], Cout_fwd = Cin of this op
      break;
    }
    case LO_LINEAR: {
      g->Hout = H; g->Wout = W; g->GH = H; g->GW = W; g->in_stride = 1; g->out_stride = 1; g->n_phase = 1;
      tap(0, 0, 0, 0, 0, 1);
      g->sn = Cin; g->sc = 1;
      break;
    }
    default:
      lo_set_error("lo_make_geom: unknown kind %d", kind);
      return LO_ERR_ARG;
  }
  int off = 0;
  for (int p = 0; p < g->n_phase; ++p) { g->wofs[p] = off; off += Cout * g->T[p] * Cin; }
  if ((g->GH & (g->GH - 1)) || (g->GW & (g->GW - 1)) || g->GH < 1 || g->GW < 1) {
    lo_set_error("lo_make_geom: output grid %dx%d must be powers of two", g->GH, g->GW);
    return LO_ERR_ARG;
  }
  while ((1 << g->lgh) < g->GH) ++g->lgh;
  while ((1 << g->lgw) < g->GW) ++g->lgw;
  auto lg2 = [](int v) { int l = 0; while ((1 << l) < v) ++l; return (1 << l) == v ? l : -1; };
  g->lg_hin = lg2(g->Hin); g->lg_win = lg2(g->Win); g->lg_cin = lg2(g->Cin);
  g->lg_hout = lg2(g->Hout); g->lg_wout = lg2(g->Wout); g->lg_cout = lg2(g->Cout);
  for (int p = 0; p < g->n_phase; ++p)
    for (int t = 0; t < g->T[p]; ++t) {
      g->dyc[p] |= (uint32_t)(g->dy[p][t] + 1) << (2 * t);
      g->dxc[p] |= (uint32_t)(g->dx[p][t] + 1) << (2 * t);
    }
  return LO_OK;
}

// ---------------------------------------------------------------------------------------------
// weight pack: canonical fp32 -> packed fp16  Wp[p][n][t*Cin + c] = W[n*sn + c*sc + rs[p][t]]
// (optionally with a row permutation for decoder.fc:  n -> row_perm(n))
// ---------------------------------------------------------------------------------------------
__global__ void lo_pack_weight_kernel(const float* __restrict__ w, f16* __restrict__ wp, LoGeom g, int total) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int p = 0;
#pragma unroll
  for (int q = 1; q < LO_MAX_PHASE; ++q) if (q < g.n_phase && i >= g.wofs[q]) p = q;
  int j = i - g.wofs[p];
  int K = g.T[p] * g.Cin;
  int n = j / K, k = j - n * K;
  int t = k / g.Cin, c = k - t * g.Cin;
  wp[i] = (f16)w[(size_t)n * g.sn + (size_t)c * g.sc + g.rs[p][t]];
}

// all packs of a model in ONE launch: jobs live in device memory (uploaded once per workspace by the executor).
// A block owns 16 output channels x 64 reduced channels x all taps: the canonical weight is read along its contiguous
// axis (the 9 or 16 taps of one (n, c) pair are adjacent floats; the pairs themselves are adjacent along c for forward
// convs / transposed-conv gradients and along n for the others), staged as fp16 in LDS, and written along c, the
// contiguous axis of the packed operand.  lo_pack_blocks() gives the block count of one job.
int lo_pack_blocks(const LoGeom& g) { return ((g.Cout + 15) / 16) * ((g.Cin + 63) / 64); }
__global__ __launch_bounds__(256) void lo_pack_all_kernel(const LoPackJob* __restrict__ jobs, int njobs, int block_base) {
  __shared__ __attribute__((aligned(16))) f16 tile[16][17][72];     // rows 144 bytes apart: 16-byte reads of eight consecutive c
  const int bid = (int)blockIdx.x + block_base;     // block_base: first block of a sub-range of the job table
  int j = 0;
  while (j + 1 < njobs && bid >= jobs[j + 1].block0) ++j;
  const LoPackJob& J = jobs[j];
  const LoGeom& g = J.g;
  const int tid = threadIdx.x;
  const int tiles_c = (g.Cin + 63) / 64;
  const int b = bid - J.block0;
  const int n0 = (b / tiles_c) * 16, c0 = (b % tiles_c) * 64;
  const bool n_fast = g.sn < g.sc;
  const int t_all = n_fast ? g.sn : g.sc;     // taps of the canonical weight (9, 16; 1 for a Linear)
  for (int q = tid; q < 1024; q += 256) {
    int nl, cl;
    if (n_fast) { nl = q & 15; cl = q >> 4; } else { cl = q & 63; nl = q >> 6; }
    const int n = n0 + nl, c = c0 + cl;
    if (n < g.Cout && c < g.Cin) {
      const float* src = J.src + (size_t)n * g.sn + (size_t)c * g.sc;
      for (int t = 0; t < t_all; ++t) tile[nl][t][cl] = (f16)src[t];
    }
  }
  __syncthreads();
  int sum_t = 0;
  for (int p = 0; p < g.n_phase; ++p) sum_t += g.T[p];
  // 16-byte stores of eight consecutive c (every Cin of the model is a multiple of 32): the 2-byte stores of the first form were
  // 65 us per step for the 15 M packed elements of the model (rocprofv3, round 4)
  const int c8 = (tid & 7) * 8, c = c0 + c8;
  for (int r = tid >> 3; r < 16 * sum_t; r += 32) {
    const int nl = r / sum_t;
    int t = r - nl * sum_t, p = 0;
    while (t >= g.T[p]) { t -= g.T[p]; ++p; }
    const int n = n0 + nl;
    if (n < g.Cout && c + 8 <= g.Cin)
      *reinterpret_cast<f16x8*>(J.dst + (size_t)g.wofs[p] + ((size_t)n * g.T[p] + t) * g.Cin + c) = *reinterpret_cast<const f16x8*>(&tile[nl][g.rs[p][t]][c8]);
    else if (n < g.Cout)
      for (int e = 0; e < 8 && c + e < g.Cin; ++e) J.dst[(size_t)g.wofs[p] + ((size_t)n * g.T[p] + t) * g.Cin + c + e] = tile[nl][g.rs[p][t]][c8 + e];
  }
}

int lo_pack_all(const LoPackJob* jobs_dev, int njobs, int nblocks, hipStream_t st, int block_base) {
  if (njobs <= 0 || nblocks <= 0) return LO_OK;
  LoProfScope _p("lo_pack_all", 0, 0, st);
  hipLaunchKernelGGL(lo_pack_all_kernel, dim3(nblocks), dim3(256), 0, st, jobs_dev, njobs, block_base);
  LO_LAUNCH_CHECK("pack_all");
  return LO_OK;
}

int lo_pack_weight(const float* w, f16* wp, const LoGeom& g, hipStream_t st) {
  int total = lo_geom_packed_elems(g);
  LoProfScope _p("lo_pack_weight", 0, 6.0 * total, st);
  hipLaunchKernelGGL(lo_pack_weight_kernel, dim3((total + 255) / 256), dim3(256), 0, st, w, wp, g, total);
  LO_LAUNCH_CHECK("pack_weight");
  return LO_OK;
}
size_t lo_packed_weight_elems(const LoGeom& g) { return (size_t)lo_geom_packed_elems(g); }
