// fp8 (e4m3) operand path of the forward convs: weight packing with one scale per output row, activation quantisation.
#include "lo_conv.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>

// fp16 packed weights -> e4m3 with one scale per (phase, output channel) row: scale = amax / 448 (1 for an all-zero row);
// wscale = scale / LO_F8_ACT_SCALE is what the conv epilogue multiplies by.  One workgroup per row; all layers of a model in
// one launch (job table in device memory, like lo_pack_all).
__device__ __forceinline__ void lo_pack_f8_row(const LoPackF8Job& J, int row) {   // row = phase * Cout + n
  __shared__ float s_red[4];
  const int p = row / J.Cout, n = row - p * J.Cout;
  const int K = J.K[p];
  const size_t o = (size_t)J.wofs[p] + (size_t)n * K;
  const f16* src = J.src + o;
  const int tid = threadIdx.x;
  float amax = 0.f;
  for (int k = tid * 8; k < K; k += 256 * 8) {
    f16x8 v = *reinterpret_cast<const f16x8*>(src + k);
#pragma unroll
    for (int q = 0; q < 8; ++q) amax = fmaxf(amax, fabsf((float)v[q]));
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) amax = fmaxf(amax, __shfl_xor(amax, s, 64));
  if ((tid & 63) == 0) s_red[tid >> 6] = amax;
  __syncthreads();
  amax = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
  const float scale = amax > 0.f ? amax * (1.0f / LO_F8_MAX) : 1.0f;
  const float inv = 1.0f / scale;
  for (int k = tid * 8; k < K; k += 256 * 8) {
    f16x8 v = *reinterpret_cast<const f16x8*>(src + k);
    u32x2 q = {lo_pack4_fp8((float)v[0] * inv, (float)v[1] * inv, (float)v[2] * inv, (float)v[3] * inv),
               lo_pack4_fp8((float)v[4] * inv, (float)v[5] * inv, (float)v[6] * inv, (float)v[7] * inv)};
    *reinterpret_cast<u32x2*>(J.dst + o + k) = q;
  }
  if (tid == 0) J.scale[row] = scale * (1.0f / LO_F8_ACT_SCALE);
}
__global__ __launch_bounds__(256) void lo_pack_f8_kernel(const LoPackF8Job* __restrict__ jobs, int njobs, int block_base) {
  const int bid = (int)blockIdx.x + block_base;
  int j = 0;
  while (j + 1 < njobs && bid >= jobs[j + 1].block0) ++j;
  lo_pack_f8_row(jobs[j], bid - jobs[j].block0);
}
__global__ __launch_bounds__(256) void lo_pack_f8_one_kernel(LoPackF8Job J) { lo_pack_f8_row(J, (int)blockIdx.x); }
int lo_pack_f8_one(const LoGeom& g, const f16* wp, uint8_t* w8, float* wscale, hipStream_t st) {
  LoPackF8Job j;
  lo_pack_f8_job(&j, g, wp, w8, wscale, 0);
  hipLaunchKernelGGL(lo_pack_f8_one_kernel, dim3(g.n_phase * g.Cout), dim3(256), 0, st, j);
  LO_LAUNCH_CHECK("pack_f8_one");
  return LO_OK;
}
// x8 = e4m3(x * LO_F8_ACT_SCALE), saturating (stand-alone form of what the GroupNorm forward emits in fp8 mode)
__global__ __launch_bounds__(256) void lo_quantize_f8_kernel(const f16* __restrict__ x, uint8_t* __restrict__ x8, size_t n) {
  size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i + 3 < n) {
    f16x4 v = *reinterpret_cast<const f16x4*>(x + i);
    *reinterpret_cast<uint32_t*>(x8 + i) = lo_pack4_fp8((float)v[0] * LO_F8_ACT_SCALE, (float)v[1] * LO_F8_ACT_SCALE,
                                                       (float)v[2] * LO_F8_ACT_SCALE, (float)v[3] * LO_F8_ACT_SCALE);
  }
}
int lo_quantize_f8(const f16* x, uint8_t* x8, size_t n, hipStream_t st) {
  LO_REQUIRE(n % 4 == 0, "lo_quantize_f8: element count must be a multiple of 4");
  hipLaunchKernelGGL(lo_quantize_f8_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, x, x8, n);
  LO_LAUNCH_CHECK("quantize_f8");
  return LO_OK;
}
void lo_pack_f8_job(LoPackF8Job* j, const LoGeom& g, const f16* src, uint8_t* dst, float* scale, int block0) {
  memset(j, 0, sizeof(*j));
  j->src = src; j->dst = dst; j->scale = scale; j->Cout = g.Cout; j->n_phase = g.n_phase; j->block0 = block0;
  for (int p = 0; p < g.n_phase; ++p) { j->K[p] = g.T[p] * g.Cin; j->wofs[p] = g.wofs[p]; }
}
int lo_pack_f8_all(const LoPackF8Job* jobs_dev, int njobs, int nblocks, hipStream_t st, int block_base) {
  if (njobs <= 0 || nblocks <= 0) return LO_OK;
  LoProfScope _p("lo_pack_f8", 0, 0, st);
  hipLaunchKernelGGL(lo_pack_f8_kernel, dim3(nblocks), dim3(256), 0, st, jobs_dev, njobs, block_base);
  LO_LAUNCH_CHECK("pack_f8");
  return LO_OK;
}
