// Device-side pieces shared by the LDS-DMA GEMM kernels (lo_igemm_nt, lo_wgrad_tn, lo_wgrad3x3_mt, lo_wgrad_s2_mt); each unit gets its
// own zero page.
#pragma once
#include "lo_common.h"

// 16 zero bytes x 16: source of every LDS-DMA lane whose row is padding / out of range
static __device__ __attribute__((aligned(256))) unsigned int lo_zero_page[64];
// its users give every padding lane the page's base: 1 address x 16 B per lane
static_assert(sizeof(lo_zero_page) >= 1 * 16, "LDS-DMA padding lanes read 16 B at offset 0 of the zero page");

#define LO_VMCNT(N) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory")

// Workgroups are dealt round-robin over the 8 XCDs (each with a private 4 MiB L2).  Map the linear block id so that
// every XCD works on ONE contiguous range of logical tile ids: tiles that re-read the same activations (the taps of a
// pixel tile, the N tiles of an M tile) then hit in that XCD's L2 instead of the Infinity Cache.  Bijective for any
// total (speed only, never correctness).
__device__ __forceinline__ int lo_xcd_remap(int bid, int total) {
  const int q = total >> 3, r = total & 7;
  const int xcd = bid & 7, loc = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
}

// Unpadded LDS tiles of [pixel rows][RB bytes of fp16 channels] read with ds_read_b64_tr_b16 (the weight-gradient kernels): the
// transposed fragment reads are kept conflict-free by XOR-swizzling 32-byte blocks inside a row:
//   256-byte rows: block ^= row & 7        128-byte rows: block ^= (row >> 1) & 3
// (128: the 8 consecutive rows a 32-lane half of a transposed read touches land on 8 distinct 32-byte slots of the 256-byte bank
// row whatever the first row is)
template <int RB>
__device__ __forceinline__ int lo_tr_swz(int row) {
  return RB == 256 ? (row & 7) : ((row >> 1) & 3);
}
