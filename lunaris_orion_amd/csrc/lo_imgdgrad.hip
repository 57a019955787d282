// Data gradient of the two 3x3 / padding 1 convolutions that read the 3-channel images: what autograd returns for an input image
// that requires grad (train_hybrid.py:845 sets images.requires_grad_(True) before self.vae(images)).
//   VAE      encoder.down1.0             Conv2d(3 -> 64, k3, s2, p1)   dy fp16 NHWC [B][64][64][64]
//   teacher  feature_extractor.conv1.0   Conv2d(3 -> 32, k3, s1, p1)   dy fp16 NHWC [B][128][128][32]
//   dx[b][c][y][x] = scale * sum_{co, ky, kx} W[co][c][ky][kx] * dy[b][oy][ox][co],  y = stride * oy - 1 + ky, x = stride * ox - 1 + kx
// into fp32 NCHW [B][3][128][128].  Output-stationary on MFMA (v_mfma_f32_16x16x32_f16): D[i][p] = sum_k A[i][k] B[k][p] over one
// tap and 32 channels co, p = 16 output pixels that share the tap, A = the weights.  A's rows carry the fp32 weights as two fp16
// halves, W = hi + lo to 2^-22: rows 0..2 = hi of c = 0..2, rows 4..6 = 4096 * lo (scaled out of the fp16 subnormal range; exact),
// so one MFMA forms both halves and lane p (rows 0..3) meets lane p + 16 (rows 4..7) in one swizzle at the end.  fp16 x fp16
// products are exact in the fp32 accumulator.  Every output element is written by one lane in a fixed order: no atomics, bitwise
// reproducible.  Each wave walks down a column strip with the dy rows it needs kept in registers (every dy row is fetched once per
// strip and shift; the shifted copies of neighbouring lanes hit L1).
#include "lo_common.h"
#include "lo_internal.h"

// the weights [cout][27] of a workgroup, staged once in LDS (coalesced) for the per-lane fragment gathers below
template <int COUT>
__device__ __forceinline__ void idg_stage_w(const float* __restrict__ w, float* ws) {
  for (int i = threadIdx.x; i < COUT * 27; i += 256) ws[i] = w[i];
  __syncthreads();
}

// A fragment of tap (ky, kx) = tap / 3, tap % 3 and channel block kb: lane l holds row l & 15, columns co = 32 kb + 8 (l >> 4) .. + 7
__device__ __forceinline__ f16x8 idg_wfrag(const float* w, int tap, int kb, int lane) {
  const int i = lane & 15, g = lane >> 4;
  const bool lo = i >= 4;
  const int c = lo ? i - 4 : i;
  f16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float v = 0.f;
    if (c < 3) {
      const float wv = w[(32 * kb + 8 * g + j) * 27 + c * 9 + tap];
      const f16 hi = (f16)wv;
      v = lo ? (wv - (float)hi) * 4096.f : (float)hi;
    }
    r[j] = (f16)v;
  }
  return r;
}

// B fragment: dy[n][oy][ox][32 kb + 8 g .. + 7] (zero outside the map: the padding of the forward)
template <int HO, int COUT>
__device__ __forceinline__ f16x8 idg_load(const f16* __restrict__ dy, int n, int oy, int ox, int kb, int g) {
  if ((unsigned)oy >= (unsigned)HO || (unsigned)ox >= (unsigned)HO) return (f16x8){0, 0, 0, 0, 0, 0, 0, 0};
  return *reinterpret_cast<const f16x8*>(dy + (((size_t)n * HO + oy) * HO + ox) * COUT + 32 * kb + 8 * g);
}

__device__ __forceinline__ f32x4 idg_mfma(f16x8 a, f16x8 b, f32x4 acc) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc, 0, 0, 0); }

// lanes 0..15: (hi + lo / 4096) * scale for c = 0..2 of their pixel (lanes 16..31 hold the lo rows; the rest is padding)
__device__ __forceinline__ f32x4 idg_finish(f32x4 acc, float scale) {
  f32x4 r;
#pragma unroll
  for (int k = 0; k < 3; ++k) r[k] = (acc[k] + __shfl_xor(acc[k], 16) * (1.0f / 4096.f)) * scale;
  r[3] = 0.f;
  return r;
}

// stride 1, 32 channels (teacher): grid (2 * 128 / ROWS, B), 4 waves; wave = 16-column strip x0 .. x0 + 15, rows y0 .. y0 + ROWS - 1.
// SEED: the store is dx = scale * conv2d_input(dy, w) + c * (recon - target), c = seed.c[0] on the device, recon / target fp32 NCHW
// read at the address of the store (the same 64-byte rows per wave) -- the last kernel of the teacher's backward then emits the whole
// d loss / d recon of a reward + MSE objective, with no add pass of its own.  The loads of a row are issued in front of its MFMAs.
// c == 0 stores the un-seeded value itself (whatever recon / target hold).  SEED = false: the kernel as it was (IdgSeed<false> is empty).
template <bool SEED> struct IdgSeed { const float *c, *recon, *target; };
template <> struct IdgSeed<false> {};
template <int ROWS, bool SEED = false>
__global__ __launch_bounds__(256) void lo_image_dgrad_s1_kernel(const f16* __restrict__ dy, const float* __restrict__ w, float scale,
                                                                float* __restrict__ dx, IdgSeed<SEED> seed = {}) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const int n = blockIdx.y;
  const int x = ((blockIdx.x & 1) * 4 + wave) * 16 + j;
  const int y0 = (blockIdx.x >> 1) * ROWS;
  __shared__ float ws[32 * 27];
  float cs = 0.f;
  if constexpr (SEED) cs = seed.c[0];
  idg_stage_w<32>(w, ws);
  f16x8 A[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) A[t] = idg_wfrag(ws, t, 0, lane);
  // win[r][kx] = dy[y - 1 + r][x + 1 - kx] for the current output row y (tap ky reads r = 2 - ky)
  f16x8 win[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) win[r][kx] = idg_load<128, 32>(dy, n, y0 - 1 + r, x + 1 - kx, 0, g);
  for (int y = y0; y < y0 + ROWS; ++y) {
    f16x8 nxt[3];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) nxt[kx] = idg_load<128, 32>(dy, n, y + 2, x + 1 - kx, 0, g);
    float sr[3], stg[3];
    if constexpr (SEED) {
      if (g == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          sr[c] = seed.recon[(((size_t)n * 3 + c) * 128 + y) * 128 + x];
          stg[c] = seed.target[(((size_t)n * 3 + c) * 128 + y) * 128 + x];
        }
      }
    }
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) acc = idg_mfma(A[ky * 3 + kx], win[2 - ky][kx], acc);
    const f32x4 o = idg_finish(acc, scale);
    if (g == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float v = o[c];
        if constexpr (SEED) v = cs != 0.f ? fmaf(cs, sr[c] - stg[c], v) : v;
        dx[(((size_t)n * 3 + c) * 128 + y) * 128 + x] = v;
      }
    }
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) { win[0][kx] = win[1][kx]; win[1][kx] = win[2][kx]; win[2][kx] = nxt[kx]; }
  }
}

// stride 2, 64 channels (VAE): grid (64 / MROWS, B), 4 waves; wave = 32-column strip 32 xb .. 32 xb + 31, dy rows m0 .. m0 + MROWS - 1
// (output rows 2 m0 .. 2 (m0 + MROWS) - 1).  The 16 pixels of one MFMA share a parity class (lane j: x = 32 xb + 2 j + px), so they
// share their taps:  y even: ky = 1 (oy = y / 2);  y odd: ky = 0 (oy = (y + 1) / 2), ky = 2 (oy = (y - 1) / 2);  likewise in x with
// ox = 16 xb + j (s = 0) or 16 xb + j + 1 (s = 1).  Per dy row m: 1 + 2 + 2 + 4 taps x 2 channel blocks = 18 MFMAs for 64 pixels.
template <int MROWS>
__global__ __launch_bounds__(256) void lo_image_dgrad_s2_kernel(const f16* __restrict__ dy, const float* __restrict__ w, float scale,
                                                                float* __restrict__ dx) {
  const int lane = threadIdx.x & 63, xb = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const int n = blockIdx.y;
  const int m0 = blockIdx.x * MROWS;
  const int ox = 16 * xb + j;
  __shared__ float ws[64 * 27];
  idg_stage_w<64>(w, ws);
  f16x8 A[9][2];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) A[t][kb] = idg_wfrag(ws, t, kb, lane);
  f16x8 cur[2][2], nxt[2][2];       // [s][kb]: dy row m resp. m + 1 at column ox + s
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) cur[s][kb] = idg_load<64, 64>(dy, n, m0, ox + s, kb, g);
  float* out = dx + (size_t)n * 3 * 16384 + 32 * xb + 2 * j;
  for (int m = m0; m < m0 + MROWS; ++m) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) nxt[s][kb] = idg_load<64, 64>(dy, n, m + 1, ox + s, kb, g);
    f32x4 ee = (f32x4){0.f, 0.f, 0.f, 0.f}, eo = ee, oe = ee, oo = ee;     // (y parity, x parity)
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      ee = idg_mfma(A[4][kb], cur[0][kb], ee);                                 // (1, 1)
      eo = idg_mfma(A[3][kb], cur[1][kb], eo);                                 // (1, 0)
      eo = idg_mfma(A[5][kb], cur[0][kb], eo);                                 // (1, 2)
      oe = idg_mfma(A[1][kb], nxt[0][kb], oe);                                 // (0, 1)
      oe = idg_mfma(A[7][kb], cur[0][kb], oe);                                 // (2, 1)
      oo = idg_mfma(A[0][kb], nxt[1][kb], oo);                                 // (0, 0)
      oo = idg_mfma(A[2][kb], nxt[0][kb], oo);                                 // (0, 2)
      oo = idg_mfma(A[6][kb], cur[1][kb], oo);                                 // (2, 0)
      oo = idg_mfma(A[8][kb], cur[0][kb], oo);                                 // (2, 2)
    }
    const f32x4 e0 = idg_finish(ee, scale), e1 = idg_finish(eo, scale), o0 = idg_finish(oe, scale), o1 = idg_finish(oo, scale);
    if (g == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        *reinterpret_cast<f32x2*>(out + (size_t)c * 16384 + (2 * m) * 128) = (f32x2){e0[c], e1[c]};
        *reinterpret_cast<f32x2*>(out + (size_t)c * 16384 + (2 * m + 1) * 128) = (f32x2){o0[c], o1[c]};
      }
    }
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) cur[s][kb] = nxt[s][kb];
  }
}

int lo_image_dgrad(const f16* dy, int cout, int stride, const float* w, int B, float scale, float* dx, hipStream_t st, const LoImgSeed* seed) {
  LO_REQUIRE(dy && w && dx, "lo_image_dgrad: null argument");
  LO_REQUIRE(!seed || (seed->c && seed->recon && seed->target), "lo_image_dgrad: seed with a null member");
  LO_REQUIRE(!seed || (stride == 1 && cout == 32), "lo_image_dgrad: the seeded form is built for (stride 1, 32 channels), got (%d, %d)", stride, cout);
  LO_REQUIRE(B > 0 && B <= 65535, "lo_image_dgrad: batch %d outside [1, 65535]", B);
  LO_REQUIRE((stride == 1 && cout == 32) || (stride == 2 && cout == 64),
             "lo_image_dgrad: built for (stride 1, 32 channels) and (stride 2, 64 channels), got (%d, %d)", stride, cout);
  const double ho = 128 / stride;
  LoProfScope _p(seed ? "lo_image_dgrad s1 seeded" : stride == 1 ? "lo_image_dgrad s1" : "lo_image_dgrad s2", 2.0 * B * ho * ho * cout * 27,
                 (double)B * (ho * ho * cout * 2 + (seed ? 3 : 1) * 3 * 16384 * 4), st);
  if (stride == 1) {
    constexpr int ROWS = 16;
    if (seed)
      hipLaunchKernelGGL((lo_image_dgrad_s1_kernel<ROWS, true>), dim3(2 * 128 / ROWS, B), dim3(256), 0, st, dy, w, scale, dx,
                         IdgSeed<true>{seed->c, seed->recon, seed->target});
    else
      hipLaunchKernelGGL((lo_image_dgrad_s1_kernel<ROWS, false>), dim3(2 * 128 / ROWS, B), dim3(256), 0, st, dy, w, scale, dx, IdgSeed<false>{});
  } else {
    constexpr int MROWS = 8;
    hipLaunchKernelGGL((lo_image_dgrad_s2_kernel<MROWS>), dim3(64 / MROWS, B), dim3(256), 0, st, dy, w, scale, dx);
  }
  LO_LAUNCH_CHECK("image_dgrad");
  return LO_OK;
}
