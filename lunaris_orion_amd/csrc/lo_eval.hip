// Held-out validation metrics on the device (include/lunaris_hip.h, "validation"): per-sample squared error and SSIM of a batch of
// reconstructions, per-sample KL of the latent, and the running sums of a whole validation pass.  Nothing here is on the training
// step; the three kernels sum in a fixed order and use no atomics, so the same inputs give the same bits.
#include "lo_common.h"
#include "lo_internal.h"
#include "../../include/lunaris_hip.h"
#include <math.h>

namespace {

constexpr int IMG = 128;                 // images are [3][128][128]
constexpr int TAPS = 11;                 // SSIM window (Wang et al. 2004): 11 x 11 Gaussian, sigma 1.5, "valid" positions only
constexpr int MAP = IMG - TAPS + 1;      // 118 x 118 SSIM values per channel
constexpr int BAND = 32;                 // SSIM rows one pass of the workgroup produces
constexpr int BAND_IN = BAND + TAPS - 1; // input rows that pass reads (its rows and the 10-row halo)
constexpr int IN_PITCH = 132;            // floats per staged input row: the last group of four columns reads up to column 131
constexpr int H_PITCH = 120;             // floats per row of a horizontally filtered field (30 groups of four columns)
constexpr int GROUPS = H_PITCH / 4;      // column groups of the horizontal pass
constexpr int THREADS = 1024;
constexpr int WAVES = THREADS / 64;

struct SsimWindow { float w[TAPS]; };    // normalised Gaussian, computed in double on the host

// Deterministic block sum of two doubles (lanes in a fixed shuffle tree, then the waves in order); the result is valid in thread 0.
__device__ __forceinline__ void block_sum2(double& a, double& b, double* red /* [2 * WAVES] */, int tid) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off, 64);
    b += __shfl_down(b, off, 64);
  }
  if ((tid & 63) == 0) { red[2 * (tid >> 6)] = a; red[2 * (tid >> 6) + 1] = b; }
  __syncthreads();
  if (tid == 0) {
    a = red[0]; b = red[1];
    for (int w = 1; w < WAVES; ++w) { a += red[2 * w]; b += red[2 * w + 1]; }
  }
}

// SSIM at one window from the five filtered fields of (x - p, y - p).  Every product and sum is rounded on its own (no FMA
// contraction): for an identical pair the numerator and the denominator are then the same bits and the value is exactly 1.
__device__ __forceinline__ float ssim_value(float mx, float my, float exx, float eyy, float exy, float p, float c1, float c2) {
#pragma clang fp contract(off)
  const float vx = exx - mx * mx, vy = eyy - my * my, cxy = exy - mx * my;
  const float ax = mx + p, ay = my + p;                                  // the means of the images themselves
  const float axy = ax * ay;
  const float num = ((axy + axy) + c1) * ((cxy + cxy) + c2);
  const float den = ((ax * ax + ay * ay) + c1) * ((vx + vy) + c2);
  return num / den;
}

// One workgroup per sample.  Per channel and band of 32 SSIM rows: stage the band's 42 input rows of both images in LDS (the squared
// error of the rows the band owns is taken from the same registers), filter the five fields x, y, x^2, y^2, xy along the rows (four
// adjacent columns per thread out of 16-byte LDS reads), then along the columns (four adjacent rows per thread, the 14 input rows
// of a column read once) and form the SSIM value where the five filtered fields meet.
// The fields are taken of x - p and y - p, p = the channel's first target pixel: variances and the covariance do not depend on a
// shift, the means get it back, and E[x^2] - mu^2 then cancels at the scale of the image's contrast instead of its level (a flat
// image gives exactly 0, not the rounding of 11 products of its level).
__global__ __launch_bounds__(THREADS) void lo_eval_image_metrics_kernel(const float* __restrict__ recon, const float* __restrict__ target,
                                                                        int n_valid, float* __restrict__ per_sample, SsimWindow win,
                                                                        float c1, float c2) {
  __shared__ __attribute__((aligned(16))) float s_in[2][BAND_IN][IN_PITCH];
  __shared__ __attribute__((aligned(16))) float s_h[5][BAND_IN][H_PITCH];
  __shared__ double s_red[2 * WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= n_valid) {                    // padding: its pixels are never read
    if (tid < 2) per_sample[2 * b + tid] = 0.f;
    return;
  }
  float sse = 0.f, ssim = 0.f;
  for (int c = 0; c < 3; ++c) {
    const float* xr = recon + ((size_t)b * 3 + c) * IMG * IMG;
    const float* yt = target + ((size_t)b * 3 + c) * IMG * IMG;
    const float p = yt[0];
    for (int r0 = 0; r0 < MAP; r0 += BAND) {
      const int rows_out = min(BAND, MAP - r0), rows_in = rows_out + TAPS - 1;
      const int own_end = (r0 + BAND >= MAP) ? IMG : r0 + BAND;        // input rows [r0, own_end) count for this band's squared error
      __syncthreads();                                                 // the previous band's column pass has read s_h / s_in
      for (int i = tid; i < rows_in * (IMG / 4); i += THREADS) {
        const int r = i >> 5, q = i & 31;
        const f32x4 x = *reinterpret_cast<const f32x4*>(xr + (size_t)(r0 + r) * IMG + 4 * q);
        const f32x4 y = *reinterpret_cast<const f32x4*>(yt + (size_t)(r0 + r) * IMG + 4 * q);
        if (r0 + r < own_end) {
          const f32x4 d = x - y;
          sse += d.x * d.x + d.y * d.y + d.z * d.z + d.w * d.w;
        }
        *reinterpret_cast<f32x4*>(&s_in[0][r][4 * q]) = x - p;
        *reinterpret_cast<f32x4*>(&s_in[1][r][4 * q]) = y - p;
      }
      __syncthreads();
      // rows: outputs 4g .. 4g+3 of row r read inputs 4g .. 4g+13 (columns past 127 are padding and only reach outputs past 117)
      for (int i = tid; i < rows_in * GROUPS; i += THREADS) {
        const int r = i / GROUPS, g = i - r * GROUPS;
        float acc[5][4] = {};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 x4 = *reinterpret_cast<const f32x4*>(&s_in[0][r][4 * (g + q)]);
          const f32x4 y4 = *reinterpret_cast<const f32x4*>(&s_in[1][r][4 * (g + q)]);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int t = 4 * q + e;
            const float x = x4[e], y = y4[e];
            const float f[5] = {x, y, x * x, y * y, x * y};
#pragma unroll
            for (int o = 0; o < 4; ++o)
              if (t - o >= 0 && t - o < TAPS) {
#pragma unroll
                for (int k = 0; k < 5; ++k) acc[k][o] += win.w[t - o] * f[k];
              }
          }
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          f32x4 v = {acc[k][0], acc[k][1], acc[k][2], acc[k][3]};
          *reinterpret_cast<f32x4*>(&s_h[k][r][4 * g]) = v;
        }
      }
      __syncthreads();
      // columns: thread (column j, rows 4v .. 4v+3 of the band); rows of s_h past rows_in only reach outputs past rows_out
      for (int i = tid; i < (BAND / 4) * MAP; i += THREADS) {
        const int v = i / MAP, j = i - v * MAP;
        if (4 * v >= rows_out) continue;
        float acc[5][4] = {};
#pragma unroll
        for (int t = 0; t < TAPS + 3; ++t) {
          float f[5];
#pragma unroll
          for (int k = 0; k < 5; ++k) f[k] = s_h[k][4 * v + t][j];
#pragma unroll
          for (int o = 0; o < 4; ++o)
            if (t - o >= 0 && t - o < TAPS) {
#pragma unroll
              for (int k = 0; k < 5; ++k) acc[k][o] += win.w[t - o] * f[k];
            }
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
          if (4 * v + o >= rows_out) continue;
          ssim += ssim_value(acc[0][o], acc[1][o], acc[2][o], acc[3][o], acc[4][o], p, c1, c2);
        }
      }
    }
  }
  double a = (double)sse, s = (double)ssim;
  block_sum2(a, s, s_red, tid);
  if (tid == 0) {
    per_sample[2 * b] = (float)a;
    per_sample[2 * b + 1] = (float)(s / (3.0 * MAP * MAP));
  }
}

// per_sample_kl[b] = -0.5 * mean_l(1 + logvar - mu^2 - exp(logvar)); one wave per sample, terms and sum in double (exp(8) beside
// exp(-8) in one mean: fp32 would spend the tolerance on the sum), lanes in a fixed shuffle tree.
__global__ __launch_bounds__(64) void lo_eval_latent_kl_kernel(const float* __restrict__ mu, const float* __restrict__ logvar, int L, int n_valid,
                                                               float* __restrict__ per_sample_kl) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= n_valid) {
    if (lane == 0) per_sample_kl[b] = 0.f;
    return;
  }
  double s = 0.0;
  for (int l = lane; l < L; l += 64) {
    const double m = (double)mu[(size_t)b * L + l], lv = (double)logvar[(size_t)b * L + l];
    s += 1.0 + lv - m * m - exp(lv);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane == 0) per_sample_kl[b] = (float)(-0.5 * s / (double)L);
}

// acc += one batch: [0] count, [1..5] sums of per-sample MSE, KL, PSNR, SSIM, mean quality score, [6] min PSNR, [7] max PSNR.  One wave:
// 64 samples at a time, each lane its sample, the lanes summed in a fixed butterfly (every lane holds the same total), chunks in order.
__global__ __launch_bounds__(64) void lo_eval_accumulate_kernel(const float* __restrict__ img, const float* __restrict__ kl,
                                                                const float* __restrict__ quality, int n_valid, double* __restrict__ acc) {
  const int lane = threadIdx.x;
  double sum[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  double lo = INFINITY, hi = -INFINITY;
  for (int base = 0; base < n_valid; base += 64) {
    const int i = base + lane;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    double plo = INFINITY, phi = -INFINITY;
    if (i < n_valid) {                   // rows past n_valid are padding and are not read
      const double mse = (double)img[2 * i] / (3.0 * IMG * IMG);
      const double psnr = 10.0 * log10(4.0 / fmax(mse, 1e-12));
      v[0] = mse; v[1] = (double)kl[i]; v[2] = psnr; v[3] = (double)img[2 * i + 1];
      if (quality) v[4] = ((double)quality[4 * i] + (double)quality[4 * i + 1] + (double)quality[4 * i + 2] + (double)quality[4 * i + 3]) * 0.25;
      plo = phi = psnr;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
      for (int k = 0; k < 5; ++k) v[k] += __shfl_xor(v[k], off, 64);
      plo = fmin(plo, __shfl_xor(plo, off, 64));
      phi = fmax(phi, __shfl_xor(phi, off, 64));
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) sum[k] += v[k];
    lo = fmin(lo, plo); hi = fmax(hi, phi);
  }
  if (lane == 0 && n_valid > 0) {
    const bool first = acc[0] == 0.0;    // a zeroed accumulator starts a run: its min / max slots hold nothing yet
    acc[0] += (double)n_valid;
#pragma unroll
    for (int k = 0; k < 5; ++k) acc[1 + k] += sum[k];
    acc[6] = first ? lo : fmin(acc[6], lo);
    acc[7] = first ? hi : fmax(acc[7], hi);
  }
}

}  // namespace

extern "C" int lo_eval_image_metrics(const float* recon, const float* target, int B, int n_valid, float* per_sample, void* stream) {
  LO_REQUIRE(recon && target && per_sample && B >= 1 && n_valid >= 0 && n_valid <= B, "lo_eval_image_metrics: bad argument (B=%d, n_valid=%d)", B, n_valid);
  LO_REQUIRE(((uintptr_t)recon | (uintptr_t)target) % 16 == 0, "lo_eval_image_metrics: recon and target must be 16-byte aligned");
  SsimWindow win;
  double g[TAPS], total = 0.0;
  for (int t = 0; t < TAPS; ++t) {
    const double d = t - (TAPS - 1) / 2;
    total += g[t] = exp(-d * d / (2.0 * 1.5 * 1.5));
  }
  for (int t = 0; t < TAPS; ++t) win.w[t] = (float)(g[t] / total);
  const float c1 = (float)((0.01 * 2.0) * (0.01 * 2.0)), c2 = (float)((0.03 * 2.0) * (0.03 * 2.0));   // data range 2
  hipStream_t st = (hipStream_t)stream;
  LoProfScope _p("lo_eval_image_metrics", 0, 2.0 * n_valid * 3 * IMG * IMG * 4, st);
  hipLaunchKernelGGL(lo_eval_image_metrics_kernel, dim3(B), dim3(THREADS), 0, st, recon, target, n_valid, per_sample, win, c1, c2);
  LO_LAUNCH_CHECK("eval_image_metrics");
  return LO_OK;
}

extern "C" int lo_eval_latent_kl(const float* mu, const float* logvar, int B, int L, int n_valid, float* per_sample_kl, void* stream) {
  LO_REQUIRE(mu && logvar && per_sample_kl && B >= 1 && n_valid >= 0 && n_valid <= B, "lo_eval_latent_kl: bad argument (B=%d, n_valid=%d)", B, n_valid);
  LO_REQUIRE(L >= 64 && L % 64 == 0, "lo_eval_latent_kl: L=%d must be a multiple of 64", L);
  hipStream_t st = (hipStream_t)stream;
  LoProfScope _p("lo_eval_latent_kl", 0, 8.0 * n_valid * L, st);
  hipLaunchKernelGGL(lo_eval_latent_kl_kernel, dim3(B), dim3(64), 0, st, mu, logvar, L, n_valid, per_sample_kl);
  LO_LAUNCH_CHECK("eval_latent_kl");
  return LO_OK;
}

extern "C" int lo_eval_accumulate(const float* per_sample_img, const float* per_sample_kl, const float* quality, int n_valid, double* acc,
                                  void* stream) {
  LO_REQUIRE(per_sample_img && per_sample_kl && acc && n_valid >= 0, "lo_eval_accumulate: bad argument (n_valid=%d)", n_valid);
  LO_REQUIRE((uintptr_t)acc % 8 == 0, "lo_eval_accumulate: acc must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  LoProfScope _p("lo_eval_accumulate", 0, 16.0 * n_valid, st);
  hipLaunchKernelGGL(lo_eval_accumulate_kernel, dim3(1), dim3(64), 0, st, per_sample_img, per_sample_kl, quality, n_valid, acc);
  LO_LAUNCH_CHECK("eval_accumulate");
  return LO_OK;
}
