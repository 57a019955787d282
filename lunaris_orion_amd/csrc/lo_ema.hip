// Exponential moving average of the flat parameter buffer: e <- e + (p - e)(1 - decay), one streaming pass (12 B per element).
#include "lo_internal.h"
#include "../../include/lunaris_hip.h"

// One element: subtract, multiply and add each round to fp32 on their own (no contraction into an fma), so that the unrolled copies
// and the scalar tail round identically, a launch over [0, n) and several over its sub-ranges give the same bits, and numpy float32
// replays the pass exactly (tests/test_ema_ops_gpu.py).  p == e gives (p - e) = +0 and e + 0 = e: an average that has reached the
// parameters stays on them (the one exception IEEE makes, -0 + +0 = +0, has the same value).
__device__ __forceinline__ float lo_ema_elem(float e, float p, float omd) {
#pragma clang fp contract(off)
  const float d = p - e;
  const float s = d * omd;
  return e + s;
}
// The shape of lo_adamw_kernel (lo_train.hip): U groups of four elements per thread and iteration, all 2 * U 16-byte loads issued before
// the first use, a grid of at most one workgroup per CU -- the pass runs on the side stream beside the next forward and must not take
// every wave slot of the chip away from it.  gate: null, or the optimizer's norm block (scratch + 1024): gate[2] == 0 is a skipped
// update (non-finite norm, or the rendezvous-failure word) and nothing is written, exactly as lo_adamw_kernel decides it.
__global__ __launch_bounds__(256) void lo_ema_kernel(float* __restrict__ e, const float* __restrict__ p, size_t n, float omd,
                                                     const float* __restrict__ gate) {
  if (gate && gate[2] == 0.f) return;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * 256;
  const size_t n4 = n / 4;
  constexpr int U = 4;
  for (size_t k0 = i; k0 < n4; k0 += U * stride) {
    f32x4 pv[U], ev[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t k = k0 + u * stride;
      if (k < n4) {
        pv[u] = reinterpret_cast<const f32x4*>(p)[k];
        ev[u] = reinterpret_cast<const f32x4*>(e)[k];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t k = k0 + u * stride;
      if (k < n4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) ev[u][j] = lo_ema_elem(ev[u][j], pv[u][j], omd);
        reinterpret_cast<f32x4*>(e)[k] = ev[u];
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (size_t k = n4 * 4; k < n; ++k) e[k] = lo_ema_elem(e[k], p[k], omd);
}

int lo_ema_run(float* ema, const float* p, size_t n, float one_minus_decay, const float* gate, hipStream_t st) {
  const uintptr_t pe = reinterpret_cast<uintptr_t>(ema), pp = reinterpret_cast<uintptr_t>(p);
  LO_REQUIRE(ema && p && n >= 1 && pe % 16 == 0 && pp % 16 == 0, "lo_ema_update: ema and p must be non-null and 16-byte aligned, n >= 1");
  LO_REQUIRE(pe + 4 * n <= pp || pp + 4 * n <= pe, "lo_ema_update: ema and p overlap");
  LO_REQUIRE(one_minus_decay >= 0.f && one_minus_decay <= 1.f, "lo_ema_update: 1 - decay = %g outside [0, 1]", (double)one_minus_decay);
  constexpr int max_blocks = 256;   // one workgroup per CU, as lo_adamw
  const size_t want = (n / 4 + 255) / 256;
  const int nblk = want >= (size_t)max_blocks ? max_blocks : (want < 1 ? 1 : (int)want);
  LoProfScope _p("lo_ema_update", 0, 12.0 * n, st);
  hipLaunchKernelGGL(lo_ema_kernel, dim3(nblk), dim3(256), 0, st, ema, p, n, one_minus_decay, gate);
  LO_LAUNCH_CHECK("ema_update");
  return LO_OK;
}

extern "C" int lo_ema_update(float* ema, const float* p, size_t n, float one_minus_decay, const float* gate, void* stream) {
  return lo_ema_run(ema, p, n, one_minus_decay, gate, S(stream));
}
