// The three Linear layers of the VAE (fc_mu | fc_logvar as one [2L, 32768] matrix, decoder.fc [32768, L]; lunar_generate.py:124-125,
// 150-152, 165, 207-208) hold 82 % of its parameters, and at batch B their weight gradients dW = dY^T X are rank-B matrices (B = 64
// against 512 .. 32768 rows and columns).  The fused training step never writes them:
//
//   * clip_grad_norm_ (train_hybrid.py:913):  ||dW||_F^2 = sum_{b,b'} (dY dY^T)[b,b'] (X X^T)[b,b']  -- two B x B Gram matrices
//     (lo_gram_small for the factor with the short rows, lo_gram_dot for the one with the long rows; the second one multiplies its
//     partial Gram blocks with the first one's entries on the way and leaves one scalar per wave in the norm's partial-sum slots);
//   * AdamW (train_hybrid.py:921):  lo_adamw_lowrank forms each 16 x 16 gradient tile on the fly -- two v_mfma_f32_16x16x32_f16 per
//     tile at B = 64, operands the transposed factors X^T [K][B], dY^T [N][B] (8.6 MB in all: cache-resident) -- and runs the
//     element update of lo_adamw on the accumulators: 24 bytes of HBM traffic per parameter (+2 for the fp16 operand copy) instead
//     of 28 + 2, and neither the 4 bytes written by a weight-gradient GEMM nor the 4 read by the norm exist.
//
// The MFMA tile is laid out so that the accumulator rows are the MEMORY-CONTIGUOUS axis of the weight matrix: D[i][j] with i = k
// (input feature) and j = n (output feature), A = X^T rows, B = dY^T rows.  A lane then owns four consecutive k of one n
// (D row = 4 (lane >> 4) + r, column = lane & 15): one 16-byte load / store per tensor and tile, 64 contiguous bytes per matrix row
// and instruction, 256 per row over the four k tiles of a wave's 64 x 64 block.
// lo_lowrank_materialize_gathered_kernel writes the same tiles (same MFMA sequence per tile, same scale) to the flat buffer: for
// tests and lo_vae_materialize_linear_grads.  No reference counterpart below aten::linear_backward / torch.optim.AdamW.
#include "lo_common.h"
#include "lo_internal.h"
#include "lo_conv_dev.h"
#include <math.h>
#include <string.h>
#include <stdlib.h>

// ---------------------------------------------------------------------------------------------
// dst[c][r] = src[r][c] (r < R), 0 for R <= r < Rp: a factor [B][C] -> its transposed, batch-padded form [C][Bp].  All factors of
// a step in ONE launch (job table by value): the four launches this replaces cost 7 us each for 8.6 MB in all.
// ---------------------------------------------------------------------------------------------
struct LoTransposeJob { const f16* src; f16* dst; int C, tile0; };
struct LoTransposeJobs { LoTransposeJob j[4]; int n, R, Rp; };
__global__ __launch_bounds__(256) void lo_transpose_pad_f16_kernel(LoTransposeJobs J) {
  __shared__ f16 t[64][72];
  int ji = 0;
#pragma unroll
  for (int q = 1; q < 4; ++q)
    if (q < J.n && (int)blockIdx.x >= J.j[q].tile0) ji = q;
  const LoTransposeJob job = J.j[ji];
  const int R = J.R, Rp = J.Rp, C = job.C;
  const int tile = blockIdx.x - job.tile0, ctiles = C / 64;
  const int c0 = (tile % ctiles) * 64, r0 = (tile / ctiles) * 64;
  const int tid = threadIdx.x;
  {
    const int r = tid >> 2, cc = (tid & 3) * 16;
    f16x8 a = {0, 0, 0, 0, 0, 0, 0, 0}, b = a;
    if (r0 + r < R) {
      const f16* p = job.src + (size_t)(r0 + r) * C + c0 + cc;
      a = *reinterpret_cast<const f16x8*>(p);
      b = *reinterpret_cast<const f16x8*>(p + 8);
    }
    *reinterpret_cast<f16x8*>(&t[r][cc]) = a;
    *reinterpret_cast<f16x8*>(&t[r][cc + 8]) = b;
  }
  __syncthreads();
  {
    const int c = tid >> 2, rr = (tid & 3) * 16;
    if (r0 + rr < Rp) {
      f16x8 a, b;
#pragma unroll
      for (int q = 0; q < 8; ++q) { a[q] = t[rr + q][c]; b[q] = t[rr + 8 + q][c]; }
      f16* p = job.dst + (size_t)(c0 + c) * Rp + r0 + rr;
      *reinterpret_cast<f16x8*>(p) = a;
      *reinterpret_cast<f16x8*>(p + 8) = b;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Gram matrices.  src: a factor in its natural layout [B][n] (row b = sample b).  Fragment of rows 16 bi .. 16 bi + 15 for the
// 32 columns of step kc: lane l holds row 16 bi + (l & 15), columns 32 kc + 8 (l >> 4) .. + 7 (one 16-byte load; rows >= B read
// as zero).  The same register is the A operand (row index = output row) and the B operand (row index = output column) of
// v_mfma_f32_16x16x32_f16, so tile (bi, bj) of src src^T is mfma(frag(bi), frag(bj)).
// Both Linear layers in one launch each (blockIdx.y / blockIdx.z = layer): a first version with one launch per layer and kernel,
// one workgroup for the small matrix and dependent loads inside the step loops, took 36 us per layer; the loads are now issued in
// batches of 8 steps (small) / 4 steps (long) before the MFMAs that consume them.
// ---------------------------------------------------------------------------------------------
// one layer of either norm (this rank's factors, natural layout, or the gathered ones, transposed): the long factor's contraction
// is cut into `chunks` pieces of `per` steps, one partial-sum slot per (chunk, cell of the Gram matrix) -- lowrank_gram_layer below
struct LoGramLayer { const f16* fshort; const f16* flong; float* gram; float* partial; int n_short, n_long, chunks, per, nslots; };
struct LoGramJobs { LoGramLayer l[2]; int B, Bp; float scale2; };
__device__ __forceinline__ f16x8 lo_gram_frag(const f16* __restrict__ src, int B, int n, int bi, int kc, int lane) {
  const int r = bi * 16 + (lane & 15);
  f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  if (r >= B) return z;
  return *reinterpret_cast<const f16x8*>(src + (size_t)r * n + kc * 32 + (lane >> 4) * 8);
}
// the factor with the short rows (n = 2L or L): its Gram matrix [Bp][Bp] (fp32).  One workgroup per 16 x 16 tile and layer; the
// four waves split the row length, each issues ALL its fragment loads before its first MFMA (up to 8 steps = 16 loads), and the
// four partial tiles are added in wave order through LDS.  (One 1024-thread workgroup per layer took 26 us: 256 KB of loads
// through one CU's vector memory path, four dependent batches.)
__global__ __launch_bounds__(256) void lo_gram_small_kernel(LoGramJobs J) {
  __shared__ f32x4 part[4][64];
  const LoGramLayer L = J.l[blockIdx.y];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int B = J.B, Bp = J.Bp, Bt = Bp / 16, n = L.n_short, steps = n / 32;
  const int tile = blockIdx.x;
  if (tile >= Bt * Bt) return;
  const int bi = tile / Bt, bj = tile - bi * Bt;
  const int per = (steps + 3) / 4, k0 = wave * per, k1 = k0 + per < steps ? k0 + per : steps;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int kc0 = k0; kc0 < k1; kc0 += 8) {
    f16x8 fa[8], fb[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int kc = kc0 + q < k1 ? kc0 + q : k1 - 1;
      fa[q] = lo_gram_frag(L.fshort, B, n, bi, kc, lane);
      fb[q] = bi == bj ? fa[q] : lo_gram_frag(L.fshort, B, n, bj, kc, lane);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (kc0 + q < k1) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[q], fb[q], acc, 0, 0, 0);
  }
  part[wave][lane] = acc;
  __syncthreads();
  if (wave == 0) {
    const f32x4 t = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
#pragma unroll
    for (int r = 0; r < 4; ++r) L.gram[(size_t)(bi * 16 + (lane >> 4) * 4 + r) * Bp + bj * 16 + (lane & 15)] = t[r];
  }
}
// the factor with the long rows (n = 32768): one wave per (column chunk, 64 x 64 block of the Gram matrix); the block's partial
// sums are multiplied with the other factor's Gram entries and reduced to ONE scalar per wave:
//   partial[slot] = scale^2 * sum_{b,b' in block} small[b][b'] * (sum_{c in chunk} src[b][c] src[b'][c])
// -- the chunk's share of ||dW||_F^2 (non-negative: it is the squared norm of the gradient's columns / rows of that chunk).
// Every one of the layer's `nslots` partial-sum slots is written (unused ones with zero).
__global__ __launch_bounds__(64) void lo_gram_dot_kernel(LoGramJobs J) {
  const LoGramLayer L = J.l[blockIdx.y];
  const int lane = threadIdx.x;
  const int B = J.B, Bp = J.Bp, Bt = Bp / 16, nblk = (Bt + 3) / 4, n = L.n_long;
  const int slot = blockIdx.x;
  const int blk = slot / L.chunks, chunk = slot - blk * L.chunks;
  if (blk >= nblk * nblk) {
    if (lane == 0 && slot < L.nslots) L.partial[slot] = 0.f;
    return;
  }
  const int bi0 = (blk / nblk) * 4, bj0 = (blk % nblk) * 4;
  const int kc0 = chunk * L.per;
  int kc1 = kc0 + L.per;
  if (kc1 > n / 32) kc1 = n / 32;
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const bool diag = bi0 == bj0;
  for (int kb = kc0; kb < kc1; kb += 4) {
    f16x8 fa[4][4], fb[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int kc = kb + q < kc1 ? kb + q : kc1 - 1;
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[q][i] = lo_gram_frag(L.flong, B, n, bi0 + i, kc, lane);
      if (!diag) {
#pragma unroll
        for (int j = 0; j < 4; ++j) fb[q][j] = lo_gram_frag(L.flong, B, n, bj0 + j, kc, lane);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (kb + q < kc1) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[q][i], diag ? fa[q][j] : fb[q][j], acc[i][j], 0, 0, 0);
      }
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (bi0 + i < Bt && bj0 + j < Bt) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          s += acc[i][j][r] * L.gram[(size_t)((bi0 + i) * 16 + (lane >> 4) * 4 + r) * Bp + (bj0 + j) * 16 + (lane & 15)];
      }
  s = lo_wave_sum(s);
  if (lane == 0) L.partial[slot] = s * J.scale2;
}

// ---------------------------------------------------------------------------------------------
// AdamW on a weight matrix whose gradient is given by its factors
// ---------------------------------------------------------------------------------------------
struct LoLowrankArgs {
  float* p; float* m; float* v;   // [N][K] fp32 (parameter, Adam moments)
  f16* cast;                      // [N][K] fp16 operand copy of the updated parameter (may be null)
  f16* cast_t;                    // [K][N] the same, transposed (operand of the layer's data gradient; may be null)
  const f16* xt;                  // X^T  [K][Bp]
  const f16* yt;                  // dY^T [N][Bp]
  int N, K, Bp;
  float gscale;                   // 1 / loss scale
  const float* norm;              // [1] clip coefficient, [2] finite flag (lo_gradnorm)
  float lr, beta1, beta2, eps, wd, bc1, bc2_sqrt;
};

// the element update of lo_adamw (lo_train.hip): same operations in the same order, contraction off
__device__ __forceinline__ void lo_adamw_elem_lr(float& p, float g, float& m, float& v, float coef, float decay, float omb1, float beta2,
                                                 float omb2, float bc2_sqrt, float eps, float step_size) {
#pragma clang fp contract(off)
  const float gg = g * coef;
  const float pp = p * decay;
  const float mm = __builtin_fmaf(gg - m, omb1, m);
  const float v2 = __builtin_fmaf(omb2 * gg, gg, v * beta2);
  const float denom = sqrtf(v2) / bc2_sqrt + eps;
  p = __builtin_fmaf(-step_size, mm / denom, pp);
  m = mm;
  v = v2;
}

// One wave owns a 64-column band of the matrix (k0 .. k0 + 63: its 4 x KB X^T fragments are loaded ONCE) and walks down the rows
// in 16-row groups: per group KB dY^T fragments and 4 tiles x (p, m, v) 16-byte loads.  The walk is software-pipelined over the
// groups, across 64-row tile boundaries: the loads of group g + 1 are issued before the MFMAs and the update of group g, so a lane
// always has 12 - 24 loads in flight; two workgroups per CU (8 waves) keep ~100 KB per CU outstanding where a wave fits into 256
// registers: KB <= 3 (the counts are at the launch, lo_adamw_lowrank).
// Both matrices of the model share ONE launch (LoLowrankPair): one ramp and one tail instead of two.
// Neighbouring waves own neighbouring bands: the 256-byte row segments of the waves of a workgroup are contiguous in memory.
// (The first version -- one wave per 64 x 64 block, nothing in flight across blocks -- ran at 4.8 TB/s against lo_adamw's 6.2.)
struct LoLowrankPair { LoLowrankArgs l[2]; int nwg0; };      // workgroups [0, nwg0) update matrix 0, the rest matrix 1
// cast_t: the transposed fp16 copy leaves through LDS -- a wave's 64 x 64 block of updated parameters is collected [k][n] in the
// wave's own 9 KB of LDS (2-byte writes as the groups complete) and stored as 64 rows of 128 contiguous bytes once the block's four
// groups are done: 2 more bytes per parameter on this pass instead of a separate transpose pass over both fp16 copies (4 bytes per
// parameter, 45 us per step for the two matrices).
#define LR_TP 72     // LDS pitch of a transposed block in halves (64 + 8: rows 144 bytes apart)
// what every element of a launch shares: clip coefficient and the constants of lo_adamw
struct LoLowrankConsts { float coef, step_size, decay, omb1, omb2; };
__device__ __forceinline__ LoLowrankConsts lo_lowrank_consts(const LoLowrankArgs& a) {
  return {a.norm ? a.norm[1] : 1.0f, a.lr / a.bc1, 1.0f - a.lr * a.wd, 1.0f - a.beta1, 1.0f - a.beta2};
}
// One 16 x 16 tile: the element update on the accumulator, p / m / v and the fp16 copy stored at element offset `off` (a lane's
// four consecutive k of one n), and the 2-byte scatter into the wave's transposed LDS block tb at rows krow .. krow + 3, column ncol
__device__ __forceinline__ void lo_lowrank_update_tile(const LoLowrankArgs& a, const LoLowrankConsts& c, size_t off, f32x4 acc, f32x4 pe,
                                                       f32x4 me, f32x4 ve, f16* tb, int krow, int ncol) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float pr = pe[r], mr = me[r], vr = ve[r];
    lo_adamw_elem_lr(pr, acc[r] * a.gscale, mr, vr, c.coef, c.decay, c.omb1, a.beta2, c.omb2, a.bc2_sqrt, a.eps, c.step_size);
    pe[r] = pr; me[r] = mr; ve[r] = vr;
  }
  *reinterpret_cast<f32x4*>(a.p + off) = pe;
  *reinterpret_cast<f32x4*>(a.m + off) = me;
  *reinterpret_cast<f32x4*>(a.v + off) = ve;
  if (a.cast) *reinterpret_cast<f16x4*>(a.cast + off) = (f16x4){(f16)pe[0], (f16)pe[1], (f16)pe[2], (f16)pe[3]};
  if (a.cast_t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) tb[(krow + r) * LR_TP + ncol] = (f16)pe[r];
  }
}
// A wave's 64 x 64 block is in (four 16-row groups): 64 rows (k, from k0) x 64 columns (n, from n_first); instruction j stores rows
// 8 j .. 8 j + 7, 128 contiguous bytes each
__device__ __forceinline__ void lo_lowrank_flush_block(const LoLowrankArgs& a, const f16* tb, int k0, size_t n_first, int lane) {
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int kk = 8 * j + (lane >> 3), ch = lane & 7;
    *reinterpret_cast<f16x8*>(a.cast_t + (size_t)(k0 + kk) * a.N + n_first + 8 * ch) = *reinterpret_cast<const f16x8*>(tb + kk * LR_TP + 8 * ch);
  }
  __builtin_amdgcn_wave_barrier();
}

template <int KB>
__global__ __launch_bounds__(256) void lo_adamw_lowrank_kernel(LoLowrankPair A) {
  __shared__ __attribute__((aligned(16))) f16 tbuf[4][64 * LR_TP];
  const bool second = (int)blockIdx.x >= A.nwg0;
  const LoLowrankArgs& a = second ? A.l[1] : A.l[0];
  const int bid = second ? (int)blockIdx.x - A.nwg0 : (int)blockIdx.x, nbl = second ? (int)gridDim.x - A.nwg0 : A.nwg0;
  const LoLowrankConsts c = lo_lowrank_consts(a);
  if (a.norm && a.norm[2] == 0.f) return;                // non-finite norm / lost launch: the update is skipped
  const int lane = threadIdx.x & 63, l15 = lane & 15, lq = lane >> 4;
  const int bands = a.K / 64, tiles_n = a.N / 64;
  const int W = nbl * 4, gw = bid * 4 + (threadIdx.x >> 6);
  const int wpb = W >= bands ? W / bands : 1;            // waves per band
  const int Bp = a.Bp;
  f16* tb = &tbuf[threadIdx.x >> 6][0];
  for (int vw = gw; vw < bands * wpb; vw += W) {
    const int band = vw % bands, sub = vw / bands;
    if (sub >= tiles_n) continue;
    const int k0 = band * 64;
    const int ngroups = ((tiles_n - sub + wpb - 1) / wpb) * 4;
    f16x8 xf[4][KB];
#pragma unroll
    for (int ik = 0; ik < 4; ++ik)
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
        xf[ik][kb] = *reinterpret_cast<const f16x8*>(a.xt + (size_t)(k0 + 16 * ik + l15) * Bp + 32 * kb + 8 * lq);
    f32x4 pv[2][4], mv[2][4], vv[2][4];
    f16x8 yf[2][KB];
    auto row_of = [&](int g) { return (size_t)((sub + (g >> 2) * wpb) * 64 + 16 * (g & 3) + l15); };
    auto load_group = [&](int g, int buf) {
      const size_t row = row_of(g);
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) yf[buf][kb] = *reinterpret_cast<const f16x8*>(a.yt + row * Bp + 32 * kb + 8 * lq);
      const size_t base = row * a.K + k0 + 4 * lq;
#pragma unroll
      for (int ik = 0; ik < 4; ++ik) {
        pv[buf][ik] = *reinterpret_cast<const f32x4*>(a.p + base + 16 * ik);
        mv[buf][ik] = *reinterpret_cast<const f32x4*>(a.m + base + 16 * ik);
        vv[buf][ik] = *reinterpret_cast<const f32x4*>(a.v + base + 16 * ik);
      }
    };
    auto do_group = [&](int g, int buf) {
      const size_t base = row_of(g) * a.K + k0 + 4 * lq;
#pragma unroll
      for (int ik = 0; ik < 4; ++ik) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(xf[ik][kb], yf[buf][kb], acc, 0, 0, 0);
        lo_lowrank_update_tile(a, c, base + 16 * ik, acc, pv[buf][ik], mv[buf][ik], vv[buf][ik], tb, 16 * ik + 4 * lq, 16 * (g & 3) + l15);
      }
      if (a.cast_t && (g & 3) == 3) lo_lowrank_flush_block(a, tb, k0, (size_t)(sub + (g >> 2) * wpb) * 64, lane);
    };
    load_group(0, 0);
    for (int g = 0; g < ngroups; g += 2) {               // ngroups is a multiple of 4
      load_group(g + 1, 1);
      do_group(g, 0);
      if (g + 2 < ngroups) load_group(g + 2, 0);
      do_group(g + 1, 1);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Data parallel: the ranks all-gather their FACTORS (8.6 MB of fp16 per rank at batch 64 / latent 512, exact) instead of exchanging
// 201 MB of weight gradients, and every rank forms the averaged gradient itself:  dW = (1 / N) sum_r dY_r^T X_r  -- the same tiles
// with the contraction running over the N gathered blocks (K = N * Bp).  One wave per 64 x 64 block of the matrix, 16 accumulator
// tiles in registers; per (rank, 32-sample step) 4 + 4 fragment loads (L2-resident: 2 N KB per 4096 elements) and 16 MFMAs.
// xt / yt point at the factor inside block 0; rstride = elements from one rank's block to the next.
// ---------------------------------------------------------------------------------------------
struct LoGatherMatArgs { float* gout; const f16* xt; const f16* yt; size_t rstride; int N, K, Bp, world; float gscale; };
__global__ __launch_bounds__(256) void lo_lowrank_materialize_gathered_kernel(LoGatherMatArgs a) {
  const int lane = threadIdx.x & 63, l15 = lane & 15, lq = lane >> 4;
  const int tiles_k = a.K / 64, total = (a.N / 64) * tiles_k, KB = a.Bp / 32;
  for (int t = blockIdx.x * 4 + (threadIdx.x >> 6); t < total; t += gridDim.x * 4) {
    const int tn = t / tiles_k, tk = t - tn * tiles_k;
    const int n0 = tn * 64, k0 = tk * 64;
    f32x4 acc[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[j][i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < a.world; ++r) {
      const f16* xr = a.xt + (size_t)r * a.rstride;
      const f16* yr = a.yt + (size_t)r * a.rstride;
      for (int kb = 0; kb < KB; ++kb) {
        f16x8 xf[4], yf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) xf[i] = *reinterpret_cast<const f16x8*>(xr + (size_t)(k0 + 16 * i + l15) * a.Bp + 32 * kb + 8 * lq);
#pragma unroll
        for (int j = 0; j < 4; ++j) yf[j] = *reinterpret_cast<const f16x8*>(yr + (size_t)(n0 + 16 * j + l15) * a.Bp + 32 * kb + 8 * lq);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xf[i], yf[j], acc[j][i], 0, 0, 0);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const f32x4 g = {acc[j][i][0] * a.gscale, acc[j][i][1] * a.gscale, acc[j][i][2] * a.gscale, acc[j][i][3] * a.gscale};
        *reinterpret_cast<f32x4*>(a.gout + (size_t)(n0 + 16 * j + l15) * a.K + k0 + 16 * i + 4 * lq) = g;
      }
  }
}

// ---------------------------------------------------------------------------------------------
// Data parallel, mode 3: the factored AdamW and the Gram norm straight from the gathered blocks -- the averaged matrices are never
// written.  KT = world * Bp <= 512 is the combined batch axis (rank-major: rank r's Bp columns at 32-sample steps r Bp / 32 ..).
//
// AdamW.  lo_adamw_lowrank keeps a band's X^T fragments in registers (4 x Bp / 32 x 4 VGPRs); at KT = 512 that alone would be 256.
// Here a workgroup of NW waves owns ONE 64-column band and NW x TPW row tiles of 64 rows: it stages the band's X^T rows of all ranks
// in LDS once (64 rows x KT halves, 64 KB at 512; rows 16 bytes apart from a multiple of 64 bytes.  By the bank rule, not by a
// counter: the 16-lane groups of a ds_read_b128 fragment read are then 2-way at worst, which at KT = 512 is about a quarter of
// the LDS time that the HBM traffic of the same group leaves room for), and
// every wave walks its row tiles (w, w + NW of the chunk) in 16-row groups like the single-process kernel: the dY^T fragments of group
// g + 1 (L2 / Infinity-Cache resident) and its p / m / v are loaded behind the MFMAs of group g, before g's element update; a wave's
// first loads are issued ahead of the staging.  NW = 4, one tile per wave up to KT = 256 (53 / 70 KB of LDS: two workgroups per
// CU); NW = 8, two tiles per wave above (137 KB: one workgroup per CU, the same 8 waves, the 64 KB of staging shared by 16 tiles).
// Neighbouring workgroups own neighbouring bands, as neighbouring waves do in lo_adamw_lowrank: what is resident on the chip covers
// whole rows of the matrix.  (lo_xcd_remap -- every XCD on its own contiguous range of bands, so that the 8 bands of decoder.fc
// that share 1 MB of Gfc^T meet in one L2 -- is NOT used: with it all XCDs start in the same two 16 KB column windows of
// fc_mu | fc_logvar's 128 KB rows, and the pass was 9 % slower at KT = 64.)  Measured: profiles/dp_factored_adamw_ab.md; still
// 1.5 x the single-process kernel, whose four waves per workgroup cover 1 KB of every row where this one covers 256 bytes.
// The contraction runs rank by rank, 32 samples at a time, in ONE accumulator per tile: a fixed order, no atomics -- every rank
// forms the same bits from the same gathered buffer.
// ---------------------------------------------------------------------------------------------
struct LoGatherPair { LoLowrankArgs l[2]; int nwg0, world; size_t rstride; };
template <int KSMAX, int NW, int TPW>
__global__ __launch_bounds__(64 * NW) void lo_adamw_lowrank_gathered_kernel(LoGatherPair A) {
  constexpr int XP = KSMAX * 32 + 8;                     // LDS pitch of a staged X^T row in halves
  __shared__ __attribute__((aligned(16))) f16 xs[64 * XP];
  __shared__ __attribute__((aligned(16))) f16 tbuf[NW][64 * LR_TP];
  const bool second = (int)blockIdx.x >= A.nwg0;
  const LoLowrankArgs& a = second ? A.l[1] : A.l[0];
  const LoLowrankConsts c = lo_lowrank_consts(a);
  if (a.norm && a.norm[2] == 0.f) return;                // non-finite norm / lost launch: the update is skipped
  const int bid = second ? (int)blockIdx.x - A.nwg0 : (int)blockIdx.x;
  // neighbouring workgroups own neighbouring bands: what is resident on the chip at any moment covers whole rows of the matrix
  const int bands = a.K / 64, tiles_n = a.N / 64;
  const int band = bid % bands, chunk = bid / bands, k0 = band * 64;
  const int Bp = a.Bp, KT = A.world * Bp, KS = KT / 32, c8n = KT / 8;
  const int lane = threadIdx.x & 63, l15 = lane & 15, lq = lane >> 4, wave = threadIdx.x >> 6;
  const int tile0 = chunk * (TPW * NW) + wave;
  const bool live = tile0 < tiles_n;                     // a wave without a row tile only helps staging
  const int ngroups = TPW == 2 && tile0 + NW < tiles_n ? 8 : 4;
  f16* tb = &tbuf[wave][0];
  size_t yoff[KSMAX];                                    // where 32-sample step ks starts inside a dY^T row: rank block + column (wave-uniform)
#pragma unroll
  for (int ks = 0; ks < KSMAX; ++ks) {
    const int col = 32 * ks, r = col / Bp;
    yoff[ks] = (size_t)r * A.rstride + (col - r * Bp);
  }
  f32x4 pv[2][4], mv[2][4], vv[2][4], acc[4];
  f16x8 yf[KSMAX];
  auto row_of = [&](int g) { return (size_t)((tile0 + NW * (g >> 2)) * 64 + 16 * (g & 3) + l15); };
  auto load_y = [&](int g) {
    const f16* yr = a.yt + row_of(g) * Bp + 8 * lq;
#pragma unroll
    for (int ks = 0; ks < KSMAX; ++ks)
      if (ks < KS) yf[ks] = *reinterpret_cast<const f16x8*>(yr + yoff[ks]);
  };
  auto load_pmv = [&](int g, int buf) {
    const size_t base = row_of(g) * a.K + k0 + 4 * lq;
#pragma unroll
    for (int ik = 0; ik < 4; ++ik) {
      pv[buf][ik] = *reinterpret_cast<const f32x4*>(a.p + base + 16 * ik);
      mv[buf][ik] = *reinterpret_cast<const f32x4*>(a.m + base + 16 * ik);
      vv[buf][ik] = *reinterpret_cast<const f32x4*>(a.v + base + 16 * ik);
    }
  };
  auto tiles = [&]() {
#pragma unroll
    for (int ik = 0; ik < 4; ++ik) acc[ik] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KSMAX; ++ks)
      if (ks < KS) {
#pragma unroll
        for (int ik = 0; ik < 4; ++ik) {
          const f16x8 xf = *reinterpret_cast<const f16x8*>(&xs[(16 * ik + l15) * XP + 32 * ks + 8 * lq]);
          acc[ik] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xf, yf[ks], acc[ik], 0, 0, 0);
        }
      }
  };
  auto update = [&](int g, int buf) {
    const size_t base = row_of(g) * a.K + k0 + 4 * lq;
#pragma unroll
    for (int ik = 0; ik < 4; ++ik)
      lo_lowrank_update_tile(a, c, base + 16 * ik, acc[ik], pv[buf][ik], mv[buf][ik], vv[buf][ik], tb, 16 * ik + 4 * lq, 16 * (g & 3) + l15);
    if (a.cast_t && (g & 3) == 3) lo_lowrank_flush_block(a, tb, k0, (size_t)(tile0 + NW * (g >> 2)) * 64, lane);
  };
  if (live) { load_y(0); load_pmv(0, 0); }
  for (int i = threadIdx.x; i < 64 * c8n; i += 64 * NW) {
    const int row = i / c8n, col = (i - row * c8n) * 8, r = col / Bp, b = col - r * Bp;
    *reinterpret_cast<f16x8*>(&xs[row * XP + col]) = *reinterpret_cast<const f16x8*>(a.xt + (size_t)r * A.rstride + (size_t)(k0 + row) * Bp + b);
  }
  __syncthreads();
  if (!live) return;                                     // (no workgroup barrier below)
  for (int g = 0; g < ngroups; g += 2) {                 // ngroups is 4 or 8
    tiles();
    load_y(g + 1);
    load_pmv(g + 1, 1);
    update(g, 0);
    tiles();
    if (g + 2 < ngroups) { load_y(g + 2); load_pmv(g + 2, 0); }
    update(g + 1, 1);
  }
}

// The norm.  ||sum_r dY_r^T X_r||_F^2 = sum_{b,b'} (dY dY^T)[b,b'] (X X^T)[b,b'] over the combined batch axis, cross-rank terms
// included.  The gathered factors are TRANSPOSED ([n][Bp] per rank): the Gram contraction runs over their slow axis, so tiles of
// [64 c][128 b] are staged in LDS (the next tile's loads in flight behind the barrier; rows c >= n are zero) and the MFMA
// fragments come from transposed LDS reads, with the image and block swizzle of the
// weight-gradient kernels (lo_tr_swz<256>, lo_conv_dev.h).  (Transposing the blocks back first would write and re-read world x 8.6 MB
// per step for a layout only this norm wants; the staged form reads each factor once per 128-sample block row or column.)
// A workgroup owns one pair (I <= J) of 128-sample blocks, its four waves a 64 x 64 quarter each (16 accumulator tiles); the Gram
// matrix is symmetric, so off-diagonal pairs count twice and pairs I > J are neither computed nor stored.
//   DOT = false  the factor with the short rows: the pair's block of its Gram matrix [KT][KT] (all c steps in one workgroup)
//   DOT = true   the factor with the long rows, one c chunk per workgroup: partial[slot] = weight * scale^2 * sum over the block of
//                small[b][b'] * (sum_{c in chunk} src[c][b] src[c][b'])  -- one slot per workgroup, added in wave order through LDS;
//                slots beyond pairs x chunks are zeroed.  (A slot of an off-diagonal pair can be negative; their sum is the norm.)
struct LoGramTJobs { LoGramLayer l[2]; size_t rstride; int Bp, KT, nb; float scale2; };
template <bool DOT>
__global__ __launch_bounds__(256) void lo_gram_gathered_kernel(LoGramTJobs J) {
  __shared__ __attribute__((aligned(1024))) unsigned char smem[2][2][64 * 256];      // [buffer][side][64 c rows][128 b]
  __shared__ float wsum[4];
  const LoGramLayer L = J.l[blockIdx.y];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
  const int nb = J.nb, npairs = nb * (nb + 1) / 2, KT = J.KT, Bp = J.Bp;
  const int slot = blockIdx.x, chunks = DOT ? L.chunks : 1;
  const int pair = slot / chunks, chunk = slot - pair * chunks;
  if (pair >= npairs) {
    if (DOT && tid == 0 && slot < L.nslots) L.partial[slot] = 0.f;
    return;
  }
  int bI = 0, rem = pair;
  while (rem >= nb - bI) { rem -= nb - bI; ++bI; }
  const int bJ = bI + rem;
  const f16* src = DOT ? L.flong : L.fshort;
  const int n = DOT ? L.n_long : L.n_short, steps = (n + 63) / 64;
  const int s0 = DOT ? chunk * L.per : 0, s1 = DOT ? (s0 + L.per < steps ? s0 + L.per : steps) : steps;
  // staging: thread -> four 16-byte chunks per side (row = c inside the step, pos = chunk of the 128 samples); samples >= KT are zero
  size_t goff[2][4];
  bool gok[2][4];
  int grow[4], soff[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int q = tid + 256 * j, row = q >> 4, pos = q & 15;
    grow[j] = row;
    soff[j] = row * 256 + ((((pos >> 1) ^ lo_tr_swz<256>(row)) << 1) | (pos & 1)) * 16;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      const int b = (side ? bJ : bI) * 128 + pos * 8, r = b / Bp;
      gok[side][j] = b < KT;
      goff[side][j] = (size_t)r * J.rstride + (size_t)row * Bp + (b - r * Bp);
    }
  }
  f16x8 reg[2][4];
  auto gload = [&](int s) {
#pragma unroll
    for (int side = 0; side < 2; ++side)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        if (gok[side][j] && s * 64 + grow[j] < n) z = *reinterpret_cast<const f16x8*>(src + goff[side][j] + (size_t)s * 64 * Bp);
        reg[side][j] = z;
      }
  };
  // transposed fragment reads as in lo_wgrad_tn: per 32 rows, lane group q reads rows 4q .. 4q + 3 and 16 + 4q .. 16 + 4q + 3 --
  // the same k permutation for both operands
  const int q16 = lane >> 4, i16 = lane & 15;
  const int trow = 4 * q16 + (i16 >> 2), tsub = (i16 & 3) * 8;
  int aoff[4][4], boff[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int R = trow + 16 * h;
      aoff[i][h] = R * 256 + (((wm * 4 + i) ^ lo_tr_swz<256>(R)) * 32) + tsub;
      boff[i][h] = 64 * 256 + R * 256 + (((wn * 4 + i) ^ lo_tr_swz<256>(R)) * 32) + tsub;
    }
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  gload(s0);
  int buf = 0;
  for (int s = s0; s < s1; ++s) {
    unsigned char* sb = &smem[buf][0][0];
#pragma unroll
    for (int side = 0; side < 2; ++side)
#pragma unroll
      for (int j = 0; j < 4; ++j) *reinterpret_cast<f16x8*>(sb + side * 64 * 256 + soff[j]) = reg[side][j];
    __syncthreads();               // one barrier per step: the other buffer is rewritten only after every wave has passed this one
    if (s + 1 < s1) gload(s + 1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      f16x8 af[4], bf[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        h16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((h16x4 __attribute__((address_space(3)))*)(sb + aoff[i][2 * kk]));
        h16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((h16x4 __attribute__((address_space(3)))*)(sb + aoff[i][2 * kk + 1]));
        af[i] = (f16x8){(f16)lo[0], (f16)lo[1], (f16)lo[2], (f16)lo[3], (f16)hi[0], (f16)hi[1], (f16)hi[2], (f16)hi[3]};
        lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((h16x4 __attribute__((address_space(3)))*)(sb + boff[i][2 * kk]));
        hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((h16x4 __attribute__((address_space(3)))*)(sb + boff[i][2 * kk + 1]));
        bf[i] = (f16x8){(f16)lo[0], (f16)lo[1], (f16)lo[2], (f16)lo[3], (f16)hi[0], (f16)hi[1], (f16)hi[2], (f16)hi[3]};
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    buf ^= 1;
  }
  // acc[i][j][r]: b = 128 I + 64 wm + 16 i + 4 (lane >> 4) + r,  b' = 128 J + 64 wn + 16 j + (lane & 15)
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int bc = bJ * 128 + wn * 64 + 16 * j + i16;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int br = bI * 128 + wm * 64 + 16 * i + 4 * q16 + r;
        if (br < KT && bc < KT) {
          if (DOT) sum += acc[i][j][r] * L.gram[(size_t)br * KT + bc];
          else L.gram[(size_t)br * KT + bc] = acc[i][j][r];
        }
      }
    }
  if (!DOT) return;
  sum = lo_wave_sum(sum);
  if (lane == 0) wsum[wave] = sum;
  __syncthreads();
  if (tid == 0) L.partial[slot] = ((wsum[0] + wsum[1]) + (wsum[2] + wsum[3])) * (bI == bJ ? 1.f : 2.f) * J.scale2;
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
int lo_lowrank_bp(int B) { return (B + 31) / 32 * 32; }
bool lo_lowrank_applies(int B, int N, int K) { return B >= 1 && B <= 128 && N % 64 == 0 && K % 64 == 0; }

// up to four factors [B][C_i] -> [C_i][Bp] in one launch
int lo_transpose_pad_f16_multi(const f16* const* src, f16* const* dst, const int* C, int njobs, int R, int Rp, hipStream_t st) {
  LO_REQUIRE(njobs >= 1 && njobs <= 4 && Rp % 16 == 0 && Rp >= R, "lo_transpose_pad_f16: bad job list (n=%d R=%d Rp=%d)", njobs, R, Rp);
  LoTransposeJobs J;
  memset(&J, 0, sizeof(J));
  J.n = njobs; J.R = R; J.Rp = Rp;
  int tiles = 0;
  double bytes = 0;
  for (int i = 0; i < njobs; ++i) {
    LO_REQUIRE(C[i] % 64 == 0, "lo_transpose_pad_f16: C=%d must be a multiple of 64", C[i]);
    J.j[i].src = src[i]; J.j[i].dst = dst[i]; J.j[i].C = C[i]; J.j[i].tile0 = tiles;
    tiles += (C[i] / 64) * ((Rp + 63) / 64);
    bytes += 2.0 * ((double)R + Rp) * C[i];
  }
  LoProfScope _p("lo_factor_transpose", 0, bytes, st);
  hipLaunchKernelGGL(lo_transpose_pad_f16_kernel, dim3(tiles), dim3(256), 0, st, J);
  LO_LAUNCH_CHECK("transpose_pad_f16");
  return LO_OK;
}

// The chunk policy of both norms: a layer's `nslots` partial-sum slots are shared out over `cells` cells of the Gram matrix (64 x 64
// blocks here, pairs of 128-sample blocks for the gathered form), and each cell's contraction over `steps` steps of the long factor
// is cut into as many equal chunks as that leaves slots for.  chunks = 0: too few slots.
static LoGramLayer lowrank_gram_layer(const LoLowrankNorm& in, int cells, int steps) {
  int chunks = in.nslots / cells, per = 0;
  if (chunks > steps) chunks = steps;
  if (chunks >= 1) {
    per = (steps + chunks - 1) / chunks;
    chunks = (steps + per - 1) / per;
  }
  return {in.fshort, in.flong, in.gram, in.partial, in.n_short, in.n_long, chunks, per, in.nslots};
}

// ||dY^T X||_F^2 * scale^2 of up to two Linear layers into their `nslots` partial-sum slots each (every slot is written).
// fshort / flong: the two factors of a layer in their natural layouts [B][n_short], [B][n_long]; gram: [Bp][Bp] fp32 scratch per layer.
int lo_lowrank_sumsq(const LoLowrankNorm* layers, int nlayers, int B, float scale, hipStream_t st) {
  const int Bp = lo_lowrank_bp(B);
  LO_REQUIRE(nlayers >= 1 && nlayers <= 2 && Bp <= 128, "lo_lowrank_sumsq: bad shape");
  const int nblk = (Bp / 16 + 3) / 4;
  LoGramJobs J;
  memset(&J, 0, sizeof(J));
  J.B = B; J.Bp = Bp; J.scale2 = scale * scale;
  int maxslots = 0;
  double bytes = 0;
  for (int i = 0; i < nlayers; ++i) {
    const LoLowrankNorm& in = layers[i];
    LO_REQUIRE(in.n_short % 32 == 0 && in.n_long % 32 == 0, "lo_lowrank_sumsq: row lengths must be multiples of 32");
    J.l[i] = lowrank_gram_layer(in, nblk * nblk, in.n_long / 32);
    LO_REQUIRE(J.l[i].chunks >= 1, "lo_lowrank_sumsq: %d partial slots are too few", in.nslots);
    maxslots = in.nslots > maxslots ? in.nslots : maxslots;
    bytes += 2.0 * B * ((double)in.n_short + in.n_long);
  }
  LoProfScope _p("lo_lowrank_sumsq", 0, bytes, st);
  hipLaunchKernelGGL(lo_gram_small_kernel, dim3((Bp / 16) * (Bp / 16), nlayers), dim3(256), 0, st, J);
  LO_LAUNCH_CHECK("gram_small");
  hipLaunchKernelGGL(lo_gram_dot_kernel, dim3(maxslots, nlayers), dim3(64), 0, st, J);
  LO_LAUNCH_CHECK("gram_dot");
  return LO_OK;
}

static int lowrank_blocks(const LoLowrankArgs& a, int cap) {
  const int total = (a.N / 64) * (a.K / 64);
  int nblk = (total + 3) / 4;
  return nblk > cap ? cap : nblk;
}
// one matrix of either AdamW launch from its table entry; returns the bytes of HBM traffic it stands for
static double lowrank_fill(LoLowrankArgs& a, const LoLowrankMat& mt, int Bp, float gscale, const LoAdamHyper& hp) {
  a.p = mt.p; a.m = mt.m; a.v = mt.v; a.cast = mt.cast; a.cast_t = mt.cast_t; a.xt = mt.xt; a.yt = mt.yt; a.N = mt.N; a.K = mt.K; a.Bp = Bp;
  a.gscale = gscale; a.norm = hp.norm; a.lr = hp.lr; a.beta1 = hp.beta1; a.beta2 = hp.beta2; a.eps = hp.eps; a.wd = hp.wd;
  a.bc1 = (float)(1.0 - pow((double)hp.beta1, (double)hp.step));
  a.bc2_sqrt = (float)sqrt(1.0 - pow((double)hp.beta2, (double)hp.step));
  return (24.0 + (mt.cast ? 2.0 : 0.0) + (mt.cast_t ? 2.0 : 0.0)) * ((double)mt.N * mt.K);
}

// AdamW of up to two factored weight matrices in ONE launch (the workgroups are shared out in proportion to the element counts)
int lo_adamw_lowrank(const LoLowrankMat* mats, int nmat, int B, float gscale, const LoAdamHyper& hp, hipStream_t st) {
  LO_REQUIRE(nmat >= 1 && nmat <= 2, "lo_adamw_lowrank: one or two matrices");
  LoLowrankPair A;
  memset(&A, 0, sizeof(A));
  double elems[2] = {0, 0}, bytes = 0;
  for (int i = 0; i < nmat; ++i) {
    const LoLowrankMat& mt = mats[i];
    LO_REQUIRE(lo_lowrank_applies(B, mt.N, mt.K), "lo_adamw_lowrank: shape B=%d N=%d K=%d not supported", B, mt.N, mt.K);
    bytes += lowrank_fill(A.l[i], mt, lo_lowrank_bp(B), gscale, hp);
    elems[i] = (double)mt.N * mt.K;
  }
  // workgroups of the larger matrix.  Registers per lane (VGPR + AGPR in the code object, allocated in eights) for KB = Bp / 32 =
  // 1 / 2 / 3 / 4: 208 / 232 / 252 / 271 -- two workgroups are resident per CU up to KB = 3, one at KB = 4.  A longer grid measured
  // better on the step (batch 64), where the kernel runs beside the next forward: 512 / 1024 / 2048 / 4096 / 8192 -> 23 310 / 23 590 /
  // 23 790 / 23 230 / 23 190 sprites/s (three interleaved rounds on one box)
  constexpr int cap = 2048;
  int nb0 = lowrank_blocks(A.l[0], cap), nb1 = 0;
  if (nmat == 2) {
    int c1 = (int)(cap * elems[1] / elems[0] + 0.5);
    nb1 = lowrank_blocks(A.l[1], c1 < 1 ? 1 : c1);
  }
  A.nwg0 = nb0;
  LoProfScope _p("lo_adamw_lowrank", 0, bytes, st);     // HBM-bound: rated against the HBM roofline (2 Bp FLOP per element ride along)
  const dim3 grid(nb0 + nb1);
  switch (A.l[0].Bp / 32) {
    case 1: LO_LAUNCH_STOP((lo_adamw_lowrank_kernel<1>), grid, dim3(256), 0, st, A); break;
    case 2: LO_LAUNCH_STOP((lo_adamw_lowrank_kernel<2>), grid, dim3(256), 0, st, A); break;
    case 3: LO_LAUNCH_STOP((lo_adamw_lowrank_kernel<3>), grid, dim3(256), 0, st, A); break;
    case 4: LO_LAUNCH_STOP((lo_adamw_lowrank_kernel<4>), grid, dim3(256), 0, st, A); break;
    default: lo_set_error("lo_adamw_lowrank: batch padding %d not supported", A.l[0].Bp); return LO_ERR_ARG;
  }
  LO_LAUNCH_CHECK("adamw_lowrank");
  return LO_OK;
}

// gout = gscale * sum_r dY_r^T X_r from `world` factor blocks, rank_stride_elems apart.  One block (this rank's own, world = 1) gives
// tile for tile what lo_adamw_lowrank forms: the same MFMAs in the same kb order, the same `* gscale`
int lo_lowrank_materialize_gathered(float* gout, const f16* xt, const f16* yt, size_t rank_stride_elems, int world, int N, int K, int B,
                                    float gscale, hipStream_t st) {
  LO_REQUIRE(lo_lowrank_applies(B, N, K) && world >= 1, "lo_lowrank_materialize_gathered: shape B=%d N=%d K=%d world=%d not supported", B, N, K, world);
  LoGatherMatArgs a{gout, xt, yt, rank_stride_elems, N, K, lo_lowrank_bp(B), world, gscale};
  const int total = (N / 64) * (K / 64);
  int nblk = (total + 3) / 4;
  if (nblk > 1024) nblk = 1024;
  LoProfScope _p("lo_lowrank_materialize_gathered", 2.0 * a.Bp * world * (double)N * K, 4.0 * (double)N * K, st);
  hipLaunchKernelGGL(lo_lowrank_materialize_gathered_kernel, dim3(nblk), dim3(256), 0, st, a);
  LO_LAUNCH_CHECK("lowrank_materialize_gathered");
  return LO_OK;
}

// ---- data parallel, mode 3: straight from the gathered blocks ---------------------------------------------------------------------
template <typename... P>
static bool lo_aligned16(const P*... p) { return ((0 | ... | reinterpret_cast<uintptr_t>(p)) & 15) == 0; }   // null pointers pass
bool lo_lowrank_gathered_applies(int world, int B) { return world >= 1 && B >= 1 && B <= 128 && (long long)world * lo_lowrank_bp(B) <= 512; }
size_t lo_lowrank_gathered_gram_elems(int world, int B) { const size_t kt = (size_t)world * lo_lowrank_bp(B); return 2 * kt * kt; }

// AdamW of up to two weight matrices whose AVERAGED gradient is gscale * sum_r dY_r^T X_r: xt / yt point at the factor inside rank 0's
// block, rank r's copy sits rank_stride_elems further on per rank.  gscale carries 1 / (loss scale * world).
int lo_adamw_lowrank_gathered(const LoLowrankMat* mats, int nmat, size_t rank_stride_elems, int world, int B, float gscale,
                              const LoAdamHyper& hp, hipStream_t st) {
  LO_REQUIRE(nmat >= 1 && nmat <= 2, "lo_adamw_lowrank_gathered: one or two matrices");
  const int Bp = lo_lowrank_bp(B);
  LO_REQUIRE(lo_lowrank_gathered_applies(world, B), "lo_adamw_lowrank_gathered: world %d x padded batch %d is outside the combined rank the "
             "gathered update is built for (1 .. 512)", world, Bp);
  LO_REQUIRE(rank_stride_elems % 8 == 0, "lo_adamw_lowrank_gathered: rank stride %zu must be a multiple of 8 elements (16-byte loads)", rank_stride_elems);
  LoGatherPair A;
  memset(&A, 0, sizeof(A));
  A.world = world; A.rstride = rank_stride_elems;
  const int KS = world * Bp / 32, nw = KS <= 8 ? 4 : 8, tpw = KS <= 8 ? 1 : 2;   // waves per workgroup, row tiles per wave
  double bytes = 0, flops = 0;
  int nwg[2] = {0, 0};
  for (int i = 0; i < nmat; ++i) {
    const LoLowrankMat& mt = mats[i];
    LO_REQUIRE(lo_lowrank_applies(B, mt.N, mt.K), "lo_adamw_lowrank_gathered: shape B=%d N=%d K=%d not supported", B, mt.N, mt.K);
    LO_REQUIRE(lo_aligned16(mt.p, mt.m, mt.v, mt.cast, mt.cast_t, mt.xt, mt.yt), "lo_adamw_lowrank_gathered: every tensor pointer must be 16-byte aligned");
    bytes += lowrank_fill(A.l[i], mt, Bp, gscale, hp);
    flops += 2.0 * world * Bp * ((double)mt.N * mt.K);
    nwg[i] = (mt.K / 64) * ((mt.N / 64 + tpw * nw - 1) / (tpw * nw));
  }
  A.nwg0 = nwg[0];
  LoProfScope _p("lo_adamw_lowrank_gathered", flops, bytes, st);
#define LO_LG(KSV, NWV, TPWV) LO_LAUNCH_STOP((lo_adamw_lowrank_gathered_kernel<KSV, NWV, TPWV>), dim3(nwg[0] + nwg[1]), dim3(64 * NWV), 0, st, A)
  if (KS <= 4) LO_LG(4, 4, 1);
  else if (KS <= 8) LO_LG(8, 4, 1);
  else LO_LG(16, 8, 2);
#undef LO_LG
  LO_LAUNCH_CHECK("adamw_lowrank_gathered");
  return LO_OK;
}

// ||sum_r dY_r^T X_r||_F^2 * scale^2 of up to two Linear layers into their partial-sum slots (every slot is written).  fshort / flong:
// the layer's two factors, TRANSPOSED ([n_short][Bp], [n_long][Bp] fp16, padding columns zero), inside rank 0's block; gram: [KT][KT]
// fp32 scratch per layer (KT = world * Bp; lo_lowrank_gathered_gram_elems for two layers).
int lo_lowrank_sumsq_gathered(const LoLowrankNorm* layers, int nlayers, size_t rank_stride_elems, int world, int B, float scale, hipStream_t st) {
  const int Bp = lo_lowrank_bp(B);
  LO_REQUIRE(nlayers >= 1 && nlayers <= 2, "lo_lowrank_sumsq_gathered: one or two layers");
  LO_REQUIRE(lo_lowrank_gathered_applies(world, B), "lo_lowrank_sumsq_gathered: world %d x padded batch %d is outside the combined rank the "
             "gathered norm is built for (1 .. 512)", world, Bp);
  LO_REQUIRE(rank_stride_elems % 8 == 0, "lo_lowrank_sumsq_gathered: rank stride %zu must be a multiple of 8 elements (16-byte loads)", rank_stride_elems);
  LoGramTJobs J;
  memset(&J, 0, sizeof(J));
  J.rstride = rank_stride_elems; J.Bp = Bp; J.KT = world * Bp; J.nb = (J.KT + 127) / 128; J.scale2 = scale * scale;
  const int npairs = J.nb * (J.nb + 1) / 2;
  int maxslots = 0;
  double bytes = 0, flops = 0;
  for (int i = 0; i < nlayers; ++i) {
    const LoLowrankNorm& in = layers[i];
    LO_REQUIRE(in.n_short >= 32 && in.n_long >= 32 && in.n_short % 32 == 0 && in.n_long % 32 == 0, "lo_lowrank_sumsq_gathered: row lengths must be multiples of 32");
    LO_REQUIRE(lo_aligned16(in.fshort, in.flong), "lo_lowrank_sumsq_gathered: the factor pointers must be 16-byte aligned");
    J.l[i] = lowrank_gram_layer(in, npairs, (in.n_long + 63) / 64);     // 64 rows of the long factor per step
    LO_REQUIRE(J.l[i].chunks >= 1, "lo_lowrank_sumsq_gathered: %d partial slots are too few", in.nslots);
    maxslots = in.nslots > maxslots ? in.nslots : maxslots;
    bytes += 2.0 * J.KT * ((double)in.n_short + in.n_long);
    flops += 2.0 * 128 * 128 * npairs * ((double)in.n_short + in.n_long);
  }
  LoProfScope _p("lo_lowrank_sumsq_gathered", flops, bytes, st);
  hipLaunchKernelGGL((lo_gram_gathered_kernel<false>), dim3(npairs, nlayers), dim3(256), 0, st, J);
  LO_LAUNCH_CHECK("gram_gathered_small");
  hipLaunchKernelGGL((lo_gram_gathered_kernel<true>), dim3(maxslots, nlayers), dim3(256), 0, st, J);
  LO_LAUNCH_CHECK("gram_gathered_dot");
  return LO_OK;
}
