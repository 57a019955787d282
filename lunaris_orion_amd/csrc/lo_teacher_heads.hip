// The teacher's heads (lunar_evaluator.py:417, 425, 431-449) on the pooled features the trunk leaves in the workspace, their backward
// (A13: the gate / quality-head gradients of the reference step; in the full-backward mode also the gradients towards the trunk), and the
// reward / baseline bookkeeping of the hybrid step.
#include "lo_teacher.h"

// ---------------------------------------------------------------------------------------------
// heads: one workgroup (256 threads) per sample; everything fp32 in LDS
//   gate: pooled_f[128] -> Linear(128,I) -> lrelu -> Linear(I,E) -> softmax
//   per expert: pooled_e -> LayerNorm -> Linear(128,I/4) -> lrelu -> Linear(I/4,4)
//   semantic (expert 0): LN -> Linear(128,I/2) -> lrelu -> Linear(I/2,1) -> sigmoid
//   comb = sum_e w_e pooled_e ; style / prompt: LN -> Linear(128,I/2) -> lrelu -> Linear(I/2,emb)
// ---------------------------------------------------------------------------------------------
struct HeadW { const float *ln_w, *ln_b, *w1, *b1, *w2, *b2; };
struct HeadsArgs {
  const float* pooled_f;         // [B][128]
  const float* pooled_e;         // [E][B][128]
  const float *g_w1, *g_b1, *g_w2, *g_b2;
  HeadW q[8];
  HeadW sem, style, prompt;
  float *quality, *weights, *style_out, *prompt_out, *sem_out;   // [B][4], [B][E], [B][emb], [B][emb], [B][1]
  float* raw_q;                  // [B][E][4] pre-weighting quality logits (kept for the backward)
  int B, E, I, emb;
  int F;                         // feature_dim: width of the experts' pooled features (the gate always sees the extractor's 128)
  // nn.Dropout after the hidden LeakyReLU of the gate and of every head (lunar_evaluator.py:353-397); thr = 0: off
  uint32_t thr; float inv_keep;
  LoDropSite ds_gate, ds_q[8], ds_sem, ds_style, ds_prompt;
};
// h[o] <- Dropout(h)[o] for sample `row` of a [B][n] hidden layer (element index row*n + o)
__device__ void t_dropout(float* h, int n, int row, LoDropSite ds, uint32_t thr, float inv_keep, int tid) {
  if (!thr) return;
  for (int o = tid; o < n; o += 256) h[o] = lo_drop_keep(ds, (uint32_t)(row * n + o), thr) ? h[o] * inv_keep : 0.f;
  __syncthreads();
}
__device__ void t_layernorm(const float* x, const float* w, const float* b, float* y, float* scratch, int tid, int F) {
  // F <= 512 features, 256 threads: two elements per thread; fixed-order wave + cross-wave sums
  float v0 = tid < F ? x[tid] : 0.f, v1 = tid + 256 < F ? x[tid + 256] : 0.f;
  float s = lo_wave_sum(v0 + v1);
  if ((tid & 63) == 0) scratch[tid >> 6] = s;
  __syncthreads();
  const float mean = (((scratch[0] + scratch[1]) + scratch[2]) + scratch[3]) / (float)F;
  __syncthreads();
  const float d0 = tid < F ? v0 - mean : 0.f, d1 = tid + 256 < F ? v1 - mean : 0.f;
  float q = lo_wave_sum(d0 * d0 + d1 * d1);
  if ((tid & 63) == 0) scratch[tid >> 6] = q;
  __syncthreads();
  const float rstd = 1.f / sqrtf((((scratch[0] + scratch[1]) + scratch[2]) + scratch[3]) / (float)F + LN_EPS);
  if (tid < F) y[tid] = d0 * rstd * w[tid] + b[tid];
  if (tid + 256 < F) y[tid + 256] = d1 * rstd * w[tid + 256] + b[tid + 256];
  __syncthreads();
}
__device__ void t_linear(const float* x, int nin, const float* w, const float* b, float* y, int nout, int lrelu, int tid) {
  for (int o = tid; o < nout; o += 256) {
    float acc = b[o];
    for (int i = 0; i < nin; ++i) acc += w[o * nin + i] * x[i];
    y[o] = (lrelu && acc < 0.f) ? 0.2f * acc : acc;
  }
  __syncthreads();
}
__global__ __launch_bounds__(256) void lo_t_heads_kernel(HeadsArgs a) {
  __shared__ float xin[T_FMAX], xn[T_FMAX], h1[256], o2[512], wts[8], ql[8][4], scratch[8], comb[T_FMAX];
  const int tid = threadIdx.x, n = blockIdx.x, F = a.F;
  // gate
  if (tid < 128) xin[tid] = a.pooled_f[n * 128 + tid];
  __syncthreads();
  t_linear(xin, 128, a.g_w1, a.g_b1, h1, a.I, 1, tid);
  t_dropout(h1, a.I, n, a.ds_gate, a.thr, a.inv_keep, tid);
  t_linear(h1, a.I, a.g_w2, a.g_b2, o2, a.E, 0, tid);
  if (tid == 0) {
    float m = -INFINITY, l = 0.f;
    for (int e = 0; e < a.E; ++e) m = fmaxf(m, o2[e]);
    for (int e = 0; e < a.E; ++e) { wts[e] = __expf(o2[e] - m); l += wts[e]; }
    for (int e = 0; e < a.E; ++e) { wts[e] /= l; a.weights[n * a.E + e] = wts[e]; }
  }
  __syncthreads();
  for (int c = tid; c < F; c += 256) comb[c] = 0.f;
  __syncthreads();
  for (int e = 0; e < a.E; ++e) {
    for (int c = tid; c < F; c += 256) { xin[c] = a.pooled_e[((size_t)e * a.B + n) * F + c]; comb[c] += wts[e] * xin[c]; }
    __syncthreads();
    t_layernorm(xin, a.q[e].ln_w, a.q[e].ln_b, xn, scratch, tid, F);
    t_linear(xn, F, a.q[e].w1, a.q[e].b1, h1, a.I / 4, 1, tid);
    t_dropout(h1, a.I / 4, n, a.ds_q[e], a.thr, a.inv_keep, tid);
    t_linear(h1, a.I / 4, a.q[e].w2, a.q[e].b2, o2, 4, 0, tid);
    if (tid < 4) { ql[e][tid] = o2[tid]; a.raw_q[((size_t)n * a.E + e) * 4 + tid] = o2[tid]; }
    __syncthreads();
    if (e == 0) {
      t_layernorm(xin, a.sem.ln_w, a.sem.ln_b, xn, scratch, tid, F);
      t_linear(xn, F, a.sem.w1, a.sem.b1, h1, a.I / 2, 1, tid);
      t_dropout(h1, a.I / 2, n, a.ds_sem, a.thr, a.inv_keep, tid);
      t_linear(h1, a.I / 2, a.sem.w2, a.sem.b2, o2, 1, 0, tid);
      if (tid == 0) a.sem_out[n] = 1.f / (1.f + __expf(-o2[0]));
      __syncthreads();
    }
  }
  if (tid < 4) {
    float t = 0.f;
    for (int e = 0; e < a.E; ++e) t += ql[e][tid] * wts[e];
    a.quality[n * 4 + tid] = 1.f / (1.f + __expf(-t));
  }
  __syncthreads();
  for (int which = 0; which < 2; ++which) {
    const HeadW& hw = which ? a.prompt : a.style;
    float* dst = which ? a.prompt_out : a.style_out;
    t_layernorm(comb, hw.ln_w, hw.ln_b, xn, scratch, tid, F);
    t_linear(xn, F, hw.w1, hw.b1, h1, a.I / 2, 1, tid);
    t_dropout(h1, a.I / 2, n, which ? a.ds_prompt : a.ds_style, a.thr, a.inv_keep, tid);
    t_linear(h1, a.I / 2, hw.w2, hw.b2, o2, a.emb, 0, tid);
    for (int o = tid; o < a.emb; o += 256) dst[(size_t)n * a.emb + o] = o2[o];
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// A13: gradients of teacher_loss = -(quality_weight/accum) * mean(quality_scores) with respect to the ONLY parameters
// that receive gradients in the reference step (gate.*, quality_heads.*).  One workgroup per sample
// recomputes the tiny head forward and writes that sample's parameter-gradient contribution into row n of `rows`
// (same relative layout as the flat state between gate.2.weight and semantic_head.2.weight); a column sum over the
// batch then gives the gradient.
// ---------------------------------------------------------------------------------------------
struct HeadsBwdArgs {
  const float* pooled_f; const float* pooled_e; const float* weights; const float* raw_q;
  const float *g_w1, *g_b1, *g_w2, *g_b2;
  HeadW q[8];
  float* rows; size_t row_len;
  size_t o_g_w1, o_g_b1, o_g_w2, o_g_b2;            // offsets inside a row
  size_t o_q[8][6];                                 // ln_w, ln_b, w1, b1, w2, b2
  float scale;                                      // -(quality_weight/accum) / (B*4)
  const float* dq_up;                               // [B][4] upstream gradient of quality_scores (NULL: the constant `scale`)
  const float* dw_up;                               // [B][E] upstream gradient of expert_weights (NULL: none)
  int B, E, I, F;
  uint32_t thr; float inv_keep;                     // the forward's dropout (same call seed): gate and quality-head hidden layers
  LoDropSite ds_gate, ds_q[8];
  // full backward (lo_teacher_full_backward): the gradients that leave the heads towards the trunk, or null
  float* d_pool_f;                                  // [B][128]  d loss / d mean_hw(features)        (through the gate)
  float* d_pool_e;                                  // [E][B][F] d loss / d mean_hw(expert_e output) (through quality head e's LayerNorm)
};
__global__ __launch_bounds__(256) void lo_t_heads_bwd_kernel(HeadsBwdArgs a) {
  __shared__ float x[128], xh[T_FMAX], ln[T_FMAX], a1[256], h1[256], dz[8], dw[8], dq[8][4], dh[256], da[256], scratch[8], wts[8];
  const int tid = threadIdx.x, n = blockIdx.x, F = a.F;
  float* row = a.rows + (size_t)n * a.row_len;
  if (tid < a.E) wts[tid] = a.weights[n * a.E + tid];
  __syncthreads();
  // d loss / d weighted logits, d q_e, d w_e
  if (tid < 4) {
    float t = 0.f;
    for (int e = 0; e < a.E; ++e) t += a.raw_q[((size_t)n * a.E + e) * 4 + tid] * wts[e];
    float y = 1.f / (1.f + __expf(-t));
    float dwq = (a.dq_up ? a.dq_up[n * 4 + tid] : a.scale) * y * (1.f - y);
    for (int e = 0; e < a.E; ++e) dq[e][tid] = dwq * wts[e];
    scratch[tid] = dwq;
  }
  __syncthreads();
  if (tid < a.E) {
    float t = 0.f;
    for (int j = 0; j < 4; ++j) t += scratch[j] * a.raw_q[((size_t)n * a.E + tid) * 4 + j];
    dw[tid] = a.dw_up ? t + a.dw_up[n * a.E + tid] : t;
  }
  __syncthreads();
  if (tid < a.E) {
    float dot = 0.f;
    for (int k = 0; k < a.E; ++k) dot += wts[k] * dw[k];
    dz[tid] = wts[tid] * (dw[tid] - dot);
  }
  // ---- gate: x = pooled_f ; a1 = W1 x + b1 ; h1 = lrelu(a1) ; z = W2 h1 + b2
  if (tid < 128) x[tid] = a.pooled_f[n * 128 + tid];
  __syncthreads();
  for (int o = tid; o < a.I; o += 256) {
    float acc = a.g_b1[o];
    for (int i = 0; i < 128; ++i) acc += a.g_w1[o * 128 + i] * x[i];
    a1[o] = acc;
    h1[o] = acc > 0.f ? acc : 0.2f * acc;
  }
  __syncthreads();
  for (int i = tid; i < a.I; i += 256) {
    const float dm = !a.thr ? 1.f : (lo_drop_keep(a.ds_gate, (uint32_t)(n * a.I + i), a.thr) ? a.inv_keep : 0.f);   // d Dropout(h)/dh
    float t = 0.f;
    for (int e = 0; e < a.E; ++e) { t += a.g_w2[e * a.I + i] * dz[e]; row[a.o_g_w2 + (size_t)e * a.I + i] = dz[e] * (h1[i] * dm); }
    da[i] = t * dm * (a1[i] > 0.f ? 1.f : 0.2f);
    row[a.o_g_b1 + i] = da[i];
  }
  if (tid < a.E) row[a.o_g_b2 + tid] = dz[tid];
  __syncthreads();
  for (int idx = tid; idx < a.I * 128; idx += 256) row[a.o_g_w1 + idx] = da[idx >> 7] * x[idx & 127];
  if (a.d_pool_f && tid < 128) {
    float t = 0.f;
    for (int o = 0; o < a.I; ++o) t += a.g_w1[o * 128 + tid] * da[o];
    a.d_pool_f[n * 128 + tid] = t;
  }
  __syncthreads();
  // ---- quality heads
  const int H = a.I / 4;
  for (int e = 0; e < a.E; ++e) {
    const HeadW& hw = a.q[e];
    const float v0 = tid < F ? a.pooled_e[((size_t)e * a.B + n) * F + tid] : 0.f;
    const float v1 = tid + 256 < F ? a.pooled_e[((size_t)e * a.B + n) * F + tid + 256] : 0.f;
    float s = lo_wave_sum(v0 + v1);
    if ((tid & 63) == 0) scratch[tid >> 6] = s;
    __syncthreads();
    const float mean = (((scratch[0] + scratch[1]) + scratch[2]) + scratch[3]) / (float)F;
    __syncthreads();
    const float d0 = tid < F ? v0 - mean : 0.f, d1 = tid + 256 < F ? v1 - mean : 0.f;
    float qv = lo_wave_sum(d0 * d0 + d1 * d1);
    if ((tid & 63) == 0) scratch[tid >> 6] = qv;
    __syncthreads();
    const float rstd = 1.f / sqrtf((((scratch[0] + scratch[1]) + scratch[2]) + scratch[3]) / (float)F + LN_EPS);
    if (tid < F) { xh[tid] = d0 * rstd; ln[tid] = xh[tid] * hw.ln_w[tid] + hw.ln_b[tid]; }
    if (tid + 256 < F) { xh[tid + 256] = d1 * rstd; ln[tid + 256] = xh[tid + 256] * hw.ln_w[tid + 256] + hw.ln_b[tid + 256]; }
    __syncthreads();
    if (tid < H) {
      float acc = hw.b1[tid];
      for (int i = 0; i < F; ++i) acc += hw.w1[tid * F + i] * ln[i];
      a1[tid] = acc;
      h1[tid] = acc > 0.f ? acc : 0.2f * acc;
    }
    __syncthreads();
    if (tid < H) {
      const float dm = !a.thr ? 1.f : (lo_drop_keep(a.ds_q[e], (uint32_t)(n * H + tid), a.thr) ? a.inv_keep : 0.f);
      float t = 0.f;
      for (int j = 0; j < 4; ++j) { t += hw.w2[j * H + tid] * dq[e][j]; row[a.o_q[e][4] + (size_t)j * H + tid] = dq[e][j] * (h1[tid] * dm); }
      da[tid] = t * dm * (a1[tid] > 0.f ? 1.f : 0.2f);
      row[a.o_q[e][3] + tid] = da[tid];
    }
    if (tid < 4) row[a.o_q[e][5] + tid] = dq[e][tid];
    __syncthreads();
    for (int idx = tid; idx < H * F; idx += 256) row[a.o_q[e][2] + idx] = da[idx / F] * ln[idx % F];
    if (a.d_pool_e) __syncthreads();      // ln is reused below for d xhat
    float p1 = 0.f, p2 = 0.f;
    for (int c = tid; c < F; c += 256) {
      float t = 0.f;
      for (int i = 0; i < H; ++i) t += hw.w1[i * F + c] * da[i];
      row[a.o_q[e][0] + c] = t * xh[c];   // d LayerNorm weight
      row[a.o_q[e][1] + c] = t;           // d LayerNorm bias
      if (a.d_pool_e) { const float dxh = t * hw.ln_w[c]; ln[c] = dxh; p1 += dxh; p2 += dxh * xh[c]; }
    }
    __syncthreads();
    if (a.d_pool_e) {
      // LayerNorm backward towards the pooled features: d v = rstd * (d xhat - mean(d xhat) - xhat * mean(d xhat * xhat))
      p1 = lo_wave_sum(p1); p2 = lo_wave_sum(p2);
      if ((tid & 63) == 0) { scratch[tid >> 6] = p1; scratch[4 + (tid >> 6)] = p2; }
      __syncthreads();
      const float m1 = (((scratch[0] + scratch[1]) + scratch[2]) + scratch[3]) / (float)F;
      const float m2 = (((scratch[4] + scratch[5]) + scratch[6]) + scratch[7]) / (float)F;
      for (int c = tid; c < F; c += 256) a.d_pool_e[((size_t)e * a.B + n) * F + c] = rstd * (ln[c] - m1 - xh[c] * m2);
      __syncthreads();
    }
  }
}

// reward / baseline / advantage bookkeeping of _process_batch (train_hybrid.py:870-892) on the device.
//   state[0] = baseline, state[1] = 1 once initialised.  out[0..6] = quality_loss, semantic_reward, quality_reward,
//   baseline, advantage(mean), teacher_loss, mean(quality_scores);  adv_dev[0] = mean advantage (input of lo_vae_loss)
__global__ void lo_hybrid_reward_kernel(const float* __restrict__ quality, const float* __restrict__ semantic, int B,
                                        float semantic_weight, float reward_scale, float momentum, float quality_weight,
                                        float accum, float* __restrict__ state, float* __restrict__ out, float* __restrict__ adv_dev) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double sq = 0.0, ss = 0.0;
  for (int n = 0; n < B; ++n) {
    sq += ((double)quality[n * 4] + quality[n * 4 + 1] + quality[n * 4 + 2] + quality[n * 4 + 3]) * 0.25;
    ss += (double)semantic[n];
  }
  float quality_reward = (float)(sq / B), semantic_reward = (float)(ss / B);
  float total = quality_reward + semantic_weight * semantic_reward;
  float baseline = state[1] != 0.f ? momentum * state[0] + (1.f - momentum) * total : total;
  state[0] = baseline; state[1] = 1.f;
  float adv = (total - baseline) * reward_scale;
  out[0] = -quality_reward;            // quality_loss = -mean(quality_scores)
  out[1] = semantic_reward;
  out[2] = quality_reward;
  out[3] = baseline;
  out[4] = adv;
  out[5] = quality_weight * (-quality_reward) / accum;
  out[6] = quality_reward;
  adv_dev[0] = adv;
}

// The reward-gradient term of the hybrid step (-weight * mean(q_eval) / accum, q_eval = the EVAL-mode teacher's quality_scores on the
// reconstruction), behind lo_loss_finalize on the same stream: out2 = {term, mean(q_eval)}; losses[2] (vae_loss) += term;
// seed_c[0] = coefs[0] / loss_scale, the un-scaled multiplier of (recon - target) in d vae_loss / d recon (what the seeded image data
// gradient adds; lo_vae_backward(fused = 2) applies the loss scale to the whole seed)
__global__ void lo_reward_term_kernel(const float* __restrict__ q_eval, int B, float weight, float accum, float loss_scale,
                                      const float* __restrict__ coefs, float* __restrict__ losses, float* __restrict__ out2,
                                      float* __restrict__ seed_c) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double sq = 0.0;
  for (int n = 0; n < B; ++n) sq += ((double)q_eval[n * 4] + q_eval[n * 4 + 1] + q_eval[n * 4 + 2] + q_eval[n * 4 + 3]) * 0.25;
  const float q_mean = (float)(sq / B);
  const float term = -weight * q_mean / accum;
  out2[0] = term;
  out2[1] = q_mean;
  losses[2] += term;
  seed_c[0] = coefs[0] / loss_scale;
}
int lo_reward_term(const float* q_eval, int B, float weight, float accum, float loss_scale, const float* coefs, float* losses, float* out2,
                   float* seed_c, hipStream_t st) {
  LO_REQUIRE(q_eval && coefs && losses && out2 && seed_c && B > 0 && accum > 0.f && loss_scale > 0.f, "lo_reward_term: bad argument");
  hipLaunchKernelGGL(lo_reward_term_kernel, dim3(1), dim3(64), 0, st, q_eval, B, weight, accum, loss_scale, coefs, losses, out2, seed_c);
  LO_LAUNCH_CHECK("reward_term");
  return LO_OK;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static HeadW t_headw(const float* P, const THeadOff& o) { return HeadW{TP(o.ln_w), TP(o.ln_b), TP(o.w1), TP(o.b1), TP(o.w2), TP(o.b2)}; }

// gate, quality heads, weighted scores, style / prompt / semantic heads from the pooled features the trunk left in the workspace
// (o_pool_f, o_pool_e): lunar_evaluator.py:417, 425, 431-449
int t_run_heads(LoTeacher* h, float* P, void* ws, float* quality, float* weights, float* style, float* prompt, float* semantic,
                const LoDropCfg& d, hipStream_t st) {
  const int B = h->B;
  const THeadsOff& o = h->heads;
  HeadsArgs a;
  memset(&a, 0, sizeof(a));
  a.pooled_f = TW(float, h->o_pool_f); a.pooled_e = TW(float, h->o_pool_e);
  a.g_w1 = TP(o.g_w1); a.g_b1 = TP(o.g_b1); a.g_w2 = TP(o.g_w2); a.g_b2 = TP(o.g_b2);
  for (int e = 0; e < h->E; ++e) a.q[e] = t_headw(P, o.q[e]);
  a.sem = t_headw(P, o.sem); a.style = t_headw(P, o.style); a.prompt = t_headw(P, o.prompt);
  a.quality = quality; a.weights = weights; a.style_out = style; a.prompt_out = prompt; a.sem_out = semantic;
  a.raw_q = TW(float, h->o_rawq);
  a.B = B; a.E = h->E; a.I = h->I; a.emb = h->emb; a.F = h->F;
  a.thr = d.thr; a.inv_keep = d.inv_keep;
  a.ds_gate = d.site(LO_DS_GATE); a.ds_sem = d.site(LO_DS_SEM); a.ds_style = d.site(LO_DS_STYLE); a.ds_prompt = d.site(LO_DS_PROMPT);
  for (int e = 0; e < h->E; ++e) a.ds_q[e] = d.site(LO_DS_QUALITY(e));
  {
    LoProfScope _p("lo_t_heads", 0, 0, st);
    hipLaunchKernelGGL(lo_t_heads_kernel, dim3(B), dim3(256), 0, st, a);
  }
  LO_LAUNCH_CHECK("t_heads");
  return LO_OK;
}

// ---- A13 + reward bookkeeping entry points --------------------------------------------------------------------------
extern "C" int lo_teacher_grad_range(const LoTeacher* h, size_t* begin, size_t* end) {
  LO_REQUIRE(h && begin && end, "lo_teacher_grad_range: null argument");
  *begin = h->heads.g_w1;          // gate.2.weight
  *end = h->heads.sem.ln_w;        // semantic_head.2.weight
  return LO_OK;
}
// rows: B * (end - begin) floats of scratch.  grads: flat gradient buffer of the teacher state layout (only [begin,end) is
// written).  The general form takes the upstream gradients of quality_scores [B][4] / expert_weights [B][E] (either may be
// NULL) and the head inputs of the forward call it differentiates (pooled features, pre-weighting logits, dropout stream), so
// that it may follow any number of later forward calls; lo_teacher_heads_saved says where lo_teacher_forward leaves them.
extern "C" int lo_teacher_heads_saved(const LoTeacher* h, size_t* byte_offsets3, size_t* elems3) {
  LO_REQUIRE(h && byte_offsets3 && elems3, "lo_teacher_heads_saved: null argument");
  byte_offsets3[0] = h->o_pool_f; elems3[0] = (size_t)h->B * 128;
  byte_offsets3[1] = h->o_pool_e; elems3[1] = (size_t)h->E * h->B * h->F;
  byte_offsets3[2] = h->o_rawq;   elems3[2] = (size_t)h->B * h->E * 4;
  return LO_OK;
}
int t_heads_backward(LoTeacher* h, const float* P, const float* pooled_f, const float* pooled_e, const float* raw_q,
                     const float* expert_weights, const float* dq_up, const float* dw_up, float coef, const LoDropCfg& d, float* rows,
                     float* grads, hipStream_t st, float* d_pool_f, float* d_pool_e) {
  size_t b0, b1;
  LO_TRYT(lo_teacher_grad_range(h, &b0, &b1));
  const THeadsOff& o = h->heads;
  HeadsBwdArgs a;
  memset(&a, 0, sizeof(a));
  a.pooled_f = pooled_f; a.pooled_e = pooled_e; a.weights = expert_weights; a.raw_q = raw_q;
  a.g_w1 = TP(o.g_w1); a.g_b1 = TP(o.g_b1); a.g_w2 = TP(o.g_w2); a.g_b2 = TP(o.g_b2);
  a.o_g_w1 = o.g_w1 - b0; a.o_g_b1 = o.g_b1 - b0; a.o_g_w2 = o.g_w2 - b0; a.o_g_b2 = o.g_b2 - b0;
  for (int e = 0; e < h->E; ++e) {
    const THeadOff& q = o.q[e];
    a.q[e] = t_headw(P, q);
    const size_t oq[6] = {q.ln_w, q.ln_b, q.w1, q.b1, q.w2, q.b2};
    for (int k = 0; k < 6; ++k) a.o_q[e][k] = oq[k] - b0;
  }
  a.rows = rows; a.row_len = b1 - b0;
  a.scale = -coef / ((float)h->B * 4.f);
  a.dq_up = dq_up; a.dw_up = dw_up;
  a.d_pool_f = d_pool_f; a.d_pool_e = d_pool_e;
  a.B = h->B; a.E = h->E; a.I = h->I; a.F = h->F;
  a.thr = d.thr; a.inv_keep = d.inv_keep;
  a.ds_gate = d.site(LO_DS_GATE);
  for (int e = 0; e < h->E; ++e) a.ds_q[e] = d.site(LO_DS_QUALITY(e));
  // grads null (the eval backward for the images' gradient alone): the per-sample rows are scratch and only d_pool_* is the result
  if (grads) LO_HIP(hipMemsetAsync(rows, 0, (size_t)h->B * a.row_len * sizeof(float), st));   // alignment padding inside the rows
  hipLaunchKernelGGL(lo_t_heads_bwd_kernel, dim3(h->B), dim3(256), 0, st, a);
  LO_LAUNCH_CHECK("t_heads_bwd");
  if (!grads) return LO_OK;
  return lo_colsum(rows, grads + b0, h->B, (int)a.row_len, (int)a.row_len, 1.0f, st);
}
// coef = quality_weight / accum.  Must follow lo_teacher_forward on the evaluated batch (uses its pooled features and masks).
extern "C" int lo_teacher_heads_backward(LoTeacher* h, const float* P, void* ws, const float* expert_weights, float coef,
                                         float* rows, float* grads, void* stream) {
  LO_REQUIRE(h && P && ws && expert_weights && rows && grads, "lo_teacher_heads_backward: null argument");
  return t_heads_backward(h, P, TW(float, h->o_pool_f), TW(float, h->o_pool_e), TW(float, h->o_rawq), expert_weights, nullptr, nullptr,
                          coef, lo_drop_cfg(h->last_p, h->last_seed), rows, grads, reinterpret_cast<hipStream_t>(stream));
}
extern "C" int lo_teacher_heads_backward_ex(LoTeacher* h, const float* P, const float* pooled_f, const float* pooled_e, const float* raw_q,
                                            const float* expert_weights, const float* d_quality, const float* d_weights, float dropout_p,
                                            uint64_t drop_seed, float* rows, float* grads, void* stream) {
  LO_REQUIRE(h && P && pooled_f && pooled_e && raw_q && expert_weights && rows && grads && (d_quality || d_weights),
             "lo_teacher_heads_backward_ex: null argument");
  // a NULL d_quality means "no gradient arrives through quality_scores": coef 0 makes the constant seed vanish
  return t_heads_backward(h, P, pooled_f, pooled_e, raw_q, expert_weights, d_quality, d_weights, 0.f, lo_drop_cfg(dropout_p, drop_seed), rows,
                          grads, reinterpret_cast<hipStream_t>(stream));
}
extern "C" int lo_hybrid_reward(const float* quality, const float* semantic, int B, float semantic_weight, float reward_scale,
                                float momentum, float quality_weight, float accum, float* state2, float* out7, float* adv_dev,
                                void* stream) {
  LO_REQUIRE(quality && semantic && state2 && out7 && adv_dev && B > 0, "lo_hybrid_reward: bad argument");
  hipLaunchKernelGGL(lo_hybrid_reward_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), quality, semantic, B,
                     semantic_weight, reward_scale, momentum, quality_weight, accum, state2, out7, adv_dev);
  LO_LAUNCH_CHECK("hybrid_reward");
  return LO_OK;
}
