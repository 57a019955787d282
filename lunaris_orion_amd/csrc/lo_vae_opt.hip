// VAE step executor: operand refresh (weight packs, fp16 / e4m3 / transposed copies) and the pipelined optimizer step.
#include "lo_vae.h"

// (re)build the job tables of the fused pack launches and upload them into the workspace (once per workspace / parameter buffer)
static int vae_ensure_pack_jobs(LoVae* h, const float* P, void* ws, hipStream_t st) {
  if (h->packjobs_for_ws == ws && h->packjobs_for_params == (const void*)P) return LO_OK;
  std::vector<LoPackJob>& jobs = h->packjobs_host;
  std::vector<LoPackF8Job>& j8 = h->packjobs8_host;
  jobs.clear();
  j8.clear();
  int blocks = 0, blocks8 = 0;
  auto add = [&](ConvLayer& c, const LoGeom& g, size_t o_dst) {
    LoPackJob j;
    j.src = PRM(c.p_w); j.dst = WSP(f16, o_dst); j.total = (int)lo_packed_weight_elems(g); j.block0 = blocks; j.g = g;
    blocks += lo_pack_blocks(g);
    jobs.push_back(j);
  };
  for_each_layer(h, [&](ConvLayer& c) {
    if (&c == &h->enc[3][0]) {   // "early" share: encoder stages 1..3
      h->n_packjobs_enc = (int)jobs.size(); h->pack_blocks_enc = blocks;
      h->n_packjobs8_enc = (int)j8.size(); h->pack_blocks8_enc = blocks8;
    }
    if (&c == &h->dec[0]) {      // the table's prefix up to and including encoder stage 4
      h->n_packjobs_s4 = (int)jobs.size(); h->pack_blocks_s4 = blocks;
      h->n_packjobs8_s4 = (int)j8.size(); h->pack_blocks8_s4 = blocks8;
    }
    if (&c == &h->enc[0][0]) return;      // the first conv reads its fp32 weights
    add(c, c.gf, c.o_wp_f);
    add(c, c.gd, c.o_wp_d);
    if (!c.f8) return;
    LoPackF8Job j;
    lo_pack_f8_job(&j, c.gf, WSP(f16, c.o_wp_f), WSP(uint8_t, c.o_wp8), WSP(float, c.o_wscale), blocks8);
    blocks8 += c.gf.n_phase * c.Cout;
    j8.push_back(j);
  });
  LO_REQUIRE(jobs.size() <= 64, "too many pack jobs");
  LO_REQUIRE(j8.size() <= 32, "too many fp8 pack jobs");
  LO_HIP(hipMemcpyAsync(WSP(void, h->o_packjobs), jobs.data(), jobs.size() * sizeof(LoPackJob), hipMemcpyHostToDevice, st));
  if (!j8.empty())
    LO_HIP(hipMemcpyAsync(WSP(void, h->o_packjobs8), j8.data(), j8.size() * sizeof(LoPackF8Job), hipMemcpyHostToDevice, st));
  h->n_packjobs = (int)jobs.size(); h->pack_blocks = blocks;
  h->n_packjobs8 = (int)j8.size(); h->pack_blocks8 = blocks8;
  h->packjobs_for_ws = ws;
  h->packjobs_for_params = (const void*)P;
  return LO_OK;
}

// side-stream bookkeeping: one event per operand-refresh level (see LoVae::ev_lvl)
static int vae_side_record(LoVae* h, int lvl, hipStream_t on) {
  LO_HIP(hipEventRecord(h->ev_lvl[lvl], on));
  h->lvl_pending[lvl] = true;
  return LO_OK;
}

// The transposed fp16 copies of the two Linear weights (operands of their data gradients), made from the fp16 forward copies that
// the same stream has just refreshed: 4 bytes of traffic per element instead of the 6 of a transposing cast from fp32, and the
// same bits.  2L and 32768 are multiples of 64 (lo_vae_create_ex).
static int vae_linear_transposes(LoVae* h, void* ws, hipStream_t st) {
  const int L = h->L;
  LO_TRY(lo_nhwc_to_nchw_f16(WSP(f16, h->o_wp_head), WSP(f16, h->o_wp_head_t), 1, 2 * L, 32768, st));   // [2L][32768] -> [32768][2L]
  return lo_nhwc_to_nchw_f16(WSP(f16, h->o_wp_dfc), WSP(f16, h->o_wp_dfc_t), 1, 32768, L, st);          // [32768][L] -> [L][32768]
}

// Operands of the attention sites (LO_VAE_ATTN): the fp16 copy of a site's [640][512] matrix (q | k | v rows, contiguous in the flat
// buffer) belongs to the level the forward waits for before the site -- 2 for the encoder's, 4 for the decoder's -- and the transposed
// copies, which only the backward reads, to level 5
static int vae_attn_cast(LoVae* h, int site, const float* P, void* ws, hipStream_t st) {
  if (!h->attn) return LO_OK;
  return lo_cast_f32_f16(PRM(h->att[site].p_w), WSP(f16, h->att[site].o_w), (size_t)640 * 512, st);
}
static int vae_attn_transposes(LoVae* h, void* ws, hipStream_t st) {
  if (!h->attn) return LO_OK;
  for (const LoAttnSite& a : h->att) LO_TRY(lo_nhwc_to_nchw_f16(WSP(f16, a.o_w), WSP(f16, a.o_wt), 1, 640, 512, st));   // [640][512] -> [512][640]
  return LO_OK;
}

// Where the two big Linear weights sit in the flat buffer (fc_mu | fc_logvar: nh elements from bh; decoder.fc: nd elements from bd;
// 82 % of the parameters), and the table the factored AdamW pass (lo_adamw_lowrank) takes for them.  casts: that pass also writes
// the fp16 forward operands and their transposed copies.
struct LoLinearRanges { size_t bh, nh, bd, nd; LoLowrankMat lrm[2]; };
static LoLinearRanges vae_linear_ranges(const LoVae* h, float* P, float* M, float* V, void* ws, bool casts) {
  const int L = h->L;
  const size_t bh = h->p_off[h->idx_fc_mu_w], bd = h->p_off[h->idx_dfc_w];
  auto copy = [&](size_t off) -> f16* { return casts ? WSP(f16, off) : nullptr; };
  // mode 3: the factors of rank 0's block of the gathered buffer (the blocks keep the workspace's layout; rank stride = block size)
  auto fac = [&](size_t off) -> const f16* { return vae_factors_gathered(h) ? vae_fac_in_block(h, h->fac.gathered, off) : WSP(f16, off); };
  return {bh, (size_t)2 * L * 32768, bd, (size_t)32768 * L,
          {{P + bh, M + bh, V + bh, copy(h->o_wp_head), copy(h->o_wp_head_t), fac(h->o_fac_xT), fac(h->o_fac_dmlT), 2 * L, 32768},
           {P + bd, M + bd, V + bd, copy(h->o_wp_dfc), copy(h->o_wp_dfc_t), fac(h->o_fac_zT), fac(h->o_fac_gfcT), 32768, L}}};
}
// AdamW of the two matrices from their factors: this rank's (mode 1) or the `fac.world` gathered blocks, 1 / world folded into the scale
static int vae_adamw_linear(const LoVae* h, const LoLinearRanges& r, const LoAdamHyper& hp, hipStream_t st) {
  if (!vae_factors_gathered(h)) return lo_adamw_lowrank(r.lrm, 2, h->B, h->fac.scale, hp, st);
  return lo_adamw_lowrank_gathered(r.lrm, 2, vae_fac_block_elems(h), h->fac.world, h->B, vae_gathered_scale(h, h->fac.world), hp, st);
}

// Levels 2..5 of a pipelined optimizer step: AdamW of everything from the encoder's last stage on, in the order the forward needs
// the results, each chunk followed by the operand refresh that depends on it.  after_main != null: the side stream first waits
// for what `after_main` has enqueued so far (the forward calls this once its first stage has been issued, so that the 1.5 GB of
// AdamW traffic runs beside the later, MFMA- and L2-bound stages instead of beside the HBM-bound first one).
int vae_flush_deferred(LoVae* h, hipStream_t after_main) {
  if (!h->defer.pending) return LO_OK;
  h->defer.pending = false;
  const auto& d = h->defer;
  float* P = d.P; const float* G = d.G; float* M = d.M; float* V = d.V; void* ws = d.ws;
  hipStream_t sd = h->side;
  if (after_main) LO_TRY(vae_order(sd, after_main, h->ev_pre));
  const LoLinearRanges r = vae_linear_ranges(h, P, M, V, ws, true);
  const size_t n = h->flat_elems, b4 = h->p_off[h->enc[3][0].p_w], bh = r.bh, nh = r.nh, bd = r.bd, nd = r.nd;
  const LoPackJob* jobs = WSP(LoPackJob, h->o_packjobs);
  const LoPackF8Job* jobs8 = WSP(LoPackF8Job, h->o_packjobs8);
  auto adam = [&](size_t lo, size_t hi, f16* cast = nullptr) {
    return hi > lo ? lo_adamw(P + lo, G + lo, M + lo, V + lo, hi - lo, d.hp, sd, cast) : LO_OK;
  };
  // level 2: encoder stage 4 (10 % of the parameters): first consumer ~0.45 ms into the forward
  LO_TRY(adam(b4, bh));
  LO_TRY(vae_attn_cast(h, 0, P, ws, sd));
  LO_TRY(lo_pack_all(jobs + h->n_packjobs_enc, h->n_packjobs_s4 - h->n_packjobs_enc, h->pack_blocks_s4 - h->pack_blocks_enc, sd, h->pack_blocks_enc));
  if (h->fp8_fwd)
    LO_TRY(lo_pack_f8_all(jobs8 + h->n_packjobs8_enc, h->n_packjobs8_s4 - h->n_packjobs8_enc, h->pack_blocks8_s4 - h->pack_blocks8_enc, sd, h->pack_blocks8_enc));
  LO_TRY(vae_side_record(h, 2, sd));
  // level 3: fc_mu / fc_logvar (weights + biases are adjacent: [bh, bd)) and their fp16 copy, which comes out of the AdamW pass itself
  // (factored: the transposed fp16 copies [32768][2L] / [L][32768] -- operands of the two Linear data gradients -- leave the same
  // pass: +0.6 % on the step against the separate transposes, 25 002 / 25 077 / 24 998 vs 24 720 / 25 047 / 24 867)
  // Factored: both matrices (fc_mu | fc_logvar and decoder.fc) in one launch: the forward needs neither before the end of the
  // encoder, ~1 ms away, and one launch has one ramp and one tail
  if (vae_opt_from_factors(h)) LO_TRY(vae_adamw_linear(h, r, d.hp, sd));
  else LO_TRY(adam(bh, bh + nh, WSP(f16, h->o_wp_head)));
  LO_TRY(adam(bh + nh, bd));
  LO_TRY(vae_side_record(h, 3, sd));
  // level 4: decoder.fc (unless it went with the encoder heads), the decoder and final convs
  if (!vae_opt_from_factors(h)) LO_TRY(adam(bd, bd + nd, WSP(f16, h->o_wp_dfc)));
  LO_TRY(adam(bd + nd, n));
  LO_TRY(vae_attn_cast(h, 1, P, ws, sd));
  LO_TRY(lo_pack_all(jobs + h->n_packjobs_s4, h->n_packjobs - h->n_packjobs_s4, h->pack_blocks - h->pack_blocks_s4, sd, h->pack_blocks_s4));
  if (h->fp8_fwd)
    LO_TRY(lo_pack_f8_all(jobs8 + h->n_packjobs8_s4, h->n_packjobs8 - h->n_packjobs8_s4, h->pack_blocks8 - h->pack_blocks8_s4, sd, h->pack_blocks8_s4));
  LO_TRY(vae_side_record(h, 4, sd));
  // level 5: the transposed copies (data gradients of the Linear layers: backward only); the factored AdamW pass has written them
  if (!vae_opt_from_factors(h)) LO_TRY(vae_linear_transposes(h, ws, sd));
  LO_TRY(vae_attn_transposes(h, ws, sd));
  return vae_side_record(h, 5, sd);
}

// `st` waits for operand-refresh level `lvl` (and with it every lower one); a deferred optimizer tail is enqueued first
int vae_wait_level(LoVae* h, hipStream_t st, int lvl) {
  if (lvl >= 2) LO_TRY(vae_flush_deferred(h, nullptr));
  for (int l = lvl; l >= 1; --l)
    if (h->lvl_pending[l]) {
      LO_HIP(hipStreamWaitEvent(st, h->ev_lvl[l], 0));      // the highest pending level <= lvl: same stream, recorded in order
      for (int k = 1; k <= l; ++k) h->lvl_pending[k] = false;
      break;
    }
  return LO_OK;
}

extern "C" int lo_vae_pack(LoVae* h, const float* P, void* ws, void* stream) {
  LO_REQUIRE(h && P && ws, "lo_vae_pack: null argument");
  hipStream_t st = S(stream);
  LO_TRY(vae_flush_deferred(h, nullptr));     // an optimizer tail still to be enqueued writes the parameters this pack reads
  LO_TRY(vae_ensure_pack_jobs(h, P, ws, st));
  // Nothing here is needed at once -- the first conv of the encoder reads the fp32 weights directly, the four Linear-layer copies
  // (0.15 ms at L=512) are not needed before the end of the encoder -- so with a side stream everything is refreshed there while the
  // encoder forward starts; the consumers wait on the level events (vae_wait_level)
  hipStream_t cs = st;
  if (vae_side_on(h)) {
    if (h->lvl_pending[5]) LO_HIP(hipStreamWaitEvent(st, h->ev_lvl[5], 0));   // order after an optimizer tail already running
    cs = h->side;
    LO_TRY(vae_order(cs, st, h->ev_pre));
  }
  LO_TRY(lo_pack_all(WSP(LoPackJob, h->o_packjobs), h->n_packjobs, h->pack_blocks, cs));
  if (h->fp8_fwd) LO_TRY(lo_pack_f8_all(WSP(LoPackF8Job, h->o_packjobs8), h->n_packjobs8, h->pack_blocks8, cs));
  LO_TRY(vae_attn_cast(h, 0, P, ws, cs));
  if (cs != st) { LO_TRY(vae_side_record(h, 1, cs)); LO_TRY(vae_side_record(h, 2, cs)); }
  const int L = h->L;
  // encoder head: [fc_mu.weight ; fc_logvar.weight] is one contiguous [2L][32768] fp32 matrix in the flat buffer
  LO_REQUIRE(h->p_off[h->idx_fc_lv_w] == h->p_off[h->idx_fc_mu_w] + (size_t)L * 32768, "flat layout: head weights not adjacent");
  LO_TRY(lo_cast_f32_f16(PRM(h->idx_fc_mu_w), WSP(f16, h->o_wp_head), (size_t)2 * L * 32768, cs));
  LO_TRY(lo_cast_f32_f16(PRM(h->idx_dfc_w), WSP(f16, h->o_wp_dfc), (size_t)32768 * L, cs));
  LO_TRY(vae_attn_cast(h, 1, P, ws, cs));
  if (cs != st) { LO_TRY(vae_side_record(h, 3, cs)); LO_TRY(vae_side_record(h, 4, cs)); }
  LO_TRY(vae_linear_transposes(h, ws, cs));
  LO_TRY(vae_attn_transposes(h, ws, cs));
  if (cs != st) LO_TRY(vae_side_record(h, 5, cs));
  return LO_OK;
}

// ---------------------------------------------------------------------------------------------
// Pipelined optimizer step: clip + AdamW + operand refresh, ordered so that the NEXT forward starts after 3 % of the update and
// the rest runs beside it where it hurts least.
//   stream:  gradient norm -> AdamW [0, b4)          (b4 = offset of the encoder's last stage: stages 1..3 hold 3 % of the bytes)
//   side  :  pack encoder stages 1..3 (level 1) -> AdamW stage 4 + its packs (level 2) -> AdamW fc_mu|fc_logvar + fp16 copy (3)
//            -> AdamW decoder.fc / decoder + copy + packs (4) -> transposed copies (5).  The forward waits for level 2 before
//            encoder stage 4, 3 before the heads, 4 before the decoder; the backward for level 5.
// Until level 4 has completed, parameters [b4, n) and their Adam moments are in flight on the side stream: lo_vae_join orders
// another stream (e.g. before the caller reads the parameters itself).  Without the side stream everything runs in order on
// `stream`.  presummed != 0: scratch[512..1024) already holds the sum of squares of [b, n) (lo_vae_set_gradnorm_scratch).
// ---------------------------------------------------------------------------------------------
extern "C" int lo_vae_optimizer_step(LoVae* h, float* P, const float* G, float* M, float* V, void* ws, float max_norm, float lr,
                                     float beta1, float beta2, float eps, float weight_decay, int step, float* scratch, int flags,
                                     void* stream) {
  LO_REQUIRE(h && P && G && M && V && ws && scratch, "lo_vae_optimizer_step: null argument");
  LO_REQUIRE((flags & ~(LO_OPT_PRESUMMED | LO_OPT_SERIAL)) == 0, "lo_vae_optimizer_step: unknown flag bits 0x%x", flags);
  const int presummed = flags & LO_OPT_PRESUMMED;
  const bool serial = (flags & LO_OPT_SERIAL) != 0;
  // a fused-GroupNorm rendezvous of this step's launches that ran out left garbage in the gradients: the clip kernel reads the word
  // and skips the update on the device, like a non-finite norm (ADVICE r3 / VERDICT r3 item 1b)
  const unsigned int* fail = WSP(unsigned int, h->o_sync_fail);
  hipStream_t st = S(stream);
  if (vae_opt_from_factors(h)) {
    if (!h->fac.ready || !presummed) {
      lo_set_error("lo_vae_optimizer_step: the factored Linear-gradient mode needs a fused lo_vae_backward (with the gradient-norm scratch set; "
                   "mode 3: lo_vae_backward_phase and lo_vae_gathered_early_norm) before every step, and LO_OPT_PRESUMMED");
      return LO_ERR_STATE;
    }
    h->fac.ready = false;
  }
  LO_TRY(vae_flush_deferred(h, nullptr));     // two optimizer steps without a forward in between
  // b: begin of the range whose sum of squares may be presummed (fc_mu.weight);  b4: begin of the encoder's last stage -- the
  // stream itself only updates stages 1..3 (3 % of the parameters, what the next forward reads in its first 0.45 ms)
  const size_t n = h->flat_elems, b = h->p_off[h->idx_fc_mu_w], b4 = h->p_off[h->enc[3][0].p_w];
  LO_TRY(vae_ensure_pack_jobs(h, P, ws, st));
  if (presummed) LO_TRY(lo_gradnorm_split(G, b, max_norm, scratch, scratch + 1024, st, fail));
  else LO_TRY(lo_gradnorm(G, n, max_norm, scratch, scratch + 1024, st, fail));
  const LoAdamHyper hp = {scratch + 1024, lr, beta1, beta2, eps, weight_decay, step};
  h->opt_tail_on_side = !serial && vae_side_on(h);
  if (!h->opt_tail_on_side) {
    auto adam = [&](size_t lo, size_t hi) { return lo_adamw(P + lo, G + lo, M + lo, V + lo, hi - lo, hp, st); };
    if (vae_opt_from_factors(h)) {
      const LoLinearRanges r = vae_linear_ranges(h, P, M, V, ws, false);      // no copies: lo_vae_pack below makes them
      LO_TRY(adam(0, r.bh));
      LO_TRY(vae_adamw_linear(h, r, hp, st));
      LO_TRY(adam(r.bh + r.nh, r.bd));
      LO_TRY(adam(r.bd + r.nd, n));
    } else {
      LO_TRY(adam(0, n));
    }
    return lo_vae_pack(h, P, ws, stream);
  }
  {
    LoHandover ho(h->ev_pre, true);      // the hand-over event rides on the AdamW launch (LO_LAUNCH_STOP)
    LO_TRY(lo_adamw(P, G, M, V, b4, hp, st));
    LO_TRY(ho.finish(st));
  }
  hipStream_t sd = h->side;
  LO_HIP(hipStreamWaitEvent(sd, h->ev_pre, 0));
  LO_TRY(lo_pack_all(WSP(LoPackJob, h->o_packjobs), h->n_packjobs_enc, h->pack_blocks_enc, sd));
  if (h->fp8_fwd) LO_TRY(lo_pack_f8_all(WSP(LoPackF8Job, h->o_packjobs8), h->n_packjobs8_enc, h->pack_blocks8_enc, sd));
  LO_TRY(vae_side_record(h, 1, sd));
  h->defer = {true, P, G, M, V, ws, hp};
  // (deferring this tail behind the next forward's first stage was measured in round 2: no difference -- where the AdamW traffic
  // lands only changes WHICH kernels it slows down, not the sum -- so it is enqueued at once)
  LO_TRY(vae_flush_deferred(h, nullptr));
  return LO_OK;
}
// EMA of the flat parameters behind an optimizer step: ema[0, n) <- ema + (P - ema)(1 - decay), gated like the step's AdamW launches.
// Ordering.  Pipelined step (side stream on): AdamW wrote [0, b4) on `stream` and writes [b4, n) on h->side, possibly still deferred.  The
// pass is enqueued on h->side behind the flushed tail: that stream is in order, so it follows the AdamW of [b4, n), and it waited on
// ev_pre -- bound to the AdamW launch of [0, b4), which itself follows the clip kernel that writes the gate -- before its first launch
// of the step.  Level 5 is then recorded again behind the pass: lo_vae_join and the next backward (vae_wait_level(.., 5)) wait for
// it, and the next write of any parameter -- the next step's AdamW, on `stream` behind that backward, then on the side stream behind
// this pass -- is ordered behind its read.  Levels 2..4 keep their events, so the next forward waits for no more than before and the
// 12 B / parameter run beside it.  Serial step or no side stream: everything the step enqueued is on `stream`, and so is the pass
// (what lo_vae_pack left on the side stream only reads the parameters, like the pass).
extern "C" int lo_vae_ema_update(LoVae* h, const float* P, float* ema, float one_minus_decay, const float* scratch, void* stream) {
  LO_REQUIRE(h && P && ema, "lo_vae_ema_update: null argument");
  const float* gate = scratch ? scratch + 1024 : nullptr;
  if (!(h->opt_tail_on_side && vae_side_on(h))) return lo_ema_run(ema, P, h->flat_elems, one_minus_decay, gate, S(stream));
  LO_TRY(vae_flush_deferred(h, nullptr));
  LO_TRY(lo_ema_run(ema, P, h->flat_elems, one_minus_decay, gate, h->side));
  return vae_side_record(h, 5, h->side);
}

// `stream` waits for whatever lo_vae_pack / lo_vae_optimizer_step left running (or still to be enqueued) on the side stream.
extern "C" int lo_vae_join(LoVae* h, void* stream) {
  LO_REQUIRE(h, "lo_vae_join: null handle");
  hipStream_t st = S(stream);
  LO_TRY(vae_flush_deferred(h, nullptr));
  for (int l = 5; l >= 1; --l)
    if (h->lvl_pending[l]) { LO_HIP(hipStreamWaitEvent(st, h->ev_lvl[l], 0)); break; }
  // the flags stay set: the executor's own stream may be a different one and still has to wait
  return LO_OK;
}

// The Linear-layer weight gradients of the last fused backward written out after all (tests, tools, anybody who reads
// parameter_grads() in the factored mode): the same MFMA tiles the AdamW pass forms, stored to flat_grads instead.  `stream` must be
// ordered behind that backward (it is, for the stream the backward ran on).
extern "C" int lo_vae_materialize_linear_grads(LoVae* h, void* ws, float* G, void* stream) {
  LO_REQUIRE(h && ws && G, "lo_vae_materialize_linear_grads: null argument");
  if (!vae_opt_from_factors(h)) return LO_OK;   // the backward (mode 2: the exchange) wrote them itself
  // mode 1: this rank's factor block in the workspace, alone; mode 3: the gathered blocks the last norm call was given
  const bool gathered = vae_factors_gathered(h);
  if (gathered && !h->fac.gathered) { lo_set_error("lo_vae_materialize_linear_grads: mode 3 has not seen lo_vae_gathered_early_norm yet"); return LO_ERR_STATE; }
  return lo_vae_materialize_gathered_linear_grads(h, gathered ? h->fac.gathered : WSP(f16, h->o_fac_dmlT), gathered ? h->fac.world : 1, G, stream);
}
