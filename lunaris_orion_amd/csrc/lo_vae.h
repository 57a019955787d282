// Private header of the native VAE step executor: one C call enqueues every kernel of LunarisCoreVAE.forward
// (lunar_generate.py:263-276) or of its backward on the given HIP stream.
//   lo_vae_plan.hip  workspace plan, create / destroy, queries
//   lo_vae_opt.hip   operand refresh (packs, casts) and the pipelined optimizer step
//   lo_vae_step.hip  forward, loss, backward
// What it launches: the convolution family (lo_conv.h), the GroupNorm family (lo_norm.h), the rest (lo_internal.h).
#pragma once
#include "lo_internal.h"
#include "lo_conv.h"
#include "lo_norm.h"
#include "../../include/lunaris_hip.h"
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <vector>

// workspace / flat parameter / flat gradient addressing: expect `ws`, `P`, `G` and `h` in scope
#define WSP(T, off) reinterpret_cast<T*>(reinterpret_cast<unsigned char*>(ws) + (off))
#define PRM(i) (P + h->p_off[(i)])
#define GRD(i) (G + h->p_off[(i)])

struct ConvLayer {           // conv + GroupNorm + Mish
  int kind = 0;              // forward kind
  int H = 0, W = 0, Cin = 0, Cout = 0;   // input spatial dims / channels
  int Ho = 0, Wo = 0;        // output spatial dims
  LoGeom gf{}, gd{};         // forward / data-gradient geometry
  int p_w = 0, p_b = 0, p_gw = 0, p_gb = 0;   // parameter indices (state_dict order)
  size_t o_wp_f = 0, o_wp_d = 0;   // workspace offsets: packed fp16 weights (fwd, dgrad)
  size_t o_v = 0, o_a = 0;   // raw conv output, activation after GN+Mish(+...)
  size_t o_part = 0, o_stats = 0;   // GN partial sums, saved stats
  size_t o_P1 = 0, o_P2 = 0; // GN backward partial sums (kept until the fused finalize at the end of backward)
  // rows of P1 / P2 per sample: what the buffers hold (setup_conv_layer) and what this backward has left in them so far (0 = nothing
  // yet; written by vae_record_rows alone, reset by VaeBackward::begin, summed by vae_gn_finalize)
  int prow_cap = 0, np1 = 0, np2 = 0;
  int gnb_ran = -2;          // how this backward ran the layer's GroupNorm backward: LoGnBwdForm; -1: the consuming layer's data gradient
                             // applied it in its epilogue; -2: not yet
  int MT = 0;
  size_t o_dv = 0;           // gradient wrt the raw conv output (GroupNorm backward -> data / weight gradient); one per layer, so the
                             // side-stream weight gradient of layer k never shares a buffer with what the main stream writes next
  // fp8 operand mode (LO_VAE_FP8_FWD): e4m3 weights + per-row scales of the forward op, e4m3 copy of the activation o_a
  bool f8 = false;           // this layer's forward conv runs on e4m3 operands
  size_t o_wp8 = 0, o_wscale = 0, o_a8 = 0;   // o_a8 = 0: no consumer needs the copy
  // GroupNorm + Mish fused into the forward conv's epilogue (LoGnFuse, lo_common.h): exchange lines, arrival counters, and how many
  // launches have used them (the counters are monotonic: launch k leaves them at k * tiles per sample)
  bool gnf = false; int gnf_mts = 0, gnf_nt = 0;
  size_t o_xbuf = 0, o_xcnt = 0;
  unsigned gnf_epoch = 0;
  // GroupNorm-backward APPLY fused into the data-gradient epilogue of the layer that CONSUMES this layer's activation (LoGnBwdFuse):
  // arrival counters [B][8], launches so far, and -- per backward -- whether o_dv / P2 were already produced that way
  size_t o_bcnt = 0;
  unsigned gba_epoch = 0;
  bool dv_done = false;
  hipEvent_t ev_ready = nullptr;   // dv_done: the event bound to the launch that wrote this layer's dv (null: none was bound)
  // few-rows layers (the 8 x 8 stage): forward / data gradient as a K-split 128 x 128-tile GEMM into fp32 slabs + ONE fused
  // (sample, group)-local pass (slab sum + bias + GroupNorm [+ Mish | backward]); 0 = the one-launch kernel
  int sk_fwd = 0, sk_dgrad = 0;
};

// How the weight gradients of fc_mu | fc_logvar and decoder.fc travel through a fused step (lo_vae_set_linear_factored's numbers;
// DESIGN.md has the table).  Readers ask the predicates below, never the value.
enum class LoLinearMode : int {
  off = 0,           // written to the flat buffer like every other gradient
  local = 1,         // single process: the backward leaves factors + their share of the norm, AdamW forms the tiles
  dp_factors = 2,    // data parallel: phase 1 leaves factors, the ranks all-gather them and write the averaged matrices out
  dp_gathered = 3,   // ... and never write them: norm and AdamW read the gathered blocks
};
// What one step leaves for the next optimizer step.  ready: a fused backward (mode 3: + lo_vae_gathered_early_norm) has left this
// step's factors and the Gram part of the gradient norm; scale: 1 / loss scale of that backward; gathered / world: the blocks
// lo_vae_gathered_early_norm was given (the caller keeps them alive and unchanged until the step that follows has read them)
struct LoFactorStep { bool ready = false; float scale = 1.f; const f16* gathered = nullptr; int world = 0; };

// One site of the bottleneck self-attention (LO_VAE_ATTN).  Parameters: gamma, then Wq | Wk | Wv and bq | bk | bv, each group contiguous
// in the flat buffer (one [640][512] matrix, one [640] bias).  Workspace: fp16 copy of the matrix and its transpose; qkv, the output y,
// the gradients dy (wrt y), dqkv, dx (wrt the site's input), the per-sample shares of dgamma
struct LoAttnSite {
  int p_gamma = 0, p_w = 0, p_b = 0;      // parameter indices of gamma, query_conv.weight, query_conv.bias (key: + 2, value: + 4)
  size_t o_w = 0, o_wt = 0;
  size_t o_qkv = 0, o_y = 0, o_dy = 0, o_dqkv = 0, o_dx = 0, o_dgpart = 0;
};

struct LoVae {
  int B = 0, L = 0;
  // parameters
  int nparam = 0;
  std::vector<size_t> p_off, p_numel;
  size_t flat_elems = 0;
  // layers: encoder stage s: enc[s][0] = strided conv, enc[s][1] = res.conv1, enc[s][2] = res.conv2
  ConvLayer enc[4][3];
  ConvLayer dec[4];
  size_t o_eout[4] = {};     // ResBlock outputs (stage outputs)
  size_t o_skipin[3] = {};   // skip feature maps handed to Decoder.forward from outside (lo_vae_decode_skips), fp16 NHWC
  // latent
  LoGeom g_head{}, g_head_d{}, g_dfc{}, g_dfc_d{};
  int head_split = 32, dfcd_split = 32;    // K splits of the two K = 32768 Linear GEMMs (8 / 16 / 32 / 64 measured in round 2: 32)
  size_t o_wp_head = 0, o_wp_head_t = 0, o_wp_dfc = 0, o_wp_dfc_t = 0;
  size_t o_xflat = 0, o_slab_head = 0, o_eps = 0, o_z = 0, o_klp = 0, o_mu = 0, o_lv = 0, o_yfc = 0, o_h0 = 0;
  size_t o_msep = 0, o_losses = 0, o_coefs = 0;
  // backward scratch
  size_t o_G[6] = {}, o_skipg[3] = {}, o_P1 = 0, o_P2 = 0, o_wslab = 0, o_wslab_lin = 0, o_fcw_part = 0, o_lc_part = 0, o_dz = 0, o_dml = 0,
         o_slab_dz = 0, o_gfc = 0;
  size_t o_packjobs = 0;
  std::vector<LoPackJob> packjobs_host;   // kept alive: source of the asynchronous table upload
  int n_packjobs = 0, pack_blocks = 0;
  int n_packjobs_enc = 0, pack_blocks_enc = 0;   // the early share of the table: encoder stages 1..3 (their jobs come first)
  const void* packjobs_for_ws = nullptr;         // workspace / parameter pointers the uploaded job table was built for
  const void* packjobs_for_params = nullptr;
  size_t ws_bytes = 0;
  int idx_fc_mu_w = 0, idx_fc_mu_b = 0, idx_fc_lv_w = 0, idx_fc_lv_b = 0, idx_dfc_w = 0, idx_dfc_b = 0, idx_final_w = 0, idx_final_b = 0;
  bool forward_done = false, loss_done = false;
  bool enc_done = false, dec_done = false;   // activations of an encoder / decoder forward are in the workspace (split module calls)
  int dec_skips = 0;         // how many skip maps the last decoder forward added (3 inside lo_vae_forward)
  // weight-gradient GEMMs run on a side stream, concurrently with the data-gradient / GroupNorm chain
  hipStream_t side = nullptr;
  hipEvent_t ev_dv[4] = {}, ev_join = nullptr, ev_pre = nullptr, ev_range = nullptr;
  bool async_handover = false, range_pending = false;   // lo_vae_set_async_handover: phase 1 / 3 leave their range's completion as an event on the side stream
  // Operand refresh on the side stream in five levels, one event each, recorded in this order (waiting for a level implies the
  // lower ones): 1 packed convs of encoder stages 1..3; 2 encoder stage 4 (parameters + packs); 3 the encoder heads (fc_mu /
  // fc_logvar: parameters + fp16 copy); 4 decoder.fc + decoder convs; 5 the transposed Linear copies only the backward reads
  hipEvent_t ev_lvl[6] = {};
  bool lvl_pending[6] = {};
  // pipelined optimizer step: levels 2..5 (AdamW of 97 % of the parameters + their operand refresh) are ENQUEUED by the next
  // forward once its first stage has run -- see lo_vae_optimizer_step
  struct { bool pending = false; float* P; const float* G; float* M; float* V; void* ws; LoAdamHyper hp; } defer;
  bool opt_tail_on_side = false;   // the last lo_vae_optimizer_step was pipelined: [b4, n) was updated on `side` (lo_vae_ema_update follows it there)
  int n_packjobs_s4 = 0, pack_blocks_s4 = 0, n_packjobs8_s4 = 0, pack_blocks8_s4 = 0;   // job-table prefix up to and including encoder stage 4
  int bwd_layer = 0;         // conv layers processed so far in the current backward (selects the dv buffer / events)
  size_t o_skslab = 0;       // slabs of the split-K convolutions (one launch at a time on the caller's stream)
  bool gn_local = true;      // LO_GN_LOCAL=0: never use the one-pass (sample, group)-local GroupNorm backward
  int nevent = 0;            // hand-over events handed out so far (ev_dv[nevent & 3])
  bool overlap = false;
  float* norm_scratch = nullptr;   // lo_vae_set_gradnorm_scratch: where a single-call backward leaves the early part of the gradient norm
  bool fuse_gnb = true;      // fuse the GroupNorm-backward reduction into the producing data-gradient epilogue
  bool fuse_gnf = false;     // fuse GroupNorm + Mish of a conv output into that conv's epilogue (sample rendezvous between its workgroups)
  bool fuse_gna = true;      // fuse the GroupNorm-backward APPLY pass into the data-gradient epilogue that already carries its reduction
  size_t o_sync_fail = 0;    // one word: set by a workgroup whose rendezvous poll ran out (never, unless a launch was lost)
  // rank-B Linear-layer weight gradients kept as their factors (lo_lowrank.hip): transposed, batch-padded factor copies
  // dml^T [2L][Bp], xflat^T [32768][Bp], Gfc^T [32768][Bp], z^T [L][Bp] (one contiguous block), Gram scratch
  LoLinearMode lin_mode = LoLinearMode::off;
  LoFactorStep fac;
  bool gathered_sum = false;   // lo_vae_set_gathered_sum: the gathered blocks are ADDED (micro-batches of one window), not averaged (ranks)
  int Bp = 0;
  size_t o_fac_dmlT = 0, o_fac_xT = 0, o_fac_gfcT = 0, o_fac_zT = 0, o_gram = 0;
  int n_cu = 0;              // compute units of the device (partition) this plan was made on; 0 = no device: nothing that waits across workgroups is planned
  bool n_cu_assumed = false; // lo_vae_plan_assume_cus: a host-only handle planning for a device it was told about
  const void* sync_for_ws = nullptr;
  // bottleneck self-attention (lo_vae_create_ex flag LO_VAE_ATTN): site 0 on the encoder's stage-4 output (before the flatten), site 1
  // on decoder.fc's output h0 (before up1).  g_att_qkv: qkv = x Wqkv^T + b (M = B * 64, K = 512, N = 640; also the geometry of the
  // weight gradient); g_att_dx: dx = dy + dqkv Wqkv on the transposed copy.  The weight-gradient slab is the sites' own.
  bool attn = false;
  LoAttnSite att[2];
  LoGeom g_att_qkv{}, g_att_dx{};
  size_t o_att_wslab = 0;
  // fp8 operand mode of the forward convs (lo_vae_create_ex flag LO_VAE_FP8_FWD)
  bool fp8_fwd = false;
  size_t o_eout8[4] = {}, o_h08 = 0, o_packjobs8 = 0;
  std::vector<LoPackF8Job> packjobs8_host;
  int n_packjobs8 = 0, pack_blocks8 = 0;
  int n_packjobs8_enc = 0, pack_blocks8_enc = 0;
};

// the 16 conv + GroupNorm + Mish layers in forward order: encoder stage 1 (strided conv, res.conv1, res.conv2) .. stage 4, then up1 .. up4
template <typename H, typename F>
static inline void for_each_layer(H* h, F&& fn) {   // H: LoVae or const LoVae
  for (int s = 0; s < 4; ++s)
    for (int k = 0; k < 3; ++k) fn(h->enc[s][k]);
  for (int s = 0; s < 4; ++s) fn(h->dec[s]);
}

// the GroupNorm of a conv layer, as lo_norm.h's calls name it: expects `P` and `ws` like the macros above
static inline LoGnLayer vae_gn_layer(const LoVae* h, const ConvLayer& c, const float* P, void* ws) {
  return {WSP(f16, c.o_v), WSP(float, c.o_stats), PRM(c.p_gw), PRM(c.p_gb), h->B, c.Ho * c.Wo, c.Cout};
}
// the ONE writer of np1 / np2, called BEFORE the launch that writes the rows: they must fit what setup_conv_layer sized P1 / P2 for.
// A count of 0 = that launch does not write the buffer: what is recorded for it stays
static inline int vae_record_rows(ConvLayer& c, LoGnRows r) {
  LO_REQUIRE(r.p1 <= c.prow_cap && r.p2 <= c.prow_cap, "GroupNorm backward %dx%dx%d: %d / %d rows of P1 / P2 per sample, room for %d",
             c.Ho, c.Wo, c.Cout, r.p1, r.p2, c.prow_cap);
  if (r.p1 > 0) c.np1 = r.p1;
  if (r.p2 > 0) c.np2 = r.p2;
  return LO_OK;
}

// ---- what a layer launches: the uses the choosers are asked with -----------------------------------------------------------------
// The executor (lo_vae_step.hip) and the plan query (lo_vae_layer_plan_ex, lo_vae_plan.hip) both come here: a choice is made once, by
// lo_conv_choose / lo_gn_bwd_choose / lo_wgrad_choose, with the use these helpers build, and the executor holds every launch that
// reports its choice to the one the helper returned (vae_require_planned).

// the chain's topology: the layer whose activation gradient the data gradient of c writes directly, so that its GroupNorm backward can
// ride on that launch (null: the data gradient of c feeds a stage output / h0 / nothing), and the layer whose data gradient does that for c
static inline const ConvLayer* vae_dgrad_prod(const LoVae* h, const ConvLayer& c) {
  for (int s = 1; s < 4; ++s) if (&c == &h->dec[s]) return &h->dec[s - 1];
  for (int s = 0; s < 4; ++s) {
    if (&c == &h->enc[s][2]) return &h->enc[s][1];
    if (&c == &h->enc[s][1]) return &h->enc[s][0];
  }
  return nullptr;
}
static inline ConvLayer* vae_dgrad_prod(LoVae* h, ConvLayer& c) {
  return const_cast<ConvLayer*>(vae_dgrad_prod(static_cast<const LoVae*>(h), static_cast<const ConvLayer&>(c)));
}
static inline const ConvLayer* vae_dgrad_consumer(const LoVae* h, const ConvLayer& c) {
  for (int s = 0; s < 3; ++s) if (&c == &h->dec[s]) return &h->dec[s + 1];
  for (int s = 0; s < 4; ++s) {
    if (&c == &h->enc[s][0]) return &h->enc[s][1];
    if (&c == &h->enc[s][1]) return &h->enc[s][2];
  }
  return nullptr;
}
// the data gradient of c adds a second gradient to its output: the ResBlock's identity branch (conv1), the decoder's skip gradient
// (the strided convs of stages 2..4)
static inline bool vae_dgrad_adds(const LoVae* h, const ConvLayer& c) {
  for (int s = 0; s < 4; ++s)
    if (&c == &h->enc[s][1] || (s > 0 && &c == &h->enc[s][0])) return true;
  return false;
}

// forward conv of layer c as conv_gn launches it.  y8: the layer's GroupNorm pass also leaves an e4m3 copy of its output
struct VaeFwdPlan { bool splitk, fuse; LoConvUse use; LoConvChoice choice; };
static inline VaeFwdPlan vae_fwd_plan(const ConvLayer& c, bool y8) {
  VaeFwdPlan p{};
  p.splitk = c.sk_fwd && !c.f8 && !y8;      // few output rows: K-split GEMM into fp32 slabs + one (sample, group)-local pass
  p.fuse = !p.splitk && c.gnf && !c.f8 && !y8;
  if (p.splitk) p.use.nsplit = c.sk_fwd;
  else { p.use.bias = true; p.use.gn_partial = !p.fuse; p.use.gf = p.fuse; p.use.f8 = c.f8; }
  p.choice = lo_conv_choose(c.gf, p.use);
  return p;
}
// data gradient of layer c.  prod: vae_dgrad_prod (null also where the caller wants no fusion); add: a second gradient is added.
// splitk: K-split GEMM + the slab form of prod's GroupNorm backward; else one launch with prod's GroupNorm-backward reduction in its
// epilogue (reduce; rows = P1 rows per sample it leaves) and, where the whole grid is resident at once, the apply pass too (apply)
struct VaeDgradPlan { bool splitk, reduce, apply; int rows; LoConvUse use; LoConvChoice choice; };
static inline VaeDgradPlan vae_dgrad_plan(const LoVae* h, const ConvLayer& c, const ConvLayer* prod, bool add) {
  VaeDgradPlan p{};
  p.splitk = prod && c.sk_dgrad && lo_gn_bwd_choose(prod->Ho * prod->Wo, prod->Cout, {.slab = true}).form == LO_GNB_SLAB_LOCAL;
  if (p.splitk) {
    p.use.nsplit = c.sk_dgrad;
  } else {
    p.use.add = add;
    if (prod && h->fuse_gnb) {
      // asked with the apply form: the same rows of P1 per sample either way (the apply form does not change the kernel)
      const LoConvChoice ch = lo_conv_choose(c.gd, {.add = add, .gb = true, .gb_apply = true});
      p.reduce = true;
      p.rows = ch.mts;
      // ... only where the whole grid is resident at once (one workgroup per CU): on the 64-channel 64 x 64 layers (1 024 tiles at
      // batch 64, two rounds of 512) the fused launch is 32-34 us longer than the 27 us pass it replaces, and the step is 0.6 %
      // faster without it there (22 309-22 332 against 22 185-22 202; nowhere: 22 238-22 316)
      p.apply = h->fuse_gna && ch.gnb_apply && h->B * ch.mts * ch.nt <= h->n_cu;
      p.use.gb = true; p.use.gb_apply = p.apply;
    }
  }
  p.choice = lo_conv_choose(c.gd, p.use);
  return p;
}
// GroupNorm backward of layer c as a launch of its own: from split-K slabs, or with rows_in_P1 rows per sample already in P1
static inline LoGnChoice vae_gn_bwd_choice(const LoVae* h, const ConvLayer& c, bool slab, int rows_in_P1) {
  return lo_gn_bwd_choose(c.Ho * c.Wo, c.Cout, {slab, rows_in_P1, h->gn_local});
}
// What the backward leaves of layer c's GroupNorm backward, replayed from the chain's topology: the executor keeps the P1 rows a
// data-gradient epilogue has written as state (ConvLayer::np1) and decides the form when it gets to the layer; the same helpers, asked
// in the order of the chain, give the plan query its answer, and a single-call backward ends by comparing the two (vae_check_gn_replay).
// form: LoGnBwdForm, or -1 = no launch of its own (the consuming layer's data gradient applied it)
struct VaeGnBwdPlan { int form, p1, p2; };
static inline VaeGnBwdPlan vae_gn_bwd_replay(const LoVae* h, const ConvLayer& c) {
  const ConvLayer* q = vae_dgrad_consumer(h, c);
  VaeDgradPlan d{};
  if (q) d = vae_dgrad_plan(h, *q, &c, vae_dgrad_adds(h, *q));
  if (q && d.apply) return {-1, d.rows, d.rows};
  const LoGnChoice g = vae_gn_bwd_choice(h, c, q && d.splitk, (q && d.reduce) ? d.rows : 0);
  return {(int)g.form, g.rows.p1 > 0 ? g.rows.p1 : d.rows, g.rows.p2};      // vae_record_rows: a count of 0 leaves what the epilogue recorded
}
static inline int vae_check_gn_replay(const LoVae* h) {
  int bad = 0;
  for_each_layer(h, [&](const ConvLayer& c) {
    const VaeGnBwdPlan p = vae_gn_bwd_replay(h, c);
    if (bad || (c.gnb_ran == p.form && c.np1 == p.p1 && c.np2 == p.p2)) return;
    lo_set_error("GroupNorm backward %dx%dx%d: the backward ran form %d and left %d / %d rows of P1 / P2 per sample, the plan has form %d, %d / %d",
                 c.Ho, c.Wo, c.Cout, c.gnb_ran, c.np1, c.np2, p.form, p.p1, p.p2);
    bad = 1;
  });
  return bad ? LO_ERR_STATE : LO_OK;
}
// a launch that reports its choice must have made the one the plan names, field by field
static inline int vae_require_planned(const LoConvChoice& ran, const LoConvChoice& plan, const char* what, const LoGeom& g) {
  if (ran.kernel == plan.kernel && ran.bm == plan.bm && ran.bn == plan.bn && ran.bk == plan.bk && ran.th == plan.th && ran.tw == plan.tw &&
      ran.grid == plan.grid && ran.mts == plan.mts && ran.rows == plan.rows && ran.nt == plan.nt && ran.gn_fuse == plan.gn_fuse &&
      ran.gnb_apply == plan.gnb_apply)
    return LO_OK;
  lo_set_error("%s %dx%d %d->%d: the launch chose kernel %d, tile %dx%dx%d / %dx%d, grid %d, rows %d / %d, n tiles %d, fusions %d %d; the plan has "
               "kernel %d, tile %dx%dx%d / %dx%d, grid %d, rows %d / %d, n tiles %d, fusions %d %d", what, g.Hout, g.Wout, g.Cin, g.Cout,
               ran.kernel, ran.bm, ran.bn, ran.bk, ran.th, ran.tw, ran.grid, ran.mts, ran.rows, ran.nt, (int)ran.gn_fuse, (int)ran.gnb_apply,
               plan.kernel, plan.bm, plan.bn, plan.bk, plan.th, plan.tw, plan.grid, plan.mts, plan.rows, plan.nt, (int)plan.gn_fuse, (int)plan.gnb_apply);
  return LO_ERR_STATE;
}

// ---- stream plumbing -------------------------------------------------------------------------------------------------------------
// work with slack (weight gradients, optimizer tail, operand refresh) goes to the side stream, if there is one; per-launch profiling
// keeps everything on one stream
static inline bool vae_side_on(const LoVae* h) { return h->overlap && !g_lo_prof_on; }
// what `behind` gets from here on runs after everything `ahead` holds now
static inline int vae_order(hipStream_t behind, hipStream_t ahead, hipEvent_t e) {
  LO_HIP(hipEventRecord(e, ahead));
  LO_HIP(hipStreamWaitEvent(behind, e, 0));
  return LO_OK;
}
static inline bool lo_event_marker() {   // LO_EVENT_MARKER=1: hipEventRecord behind the launch, as before round 3 (A/B: -0.5 %)
  static const bool on = getenv("LO_EVENT_MARKER") != nullptr;
  return on;
}
// Hand-over of a buffer to the side stream.  The event rides on the launch that writes the buffer (LO_LAUNCH_STOP, lo_common.h): a
// hipEventRecord behind that launch costs the caller's stream 3.5-4.7 us per hand-over (a marker packet the next kernel waits
// for), the kernel's own completion signal 0.9-1.3 us (tools/probe/ev_probe.hip).  Construct it right before the launcher whose LAST
// launch writes the buffer and call finish() right after it; the armed event never outlives the object (error returns included).
// Never two of them alive at once.
struct LoHandover {
  hipEvent_t ev = nullptr;                                                             // null: no side stream, nothing handed over
  LoHandover(hipEvent_t e, bool on) { if (on) { ev = e; if (!lo_event_marker()) g_lo_stop_event = e; } }
  LoHandover(LoVae* h, bool on) : LoHandover(on ? h->ev_dv[h->nevent & 3] : nullptr, on) { if (on) ++h->nevent; }   // next of the ring
  ~LoHandover() { g_lo_stop_event = nullptr; }
  int finish(hipStream_t st) {   // nobody consumed it (a launcher path without LO_LAUNCH_STOP, or LO_EVENT_MARKER): fall back to a marker
    if (ev && (g_lo_stop_event || lo_event_marker())) {
      g_lo_stop_event = nullptr;
      LO_HIP(hipEventRecord(ev, st));
    }
    return LO_OK;
  }
};

// Names the profiler records opened while it lives (per-call-site breakdowns of a LO_PROF_LAYERS run).  The records keep the
// pointer: the text is interned.  Never two of them alive at once (the end of any one clears the tag).
struct LoProfTag {
  template <typename... A>
  explicit LoProfTag(const char* fmt, A... a) {
    if (!(g_lo_prof_on && g_lo_prof_layers)) return;
    char text[64];
    snprintf(text, sizeof(text), fmt, a...);
    g_lo_prof_tag = lo_prof_intern(text);
  }
  void end() { g_lo_prof_tag = nullptr; }     // ahead of the scope's end: what is launched next keeps its own name
  ~LoProfTag() { end(); }
};

// the optimizer step forms the tiles of the two Linear weight gradients from factors (modes 1, 3)
static inline bool vae_opt_from_factors(const LoVae* h) { return h->lin_mode == LoLinearMode::local || h->lin_mode == LoLinearMode::dp_gathered; }
// ... and those factors are the gathered blocks of every rank, not this rank's own in the workspace (mode 3)
static inline bool vae_factors_gathered(const LoVae* h) { return h->lin_mode == LoLinearMode::dp_gathered; }
// a fused single-call backward leaves factors and their share of the norm instead of the two matrices (mode 1)
static inline bool vae_single_leaves_factors(const LoVae* h) { return h->lin_mode == LoLinearMode::local; }
// a fused phase-1 backward leaves factors for the ranks to all-gather instead of the two matrices (modes 2, 3)
static inline bool vae_phased_leaves_factors(const LoVae* h) { return h->lin_mode == LoLinearMode::dp_factors || h->lin_mode == LoLinearMode::dp_gathered; }
// the flat gradient buffer lacks the two matrices after a step: the mode's number (1 / 3), else 0 -- what lo_vae_linear_factored returns
static inline int vae_flat_lacks_linear(const LoVae* h) { return vae_opt_from_factors(h) ? (int)h->lin_mode : 0; }
// Gathered factor blocks (data parallel): every rank's block keeps the workspace's layout dml^T | xflat^T | Gfc^T | z^T.  Elements from
// one rank's block to the next, and where the factor at workspace offset o_fac sits inside rank 0's block of `gathered`:
// what multiplies sum_r dY_r^T X_r of `world` gathered blocks: 1 / loss scale, over `world` for the ranks' average
static inline float vae_gathered_scale(const LoVae* h, int world) { return h->gathered_sum ? h->fac.scale : h->fac.scale / (float)world; }
static inline size_t vae_fac_block_elems(const LoVae* h) { return (h->o_gram - h->o_fac_dmlT) / 2; }
static inline const f16* vae_fac_in_block(const LoVae* h, const f16* gathered, size_t o_fac) { return gathered + (o_fac - h->o_fac_dmlT) / 2; }

// ---- across the units ------------------------------------------------------------------------------------------------------------
int vae_flush_deferred(LoVae* h, hipStream_t after_main);    // lo_vae_opt.hip: enqueue a pipelined optimizer step's tail
int vae_wait_level(LoVae* h, hipStream_t st, int lvl);       // lo_vae_opt.hip: `st` waits for operand-refresh level lvl
// where the site's input lives: the encoder's stage-4 output / the decoder's h0
static inline size_t vae_attn_input(const LoVae* h, int site) { return site == 0 ? h->o_eout[3] : h->o_h0; }
