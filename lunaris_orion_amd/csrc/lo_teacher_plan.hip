// Teacher engine: state table in the reference's state_dict order, the parameter offsets resolved from its names, geometries and the
// workspace plan, create / destroy, the state-table queries and the operand pack (lo_teacher.h).
#include "lo_teacher.h"
#include "lo_conv.h"
#include <memory>
#include <unordered_map>

// ---- state table in the reference's state_dict order (lunar_evaluator.py; checked against the oracle in tests)
static void t_state_table(LoTeacher* h) {
  const int F = h->F;
  auto add = [&](const std::string& k, size_t n, bool f = true) { h->names.push_back(k); h->numel.push_back(n); h->is_float.push_back(f); };
  auto conv = [&](const std::string& p, int co, int ci, int k, int groups = 1) { add(p + ".weight", (size_t)co * (ci / groups) * k * k); add(p + ".bias", co); };
  auto bn = [&](const std::string& p, int c) { add(p + ".weight", c); add(p + ".bias", c); add(p + ".running_mean", c); add(p + ".running_var", c); add(p + ".num_batches_tracked", 1, false); };
  auto lin = [&](const std::string& p, int o, int i) { add(p + ".weight", (size_t)o * i); add(p + ".bias", o); };
  std::string fe = "feature_extractor";
  conv(fe + ".conv1.0", 32, 3, 3); bn(fe + ".conv1.2", 32);
  const char* brs[3] = {"edge_branch", "color_branch", "detail_branch"};
  const int brk[3] = {3, 5, 3};
  for (int b = 0; b < 3; ++b) {
    std::string q = fe + "." + brs[b];
    conv(q + ".0", 32, 32, brk[b], 32); conv(q + ".1", 64, 32, 1); bn(q + ".3", 64);
  }
  conv(fe + ".fusion.0", 128, 192, 1); bn(fe + ".fusion.2", 128);
  for (int e = 0; e < h->E; ++e)
    for (int l = 0; l < 3; ++l) {
      std::string p = "experts." + std::to_string(e) + "." + std::to_string(l);
      const int cin = l == 0 ? 128 : F;
      add(p + ".layer_scale", F);
      conv(p + ".conv1.0", F, cin, 3); bn(p + ".conv1.2", F);
      add(p + ".attention.rel_pos_h", 64); add(p + ".attention.rel_pos_w", 64); add(p + ".attention.last_spatial_shapes", 2);
      conv(p + ".attention.qkv", 3 * F, F, 1); conv(p + ".attention.proj", F, F, 1);
      conv(p + ".conv2.0", F, F, 3); bn(p + ".conv2.2", F);
      if (cin != F) { conv(p + ".shortcut.0", F, cin, 1); bn(p + ".shortcut.1", F); }   // ExpertBlock.shortcut (lunar_evaluator.py:254-257)
    }
  lin("gate.2", 256, 128); lin("gate.5", h->E, 256);
  for (int e = 0; e < h->E; ++e) {
    std::string p = "quality_heads." + std::to_string(e);
    add(p + ".2.weight", F); add(p + ".2.bias", F); lin(p + ".3", 64, F); lin(p + ".6", 4, 64);
  }
  const char* hn[3] = {"semantic_head", "style_net", "prompt_net"};
  const int ho[3] = {1, h->emb, h->emb};
  for (int k = 0; k < 3; ++k) {
    std::string p = hn[k];
    add(p + ".2.weight", F); add(p + ".2.bias", F); lin(p + ".3", 128, F); lin(p + ".6", ho[k], 128);
  }
  size_t o = 0;
  h->off.assign(h->names.size(), 0);
  for (size_t i = 0; i < h->names.size(); ++i) {
    h->off[i] = o;
    if (h->is_float[i]) o += (h->numel[i] + 63) & ~(size_t)63;
  }
  h->flat_elems = o;
}

// names -> offsets, once: the executors address parameters through h->fe / h->blk / h->heads and never build a name again
static int t_resolve(LoTeacher* h) {
  std::unordered_map<std::string, size_t> index;
  for (size_t i = 0; i < h->names.size(); ++i) index[h->names[i]] = h->off[i];
  std::string missing;
  auto at = [&](const std::string& k) -> size_t {
    auto it = index.find(k);
    if (it != index.end()) return it->second;
    if (missing.empty()) missing = k;
    return 0;
  };
  auto bn = [&](const std::string& p) { return TBnOff{at(p + ".weight"), at(p + ".bias"), at(p + ".running_mean"), at(p + ".running_var")}; };
  auto head = [&](const std::string& p) { return THeadOff{at(p + ".2.weight"), at(p + ".2.bias"), at(p + ".3.weight"), at(p + ".3.bias"), at(p + ".6.weight"), at(p + ".6.bias")}; };
  const std::string fe = "feature_extractor";
  h->fe.conv1_w = at(fe + ".conv1.0.weight"); h->fe.conv1_b = at(fe + ".conv1.0.bias"); h->fe.bn1 = bn(fe + ".conv1.2");
  const char* brs[3] = {"edge_branch", "color_branch", "detail_branch"};
  for (int b = 0; b < 3; ++b) {
    const std::string q = fe + "." + brs[b];
    h->fe.br[b] = TBranchOff{at(q + ".0.weight"), at(q + ".0.bias"), at(q + ".1.weight"), at(q + ".1.bias"), bn(q + ".3")};
  }
  h->fe.fus_w = at(fe + ".fusion.0.weight"); h->fe.fus_b = at(fe + ".fusion.0.bias"); h->fe.bn_fus = bn(fe + ".fusion.2");
  for (int e = 0; e < h->E; ++e)
    for (int l = 0; l < 3; ++l) {
      const std::string p = "experts." + std::to_string(e) + "." + std::to_string(l);
      TBlockOff& k = h->blk[e][l];
      k.layer_scale = at(p + ".layer_scale");
      k.conv1_w = at(p + ".conv1.0.weight"); k.conv1_b = at(p + ".conv1.0.bias"); k.bn1 = bn(p + ".conv1.2");
      k.qkv_w = at(p + ".attention.qkv.weight"); k.qkv_b = at(p + ".attention.qkv.bias");
      k.proj_w = at(p + ".attention.proj.weight"); k.proj_b = at(p + ".attention.proj.bias");
      k.conv2_w = at(p + ".conv2.0.weight"); k.conv2_b = at(p + ".conv2.0.bias"); k.bn2 = bn(p + ".conv2.2");
      if (h->F != 128 && l == 0) { k.sc_w = at(p + ".shortcut.0.weight"); k.sc_b = at(p + ".shortcut.0.bias"); k.bn_sc = bn(p + ".shortcut.1"); }
    }
  h->heads.g_w1 = at("gate.2.weight"); h->heads.g_b1 = at("gate.2.bias"); h->heads.g_w2 = at("gate.5.weight"); h->heads.g_b2 = at("gate.5.bias");
  for (int e = 0; e < h->E; ++e) h->heads.q[e] = head("quality_heads." + std::to_string(e));
  h->heads.sem = head("semantic_head"); h->heads.style = head("style_net"); h->heads.prompt = head("prompt_net");
  LO_REQUIRE(missing.empty(), "lo_teacher_create: the state table has no tensor '%s'", missing.c_str());
  return LO_OK;
}

// ---- geometries
static int t_make_geoms(LoTeacher* h) {
  const int B = h->B, F = h->F;
  LO_TRYT(lo_make_geom(&h->g3, LO_CONV3_S1, B, 128, 128, 128, 128));
  LO_TRYT(lo_make_geom(&h->gq, LO_LINEAR, B, 128, 128, 128, 384));
  LO_TRYT(lo_make_geom(&h->gp, LO_LINEAR, B, 128, 128, 128, 128));
  LO_TRYT(lo_make_geom(&h->gpw, LO_LINEAR, B, 128, 128, 32, 64));
  LO_TRYT(lo_make_geom(&h->gfus, LO_LINEAR, B, 128, 128, 192, 128));
  // plain form of a block: lo_teacher_forward takes it for feature_dim 256 / 512, the full-backward mode for every feature_dim
  LO_TRYT(lo_make_geom(&h->g3a, LO_CONV3_S1, B, 128, 128, 128, F));
  LO_TRYT(lo_make_geom(&h->g3b, LO_CONV3_S1, B, 128, 128, F, F));
  LO_TRYT(lo_make_geom(&h->gqF, LO_LINEAR, B, 128, 128, F, 3 * F));
  LO_TRYT(lo_make_geom(&h->gsc, LO_LINEAR, B, 128, 128, 128, F));
  LO_TRYT(lo_make_geom(&h->gpc, LO_LINEAR, B, 8, 128, F, F));
  LO_TRYT(lo_make_geom(&h->gfw, LO_LINEAR, B, 128, 128, 64, 128));
  h->qrows = ((B * 543 + 127) / 128) * 128;
  LO_TRYT(lo_make_geom(&h->gU, LO_LINEAR, h->qrows / 128, 1, 128, 128, 1024));
  LO_TRYT(lo_make_geom(&h->gZ, LO_LINEAR, B, 8, 128, 1088, 128));
  LO_TRYT(lo_make_geom(&h->g3c, LO_CONV3_S1, B, 8, 128, 128, 128));
  return LO_OK;
}

// ---- workspace plan (after t_make_geoms: two switches depend on what the conv kernels support for g3)
static int t_plan_workspace(LoTeacher* h, unsigned flags) {
  const int B = h->B, F = h->F, E = h->E;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t r = off; off += (bytes + 255) & ~(size_t)255; return r; };
  const size_t px = (size_t)B * T_HW;
  h->o_raw32 = take(px * 32 * 2); h->o_dw = take(px * 32 * 2);
  for (int b = 0; b < 3; ++b) h->o_br[b] = take(px * 64 * 2);
  h->o_cat = take(px * 192 * 2);
  h->o_feat = take(px * 128 * 2); h->o_x0 = take(px * F * 2); h->o_x1 = take(px * F * 2);
  h->o_rawA = take(px * F * 2); h->o_bnA = take(px * F * 2); h->o_qkv = take(px * 3 * F * 2);
  h->o_att = take(px * 128 * 2); h->o_proj = take(px * F * 2); h->o_rawB = take(px * F * 2);
  h->o_bnp = take((size_t)(px / 64) * F * 2 * 4 + 65536);   // BatchNorm partial rows: one per >= 64-pixel tile, C <= F
  h->o_bnpre = take((size_t)64 * F * 2 * 4);
  h->o_ss = take((size_t)(2 * T_FMAX + 2 * 192 + 64) * 4);   // [C <= 512][2], then the feature extractor's private 32-channel table
  h->o_poolp = take((size_t)B * 64 * F * 4);
  h->o_pool_f = take((size_t)B * 128 * 4);
  h->o_pool_e = take((size_t)E * B * F * 4);
  h->o_rawq = take((size_t)B * E * 4 * 4);
  for (int e = 0; e < E; ++e)
    for (int l = 0; l < 3; ++l) {
      for (int c = 0; c < 2; ++c) h->o_wp3[e][l][c] = take((size_t)F * 9 * F * 2);
      h->o_wqkv[e][l] = take((size_t)3 * F * F * 2);
      h->o_wproj[e][l] = take((size_t)F * F * 2);
    }
  if (F != 128) {
    for (int e = 0; e < E; ++e) h->o_wsc[e] = take((size_t)F * 128 * 2);
    h->o_sc = take(px * F * 2);
    h->o_ss_sc = take((size_t)F * 2 * 4);
    h->o_attc = take((size_t)B * 1024 * F * 2);
  }
  for (int b = 0; b < 3; ++b) h->o_wpw[b] = take((size_t)64 * 32 * 2);
  h->o_wfus = take((size_t)128 * 192 * 2);
  h->o_wfus_fold = take((size_t)128 * 192 * 2);
  h->o_bfus_fold = take(128 * 4);
  h->o_ss_cat = take(192 * 2 * 4);
  const char* dense = getenv("LO_T_DENSE");
  h->sparse = !(dense && atoi(dense) != 0);
  const char* shared = getenv("LO_T_BWD_SHARED");
  h->bwd_shared = shared && atoi(shared) != 0;
  const size_t cpx = (size_t)B * 1024;
  h->o_qin = take((size_t)h->qrows * 128 * 2); h->o_U = take((size_t)h->qrows * 1024 * 2); h->o_Z = take(cpx * 1088 * 2);
  h->o_projc = take(cpx * 128 * 2); h->o_rawBc = take(cpx * 128 * 2);
  {
    const char* ft = getenv("LO_T_FUSE_TAIL");
    h->fuse_tail = F == 128 && h->sparse && !(ft && atoi(ft) == 0) && lo_conv3_pp_applies(h->g3);
  }
  for (int k = 0; k < 2; ++k) h->o_xc[k] = take(cpx * 128 * 2);
  h->o_xc3 = take((size_t)E * cpx * 128 * 2);
  h->o_poolpe = take((size_t)E * B * 64 * 128 * 4);
  {
    const size_t kx0 = take((size_t)E * 3 * 6 * 128 * 2);
    for (int e = 0; e < E; ++e) h->o_kx[e] = kx0 + (size_t)e * 3 * 6 * 128 * 2;
  }
  for (int e = 0; e < E; ++e)
    for (int l = 0; l < 3; ++l) {
      h->o_cvec[e][l] = take(6 * 128 * 4);
      h->o_wu[e][l] = take((size_t)1024 * 128 * 2); h->o_ub[e][l] = take(1024 * 4); h->o_wz[e][l] = take((size_t)128 * 1088 * 2);
    }
  h->o_ssb = take((size_t)B * F * 2 * 4);
  if (flags & LO_TEACHER_FP8_CONV) {
    if (F == 128) h->fp8 = lo_conv3_pp_f8_applies(h->g3);
    else {
      // the plain form: each geometry on its own, where lo_conv_choose serves the teacher epilogue on e4m3 operands
      LoConvUse u;
      u.bias = u.ex = u.f8 = true;
      h->fp8a = lo_conv_choose(h->g3a, u).kernel == LO_CK_IGEMM_F8;
      h->fp8b = lo_conv_choose(h->g3b, u).kernel == LO_CK_IGEMM_F8;
      h->fp8 = h->fp8a || h->fp8b;
    }
  }
  if (h->fp8) {
    for (int e = 0; e < E; ++e)
      for (int l = 0; l < 3; ++l)
        for (int c = 0; c < 2; ++c) { h->o_w8[e][l][c] = take((size_t)F * 9 * F); h->o_ws8[e][l][c] = take((size_t)F * 4); }
    h->o_feat8 = take(px * 128); h->o_x8[0] = take(px * F); h->o_x8[1] = take(px * F); h->o_proj8 = take(px * F);
  }
  h->ws_bytes = off;
  return LO_OK;
}

extern "C" int lo_teacher_create(int B, int num_experts, int feature_dim, int embedding_dim, LoTeacher** out) {
  return lo_teacher_create_ex(B, num_experts, feature_dim, embedding_dim, 0u, out);
}
extern "C" int lo_teacher_create_ex(int B, int num_experts, int feature_dim, int embedding_dim, unsigned flags, LoTeacher** out) {
  LO_REQUIRE(out && B >= 1, "lo_teacher_create: bad argument");
  LO_REQUIRE((flags & ~(unsigned)LO_TEACHER_FP8_CONV) == 0, "lo_teacher_create_ex: unknown flag bits 0x%x", flags);
  LO_REQUIRE(feature_dim == 128 || feature_dim == 256 || feature_dim == 512,
             "lo_teacher_create: feature_dim %d is not built (128 = the CLI default, 256, 512 = the README's High-End recipe)", feature_dim);
  LO_REQUIRE(num_experts >= 1 && num_experts <= 8, "lo_teacher_create: num_experts %d out of range", num_experts);
  LO_REQUIRE(embedding_dim >= 1 && embedding_dim <= 512, "lo_teacher_create: embedding_dim %d out of range", embedding_dim);
  std::unique_ptr<LoTeacher> h(new LoTeacher());     // a failing step below frees the handle
  h->B = B; h->E = num_experts; h->emb = embedding_dim; h->F = feature_dim;
  t_state_table(h.get());
  LO_TRYT(t_resolve(h.get()));
  LO_TRYT(t_make_geoms(h.get()));
  LO_TRYT(t_plan_workspace(h.get(), flags));
  *out = h.release();
  return LO_OK;
}
extern "C" int lo_teacher_last_path(const LoTeacher* h) { return h ? h->last_path : -1; }
extern "C" void lo_teacher_destroy(LoTeacher* h) { delete h; }
extern "C" int lo_teacher_num_tensors(const LoTeacher* h) { return (int)h->names.size(); }
extern "C" const char* lo_teacher_tensor_name(const LoTeacher* h, int i) { return (i >= 0 && i < (int)h->names.size()) ? h->names[i].c_str() : nullptr; }
extern "C" size_t lo_teacher_tensor_numel(const LoTeacher* h, int i) { return (i >= 0 && i < (int)h->names.size()) ? h->numel[i] : 0; }
extern "C" long long lo_teacher_tensor_offset(const LoTeacher* h, int i) {   // -1 for non-float buffers (kept by the host)
  if (i < 0 || i >= (int)h->names.size() || !h->is_float[i]) return -1;
  return (long long)h->off[i];
}
extern "C" size_t lo_teacher_flat_elems(const LoTeacher* h) { return h->flat_elems; }
extern "C" size_t lo_teacher_workspace_bytes(const LoTeacher* h) { return h->ws_bytes; }

extern "C" int lo_teacher_pack(LoTeacher* h, const float* P, void* ws, void* stream) {
  LO_REQUIRE(h && P && ws, "lo_teacher_pack: null argument");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int F = h->F;
  for (int e = 0; e < h->E; ++e)
    for (int l = 0; l < 3; ++l) {
      const TBlockOff& k = h->blk[e][l];
      // feature_dim 128: the fast paths' geometry and their folded operands; else plain operand copies, nothing folded
      LO_TRYT(lo_pack_weight(TP(k.conv1_w), TW(f16, h->o_wp3[e][l][0]), F != 128 ? (l == 0 ? h->g3a : h->g3b) : h->g3, st));
      LO_TRYT(lo_pack_weight(TP(k.conv2_w), TW(f16, h->o_wp3[e][l][1]), F != 128 ? h->g3b : h->g3, st));
      for (int c = 0; c < 2 && h->fp8; ++c) {
        const bool first = l == 0 && c == 0;     // the 128 -> F conv
        if (F != 128 && !(first ? h->fp8a : h->fp8b)) continue;
        LO_TRYT(lo_pack_f8_one(F == 128 ? h->g3 : (first ? h->g3a : h->g3b), TW(f16, h->o_wp3[e][l][c]), TW(uint8_t, h->o_w8[e][l][c]),
                               TW(float, h->o_ws8[e][l][c]), st));
      }
      LO_TRYT(lo_cast_f32_f16(TP(k.qkv_w), TW(f16, h->o_wqkv[e][l]), (size_t)3 * F * F, st));
      LO_TRYT(lo_cast_f32_f16(TP(k.proj_w), TW(f16, h->o_wproj[e][l]), (size_t)F * F, st));
      if (F != 128 && l == 0) LO_TRYT(lo_cast_f32_f16(TP(k.sc_w), TW(f16, h->o_wsc[e]), (size_t)F * 128, st));
      if (F == 128) LO_TRYT(t_pack_f128(h, P, ws, e, l, st));
    }
  for (int b = 0; b < 3; ++b) LO_TRYT(lo_cast_f32_f16(TP(h->fe.br[b].pw_w), TW(f16, h->o_wpw[b]), (size_t)64 * 32, st));
  LO_TRYT(lo_cast_f32_f16(TP(h->fe.fus_w), TW(f16, h->o_wfus), (size_t)128 * 192, st));
  return LO_OK;
}
