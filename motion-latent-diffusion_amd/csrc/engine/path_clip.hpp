// The CLIP text tower (mldhip_text_encode; config field clip_layers > 0): token ids -> [P][1][text_dim] embeddings, the math of transformers'
// CLIPModel.get_text_features.  Three things make it cheaper than the padded [P][77] tower without changing a bit of what it computes:
//   1. causality -- the attention is causal and the output is read at the EOS row, so rows behind EOS are never built: prompt p
//      contributes n_p = eos_pos[p] + 1 rows, all prompts packed into one [sum n_p][D] activation;
//   2. duplicates -- identical id rows (the B copies of "" of a classifier-free-guidance batch) are computed once and stored to every copy;
//   3. the pooled output needs final_layer_norm and the projection at the EOS rows only.
// Issued eagerly (the row total changes per call: no hipGraph).  Part of libmldhip's single translation unit; include order: see mldhip.hip.
#pragma once

namespace {

constexpr int kClipAttnX3LdsBytes = attn_x3_lds_bytes<kClipKeyTiles>();

struct ClipLayerP {
  const float *ln1_w, *ln1_b, *ln2_w, *ln2_b, *qkv_w, *qkv_b, *out_w, *out_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
};
ClipLayerP bind_clip_layer(E* e, int i) {
  const std::string p = clip_layer(i);
  ClipLayerP L;
  L.ln1_w = P(e, p + ".layer_norm1.weight"); L.ln1_b = P(e, p + ".layer_norm1.bias");
  L.ln2_w = P(e, p + ".layer_norm2.weight"); L.ln2_b = P(e, p + ".layer_norm2.bias");
  L.qkv_w = P(e, p + ".self_attn.q_proj.weight"); L.qkv_b = P(e, p + ".self_attn.q_proj.bias");      // q | k | v back to back (declare_clip_params)
  L.out_w = P(e, p + ".self_attn.out_proj.weight"); L.out_b = P(e, p + ".self_attn.out_proj.bias");
  L.fc1_w = P(e, p + ".mlp.fc1.weight"); L.fc1_b = P(e, p + ".mlp.fc1.bias");
  L.fc2_w = P(e, p + ".mlp.fc2.weight"); L.fc2_b = P(e, p + ".mlp.fc2.bias");
  return L;
}

// count: the call's non-finite output values go into the handle's sticky counter (the range probe's own calls do not: engine/probe.hpp)
int text_encode_impl(E* e, const int32_t* ids_host, const int32_t* eos_host, int NP, float* out_dev, hipStream_t stream, bool count = true) {
  const auto& cfg = e->cfg;
  if (cfg.clip_layers <= 0) return e->fail(MLDHIP_ESTATE, "mldhip_text_encode: the handle was created without a text tower (mldhip_config.clip_layers = 0)");
  if (!e->finalized || !e->group_ready[kGroupClip]) return e->fail(MLDHIP_ESTATE, "mldhip_text_encode before finalize / text_encoder.* tower tensors not loaded");
  if (!ids_host || !eos_host || !out_dev) return e->fail(MLDHIP_EINVAL, "null pointer");
  if (NP < 1 || NP > cfg.clip_max_prompts) return e->fail(MLDHIP_EINVAL, "P=%d must be in 1..clip_max_prompts=%d", NP, cfg.clip_max_prompts);
  const int ctx = cfg.clip_ctx, W = cfg.text_dim, H = cfg.clip_heads;
  for (int p = 0; p < NP; ++p) {
    if (eos_host[p] < 0 || eos_host[p] >= ctx) return e->fail(MLDHIP_EINVAL, "eos_pos[%d]=%d outside [0, clip_ctx=%d)", p, eos_host[p], ctx);
    for (int t = 0; t < ctx; ++t) {
      const int32_t id = ids_host[(size_t)p * ctx + t];
      if (id < 0 || id >= cfg.clip_vocab) return e->fail(MLDHIP_EINVAL, "ids[%d][%d]=%d outside [0, clip_vocab=%d)", p, t, id, cfg.clip_vocab);
    }
  }
  // ---- dedupe on the id rows up to EOS; pack the unique prompts' rows
  std::map<std::vector<int32_t>, int> seen;
  std::vector<int> dup(NP), first;      // unique index per prompt; first prompt of every unique index
  for (int p = 0; p < NP; ++p) {
    std::vector<int32_t> key(ids_host + (size_t)p * ctx, ids_host + (size_t)p * ctx + eos_host[p] + 1);
    auto it = seen.find(key);
    if (it == seen.end()) { it = seen.emplace(std::move(key), (int)first.size()).first; first.push_back(p); }
    dup[p] = it->second;
  }
  const int U = (int)first.size();
  int R = 0;
  for (int u = 0; u < U; ++u) R += eos_host[first[u]] + 1;
  CtxUse use(e, stream);
  if (use.rc) return use.rc;
  std::vector<int32_t>& tab = e->ctxs[e->cur_ctx].clip_tab_host;
  tab.assign((size_t)2 * R + 3 * U + NP, 0);
  int32_t *row_tok = tab.data(), *row_pos = row_tok + R, *off = row_pos + R, *cnt = off + U, *eos_row = cnt + U, *dupv = eos_row + U;
  for (int u = 0, r = 0; u < U; ++u) {
    const int p = first[u], n = eos_host[p] + 1;
    off[u] = r; cnt[u] = n; eos_row[u] = r + n - 1;
    for (int t = 0; t < n; ++t, ++r) { row_tok[r] = ids_host[(size_t)p * ctx + t]; row_pos[r] = t; }
  }
  for (int p = 0; p < NP; ++p) dupv[p] = dup[p];
  int32_t* dtab = reinterpret_cast<int32_t*>(e->cTab);
  HIP_TRY(e, hipMemcpyAsync(dtab, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  const int32_t *d_tok = dtab, *d_pos = d_tok + R, *d_off = d_pos + R, *d_cnt = d_off + U, *d_eos = d_cnt + U, *d_dup = d_eos + U;

  Ctx c{e, stream};
  const bool x3 = cfg.precision == MLDHIP_PREC_F16X3 && e->arena_x3 && e->probe[kProbeText].ok;      // the verdict of finalize's range probe
  const unsigned ew = (unsigned)std::min<long long>(2048, ((long long)R * W / 4 + 255) / 256);
  MLD_LAUNCH(clip_embed_kernel, dim3(ew), dim3(256), 0, stream, P(e, std::string(kClipText) + "embeddings.token_embedding.weight"),
             P(e, std::string(kClipText) + "embeddings.position_embedding.weight"), d_tok, d_pos, e->cX, R, W);
  if (check_launch(c, "clip_embed")) return c.rc;
  auto layernorm = [&](const float* X, float* Y, const float* g, const float* b, const int* gather, int M) {
    MLD_LAUNCH(clip_layernorm_kernel<3>, dim3((M + 3) / 4), dim3(256), 0, stream, X, Y, g, b, gather, M);
    check_launch(c, "clip_layernorm");
  };
  for (int i = 0; i < cfg.clip_layers && !c.rc; ++i) {
    const ClipLayerP L = bind_clip_layer(e, i);
    layernorm(e->cX, e->cLN, L.ln1_w, L.ln1_b, nullptr, R);
    gemm_clip(c, lin_args(e->cLN, W, W, L.qkv_w, L.qkv_b, e->cQKV, 3 * W, R, 3 * W), x3);
    if (x3) { MLD_LAUNCH(clip_attn_x3_kernel, dim3(U * H), dim3(kClipAttnWaves * 64), kClipAttnX3LdsBytes, stream, e->cQKV, e->cAO, d_off, d_cnt, H); }
    else { MLD_LAUNCH(clip_attn_kernel, dim3(U * H), dim3(kClipAttnWaves * 64), kClipAttnLdsBytes, stream, e->cQKV, e->cAO, d_off, d_cnt, H); }
    check_launch(c, "clip_attn");
    GemmArgs o = lin_args(e->cAO, W, W, L.out_w, L.out_b, e->cX, W, R, W);
    o.res = e->cX; o.ldres = W;
    gemm_clip(c, o, x3);
    layernorm(e->cX, e->cLN, L.ln2_w, L.ln2_b, nullptr, R);
    GemmArgs f1 = lin_args(e->cLN, W, W, L.fc1_w, L.fc1_b, e->cFF, cfg.clip_ff, R, cfg.clip_ff);
    f1.act = ACT_QGELU;
    gemm_clip(c, f1, x3);
    GemmArgs f2 = lin_args(e->cFF, cfg.clip_ff, cfg.clip_ff, L.fc2_w, L.fc2_b, e->cX, W, R, W);
    f2.res = e->cX; f2.ldres = W;
    gemm_clip(c, f2, x3);
  }
  if (c.rc) return c.rc;
  // final_layer_norm on the EOS rows only, text_projection (no bias), every prompt reads its unique representative's row
  layernorm(e->cX, e->cE0, P(e, std::string(kClipText) + "final_layer_norm.weight"), P(e, std::string(kClipText) + "final_layer_norm.bias"), d_eos, U);
  gemm_clip(c, lin_args(e->cE0, W, W, P(e, "text_encoder.text_model.text_projection.weight"), nullptr, e->cE1, W, U, W), x3);
  if (c.rc) return c.rc;
  MLD_LAUNCH(clip_scatter_kernel, dim3((unsigned)std::min(1024, (NP * W / 4 + 255) / 256)), dim3(256), 0, stream, e->cE1, d_dup, out_dev, NP, W);
  if (check_launch(c, "clip_scatter") || !count) return c.rc;
  MLD_LAUNCH(count_nonfinite_kernel, dim3((unsigned)std::min(256, (NP * W + 255) / 256)), dim3(256), 0, stream, out_dev, (long long)NP * W, e->nonfinite);
  return check_launch(c, "count_nonfinite");
}

}  // namespace
