// Finalize-time derived weight images: the item streams of the persistent loop, the cluster loop and the decoder / encoder row-strip kernels.
// Part of libmldhip's single translation unit; include order: see mldhip.hip.  Internal linkage throughout (anonymous namespace) except the handle type itself.
#pragma once

namespace {

// What a builder collects: element [row0][k0] of a weight as (floats into the arena, row stride, pad) in the order the image's kernel consumes them.
// LoopItem and ClFrag have the same three fields; each is the argument type of its own pack kernel, hence the template.
template <class Item>
struct ItemList {
  const float* arena;
  std::vector<Item> v;
  void push(const float* w, int ld, int row0, int k0, int pad = 0) { v.push_back(Item{(long long)(w - arena) + (long long)row0 * ld + k0, ld, pad}); }
  size_t size() const { return v.size(); }
};

// items [first, first + n) through `kernel` (a workgroup of `threads` per item) into `dst`: uploads them, waits for the launch, frees the device list.
// `what` names the image in the handle's error message, `kname` the launch.
template <class Item>
int pack_items(Ctx& c, const char* what, const char* kname, void (*kernel)(const float*, const Item*, float*), unsigned threads,
               const ItemList<Item>& items, size_t first, size_t n, float* dst) {
  E* e = c.e;
  Item* dev = nullptr;
  if (hipMalloc((void**)&dev, n * sizeof(Item)) != hipSuccess) return e->fail(MLDHIP_EHIP, "hipMalloc(%s)", what);
  hipError_t st = hipMemcpy(dev, items.v.data() + first, n * sizeof(Item), hipMemcpyHostToDevice);
  if (st == hipSuccess) {
    MLD_LAUNCH(kernel, dim3((unsigned)n), dim3(threads), 0, c.stream, (const float*)e->arena, (const Item*)dev, dst);
    check_launch(c, kname);
    st = hipStreamSynchronize(c.stream);
  }
  (void)hipFree(dev);
  if (st != hipSuccess) return e->fail(MLDHIP_EHIP, "%s: %s", what, hipGetErrorString(st));
  return c.rc;
}

// The feed-forward block's items in the order of the software pipeline (loop_fused.hpp, ffn_strip.hpp): linear1 of block 0, then
// [linear1 of block hb + 1, linear2's share of block hb]
void push_ffn(ItemList<LoopItem>& items, const float* w1, const float* w2, int F) {
  auto f1 = [&](int hb) { for (int kc = 0; kc < 8; ++kc) items.push(w1, 256, hb * 128, kc * 32); };
  auto f2 = [&](int hb) { for (int kc = 0; kc < 4; ++kc) for (int cb = 0; cb < 2; ++cb) items.push(w2, F, cb * 128, hb * 128 + kc * 32); };
  f1(0);
  for (int hb = 0; hb < 8; ++hb) {
    if (hb < 7) f1(hb + 1);
    f2(hb);
  }
}

// finalize-time: the denoiser's GEMM weights as the item stream the loop kernel consumes, its small parameters packed, the
// DDIM coefficients of the scheduler's steps.  Item order = the kernel's phase order (loop_fused.hpp).
int build_loop_stream(Ctx& c) {
  E* e = c.e;
  e->loop_ips = 0;
  if (!fused_built(e) || !e->group_ready[kGroupDenoiser]) return 0;
  const int L = e->cfg.num_layers, nb = (L - 1) / 2, n = e->cfg.num_inference_steps, F = e->cfg.ff_size;
  ItemList<LoopItem> items{e->arena};
  // chunk-major inside a group: the items that multiply the same 32 columns of A are adjacent (loop_fused.hpp run2 / run3)
  for (int l = 0; l < L; ++l) {
    const EncLayerP& P_ = e->den[l];
    for (int hp = 0; hp < 2; ++hp)
      for (int kc = 0; kc < 8; ++kc)
        for (int part = 0; part < 3; ++part) items.push(P_.in_w, 256, part * 256 + hp * 128, kc * 32);
    for (int kc = 0; kc < 8; ++kc)
      for (int cb = 0; cb < 2; ++cb) items.push(P_.out_w, 256, cb * 128, kc * 32);
    push_ffn(items, P_.l1_w, P_.l2_w, F);
    if (l >= nb && l + 1 < L) {
      const float* w = P(e, "denoiser.encoder.linear_blocks." + std::to_string(l - nb) + ".weight");
      for (int half = 0; half < 2; ++half)
        for (int kc = 0; kc < 8; ++kc)
          for (int cb = 0; cb < 2; ++cb) items.push(w, 512, cb * 128, half * 256 + kc * 32);
    }
  }
  const size_t ips = items.size();
  for (int j = 0; j < 8; ++j) items.v.push_back(items.v[j]);      // the ring's look-ahead across the end of a step (loop_fused.hpp gload)
  const size_t nit = items.size(), small_floats = (size_t)L * kLsLayer + (size_t)nb * 256 + 768, tail = (size_t)n * 6;
  if (e->loop_stream) { (void)hipFree(e->loop_stream); e->loop_stream = nullptr; }
  if (e->loop_small) { (void)hipFree(e->loop_small); e->loop_small = nullptr; }
  if (e->loop_stream_x3) { (void)hipFree(e->loop_stream_x3); e->loop_stream_x3 = nullptr; }
  const bool want_x3 = e->cfg.precision == MLDHIP_PREC_F16X3;      // the split mode: a second image of the stream
  const char* what = "sample-major loop tables";
  if (hipMalloc((void**)&e->loop_stream, nit * kLoopItemFloats * sizeof(float)) != hipSuccess ||
      (want_x3 && hipMalloc((void**)&e->loop_stream_x3, nit * kLoopItemFloats * sizeof(float)) != hipSuccess) ||
      hipMalloc((void**)&e->loop_small, (small_floats + tail) * sizeof(float)) != hipSuccess)
    return e->fail(MLDHIP_EHIP, "hipMalloc(%s)", what);
  e->loop_ddim = e->loop_small + small_floats;
  e->loop_eta = e->loop_ddim + (size_t)n * 4;
  if (int rc = pack_items(c, what, "pack_loop_stream", pack_loop_stream_kernel<false>, 512, items, 0, nit, e->loop_stream)) return rc;
  if (want_x3)
    if (int rc = pack_items(c, what, "pack_loop_stream", pack_loop_stream_kernel<true>, 512, items, 0, nit, e->loop_stream_x3)) return rc;
  hipError_t st = hipSuccess;
  auto put = [&](size_t off, const float* src, size_t nfl) {
    if (st == hipSuccess) st = hipMemcpy(e->loop_small + off, src, nfl * sizeof(float), hipMemcpyDeviceToDevice);
  };
  for (int l = 0; l < L; ++l) {
    const EncLayerP& P_ = e->den[l];
    const size_t o = (size_t)l * kLsLayer;
    put(o + kLsInB, P_.in_b, 768); put(o + kLsOutB, P_.out_b, 256); put(o + kLsN1W, P_.n1_w, 256); put(o + kLsN1B, P_.n1_b, 256);
    put(o + kLsL1B, P_.l1_b, 1024); put(o + kLsL2B, P_.l2_b, 256); put(o + kLsN2W, P_.n2_w, 256); put(o + kLsN2B, P_.n2_b, 256);
  }
  size_t o = (size_t)L * kLsLayer;
  for (int i = 0; i < nb; ++i, o += 256) put(o, P(e, "denoiser.encoder.linear_blocks." + std::to_string(i) + ".bias"), 256);
  put(o, P(e, "denoiser.encoder.norm.weight"), 256);
  put(o + 256, P(e, "denoiser.encoder.norm.bias"), 256);
  put(o + 512, P(e, "denoiser.query_pos.pe"), 256);
  std::vector<float> coef((size_t)n * 4);
  for (int s = 0; s < n; ++s) {
    const DdimCoef k = ddim_coef(e, e->timesteps[s]);
    coef[4 * s] = k.sqrt_at; coef[4 * s + 1] = k.sqrt_1mat; coef[4 * s + 2] = k.sqrt_ap; coef[4 * s + 3] = k.sqrt_1map;
  }
  if (st == hipSuccess) st = hipMemcpy(e->loop_ddim, coef.data(), coef.size() * sizeof(float), hipMemcpyHostToDevice);
  std::vector<float> etab((size_t)n * 2);
  for (int s = 0; s < n; ++s) {
    const DdimEta k = ddim_eta(e, e->timesteps[s]);
    etab[2 * s] = k.c_eps; etab[2 * s + 1] = k.sigma;
  }
  if (st == hipSuccess) st = hipMemcpy(e->loop_eta, etab.data(), etab.size() * sizeof(float), hipMemcpyHostToDevice);
  if (st != hipSuccess) return e->fail(MLDHIP_EHIP, "%s: %s", what, hipGetErrorString(st));
  e->loop_ips = (int)ips;
  return 0;
}

// finalize-time: per column group and wave, the weight fragments (16 rows x 32 k, split-f16) in the order den_cluster_kernel consumes them;
// needs the packed small parameters / DDIM table of build_loop_stream
int build_cluster_stream(Ctx& c) {
  E* e = c.e;
  if (e->cl_stream) { (void)hipFree(e->cl_stream); e->cl_stream = nullptr; }
  if (!fused_built(e) || !e->group_ready[kGroupDenoiser] || !e->loop_ips || e->cfg.precision != MLDHIP_PREC_F16X3) return 0;
  const int L = e->cfg.num_layers, nb = (L - 1) / 2, F = e->cfg.ff_size;
  ItemList<ClFrag> frags{e->arena};
  // Ph1 and the out-projection of head hc, the same in both forms: waves 0-3 [Q, K], waves 4-7 [V]; then the head's K slice of the out-projection:
  // columns 32 w + 16 j, k = 64 hc + 32 kc
  auto head = [&](const EncLayerP& P_, int hc, int w) {
    for (int kc = 0; kc < 8; ++kc) {
      if (w < 4) { frags.push(P_.in_w, 256, 64 * hc + 16 * w, 32 * kc); frags.push(P_.in_w, 256, 256 + 64 * hc + 16 * w, 32 * kc); }
      else frags.push(P_.in_w, 256, 512 + 64 * hc + 16 * (w - 4), 32 * kc);
    }
    for (int kc = 0; kc < 2; ++kc)
      for (int j = 0; j < 2; ++j) frags.push(P_.out_w, 256, 32 * w + 16 * j, 64 * hc + 32 * kc);
  };
  // the narrow form (den_cluster_kernel<.., 4>) in wave offsets [0, 32), then the wide form (<.., 8>) in [32, 96): 8 column groups; groups 0-3 are the heads,
  // every group holds an eighth of the feed-forward block
  for (int groups = 4; groups <= 8; groups += 4)
    for (int hc = 0; hc < groups; ++hc)
      for (int w = 0; w < 8; ++w) {
        e->cl_wave_off[(groups == 8 ? 32 : 0) + hc * 8 + w] = (unsigned)(frags.size() * kClFragFloats);
        const size_t first = frags.size();
        for (int l = 0; l < L; ++l) {
          const EncLayerP& P_ = e->den[l];
          const float* ws = l >= nb && l + 1 < L ? P(e, "denoiser.encoder.linear_blocks." + std::to_string(l - nb) + ".weight") : nullptr;
          if (hc < 4) head(P_, hc, w);
          if (groups == 4) {
            for (int kc = 0; kc < 8; ++kc)                                             // linear1: hidden columns 256 hc + 32 w + 16 j
              for (int j = 0; j < 2; ++j) frags.push(P_.l1_w, 256, 256 * hc + 32 * w + 16 * j, 32 * kc);
            for (int kc = 0; kc < 16; ++kc) frags.push(P_.l2_w, F, 64 * hc + 16 * (w & 3), 512 * (w >> 2) + 32 * kc);      // linear2: K half w >> 2
            for (int kc = 0; ws && kc < 8; ++kc) frags.push(ws, 512, 64 * hc + 16 * (w & 3), 256 * (w >> 2) + 32 * kc);    // skip linear: x half / parked half
          } else {
            for (int kc = 0; kc < 8; ++kc) frags.push(P_.l1_w, 256, 128 * hc + 16 * w, 32 * kc);                           // linear1: hidden columns 128 hc + 16 w
            for (int kc = 0; kc < 8; ++kc) frags.push(P_.l2_w, F, 32 * hc + 16 * (w & 1), 256 * (w >> 1) + 32 * kc);        // linear2: tile w & 1, K quarter w >> 1
            for (int kc = 0; ws && kc < 4; ++kc) frags.push(ws, 512, 32 * hc + 16 * (w & 1), 128 * (w >> 1) + 32 * kc);     // skip linear: K quarter w >> 1 (0, 1: x; 2, 3: parked)
          }
        }
        for (int j = 0; j < kClRing; ++j) frags.v.push_back(frags.v[first + j]);        // look-ahead across the end of a step
      }
  if (!e->cl_wave_off_dev && hipMalloc((void**)&e->cl_wave_off_dev, 96 * sizeof(unsigned)) != hipSuccess) return e->fail(MLDHIP_EHIP, "hipMalloc(cluster loop offsets)");
  if (hipMemcpy(e->cl_wave_off_dev, e->cl_wave_off, 96 * sizeof(unsigned), hipMemcpyHostToDevice) != hipSuccess) return e->fail(MLDHIP_EHIP, "cluster loop offsets");
  if (hipMalloc((void**)&e->cl_stream, frags.size() * (size_t)kClFragFloats * sizeof(float)) != hipSuccess) return e->fail(MLDHIP_EHIP, "hipMalloc(cluster loop stream)");
  return pack_items(c, "cluster loop stream", "pack_cluster_frags", pack_cluster_frags_kernel, 64, frags, 0, frags.size(), e->cl_stream);
}

// feature columns feats2joints_kernel reads: 0 .. 3 (root) and 4 + 3 (j - 1) + {0, 1, 2} for the other joints -- 67 on HumanML3D
int joint_feat_cols(const E* e) { return 4 + 3 * (e->cfg.njoints - 1); }

// 128-column blocks of the one-launch final stage of MldVae.decode (kernels/final_strip.hpp), 0 = the width has none: 3 for 256 < nfeats <= 264,
// 2 for 128 < nfeats < 256; 128 and 256 themselves are whole staged tiles and stay on the staged GEMM
int final_strip_blocks(const E* e) {
  const int NF = e->cfg.nfeats;
  if (is_actor(e) || is_novae(e)) return 0;
  return NF > 256 && NF <= kFsXs ? 3 : NF > 128 && NF < 256 ? 2 : 0;
}

// finalize-time (split precision modes): linear1 / linear2 of every decoder / encoder layer in the item order of
// kernels/ffn_strip.hpp -- run1(0), then [run1(hb), run2(hb - 1)] for hb = 1..7, then run2(7) -- as split-f16 fragment images
int build_ffn_streams(Ctx& c) {
  E* e = c.e;
  e->ffn_stream_of.clear();
  e->gemm_stream_of.clear();
  e->final_stream = nullptr;
  e->final_joints_stream = nullptr;
  if (e->ffn_streams) { (void)hipFree(e->ffn_streams); e->ffn_streams = nullptr; }
  const bool split = e->cfg.precision == MLDHIP_PREC_F16X3;
  if (!split || is_novae(e) || e->cfg.latent_dim != 256 || e->cfg.ff_size != 1024) return 0;
  std::vector<std::pair<const float*, const float*>> layers;
  if (e->group_ready[kGroupVaeDecoder]) for (auto& L : e->dec) layers.push_back({L.l1_w, L.l2_w});
  if (e->group_ready[kGroupVaeEncoder]) for (auto& L : e->venc) layers.push_back({L.l1_w, L.l2_w});
  if (layers.empty()) return 0;
  ItemList<LoopItem> items{e->arena};
  for (auto& lw : layers) push_ffn(items, lw.first, lw.second, 1024);
  // the row-strip GEMMs (kernels/gemm_strip_x3.hpp): per pair of 128-column blocks, per K segment, per chunk, [block 2p, block 2p + 1]
  std::vector<std::pair<const float*, size_t>> gemm_first;          // weight -> first item of its stream
  auto gstream = [&](const float* w, int N, int K) {
    gemm_first.push_back({w, items.size()});
    for (int pr = 0; pr < N / 256; ++pr)
      for (int sg = 0; sg < K / 256; ++sg)
        for (int kc = 0; kc < 8; ++kc)
          for (int cb = 0; cb < 2; ++cb) items.push(w, K, (2 * pr + cb) * 128, sg * 256 + kc * 32);
  };
  const int nbv = (e->cfg.num_layers - 1) / 2;
  if (e->group_ready[kGroupVaeDecoder]) {
    for (auto& L : e->dec) { gstream(L.in_w, 768, 256); gstream(L.out_w, 256, 256); }
    if (!is_actor(e)) for (int i = 0; i < nbv; ++i) gstream(P(e, "vae.decoder.linear_blocks." + std::to_string(i) + ".weight"), 256, 512);
  }
  if (e->group_ready[kGroupVaeEncoder]) {
    for (auto& L : e->venc) { gstream(L.in_w, 768, 256); gstream(L.out_w, 256, 256); }
    if (!is_actor(e)) for (int i = 0; i < nbv; ++i) gstream(P(e, "vae.encoder.linear_blocks." + std::to_string(i) + ".weight"), 256, 512);
  }
  // kernels/final_strip.hpp: vae.final_layer.weight [NF][256], 256 < NF <= 264 (the strip's 48 x NF results are parked in its 48 x 264-word image),
  // zero-padded to three 128-row blocks: per chunk [block 0, 1, 2]; pad = valid rows of the block (pack_stream_rows_kernel zero-fills the rest).
  // 128 < NF < 256 (KIT-ML: 251): two blocks, per chunk [block 0, 1] (final_strip2_x3_kernel)
  const size_t final_first = items.size();
  const int NFv = e->cfg.nfeats, final_blocks = final_strip_blocks(e);
  if (e->group_ready[kGroupVaeDecoder] && final_blocks) {
    const float* wf = P(e, "vae.final_layer.weight");
    for (int kc = 0; kc < 8; ++kc)
      for (int blk = 0; blk < final_blocks; ++blk) items.push(wf, 256, blk * 128, kc * 32, std::min(128, NFv - blk * 128));
  }
  // ... and block 0 cut to the rows feats2joints reads (joint_feat_cols), per chunk: the joints-only final stage (final_joints_x3_kernel)
  const size_t joints_first = items.size();
  if (items.size() > final_first && joint_feat_cols(e) <= std::min(128, NFv)) {
    const float* wf = P(e, "vae.final_layer.weight");
    for (int kc = 0; kc < 8; ++kc) items.push(wf, 256, 0, kc * 32, joint_feat_cols(e));
  }
  const char* what = "feed-forward weight streams";
  if (hipMalloc((void**)&e->ffn_streams, items.size() * kLoopItemFloats * sizeof(float)) != hipSuccess) return e->fail(MLDHIP_EHIP, "hipMalloc(%s)", what);
  if (int rc = pack_items(c, what, "pack_ffn_streams", pack_loop_stream_kernel<true>, 512, items, 0, final_first, e->ffn_streams)) return rc;
  if (items.size() > final_first)
    if (int rc = pack_items(c, what, "pack_final_stream", pack_stream_rows_kernel, 512, items, final_first, items.size() - final_first,
                            e->ffn_streams + final_first * (size_t)kLoopItemFloats)) return rc;
  for (size_t i = 0; i < layers.size(); ++i) e->ffn_stream_of[layers[i].first] = e->ffn_streams + i * (size_t)kFfnStripItems * kLoopItemFloats;
  for (auto& gf : gemm_first) e->gemm_stream_of[gf.first] = e->ffn_streams + gf.second * (size_t)kLoopItemFloats;
  if (items.size() > final_first) e->final_stream = e->ffn_streams + final_first * (size_t)kLoopItemFloats;
  if (items.size() > joints_first) e->final_joints_stream = e->ffn_streams + joints_first * (size_t)kLoopItemFloats;
  return c.rc;
}

}  // namespace
