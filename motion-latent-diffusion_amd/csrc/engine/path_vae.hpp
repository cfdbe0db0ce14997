// The VAE of the latent models: MldVae / ActorVae decode and encode on the decoder's kernels, feats2joints.
// Part of libmldhip's single translation unit; include order: see mldhip.hip.  Internal linkage throughout (anonymous namespace) except the handle type itself.
#pragma once

namespace {

int pick_nkt(int T) { return T <= 64 ? 4 : T <= 112 ? 7 : T <= 208 ? 13 : 18; }

// shared_qkv: QKV holds ONE sample's projections [T][3D], read by every (sample, head) workgroup (decoder layer 0, dec_layer)
// rep != nullptr (decoder layer 0 under "dec_lean"): only the samples that are their own representative compute (length_reps_kernel)
void dec_attention(Ctx& c, int B, int T, const int32_t* lens = nullptr, int shared_qkv = 0, const int* rep = nullptr) {
  if (!lens) lens = c.e->lens_dev;
  E* e = c.e;
  const int H = e->cfg.num_heads;
  const int nkt = pick_nkt(T);
  dim3 grid(B * H), block(512);
  if (staged_prec(e) != PREC_F32) {
    // the modes that run the decoder GEMMs on 16-bit MFMAs run its attention split-f16 as well (attention.hpp)
    // key-blocked form (40 KB of LDS, two workgroups per CU, any T): pays once there is more than one workgroup per CU to overlap
    // (B H >= 512: 108 vs 133 us at 1 280 workgroups); with one per CU the whole-K/V kernel below is 5 % faster (28.9 vs 30.3 us)
    // (it covers 16 query tiles = 256 frames per (sample, head); longer sequences take the whole-K/V kernel)
    if (T <= 256 && (e->flash_attn == 2 || (e->flash_attn == 1 && B * H >= 512))) {
      // V staged row-major and read as MFMA fragments through ds_read_b64_tr_b16 (r03: 454 -> 417 us per launch at 2 048 motions against
      // transposed V planes written with 2-byte stores; streaming hints on its loads / stores measured level: both alternatives retired in r04)
      MLD_COUNTED(c, "attn_flash_x3", MLD_LAUNCH(attn_flash_x3_kernel, grid, block, kFlashLdsBytes, c.stream, e->QKV, e->AO, lens, T, H, shared_qkv, rep));
      return;
    }
    switch (nkt) {
      case 4: MLD_COUNTED(c, "attn_decode_x3", MLD_LAUNCH((attn_decode_x3_kernel<4>), grid, block, attn_x3_lds_bytes<4>(), c.stream, e->QKV, e->AO, lens, T, H, shared_qkv, rep)); break;
      case 7: MLD_COUNTED(c, "attn_decode_x3", MLD_LAUNCH((attn_decode_x3_kernel<7>), grid, block, attn_x3_lds_bytes<7>(), c.stream, e->QKV, e->AO, lens, T, H, shared_qkv, rep)); break;
      case 13: MLD_COUNTED(c, "attn_decode_x3", MLD_LAUNCH((attn_decode_x3_kernel<13>), grid, block, attn_x3_lds_bytes<13>(), c.stream, e->QKV, e->AO, lens, T, H, shared_qkv, rep)); break;
      default: MLD_COUNTED(c, "attn_decode_x3", MLD_LAUNCH((attn_decode_x3_kernel<18>), grid, block, attn_x3_lds_bytes<18>(), c.stream, e->QKV, e->AO, lens, T, H, shared_qkv, rep)); break;
    }
    return;
  }
  const size_t shmem = (size_t)2 * nkt * 16 * 68 * sizeof(float);
  switch (nkt) {
    case 4: MLD_COUNTED(c, "attn_decode", MLD_LAUNCH((attn_decode_kernel<4>), grid, block, shmem, c.stream, e->QKV, e->AO, lens, T, H, shared_qkv)); break;
    case 7: MLD_COUNTED(c, "attn_decode", MLD_LAUNCH((attn_decode_kernel<7>), grid, block, shmem, c.stream, e->QKV, e->AO, lens, T, H, shared_qkv)); break;
    case 13: MLD_COUNTED(c, "attn_decode", MLD_LAUNCH((attn_decode_kernel<13>), grid, block, shmem, c.stream, e->QKV, e->AO, lens, T, H, shared_qkv)); break;
    default: MLD_COUNTED(c, "attn_decode", MLD_LAUNCH((attn_decode_kernel<18>), grid, block, shmem, c.stream, e->QKV, e->AO, lens, T, H, shared_qkv)); break;
  }
}

// rows per strip of the register-direct decoder kernels: 96 (six row tiles: 2 MB of weights per 96 rows) when the launch fills the chip
// several times over, 64 when it would not -- one bs-64 request is 12 544 frame rows = 131 strips of 96 on 256 CUs, but 196 of 64,
// each a third shorter ("ffn_strip" 1 = this rule, 4 / 6 = always)
int strip_rows_rt(const E* e, int M) {
  if (e->ffn_strip == 4 || e->ffn_strip == 6) return e->ffn_strip;
  return (M + 63) / 64 <= 512 ? 4 : 6;
}

// Row-strip form of a decoder / encoder GEMM in the split modes (kernels/gemm_strip_x3.hpp) when the shape is one it is built for
// and the weight has a fragment-ordered stream; returns false when the caller should take the staged tiles instead.
bool strip_gemm(Ctx& c, const GemmArgs& g, bool ln) {
  E* e = c.e;
  const int rt = strip_rows_rt(e, g.M);
  if (!e->strip_gemm || staged_prec(e) != PREC_F16X3 || e->trace_on || g.M <= e->small_m) return false;
  if (g.K1 != 256 || g.lda != 256 || (g.K2 != 0 && (g.K2 != 256 || g.lda2 != 256)) || g.N % 256 || g.act != ACT_NONE || g.relu_in || g.lens) return false;
  auto it = e->gemm_stream_of.find(g.W);
  if (it == e->gemm_stream_of.end()) return false;
  StripGemmArgs a;
  a.A = g.A; a.A2 = g.A2; a.W = it->second; a.bias = g.bias; a.Y = g.Y; a.ldy = g.ldy; a.M = g.M; a.N = g.N;
  a.skip_lens = g.skip_lens; a.skip_rpg = g.skip_rpg;
  if (ln) {
    if (g.N != 256 || g.K2 != 0 || !g.res || g.ldres != 256 || !g.g1) return false;
    a.res = g.res; a.g1 = g.g1; a.b1 = g.b1; a.cvec = g.cvec; a.rpg = g.rows_per_group; a.g2 = g.g2; a.b2 = g.b2;
    if (g.cvec && (g.ldcvec != 256 || !g.g2)) return false;
    if (rt == 4) MLD_COUNTED(c, "strip_gemm_x3", MLD_LAUNCH((strip_gemm_x3_kernel<4, 1, true, false>), dim3((g.M + 63) / 64), dim3(512), (strip_gemm_lds_bytes<4, 1, false>()), c.stream, a));
    else MLD_COUNTED(c, "strip_gemm_x3", MLD_LAUNCH((strip_gemm_x3_kernel<6, 1, true, false>), dim3((g.M + 95) / 96), dim3(512), (strip_gemm_lds_bytes<6, 1, false>()), c.stream, a));
  } else if (g.K2 == 256) {
    if (g.N != 256) return false;
    // (streaming hints measured level on this form -- 414.6 vs 413.7 us, r03c_kernel_stats_ab.csv -- so it has no hinted build)
    MLD_COUNTED(c, "strip_gemm_x3", MLD_LAUNCH((strip_gemm_x3_kernel<4, 2, false, false>), dim3((g.M + 63) / 64), dim3(512), (strip_gemm_lds_bytes<4, 2, false>()), c.stream, a));
  } else if (rt == 4) {
    // in-projection (N = 768): row strips loaded and outputs stored with the streaming hint (527 -> 504 us per launch at 2 048 motions, r03c)
    MLD_COUNTED(c, "strip_gemm_x3", MLD_LAUNCH((strip_gemm_x3_kernel<4, 1, false, true, true>), dim3((g.M + 63) / 64), dim3(512), (strip_gemm_lds_bytes<4, 1, true>()), c.stream, a));
  } else {
    MLD_COUNTED(c, "strip_gemm_x3", MLD_LAUNCH((strip_gemm_x3_kernel<6, 1, false, true, true>), dim3((g.M + 95) / 96), dim3(512), (strip_gemm_lds_bytes<6, 1, true>()), c.stream, a));
  }
  return true;
}

// linear1 + GELU + linear2 + residual + LayerNorm of a post-norm layer.  Split modes with D = 256, FF = 1024: ONE launch
// (kernels/ffn_strip.hpp) reading its fragment-ordered weight stream; otherwise the two staged GEMMs.  ragged_T > 0: skip all-padding row tiles.
void ffn_block(Ctx& c, const float* x, float* y, int M, const float* w1, const float* b1, const float* w2, const float* b2,
               const float* gamma, const float* beta, int ragged_T) {
  E* e = c.e;
  const int D = e->cfg.latent_dim, F = e->cfg.ff_size;
  if (staged_prec(e) == PREC_F16X3 && e->ffn_strip && D == 256 && F == 1024 && M > e->small_m && !e->trace_on && e->ffn_stream_of.count(w1)) {
    // register-direct form (kernels/ffn_strip.hpp): weights from the layer's fragment-ordered stream, 96- or 64-row strips
    FfnArgs a;
    a.X = x; a.W1 = e->ffn_stream_of[w1]; a.b1 = b1; a.b2 = b2; a.gamma = gamma; a.beta = beta; a.Y = y; a.M = M;
    if (ragged_T > 0) { a.skip_lens = e->lens_dev; a.skip_rpg = ragged_T; }
    // auto: 48-row strips, two workgroups per CU (four waves per SIMD, 128 registers each) for launches that fill the chip: 2 % off the
    // decoder against 96-row strips (r03, 2 048 motions: 25.2 vs 25.8 ms) although the weights are streamed twice as often
    if (e->ffn_strip == 3 || (e->ffn_strip == 1 && strip_rows_rt(e, M) == 6)) MLD_COUNTED(c, "ffn_strip_x3", MLD_LAUNCH(ffn_strip_x3_kernel<3>, dim3((M + 47) / 48), dim3(512), ffn_strip_lds_bytes<3>(), c.stream, a));
    else if (strip_rows_rt(e, M) == 6) MLD_COUNTED(c, "ffn_strip_x3", MLD_LAUNCH(ffn_strip_x3_kernel<6>, dim3((M + 95) / 96), dim3(512), ffn_strip_lds_bytes<6>(), c.stream, a));
    else MLD_COUNTED(c, "ffn_strip_x3", MLD_LAUNCH(ffn_strip_x3_kernel<4>, dim3((M + 63) / 64), dim3(512), ffn_strip_lds_bytes<4>(), c.stream, a));
    return;
  }
  GemmArgs f1 = lin_args(x, D, D, w1, b1, e->FF, F, M, F);
  f1.act = ACT_GELU;
  GemmArgs f2 = lin_args(e->FF, F, F, w2, b2, y, D, M, D);
  f2.res = x; f2.ldres = D; f2.g1 = gamma; f2.b1 = beta;
  if (ragged_T > 0) {
    f1.skip_lens = f2.skip_lens = e->lens_dev;
    f1.skip_rpg = f2.skip_rpg = ragged_T;
  }
  gemm(c, f1);
  gemm_ln(c, f2);
}

// The decoder's self-attention block on half Q | K | V (kernels/dec_half.hpp; option "dec_half", verdict of finalize's probe in probe[kProbeDecodeHalf]): split mode,
// row-strip kernels on, D = 256 as 4 heads of 64, at most 16 query tiles per (sample, head)
bool dec_half_on(const E* e, int T) {
  return e->dec_half && (e->probe[kProbeDecodeHalf].ok || e->dec_half == 2) && staged_prec(e) == PREC_F16X3 && e->strip_gemm && !e->trace_on && e->cfg.latent_dim == 256 &&
         e->cfg.num_heads == 4 && T <= 256;
}

// the rest of a decoder layer behind its self-attention as ONE launch (kernels/ffn_strip.hpp TAIL form, "dec_tail")
bool dec_tail_on(E* e, const DecLayerP& L, int M) {
  return e->dec_tail && staged_prec(e) == PREC_F16X3 && e->strip_gemm && (e->ffn_strip == 3 || (e->ffn_strip == 1 && strip_rows_rt(e, M) == 6)) &&
         e->cfg.latent_dim == 256 && e->cfg.ff_size == 1024 && !e->trace_on && M > e->small_m && e->ffn_stream_of.count(L.l1_w) && e->gemm_stream_of.count(L.out_w);
}
// "dec_lean", layer 0 where it runs through "dec_l0_once" and the fused tail: the positional table itself is the layer input (no init_queries copy
// per sample: decode_body), the tail reads the attention output of each sample's length representative (dec_tail_l0_x3_kernel)
bool dec_l0_lean(E* e, int B, int T) {
  return e->dec_lean && e->dec_l0_once && B > 1 && T <= kMaxRepFrames && !e->dec.empty() && dec_tail_on(e, e->dec[0], B * T);
}

// One decoder layer over M = B*T frame rows with memory = the sample's latent (cross_attention.py:323-345).
// pos_input: xin holds the time queries themselves (zeros + positional rows, init_queries_kernel): row t of EVERY sample is pe[t], so
// the layer's Q, K, V depend on t only.  They are then projected once, for sample 0's T rows, and read by every (sample, head)
// attention workgroup (which still applies its own sample's length mask): exact, and the [B T][3 D] tensor of that layer -- 1.23 GB
// written and read back at 2 048 motions -- never exists ("dec_l0_once").
// lean (pos_input only): xin is the positional table [T][D] itself, see dec_l0_lean
void dec_layer(Ctx& c, int l, const float* xin, float* xout, int B, int T, bool pos_input = false, bool lean = false) {
  E* e = c.e;
  const DecLayerP& L = e->dec[l];
  const int D = e->cfg.latent_dim, M = B * T;
  const int* rep = lean ? reinterpret_cast<const int*>(e->len_rep) : nullptr;
  auto ragged = [&](GemmArgs g) { g.skip_lens = e->lens_dev; g.skip_rpg = T; return g; };   // skip all-padding row tiles
  const bool once = pos_input && e->dec_l0_once && B > 1;
  if (dec_half_on(e, T) && e->gemm_stream_of.count(L.in_w) && (once || M > e->small_m)) {
    // the self-attention block on half Q | K | V (kernels/dec_half.hpp, "dec_half"): in-projection = half rows x split weights, output packed
    // [row][768] halves with q pre-scaled; attention on plain half operands
    unsigned* qh = reinterpret_cast<unsigned*>(e->QKV);
    if (once) {
      // one sample's T rows through the fp32 projection (a launch of a few microseconds), then converted; the halves sit behind the fp32 rows
      // (B > 1: the buffer holds at least two samples' rows)
      gemm(c, lin_args(xin, D, D, L.in_w, L.in_b, e->QKV, 3 * D, T, 3 * D));
      qh += (size_t)T * 3 * D;
      MLD_COUNTED(c, "qkv_to_half", MLD_LAUNCH(qkv_to_half_kernel, dim3((T * 96 + 255) / 256), dim3(256), 0, c.stream, e->QKV, qh, T));
    } else {
      InprojHArgs a;
      a.A = xin; a.W = e->gemm_stream_of[L.in_w]; a.bias = L.in_b; a.Y = qh; a.M = M; a.skip_lens = e->lens_dev; a.skip_rpg = T;
      // 64-row strips, two workgroups per CU (69 KB of LDS, 128 registers): one workgroup's row loads / output stores run under the other's products
      // ("dec_half" 6: 96-row strips, one per CU -- a third less weight traffic per row)
      if (e->dec_half == 6) MLD_COUNTED(c, "strip_inproj_h", MLD_LAUNCH(strip_inproj_h_kernel<6>, dim3((M + 95) / 96), dim3(512), inproj_h_lds_bytes<6>(), c.stream, a));
      else MLD_COUNTED(c, "strip_inproj_h", MLD_LAUNCH(strip_inproj_h_kernel<4>, dim3((M + 63) / 64), dim3(512), inproj_h_lds_bytes<4>(), c.stream, a));
    }
    MLD_COUNTED(c, "attn_flash_h", MLD_LAUNCH(attn_flash_h_kernel, dim3(B * e->cfg.num_heads), dim3(512), kFlashHLdsBytes, c.stream, qh, e->AO, e->lens_dev, T, e->cfg.num_heads, once ? 1 : 0, rep));
  } else {
    // once: all T rows (no ragged skip: sample 0 may be shorter than the samples that read its rows)
    const GemmArgs q = once ? lin_args(xin, D, D, L.in_w, L.in_b, e->QKV, 3 * D, T, 3 * D) : ragged(lin_args(xin, D, D, L.in_w, L.in_b, e->QKV, 3 * D, M, 3 * D));
    if (!strip_gemm(c, q, false)) gemm(c, q);
    dec_attention(c, B, T, nullptr, once ? 1 : 0, rep);
  }
  // Chip-filling launches of the split modes: the rest of the layer in ONE launch (kernels/ffn_strip.hpp, TAIL form) -- the H1 tensor
  // between the out-projection kernel and the feed-forward kernel is not written and read back ("dec_tail", on by default)
  if (dec_tail_on(e, L, M)) {
    FfnArgs a;
    a.W1 = e->ffn_stream_of[L.l1_w]; a.b1 = L.l1_b; a.b2 = L.l2_b; a.gamma = L.n3_w; a.beta = L.n3_b; a.Y = xout; a.M = M;
    a.skip_lens = e->lens_dev; a.skip_rpg = T;
    a.AO = e->AO; a.Wo = e->gemm_stream_of[L.out_w]; a.bo = L.out_b; a.res = xin; a.g1 = L.n1_w; a.be1 = L.n1_b;
    a.cvec = e->cvec + (size_t)l * e->cfg.max_batch * D; a.rpg = T; a.g2 = L.n2_w; a.be2 = L.n2_b;
    // (LDS images row-swizzled like the persistent loop's: 1 476 -> 1 457 us per launch at 2 048 motions, r04a; the plain-image build is retired)
    if (lean) MLD_COUNTED(c, "dec_tail_x3", MLD_LAUNCH(dec_tail_l0_x3_kernel, dim3((M + 47) / 48), dim3(512), ffn_strip_lds_bytes<3>(), c.stream, a, rep));      // a.res = the positional table
    else MLD_COUNTED(c, "dec_tail_x3", MLD_LAUNCH((ffn_strip_x3_kernel<3, true, true>), dim3((M + 47) / 48), dim3(512), ffn_strip_lds_bytes<3>(), c.stream, a));
    return;
  }
  // out-proj + residual + norm1, then the 1-key cross-attention (a per-sample vector) + norm2
  GemmArgs o = lin_args(e->AO, D, D, L.out_w, L.out_b, e->H1, D, M, D);
  o.res = xin; o.ldres = D; o.g1 = L.n1_w; o.b1 = L.n1_b;
  o.cvec = e->cvec + (size_t)l * e->cfg.max_batch * D; o.ldcvec = D; o.rows_per_group = T;
  o.g2 = L.n2_w; o.b2 = L.n2_b;
  if (!strip_gemm(c, ragged(o), true)) gemm_ln(c, ragged(o));
  ffn_block(c, e->H1, xout, M, L.l1_w, L.l1_b, L.l2_w, L.l2_b, L.n3_w, L.n3_b, T);
}

void skip_linear(Ctx& c, const std::string& prefix, int i, const float* x, const float* skip, float* y, int M, int ragged_T = 0) {
  E* e = c.e;
  const int D = e->cfg.latent_dim;
  GemmArgs g;
  g.A = x; g.lda = D; g.K1 = D; g.A2 = skip; g.lda2 = D; g.K2 = D;
  g.W = P(e, prefix + ".linear_blocks." + std::to_string(i) + ".weight"); g.ldw = 2 * D;
  g.bias = P(e, prefix + ".linear_blocks." + std::to_string(i) + ".bias");
  g.Y = y; g.ldy = D; g.M = M; g.N = D;
  if (ragged_T > 0) { g.skip_lens = e->lens_dev; g.skip_rpg = ragged_T; }   // decoder: skip all-padding row tiles
  if (!strip_gemm(c, g, false)) gemm(c, g);
}

// MldVae.decode (mld_vae.py:186-248).  z [B, D]; lens_dev already holds the lengths.
// joints_only: nobody reads the features but feats2joints -- feats_out then receives [M][joints_pitch] rows (columns 0 .. joint_feat_cols - 1 + padding) where the
// joints-only final stage is built ("dec_lean"; *joints_pitch says which layout was written)
void decode_body(Ctx& c, const float* z, int B, int T, float* feats_out, bool joints_only = false, int* joints_pitch = nullptr) {
  E* e = c.e;
  const int D = e->cfg.latent_dim, NF = e->cfg.nfeats, nb = (e->cfg.num_layers - 1) / 2, M = B * T;
  const int L = vae_layers(e);
  // cross-attention with ONE memory token: softmax == 1, so the sub-layer adds
  // out_proj(v_proj(z_b)) to every frame of sample b (exact).  All layers at once.
  {
    GemmArgs v = lin_args(z, D, D, e->dec[0].cin_w + (size_t)2 * D * D, e->dec[0].cin_b + 2 * D, e->cv1, D, B, D);
    v.sW = (long long)e->dec_layer_stride; v.sBias = (long long)e->dec_layer_stride; v.sY = (long long)e->cfg.max_batch * D;
    gemm(c, v, L);
    GemmArgs o = lin_args(e->cv1, D, D, e->dec[0].cout_w, e->dec[0].cout_b, e->cvec, D, B, D);
    o.sA = (long long)e->cfg.max_batch * D; o.sW = (long long)e->dec_layer_stride; o.sBias = (long long)e->dec_layer_stride;
    o.sY = (long long)e->cfg.max_batch * D;
    gemm(c, o, L);
  }
  // time queries = zeros + PE rows (learned: mld_vae.py:216-222; sinusoidal: actor_vae.py:221-222)
  const float* pe = P(e, is_actor(e) ? "vae.decoder.sequence_pos_encoding.pe" : "vae.query_pos_decoder.pe");
  const bool lean0 = dec_l0_lean(e, B, T);
  if (lean0) {
    // layer 0 reads the table itself; what it needs per sample is the representative of its length (on device data: graphs stay keyed by shape)
    MLD_COUNTED(c, "length_reps", MLD_LAUNCH(length_reps_kernel, dim3(1), dim3(256), 0, c.stream, e->lens_dev, reinterpret_cast<int*>(e->len_rep), B, T));
  } else {
    MLD_COUNTED(c, "init_queries", MLD_LAUNCH(init_queries_kernel, dim3(std::min(2048, (M * D / 4 + 255) / 256)), dim3(256), 0, c.stream, e->X0, pe, B, T, D));
  }
  if (is_actor(e)) {
    // ActorAgnosticDecoder (actor_vae.py:224-235): plain stack, no skip links, no final LayerNorm
    const float* xin = lean0 ? pe : e->X0;
    for (int l = 0; l < L; ++l) {
      float* xout = (l & 1) ? e->Hb : e->Ha;
      dec_layer(c, l, xin, xout, B, T, l == 0, l == 0 && lean0);
      xin = xout;
    }
    GemmArgs f = lin_args(xin, D, D, P(e, "vae.decoder.final_layer.weight"), P(e, "vae.decoder.final_layer.bias"), feats_out, NF, M, NF);
    f.lens = e->lens_dev; f.rows_per_group = T;   // output[~mask.T] = 0 (actor_vae.py:231)
    gemm(c, f);
    return;
  }
  const float* x = lean0 ? pe : e->X0;
  for (int l = 0; l < nb; ++l) {
    dec_layer(c, l, x, e->S[l], B, T, l == 0, l == 0 && lean0);
    x = e->S[l];
  }
  dec_layer(c, nb, x, e->Ha, B, T, nb == 0, nb == 0 && lean0);
  for (int i = 0; i < nb; ++i) {
    skip_linear(c, "vae.decoder", i, e->Ha, e->S[nb - 1 - i], e->Hb, M, T);
    dec_layer(c, nb + 1 + i, e->Hb, e->Ha, B, T);
  }
  if (e->final_stream && staged_prec(e) == PREC_F16X3 && D == 256 && !e->trace_on && M > e->small_m) {
    // decoder.norm + final_layer + output[~mask.T] = 0 as one row-strip launch (kernels/final_strip.hpp, "final_strip")
    FinalStripArgs a;
    a.X = e->Ha; a.gamma = P(e, "vae.decoder.norm.weight"); a.beta = P(e, "vae.decoder.norm.bias"); a.W = e->final_stream;
    a.bias = P(e, "vae.final_layer.bias"); a.Y = feats_out; a.M = M; a.NF = NF; a.lens = e->lens_dev; a.rpg = T;
    if (joints_only && e->dec_lean && e->final_joints_stream) {
      // block 0 alone, rows of joint_feat_cols rounded up to 4 floats (HumanML3D: 67 + 1 pad, KIT-ML: 64): the same chunk order and split products per column as the full kernel -> the same bits
      a.W = e->final_joints_stream; a.NV = joint_feat_cols(e); a.NF = (a.NV + 3) / 4 * 4;
      if (joints_pitch) *joints_pitch = a.NF;
      MLD_COUNTED(c, "final_joints_x3", MLD_LAUNCH(final_joints_x3_kernel, dim3((M + kFinalStripRows - 1) / kFinalStripRows), dim3(512), final_strip_lds_bytes(), c.stream, a));
      return;
    }
    if (final_strip_blocks(e) == 2) MLD_COUNTED(c, "final_strip2_x3", MLD_LAUNCH(final_strip2_x3_kernel, dim3((M + kFinalStripRows - 1) / kFinalStripRows), dim3(512), final_strip_lds_bytes(), c.stream, a));
    else MLD_COUNTED(c, "final_strip_x3", MLD_LAUNCH(final_strip_x3_kernel, dim3((M + kFinalStripRows - 1) / kFinalStripRows), dim3(512), final_strip_lds_bytes(), c.stream, a));
    return;
  }
  MLD_COUNTED(c, "layernorm_rows", MLD_LAUNCH(layernorm_rows_kernel, dim3((M + 3) / 4), dim3(256), 0, c.stream, e->Ha, e->LNO, P(e, "vae.decoder.norm.weight"), P(e, "vae.decoder.norm.bias"), M));
  GemmArgs f = lin_args(e->LNO, D, D, P(e, "vae.final_layer.weight"), P(e, "vae.final_layer.bias"), feats_out, NF, M, NF);
  f.lens = e->lens_dev; f.rows_per_group = T;   // output[~mask.T] = 0 (mld_vae.py:245)
  gemm(c, f);
}

// One post-norm encoder layer over M = B*S token rows with a key-padding mask (cross_attention.py:259-272),
// on the decoder's kernels: packed in-proj GEMM, masked MFMA attention, out-proj + res + norm1, FFN.
void venc_layer(Ctx& c, const EncLayerP& L, const float* xin, float* xout, int B, int S) {
  E* e = c.e;
  const int D = e->cfg.latent_dim, M = B * S;
  {
    const GemmArgs q = lin_args(xin, D, D, L.in_w, L.in_b, e->QKV, 3 * D, M, 3 * D);
    if (!strip_gemm(c, q, false)) gemm(c, q);
  }
  dec_attention(c, B, S, e->lens2_dev);
  GemmArgs o = lin_args(e->AO, D, D, L.out_w, L.out_b, e->H1, D, M, D);
  o.res = xin; o.ldres = D; o.g1 = L.n1_w; o.b1 = L.n1_b;
  if (!strip_gemm(c, o, true)) gemm_ln(c, o);
  ffn_block(c, e->H1, xout, M, L.l1_w, L.l1_b, L.l2_w, L.l2_b, L.n2_w, L.n2_b, 0);
}

// MldVae.encode (mld_vae.py:124-184): feats [B,T,nfeats] -> mu, logvar (and latent = mu + exp(logvar)^0.5 * eps).
void encode_body(Ctx& c, const float* feats, int B, int T, const float* eps, float* latent, float* mu, float* logvar) {
  E* e = c.e;
  const int D = e->cfg.latent_dim, NF = e->cfg.nfeats, KP = (NF + 31) / 32 * 32, nb = (e->cfg.num_layers - 1) / 2;
  const int S = T + 2, M = B * S;
  // skel_embedding: K = 263 is padded to 288 so the MFMA K chunks stay full (zeros contribute nothing)
  MLD_COUNTED(c, "pad_cols", MLD_LAUNCH(pad_cols_kernel, dim3(std::min(4096, (B * T * KP + 255) / 256)), dim3(256), 0, c.stream, feats, e->FF, B * T, NF, KP));
  const bool actor = is_actor(e);
  {
    GemmArgs g = lin_args(e->FF, KP, KP, e->WskelP, P(e, actor ? "vae.encoder.skel_embedding.bias" : "vae.skel_embedding.bias"), e->LNO, D,
                          B * T, D);
    gemm(c, g);
  }
  // [token 0, token 1, frames] + positional rows (MldVae: global_motion_token + learned PE, mld_vae.py:150-163;
  // ActorVae: [mu_token, logvar_token] + sinusoidal PE, actor_vae.py:141-163)
  MLD_COUNTED(c, "enc_tokens", MLD_LAUNCH(enc_tokens_kernel, dim3(std::min(4096, (M * D / 4 + 255) / 256)), dim3(256), 0, c.stream, e->LNO,
         P(e, actor ? "vae.encoder.mu_token" : "vae.global_motion_token"), P(e, actor ? "vae.encoder.sequence_pos_encoding.pe" : "vae.query_pos_encoder.pe"), e->X0, B, T, D));
  if (actor) {
    // ActorAgnosticEncoder (actor_vae.py:164-170): stock nn.TransformerEncoder, no skip links, NO final norm
    const float* xin = e->X0;
    for (int l = 0; l < (int)e->venc.size(); ++l) {
      float* xout = (l & 1) ? e->Hb : e->Ha;
      venc_layer(c, e->venc[l], xin, xout, B, S);
      xin = xout;
    }
    MLD_COUNTED(c, "enc_finish", MLD_LAUNCH(enc_finish_kernel, dim3(B), dim3(256), 0, c.stream, xin, nullptr, nullptr, eps, latent, mu, logvar, S));
    return;
  }
  const float* x = e->X0;
  for (int l = 0; l < nb; ++l) {
    venc_layer(c, e->venc[l], x, e->S[l], B, S);
    x = e->S[l];
  }
  venc_layer(c, e->venc[nb], x, e->Ha, B, S);
  for (int i = 0; i < nb; ++i) {
    skip_linear(c, "vae.encoder", i, e->Ha, e->S[nb - 1 - i], e->Hb, M);
    venc_layer(c, e->venc[nb + 1 + i], e->Hb, e->Ha, B, S);
  }
  MLD_COUNTED(c, "enc_finish", MLD_LAUNCH(enc_finish_kernel, dim3(B), dim3(256), 0, c.stream, e->Ha, P(e, "vae.encoder.norm.weight"), P(e, "vae.encoder.norm.bias"), eps, latent, mu, logvar, S));
}

// pitch: floats between feature rows (0: nfeats); counter: where the kernel counts the non-finite joints it stores (nullptr: it does not)
void joints_body(Ctx& c, const float* feats, int B, int T, float* joints, int pitch = 0, unsigned* counter = nullptr) {
  E* e = c.e;
  if (pitch <= 0) pitch = e->cfg.nfeats;
  if (T <= 256) {
    MLD_COUNTED(c, "feats2joints", MLD_LAUNCH(feats2joints_kernel<256>, dim3(B), dim3(256), 0, c.stream, feats, joints, P(e, "mean"), P(e, "std"), T, pitch, e->cfg.njoints, counter));
  } else {
    MLD_COUNTED(c, "feats2joints", MLD_LAUNCH(feats2joints_kernel<512>, dim3(B), dim3(256), 0, c.stream, feats, joints, P(e, "mean"), P(e, "std"), T, pitch, e->cfg.njoints, counter));
  }
}

}  // namespace
