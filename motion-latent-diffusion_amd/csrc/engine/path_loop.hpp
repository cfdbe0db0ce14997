// The reverse loop of the latent models (configs 1-3, 5): the per-launch denoiser chain on its two kernel families, which family or loop kernel a call
// takes, and the launches of the persistent loop and the cluster loop.
// Part of libmldhip's single translation unit; include order: see mldhip.hip.  Internal linkage throughout (anonymous namespace) except the handle type itself.
#pragma once

namespace {

// ---- denoiser layer pipeline (4 launches per encoder layer) on one of two kernel families -------------------------
//   latency    (kernels/tile32.hpp): everything loaded before the first MFMA, split-K slabs summed by the consumer;
//              M = 6B <= a few hundred rows (one bs-64 request: 384).
//   throughput (kernels/strip.hpp + the 32x64 staged GEMM): A strip resident, weights streamed, 3 workgroups per CU,
//              no split-K (one raw slab per GEMM); M >= strip_min_rows (several requests coalesced into one chain).
// Both use the same data flow: a GEMM with K > 256 or a following LayerNorm leaves RAW fp32 partial slabs, and the
// consumer's A prologue applies slab sum + bias + residual + LayerNorm (or the 3-token attention).

void tile32(Ctx& c, const Tile32Args& a_, int nz) {
  Tile32Args a = a_;
  a.trace = c.e->trace_on;
  // 16-row K-split tiles for the narrow (N = 256) GEMMs: more workgroups, fewer bytes and MFMAs per CU
  const bool mt16 = a.N <= 256 && ((a.M + 15) / 16) * ((a.N + 63) / 64) * nz <= 256;
  const int mt = mt16 ? 16 : 32;
  dim3 grid((a.M + mt - 1) / mt, (a.N + 63) / 64, nz);
  const int ns = a.src[0].attn_R > 0 ? 0 : a.src[0].nsplit;
  const int prec = latency_prec(c.e);
  if (prec == PREC_F16X3 && c.e->arena_x3 && a.W >= c.e->arena && a.W < c.e->arena + c.e->arena_floats &&
      (a.W - c.e->arena) % 32 == 0 && a.ldw % 32 == 0) {
    a.W = c.e->arena_x3 + (a.W - c.e->arena);
    a.w_split = 1;
  }
  const bool attn = a.src[0].attn_R > 0, two = ns > 0 && nz > a.nz0;
#define MLD_T32P(MT, NS, MODE)                                                                                   \
  do {                                                                                                           \
    if (a.trace && prec == PREC_F16X3) MLD_COUNTED(c, "gemm_tile32", MLD_LAUNCH((gemm_tile32_kernel<MT, NS, true, PREC_F16X3, MODE>), grid, dim3(512), kT32LdsBytes, c.stream, a)); \
    else if (a.trace) MLD_COUNTED(c, "gemm_tile32", MLD_LAUNCH((gemm_tile32_kernel<MT, NS, true, PREC_F32, MODE>), grid, dim3(512), kT32LdsBytes, c.stream, a));   \
    else if (prec == PREC_BF16) MLD_COUNTED(c, "gemm_tile32", MLD_LAUNCH((gemm_tile32_kernel<MT, NS, false, PREC_BF16, MODE>), grid, dim3(512), kT32LdsBytes, c.stream, a)); \
    else if (prec == PREC_F16X3) MLD_COUNTED(c, "gemm_tile32", MLD_LAUNCH((gemm_tile32_kernel<MT, NS, false, PREC_F16X3, MODE>), grid, dim3(512), kT32LdsBytes, c.stream, a)); \
    else MLD_COUNTED(c, "gemm_tile32", MLD_LAUNCH((gemm_tile32_kernel<MT, NS, false, PREC_F32, MODE>), grid, dim3(512), kT32LdsBytes, c.stream, a));               \
  } while (0)
#define MLD_T32(MT, NS)                                                                                          \
  do { if ((NS) == 0 ? attn : two) MLD_T32P(MT, NS, 1); else MLD_T32P(MT, NS, 0); } while (0)
#define MLD_T32_NS(MT)                                                                                           \
  switch (ns) {                                                                                                  \
    case 0: MLD_T32(MT, 0); break;                                                                               \
    case 1: MLD_T32(MT, 1); break;                                                                               \
    case 2: MLD_T32(MT, 2); break;                                                                               \
    case 4: MLD_T32(MT, 4); break;                                                                               \
    default: c.rc = c.e->fail(MLDHIP_EINVAL, "tile32: unsupported slab count %d", ns); return;                   \
  }
  if (mt16) { MLD_T32_NS(16) } else { MLD_T32_NS(32) }
#undef MLD_T32_NS
#undef MLD_T32
#undef MLD_T32P
}

// throughput family: K = 256 (one source) or 512 (skip linear: src[0] | src[1]); src[0] plain, 1- or 2-slab combine, or attention.
// Wide GEMMs (N a multiple of 128, N >= 512: QKV, FFN1) take 32 x 128 tiles: half as many workgroups repeat one A prologue.
// (QKV alone is faster on 32 x 64 tiles at 1 920 rows -- 13.5 vs 14.9 us, one resident round of 720 workgroups -- but with four
// calls in flight the end-to-end rate is 2 % LOWER: 12.77 vs 13.04 k motions/s, profiles/r02_strip_options_ab.json.)
void strip(Ctx& c, const Tile32Args& a_, int nsrc) {
  Tile32Args a = a_;
  a.trace = c.e->trace_on;
  const bool attn = a.src[0].attn_R > 0;
  const int ns = attn ? 0 : a.src[0].nsplit;
  const bool wide = !attn && nsrc == 1 && a.N % 128 == 0 && a.N >= 512;      // (round 2's "strip_wide" / "strip_waves" / "strip_ffn2_split" knobs were retired in round 6: the settled forms are how it works)
  const dim3 grid((a.M + 31) / 32, wide ? a.N / 128 : (a.N + 63) / 64, 1);
  const int prec = loop_prec(c.e);
#define MLD_STRIP(NS, NSRC, ATTN, ACT, CT, NW)                                                                                     \
  do {                                                                                                                             \
    if (prec == PREC_BF16) MLD_COUNTED(c, "gemm_strip", MLD_LAUNCH((gemm_strip_kernel<NS, NSRC, ATTN, PREC_BF16, ACT, CT, NW>), grid, dim3(64 * NW), (strip_lds_bytes<NSRC, CT>()), c.stream, a)); \
    else MLD_COUNTED(c, "gemm_strip", MLD_LAUNCH((gemm_strip_kernel<NS, NSRC, ATTN, PREC_F32, ACT, CT, NW>), grid, dim3(64 * NW), (strip_lds_bytes<NSRC, CT>()), c.stream, a));           \
  } while (0)
  // 8 waves per workgroup (one 16-row tile per wave)
#define MLD_STRIP_W(NS, NSRC, ATTN, ACT)                                            \
  do {                                                                              \
    if (wide) MLD_STRIP(NS, NSRC, ATTN, ACT, 2, 8);                                 \
    else MLD_STRIP(NS, NSRC, ATTN, ACT, 1, 8);                                      \
  } while (0)
  if (a.trace) {                              // measurement builds (mldhip_profile_trace): the fp32 8-wave kernels of the encoder layer
    if (prec != PREC_F32 || nsrc != 1) { c.rc = c.e->fail(MLDHIP_EINVAL, "strip: traces exist for the fp32 8-wave layer kernels only"); return; }
    if (attn) MLD_COUNTED(c, "gemm_strip(trace)", MLD_LAUNCH((gemm_strip_kernel<0, 1, true, PREC_F32, 0, 1, 8, true>), grid, dim3(512), (strip_lds_bytes<1, 1>()), c.stream, a));
    else if (wide && ns == 1 && a.act == 1) MLD_COUNTED(c, "gemm_strip(trace)", MLD_LAUNCH((gemm_strip_kernel<1, 1, false, PREC_F32, 1, 2, 8, true>), grid, dim3(512), (strip_lds_bytes<1, 2>()), c.stream, a));
    else if (wide && ns == 2 && a.act == 0) MLD_COUNTED(c, "gemm_strip(trace)", MLD_LAUNCH((gemm_strip_kernel<2, 1, false, PREC_F32, 0, 2, 8, true>), grid, dim3(512), (strip_lds_bytes<1, 2>()), c.stream, a));
    else c.rc = c.e->fail(MLDHIP_EINVAL, "strip: no traced build of this shape");
    return;
  }
  if (a.act != 0 && !(a.act == 1 && ns == 1 && nsrc == 1 && !attn)) { c.rc = c.e->fail(MLDHIP_EINVAL, "strip: activation %d is built for the FFN1 shape only", a.act); return; }
  if (attn && nsrc == 1) MLD_STRIP(0, 1, true, 0, 1, 8);
  else if (ns == 0 && nsrc == 1) MLD_STRIP_W(0, 1, false, 0);
  else if (ns == 1 && nsrc == 1 && a.act == 1) MLD_STRIP_W(1, 1, false, 1);
  else if (ns == 1 && nsrc == 1) MLD_STRIP_W(1, 1, false, 0);
  else if (ns == 2 && nsrc == 1) MLD_STRIP_W(2, 1, false, 0);
  else if (ns == 1 && nsrc == 2) MLD_STRIP(1, 2, false, 0, 1, 8);
  else if (ns == 2 && nsrc == 2) MLD_STRIP(2, 2, false, 0, 1, 8);
  else { c.rc = c.e->fail(MLDHIP_EINVAL, "strip: unsupported source (slabs %d, segments %d)", ns, nsrc); return; }
#undef MLD_STRIP_W
#undef MLD_STRIP
}

// ---- which kernels run the reverse loop of a call: the two families above, the persistent loop, the cluster loop -------------------------
// Which family runs the reverse loop of a call is a measured table (tools/ab_crossover.py -> profiles/r04_loop_crossover.json; ms per loop-only
// call of B motions, MI355X):          B =    64    128    192    256    320    640  | exact fp32:  256    640   1 024  1 280  1 536
//   latency kernels (tile32.hpp)           11.1   15.2   19.0   21.0     --     --  |             27.2     --     --     --     --
//   column-split throughput (strip.hpp)    18.3   18.4   23.2   25.4   26.3   40.7  |             25.4   40.5   59.9   74.4   87.1
//   persistent loop (loop_fused.hpp)       19.8   19.5   19.3   19.2   19.1   18.9  |             73.0   73.2   73.5   73.7   73.8
// Split-f16 mode: the latency kernels (split-f16 MFMAs under "tile_x3") up to 191 motions, the persistent loop from 192 -- the
// column-split family, whose loop arithmetic is fp32 in that mode, never wins there.  Exact fp32: latency kernels below 128 motions
// ("strip_min_rows" 768), column-split up to 1 279, persistent loop from 1 280.
bool use_strip(const E* e, int rows) {
  if (e->loop_kernel == 2) return true;
  if (e->loop_kernel != 0) return false;
  if (latency_prec(e) == PREC_F16X3 && rows < 6 * 256) return false;      // split-f16 latency kernels beat the fp32 column-split ones wherever both run
  return rows >= e->strip_min_rows;
}

// ---- sample-major persistent loop (kernels/loop_fused.hpp): built for the configurations the released checkpoints use
bool fused_built(const E* e) {
  return !is_novae(e) && e->cfg.latent_dim == 256 && e->cfg.ff_size == 1024 && e->cfg.num_heads == 4 && loop_prec(e) == PREC_F32;
}
bool use_fused(const E* e, int B) {
  // auto: the persistent loop takes the same time for any batch up to 8 x #CUs motions -- 19 ms on split-f16 MFMAs, 73 ms on exact-fp32
  // ones (r04) -- see the measured table at use_strip above: cross-over by operand format
  const int auto_min = e->fused_min_batch > 0 ? e->fused_min_batch : (fused_split(e) ? 192 : 1280);
  return e->loop_ips > 0 && (e->loop_kernel == 3 || (e->loop_kernel == 0 && B >= auto_min));
}

// ---- cluster loop (kernels/loop_cluster.hpp): one bs-64 request (up to 8 x kClMaxClusters motions) as ONE launch of 12-workgroup clusters
constexpr int kCusPerXcd = 32;      // MI355X: 8 XCDs x 32 CUs; partitions (CPX / DPX / QPX) expose whole XCDs

// column groups per token of a cluster call: 8 (24 workgroups per cluster: the feed-forward block on twice the CUs) while every cluster still has an XCD's 32 CUs
// to itself (up to 8 clusters = 64 motions), 4 (12 workgroups) above; option "cluster_groups" 4 / 8 forces one (8 only where it fits)
int cluster_groups(const E* e, int B) {
  const int xcds = std::max(1, std::min(8, e->num_cus / kCusPerXcd));
  const bool fits8 = (B + 7) / 8 <= 8 && 24 * ((B + 7) / 8) <= e->num_cus && 24 * (((B + 7) / 8 + xcds - 1) / xcds) <= e->num_cus / xcds;
  if (e->cluster_groups == 4 || !fits8) return 4;
  return 8;
}

bool use_cluster(const E* e, int B) {
  if (!e->cl_stream || !fused_split(e) || e->cluster_failed || e->cluster_foreign || B > kClMaxCall || B > e->cfg.max_batch) return false;
  // every workgroup of a launch needs a CU of its own (125 KB of LDS each) at the same time: the biggest launch of the call against the device's CUs --
  // in total AND per XCD (advisor r5): workgroups go round the XCDs, so the clusters that share a physical XCD (ceil(clusters / XCDs)) must fit its 32 CUs;
  // a partitioned device (2 XCDs, 64 CUs) with 5 clusters x 12 workgroups would put 36 workgroups on a 32-CU XCD and time out on every call
  const int nm = std::min(B, e->cluster_chunk);
  const int members = 3 * cluster_groups(e, nm), ncl = (nm + 7) / 8;
  if (members * ncl > e->num_cus) return false;
  const int xcds = std::max(1, std::min(8, e->num_cus / kCusPerXcd)), per_xcd = e->num_cus / xcds;
  if (members * ((ncl + xcds - 1) / xcds) > per_xcd) return false;
  return e->loop_kernel == 4 || (e->loop_kernel == 0 && B <= e->cluster_max_batch);
}

// sticky status word [2] of any workspace context: a cluster launch of this handle ran into its wait bound since the last look (synchronous: call it behind a sync); clears it
bool cluster_timed_out(E* e) {
  if (!e->cl_flags) return false;
  const size_t words = (size_t)std::min<size_t>(kClMaxClusters, (e->cfg.max_batch + 7) / 8) * kClFlagWords;
  size_t off = 0;
  bool found = false, hit = false;
  for (auto& cv : e->carve) if (cv.first == &e->cl_flags) { off = cv.second; found = true; }
  if (!found) return false;
  for (auto& x : e->ctxs) {
    unsigned st = 0;
    unsigned* w = x.ws ? reinterpret_cast<unsigned*>(x.ws + off) + words + 2 : nullptr;
    if (w && hipMemcpy(&st, w, sizeof st, hipMemcpyDeviceToHost) == hipSuccess && st != 0u) { hit = true; (void)hipMemset(w, 0, sizeof st); }
  }
  return hit;
}

// ---- the per-launch denoiser chain -------------------------
ASrc plain_src(const float* base, int ld) {
  ASrc s;
  s.base = base; s.ld = ld;
  return s;
}
ASrc combine_src(const float* slabs, int nsplit, long long pstride, const float* bias, const float* res,
                 const float* gamma, const float* beta, float* out) {
  ASrc s;
  s.base = slabs; s.ld = 256; s.nsplit = nsplit; s.pstride = pstride; s.bias = bias; s.res = res; s.ldres = 256;
  s.gamma = gamma; s.beta = beta; s.out = out; s.ldout = 256;
  return s;
}

// The denoiser workspace as one chain sees it: rows [0, 3R) of every row-indexed buffer.
struct DenView {
  float *X0, *QKV, *FF, *H1, *Ha, *Po, *Pf, *Ps, *S[8], *lat;
  int R;            // samples in the CFG batch (uncond half first)
  bool strip;       // throughput kernel family (see above)
  int ffn_slabs, skip_slabs;   // raw partial slabs FFN2 / the skip linear leave behind
};

DenView den_view(E* e, int R) {
  DenView v;
  v.X0 = e->X0; v.QKV = e->QKV; v.FF = e->FF; v.H1 = e->H1; v.Ha = e->Ha;
  v.Po = e->Po; v.Pf = e->Pf; v.Ps = e->Ps;
  for (int i = 0; i < 8; ++i) v.S[i] = e->S[i];
  v.lat = e->lat;
  v.R = R;
  v.strip = use_strip(e, 3 * R);
  // throughput kernels: K slices of FFN2 no narrower than 256 (the staged GEMM takes K in {256, 512, 1024})
  v.ffn_slabs = v.strip ? std::min(2, e->cfg.ff_size / 256) : e->cfg.ff_size / 256;
  v.skip_slabs = v.strip ? 1 : 2;
  return v;
}
long long den_slab(const E* e) { return (long long)6 * e->cfg.max_batch * 256; }

// QKV projection; `x` describes how the layer input rows are obtained (and where they are written back).
void den_qkv(Ctx& c, const DenView& v, const EncLayerP& L, const ASrc& x) {
  Tile32Args a;
  a.src[0] = x; a.nz0 = 1; a.W = L.in_w; a.ldw = 256; a.bias = L.in_b; a.Y = v.QKV; a.ldy = 768; a.M = 3 * v.R; a.N = 768;
  if (v.strip) strip(c, a, 1); else tile32(c, a, 1);
}
// out-projection of the 3-token self-attention (computed while the A tile is assembled) -> raw slab Po
void den_outproj(Ctx& c, const DenView& v, const EncLayerP& L) {
  Tile32Args a;
  a.src[0].base = v.QKV; a.src[0].attn_R = v.R;
  a.nz0 = 1; a.W = L.out_w; a.ldw = 256; a.P = v.Po; a.pstride = 0; a.M = 3 * v.R; a.N = 256;
  if (v.strip) strip(c, a, 1); else tile32(c, a, 1);
}
// h1 = LN1(x + out_proj) assembled on load (written to H1), FF = gelu(h1 W1^T + b1)
void den_ffn1(Ctx& c, const DenView& v, const EncLayerP& L, const float* xn) {
  const int F = c.e->cfg.ff_size;
  Tile32Args a;
  a.src[0] = combine_src(v.Po, 1, 0, L.out_b, xn, L.n1_w, L.n1_b, v.H1);
  a.nz0 = 1; a.W = L.l1_w; a.ldw = 256; a.bias = L.l1_b; a.act = 1; a.Y = v.FF; a.ldy = F; a.M = 3 * v.R; a.N = F;
  if (v.strip) strip(c, a, 1); else tile32(c, a, 1);
}
// FFN2 -> raw slabs Pf (ff_size/256 K-slices on the latency kernels, one full-K slab on the throughput kernels);
// bias, residual and norm2 are applied by whoever reads them
void den_ffn2(Ctx& c, const DenView& v, const EncLayerP& L) {
  const int F = c.e->cfg.ff_size;
  if (v.strip) {
    // `ffn_slabs` K slices (blockIdx.z) -> as many raw slabs: with one slice the N = 256 GEMM has M/32 x 4 workgroups, fewer
    // than CUs at M <= 2 048, each walking all 32 K chunks behind a 4-deep prefetch ring (latency bound: 51 TF measured)
    const int nz = v.ffn_slabs, Kz = F / nz;
    GemmArgs g = lin_args(v.FF, F, Kz, L.l2_w, nullptr, v.Pf, 256, 3 * v.R, 256);
    g.ldw = F; g.sA = Kz; g.sW = Kz; g.sY = den_slab(c.e);
    gemm_tile_32x64(c, g, loop_prec(c.e), nz);
    return;
  }
  Tile32Args a;
  a.src[0] = plain_src(v.FF, F);
  a.nz0 = F / 256; a.W = L.l2_w; a.ldw = F; a.P = v.Pf; a.pstride = den_slab(c.e); a.M = 3 * v.R; a.N = 256;
  tile32(c, a, F / 256);
}
ASrc den_layer_output(E* e, const DenView& v, const EncLayerP& L, float* write_back) {   // LN2(sum Pf + b2 + h1)
  return combine_src(v.Pf, v.ffn_slabs, den_slab(e), L.l2_b, v.H1, L.n2_w, L.n2_b, write_back);
}

// SkipTransformerEncoder over the 3-token sequences (cross_attention.py:41-64).  Leaves the last layer's
// FFN2 slabs in Pf and its norm1 output in H1; the caller applies norm2 + encoder.norm (FinalArgs).
void denoiser_body(Ctx& c, const DenView& v) {
  E* e = c.e;
  const int nb = (e->cfg.num_layers - 1) / 2, L = e->cfg.num_layers;
  ASrc x = plain_src(v.X0, 256);
  const float* xn = v.X0;                  // where the (normalised) layer input lives, for the norm1 residual
  for (int l = 0; l < L; ++l) {
    const EncLayerP& P_ = e->den[l];
    den_qkv(c, v, P_, x);
    den_outproj(c, v, P_);
    den_ffn1(c, v, P_, xn);
    den_ffn2(c, v, P_);
    if (l + 1 == L) break;
    if (l < nb) {
      // next layer input = LN2(...), kept in S[l] for the skip connection (written by the next QKV prologue)
      x = den_layer_output(e, v, P_, v.S[l]);
      xn = v.S[l];
    } else {
      // Linear(cat[x, skip]) as two K segments (cross_attention.py:56-58): segment 0 assembles x = LN2(...) on load,
      // segment 1 reads the stored skip activation; the bias is added by the next QKV prologue.
      const int i = l - nb;
      Tile32Args a;
      a.src[0] = den_layer_output(e, v, P_, nullptr);
      a.src[1] = plain_src(v.S[nb - 1 - i], 256);
      a.nz0 = 1;
      a.W = P(e, "denoiser.encoder.linear_blocks." + std::to_string(i) + ".weight"); a.ldw = 512;
      a.P = v.Ps; a.pstride = den_slab(e); a.M = 3 * v.R; a.N = 256;
      if (v.strip) strip(c, a, 2); else tile32(c, a, 2);
      x = combine_src(v.Ps, v.skip_slabs, den_slab(e), P(e, "denoiser.encoder.linear_blocks." + std::to_string(i) + ".bias"), nullptr,
                      nullptr, nullptr, v.Ha);
      xn = v.Ha;
    }
  }
}

FinalArgs den_final_args(E* e, const DenView& v) {
  const EncLayerP& L = e->den.back();
  FinalArgs f;
  f.P = v.Pf; f.nsplit = v.ffn_slabs; f.pstride = den_slab(e);
  f.b2 = L.l2_b; f.H1 = v.H1; f.g2 = L.n2_w; f.be2 = L.n2_b;
  f.gf = P(e, "denoiser.encoder.norm.weight"); f.bef = P(e, "denoiser.encoder.norm.bias");
  return f;
}

// the whole reverse loop (or its first `n` steps: finalize's range probe) as one persistent launch: a workgroup per 8 motions (kernels/loop_fused.hpp)
void launch_fused_loop(Ctx& c, const float* init_lat, int B, int n, float guidance) {
  E* e = c.e;
  LoopArgs a;
  const bool x3 = fused_split(e);
  a.stream = x3 ? e->loop_stream_x3 : e->loop_stream; a.ips = e->loop_ips; a.small = e->loop_small; a.T1 = e->T1; a.TP = e->TP; a.init_lat = init_lat;
  a.lat = e->lat; a.skip = e->FS; a.ddim = e->loop_ddim; a.B = B; a.L = e->cfg.num_layers; a.n = n;
  a.guidance = guidance; a.init_sigma = 1.0f;
  a.traj = traj_table(e);
  a.lean = e->loop_lean;
  const dim3 grid((B + 7) / 8);
  if (e->from_on) {                     // mldhip_sample_many_from: the from-forms on the context's start table, with or without noise
    a.starts = e->starts_dev;
    if (eta_live(e)) {
      a.eta = e->loop_eta; a.keys = e->keys_dev;
      if (x3) MLD_COUNTED(c, "den_loop", MLD_LAUNCH((den_loop_kernel<true, kLoopFromEta>), grid, dim3(512), kLoopLdsBytes, c.stream, a));
      else MLD_COUNTED(c, "den_loop", MLD_LAUNCH((den_loop_kernel<false, kLoopFromEta>), grid, dim3(512), kLoopLdsBytes, c.stream, a));
    } else if (x3) MLD_COUNTED(c, "den_loop", MLD_LAUNCH((den_loop_kernel<true, kLoopFrom>), grid, dim3(512), kLoopLdsBytes, c.stream, a));
    else MLD_COUNTED(c, "den_loop", MLD_LAUNCH((den_loop_kernel<false, kLoopFrom>), grid, dim3(512), kLoopLdsBytes, c.stream, a));
  } else
  if (eta_live(e)) {                    // stochastic DDIM: the step's second table row + the call's noise keys
    a.eta = e->loop_eta; a.keys = e->keys_dev;
    if (x3) MLD_COUNTED(c, "den_loop", MLD_LAUNCH((den_loop_kernel<true, kLoopEta>), grid, dim3(512), kLoopLdsBytes, c.stream, a));
    else MLD_COUNTED(c, "den_loop", MLD_LAUNCH((den_loop_kernel<false, kLoopEta>), grid, dim3(512), kLoopLdsBytes, c.stream, a));
  } else
#if defined(MLDHIP_HOOKS)
  if (x3 && e->fused_dbg == 5) { a.trace = reinterpret_cast<unsigned long long*>(e->trace_buf); MLD_COUNTED(c, "den_loop", MLD_LAUNCH((den_loop_kernel<true, 5>), grid, dim3(512), kLoopLdsBytes, c.stream, a)); }
  else
#endif
  if (x3) MLD_COUNTED(c, "den_loop", MLD_LAUNCH((den_loop_kernel<true>), grid, dim3(512), kLoopLdsBytes, c.stream, a));
  else MLD_COUNTED(c, "den_loop", MLD_LAUNCH((den_loop_kernel<false>), grid, dim3(512), kLoopLdsBytes, c.stream, a));
}

// the whole reverse loop (or its first `n` steps) of up to 8 x kClMaxClusters motions as one launch of clusters (kernels/loop_cluster.hpp)
// motions [s_base, s_base + nm) of a call of B
void launch_cluster_chunk(Ctx& c, const float* init_lat, int B, int s_base, int nm, int n, float guidance) {
  E* e = c.e;
  ClusterArgs a;
  const int cg = cluster_groups(e, nm), members = 3 * cg;
  a.s_base = s_base; a.s_end = s_base + nm;
  a.timeout = e->cluster_timeout ? (unsigned)e->cluster_timeout : kClTimeoutTicks; a.mute = e->cluster_mute;
  a.stream = e->cl_stream;
  a.wave_off = e->cl_wave_off_dev + (cg == 8 ? 32 : 0);
  a.small = e->loop_small; a.T1 = e->T1; a.TP = e->TP; a.init_lat = init_lat; a.lat = e->lat; a.park = e->cl_park; a.ddim = e->loop_ddim;
  a.xbuf = e->cl_xbuf;
  a.host_status = e->cl_host_status;
  a.ncl = (nm + 7) / 8;
  a.flags = reinterpret_cast<unsigned*>(e->cl_flags);
  a.status = a.flags + (size_t)std::min<size_t>(kClMaxClusters, (e->cfg.max_batch + 7) / 8) * kClFlagWords;
  a.B = B; a.L = e->cfg.num_layers; a.n = n; a.guidance = guidance; a.init_sigma = 1.0f;
  a.traj = traj_table(e);
#if defined(MLDHIP_SIM)
  a.xslots = std::min(a.ncl, 8);          // the simulator creates a fiber per work-item of every block: no idle XCD slots
#else
  a.xslots = 8;                           // block b -> XCD b % 8 (observed placement): a cluster's members share a slot
#endif
  // every polled word is zero at the start of every call (Guideline 16 "Re-initialise every call")
  const int words = (int)(a.status - a.flags) + 2;        // the flags and the two per-launch status words (status[2] is sticky: cluster_timed_out)
  if (e->sample_part != 2)
  MLD_LAUNCH(clear_cluster_flags_kernel, dim3(1), dim3(256), 0, c.stream, a.flags, words);      // (a kernel, NOT a memset node: replays of a captured hipMemsetAsync left address-like words here on this runtime, DESIGN.md 3a -- the entry check of the kernel now catches such a launch)
#if defined(MLDHIP_HOOKS)
  if (e->cluster_stale && e->sample_part != 2) MLD_LAUNCH(poke_cluster_flag_kernel, dim3(1), dim3(1), 0, c.stream, a.flags + kFlagH * kClFlagLine + 3, 77u);
#endif
  if (e->sample_part == 1) return;               // (the pipelined form captures what precedes the launch as a graph of its own)
  const dim3 grid((unsigned)(a.xslots * members * ((a.ncl + a.xslots - 1) / a.xslots)));
  // the kernel by (eta, "cluster_wt", column groups)
  using K = void (*)(ClusterArgs);
  const K plain[2][2] = {{den_cluster_kernel<false, 4>, den_cluster_kernel<false, 8>}, {den_cluster_kernel<true, 4>, den_cluster_kernel<true, 8>}};
  const K eta[2][2] = {{den_cluster_eta_kernel<false, 4>, den_cluster_eta_kernel<false, 8>}, {den_cluster_eta_kernel<true, 4>, den_cluster_eta_kernel<true, 8>}};
  if (eta_live(e)) { a.eta = e->loop_eta; a.keys = e->keys_dev; }      // stochastic DDIM: the step's second table row + the call's noise keys
  const K from[2][2] = {{den_cluster_from_kernel<false, 4>, den_cluster_from_kernel<false, 8>}, {den_cluster_from_kernel<true, 4>, den_cluster_from_kernel<true, 8>}};
  const K from_eta[2][2] = {{den_cluster_from_eta_kernel<false, 4>, den_cluster_from_eta_kernel<false, 8>}, {den_cluster_from_eta_kernel<true, 4>, den_cluster_from_eta_kernel<true, 8>}};
  if (e->from_on) a.starts = e->starts_dev;                            // mldhip_sample_many_from: the from-forms on the context's start table
  const K k = (e->from_on ? (eta_live(e) ? from_eta : from) : (eta_live(e) ? eta : plain))[e->cluster_wt ? 1 : 0][cg == 8 ? 1 : 0];
  MLD_COUNTED(c, "den_cluster", MLD_LAUNCH_CORESIDENT(k, grid, dim3(512), kClLdsBytes, c.stream, a));
}

// up to 128 motions: one launch; up to kClMaxCall = 256: two launches one after the other on the call's stream (they share the exchange regions and flags; 2 x 7.6 ms
// against the sample-major loop's flat 18.7 ms) -- never side by side: 2 x 192 workgroups are not co-resident
void launch_cluster_loop(Ctx& c, const float* init_lat, int B, int n, float guidance) {
  const int chunk = c.e->cluster_chunk;          // 128 (hooks / simulator builds: "cluster_chunk" makes the two-launch path testable on a few motions)
  for (int s = 0; s < B && !c.rc; s += chunk) launch_cluster_chunk(c, init_lat, B, s, std::min(chunk, B - s), n, guidance);
}

}  // namespace
