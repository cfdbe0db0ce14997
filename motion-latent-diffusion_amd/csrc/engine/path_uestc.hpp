// The UESTC recognition ST-GCN (mldhip_uestc_recognize; config fields uestc_rec = 1, uestc_max_motions, uestc_classes): rot6d motions [B][24][6][T] behind
// any four strides -> logits [B][NC] and features [B][256], the math of STGCN in eval mode as UESTCMetrics runs it (include/mldhip.h has the contract;
// kernels/stgcn.hpp the layouts and the kernels).
//
// FINALIZE folds on the host, in double, everything that is affine in eval mode (build_uestc_tables):
//   data_bn -> scale / offset [24][6];  Am_i = A * edge_importance[i];
//   graph convolution: the mix runs FIRST (z[w][k Cin + c] = sum_v Am[k][v][w] x[v][c]), so the 1x1 convolution is one GEMM of K = 3 Cin on z with the
//     weight [Cout][k Cin + c] = s1[co] W[k Cout + co][c] (s1 / o1: the BN behind it) and the bias TABLE [w][co] = s1[co] sum_k b[k Cout + co] colsum_k[w] + o1[co];
//   temporal convolution: tap-major [Cout][9 C] with the BN behind it folded into weights and bias;  residual convolution (blocks 4, 7) likewise;
//   every K is zero-padded to a multiple of 128 (18 -> 128, 192 -> 256, 576 -> 640, 64 -> 128);  F16X3 handles get the split image of the whole table.
// A CALL runs chunks of as many motions as the workspace holds at the call's T.  Per chunk: input stage (gather, data_bn, block 0's mix), then per block
//   [mix] -> graph GEMM (+ bias table, ReLU) into the padded H -> [residual GEMM into R] -> temporal GEMM over overlapping rows of H (+ bias, + residual, ReLU)
//   into the padded input of the next block;  then the pool + head kernel.  Zero rows of a padded buffer are rewritten only when its geometry changes.
// Issued eagerly.  Part of libmldhip's single translation unit; include order: see mldhip.hip.
#pragma once

namespace {

int uestc_pad128(int k) { return (k + 127) / 128 * 128; }
// floats per motion of a padded buffer / of the compact graph operand at T frames (upper bounds over the three stages: T, ceil(T / 2), ceil(T / 4))
size_t uestc_pad_floats(int T) { return (size_t)kStgJoints * (128 * (size_t)T + 2304); }
size_t uestc_z_floats(int T) { return (size_t)kStgJoints * (256 * (size_t)T + 576); }
#if defined(MLDHIP_SIM)
constexpr int kUestcChunk = 2;       // (the functional simulator's tests reach the chunk loop with 3 motions)
#else
constexpr int kUestcChunk = 64;      // motions the workspace holds at T = max_frames (a shorter call fits more per chunk; the numbers do not depend on it):
                                     // 64 x 24 x 60 = 92 160 rows = 1 440 row tiles at UESTC's length, several per CU
#endif
constexpr size_t kUestcWsCap = (size_t)128 << 20;      // ... but no more than 512 MB of workspace (33 motions at 196 frames), and at least one motion
constexpr size_t kUestcSlack = 2 * kStgFeat;

bool uestc_x3(const E* e) { return e->cfg.precision == MLDHIP_PREC_F16X3 && e->uestc_tabs_x3 && e->probe[kProbeUestc].ok; }      // the verdict of finalize's range probe

int build_uestc_tables(Ctx& c) {
  E* e = c.e;
  if (!e->cfg.uestc_rec || !e->group_ready[kGroupUestc]) return MLDHIP_OK;
  const std::string p = "uestc_rec.";
  auto host = [&](const std::string& key, std::vector<double>& out) -> int {
    const Param& q = e->params[e->index.at(p + key)];
    std::vector<float> f(q.numel);
    HIP_TRY(e, hipMemcpy(f.data(), e->arena + q.offset, q.numel * sizeof(float), hipMemcpyDeviceToHost));
    out.assign(f.begin(), f.end());
    return MLDHIP_OK;
  };
  // BN in eval mode: y = x s + o
  auto bn = [&](const std::string& q, std::vector<double>& s, std::vector<double>& o) -> int {
    std::vector<double> g, b, m, v;
    if (int rc = host(q + "weight", g)) return rc;
    if (int rc = host(q + "bias", b)) return rc;
    if (int rc = host(q + "running_mean", m)) return rc;
    if (int rc = host(q + "running_var", v)) return rc;
    s.resize(g.size()); o.resize(g.size());
    for (size_t i = 0; i < g.size(); ++i) { s[i] = g[i] / std::sqrt(v[i] + 1e-5); o[i] = b[i] - m[i] * s[i]; }
    return MLDHIP_OK;
  };
  std::vector<float> tab;
  auto place = [&](size_t n) { const size_t off = tab.size(); tab.resize(off + align_up(n), 0.f); return off; };
  std::vector<double> A, s, o;
  if (int rc = host("A", A)) return rc;
  if (int rc = bn("data_bn.", s, o)) return rc;
  e->uestc_dbn = place(2 * kStgJoints * kStgIn);
  for (int i = 0; i < kStgJoints * kStgIn; ++i) { tab[e->uestc_dbn + i] = (float)s[i]; tab[e->uestc_dbn + kStgJoints * kStgIn + i] = (float)o[i]; }
  for (int i = 0; i < kStgBlocks; ++i) {
    auto& B = e->uestc_blk[i];
    B.cin = uestc_cin(i); B.cout = uestc_cout(i); B.stride = uestc_stride(i);
    B.kg = uestc_pad128(kStgK * B.cin); B.kt = uestc_pad128(kStgTaps * B.cout); B.kr = (i > 0 && B.cin != B.cout) ? uestc_pad128(B.cin) : 0;
    const std::string b = "st_gcn_networks." + std::to_string(i) + ".";
    std::vector<double> imp, w, bias, s1, o1;
    if (int rc = host("edge_importance." + std::to_string(i), imp)) return rc;
    B.am = place(kStgA);
    std::vector<double> am(kStgA), colsum(kStgK * kStgJoints, 0.0);
    for (int j = 0; j < kStgA; ++j) { am[j] = A[j] * imp[j]; tab[B.am + j] = (float)am[j]; }
    // (the kernels multiply by the ROUNDED coefficients: the bias table sums those)
    for (int k = 0; k < kStgK; ++k)
      for (int v = 0; v < kStgJoints; ++v)
        for (int x = 0; x < kStgJoints; ++x) colsum[k * kStgJoints + x] += (double)tab[B.am + (k * kStgJoints + v) * kStgJoints + x];
    if (int rc = host(b + "gcn.conv.weight", w)) return rc;
    if (int rc = host(b + "gcn.conv.bias", bias)) return rc;
    if (int rc = bn(b + "tcn.0.", s1, o1)) return rc;
    B.gw = place((size_t)B.cout * B.kg);
    for (int co = 0; co < B.cout; ++co)
      for (int k = 0; k < kStgK; ++k)
        for (int ci = 0; ci < B.cin; ++ci) tab[B.gw + (size_t)co * B.kg + k * B.cin + ci] = (float)(s1[co] * w[(size_t)(k * B.cout + co) * B.cin + ci]);
    B.gb = place((size_t)kStgJoints * B.cout);
    for (int x = 0; x < kStgJoints; ++x)
      for (int co = 0; co < B.cout; ++co) {
        double t = 0.0;
        for (int k = 0; k < kStgK; ++k) t += bias[k * B.cout + co] * colsum[k * kStgJoints + x];
        tab[B.gb + (size_t)x * B.cout + co] = (float)(s1[co] * t + o1[co]);
      }
    if (int rc = host(b + "tcn.2.weight", w)) return rc;
    if (int rc = host(b + "tcn.2.bias", bias)) return rc;
    if (int rc = bn(b + "tcn.3.", s1, o1)) return rc;
    B.tw = place((size_t)B.cout * B.kt);
    for (int co = 0; co < B.cout; ++co)
      for (int tap = 0; tap < kStgTaps; ++tap)
        for (int ci = 0; ci < B.cout; ++ci) tab[B.tw + (size_t)co * B.kt + tap * B.cout + ci] = (float)(s1[co] * w[((size_t)co * B.cout + ci) * kStgTaps + tap]);
    B.tb = place(B.cout);
    for (int co = 0; co < B.cout; ++co) tab[B.tb + co] = (float)(s1[co] * bias[co] + o1[co]);
    if (B.kr) {
      if (int rc = host(b + "residual.0.weight", w)) return rc;
      if (int rc = host(b + "residual.0.bias", bias)) return rc;
      if (int rc = bn(b + "residual.1.", s1, o1)) return rc;
      B.rw = place((size_t)B.cout * B.kr);
      for (int co = 0; co < B.cout; ++co)
        for (int ci = 0; ci < B.cin; ++ci) tab[B.rw + (size_t)co * B.kr + ci] = (float)(s1[co] * w[(size_t)co * B.cin + ci]);
      B.rb = place(B.cout);
      for (int co = 0; co < B.cout; ++co) tab[B.rb + co] = (float)(s1[co] * bias[co] + o1[co]);
    }
  }
  if (!e->uestc_tabs && hipMalloc((void**)&e->uestc_tabs, tab.size() * sizeof(float)) != hipSuccess) return e->fail(MLDHIP_EHIP, "hipMalloc(ST-GCN tables)");
  HIP_TRY(e, hipMemcpy(e->uestc_tabs, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
  if (e->cfg.precision == MLDHIP_PREC_F16X3) {
    if (!e->uestc_tabs_x3 && hipMalloc((void**)&e->uestc_tabs_x3, tab.size() * sizeof(float)) != hipSuccess) return e->fail(MLDHIP_EHIP, "hipMalloc(ST-GCN split tables)");
    const long long groups = (long long)(tab.size() / 32);      // every table starts on a 64-float boundary: whole groups of the split image
    MLD_LAUNCH(split_bf16_weights_kernel, dim3((unsigned)((groups + 15) / 16)), dim3(256), 0, c.stream, e->uestc_tabs, e->uestc_tabs_x3, groups);
    if (check_launch(c, "split_bf16_weights")) return c.rc;
  }
  return MLDHIP_OK;
}

void uestc_gemm(Ctx& c, StgGemmArgs a, bool x3) {
  E* e = c.e;
  if (x3) a.W = e->uestc_tabs_x3 + (a.W - e->uestc_tabs);      // the split image of the same table
  if (a.N == 64) {
    const dim3 grid((a.M + 63) / 64, 1);
    if (x3) { MLD_LAUNCH((stgcn_gemm_kernel<PREC_F16X3, 1>), grid, dim3(512), 0, c.stream, a); }
    else { MLD_LAUNCH((stgcn_gemm_kernel<PREC_F32, 1>), grid, dim3(512), 0, c.stream, a); }
  } else {
    const dim3 grid((a.M + 63) / 64, a.N / 128);
    if (x3) { MLD_LAUNCH((stgcn_gemm_kernel<PREC_F16X3, 2>), grid, dim3(512), 0, c.stream, a); }
    else { MLD_LAUNCH((stgcn_gemm_kernel<PREC_F32, 2>), grid, dim3(512), 0, c.stream, a); }
  }
  check_launch(c, "stgcn_gemm");
}

// a padded buffer and the geometry its zero rows were last written for
struct UestcPadded { float* p; int G = 0, T = 0, C = 0; };
void uestc_pads(Ctx& c, UestcPadded& b, int G, int T, int C) {
  if (b.G == G && b.T == T && b.C == C) return;
  const long long quads = ((long long)G * 2 * kStgPad + 2) * (C / 4);
  MLD_LAUNCH(stgcn_zero_pads_kernel, dim3((unsigned)std::min<long long>(2048, (quads + 255) / 256)), dim3(256), 0, c.stream, b.p, G, T, T + 2 * kStgPad, C, 2);
  check_launch(c, "stgcn_zero_pads");
  b.G = G; b.T = T; b.C = C;
}

// count: the call's non-finite output values go into the handle's sticky counter (the range probe's own calls do not)
int uestc_recognize_impl(E* e, const float* x_dev, const int64_t* strides, int B, int T, float* logits_dev, float* feat_dev, hipStream_t stream, bool count = true) {
  const auto& cfg = e->cfg;
  if (!cfg.uestc_rec) return e->fail(MLDHIP_ESTATE, "mldhip_uestc_recognize: the handle was created without the recognition ST-GCN (mldhip_config.uestc_rec = 0)");
  if (!e->finalized || !e->group_ready[kGroupUestc]) return e->fail(MLDHIP_ESTATE, "mldhip_uestc_recognize before finalize / the uestc_rec.* tensors not loaded");
  if (!x_dev || !strides) return e->fail(MLDHIP_EINVAL, "null pointer");
  if (!logits_dev && !feat_dev) return e->fail(MLDHIP_EINVAL, "logits_out_dev and feat_out_dev are both NULL: nothing to compute");
  if (B < 1 || B > cfg.uestc_max_motions) return e->fail(MLDHIP_EINVAL, "B=%d must be in 1..uestc_max_motions=%d", B, cfg.uestc_max_motions);
  if (T < 1 || T > cfg.max_frames) return e->fail(MLDHIP_EINVAL, "T=%d must be in 1..max_frames=%d", T, cfg.max_frames);
  for (int i = 0; i < 4; ++i)
    if (strides[i] < 1) return e->fail(MLDHIP_EINVAL, "strides[%d]=%lld must be positive (elements)", i, (long long)strides[i]);
  CtxUse use(e, stream);
  if (use.rc) return use.rc;
  Ctx c{e, stream};
  const bool x3 = uestc_x3(e);
  const float* tabs = e->uestc_tabs;
  const int NC = cfg.uestc_classes;
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, e->uestc_ws_floats / (uestc_z_floats(T) + 4 * uestc_pad_floats(T))));
  const size_t pf = uestc_pad_floats(T) * chunk + kUestcSlack;
  // (the five buffers share one carve: their sizes depend on the call's T)
  float* Z = e->uZ;
  UestcPadded Xa{Z + align_up(uestc_z_floats(T) * chunk)}, Xb{Xa.p + align_up(pf)}, H{Xb.p + align_up(pf)}, R{H.p + align_up(pf)};
  for (int b0 = 0; b0 < B && !c.rc; b0 += chunk) {
    const int Bc = std::min(chunk, B - b0), G = Bc * kStgJoints;
    StgInputArgs in;
    in.x = x_dev + (long long)b0 * strides[0]; in.sn = strides[0]; in.sv = strides[1]; in.sc = strides[2]; in.st = strides[3];
    in.scale = tabs + e->uestc_dbn; in.offset = in.scale + kStgJoints * kStgIn; in.Am = tabs + e->uestc_blk[0].am; in.Z = Z; in.B = Bc; in.T = T;
    MLD_LAUNCH(stgcn_input_kernel, dim3((unsigned)(Bc * T)), dim3(128), 0, stream, in);
    if (check_launch(c, "stgcn_input")) return c.rc;
    UestcPadded *cur = &Xb, *nxt = &Xa;
    int Tin = T;
    for (int i = 0; i < kStgBlocks && !c.rc; ++i) {
      const auto& K = e->uestc_blk[i];
      const int Tout = (Tin - 1) / K.stride + 1, TPin = Tin + 2 * kStgPad, TPout = Tout + 2 * kStgPad;
      if (i > 0) {
        StgMixArgs m;
        m.X = cur->p; m.Am = tabs + K.am; m.Z = Z; m.B = Bc; m.T = Tin; m.TP = TPin; m.KP = K.kg;
        const long long frames = (long long)Bc * Tin;
        if (K.cin == 64) { MLD_LAUNCH((stgcn_mix_kernel<64>), dim3((unsigned)((frames + 3) / 4)), dim3(256), 0, stream, m); }
        else if (K.cin == 128) { MLD_LAUNCH((stgcn_mix_kernel<128>), dim3((unsigned)((frames + 1) / 2)), dim3(256), 0, stream, m); }
        else { MLD_LAUNCH((stgcn_mix_kernel<256>), dim3((unsigned)frames), dim3(256), 0, stream, m); }
        if (check_launch(c, "stgcn_mix")) return c.rc;
      }
      uestc_pads(c, H, G, Tin, K.cout);
      StgGemmArgs g;      // graph convolution on the mixed rows -> H (padded)
      g.A = Z; g.a_gs = (long long)Tin * K.kg; g.lda = K.kg; g.rpg = Tin; g.W = tabs + K.gw; g.K = K.kg; g.bias = tabs + K.gb; g.brows = kStgJoints;
      g.Y = H.p; g.y_gr = TPin; g.y_r0 = kStgPad; g.relu = 1; g.M = G * Tin; g.N = K.cout;
      uestc_gemm(c, g, x3);
      const float* res = i == 0 ? nullptr : cur->p;
      if (K.kr) {         // residual convolution (1x1, stride 2) + its BN -> R, in the output's padded layout
        StgGemmArgs r;
        r.A = cur->p + (size_t)kStgPad * K.cin; r.a_gs = (long long)TPin * K.cin; r.lda = K.stride * K.cin; r.rpg = Tout; r.W = tabs + K.rw; r.K = K.kr; r.bias = tabs + K.rb;
        r.Y = R.p; r.y_gr = TPout; r.y_r0 = kStgPad; r.M = G * Tout; r.N = K.cout;
        uestc_gemm(c, r, x3);
        res = R.p;
      }
      uestc_pads(c, *nxt, G, Tout, K.cout);
      StgGemmArgs t;      // temporal convolution: row (group, o) = the 9 padded rows from s o on
      t.A = H.p; t.a_gs = (long long)TPin * K.cout; t.lda = K.stride * K.cout; t.rpg = Tout; t.W = tabs + K.tw; t.K = K.kt; t.bias = tabs + K.tb;
      t.res = res; t.Y = nxt->p; t.y_gr = TPout; t.y_r0 = kStgPad; t.relu = 1; t.M = G * Tout; t.N = K.cout;
      uestc_gemm(c, t, x3);
      std::swap(cur, nxt);
      Tin = Tout;
    }
    if (c.rc) return c.rc;
    StgHeadArgs h;
    h.X = cur->p; h.fw = P(e, "uestc_rec.fcn.weight"); h.fb = P(e, "uestc_rec.fcn.bias");
    h.logits = logits_dev ? logits_dev + (size_t)b0 * NC : nullptr; h.feat = feat_dev ? feat_dev + (size_t)b0 * kStgFeat : nullptr;
    h.counter = count ? e->nonfinite : nullptr; h.T = Tin; h.TP = Tin + 2 * kStgPad; h.NC = NC;
    MLD_LAUNCH(stgcn_head_kernel, dim3((unsigned)Bc), dim3(256), 0, stream, h);
    check_launch(c, "stgcn_head");
  }
  return c.rc;
}

}  // namespace
