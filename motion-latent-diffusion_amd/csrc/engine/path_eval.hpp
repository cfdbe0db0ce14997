// The T2M evaluator towers (mldhip_t2m_motion_embed / mldhip_t2m_text_embed; config field t2m_eval = 1): motions [B][T][nfeats] and captions
// [B][L][300 | 15] -> [B][512] embeddings, the math of MovementConvEncoder -> MotionEncoderBiGRUCo and of TextEncoderBiGRUCo as MLD.t2m_eval runs them
// (include/mldhip.h has the contract, the padded-frame rule included).
//
// Motion tower, per chunk of up to kEvalChunk motions:
//   staging     feats -> G0 [B][TP][288]: per motion one zero row, the T frame rows (renormalised, columns 0 .. nfeats - 5, channels zero-padded), zero rows up to
//               TP = the multiple of 4 >= T + 4 (kernels/gru.hpp eval_stage_motion_kernel);
//   conv 1      a GEMM over G0 with lda = 2 x 288, K = 4 x 288: row m = b TP/2 + o of the GEMM is output step o of motion b (it reads staging rows 2o .. 2o + 3, i.e.
//               frames 2o - 1 .. 2o + 2).  It stores to G1 ONE ROW DOWN, so motion b's outputs land behind a zero row again: rows o >= floor(T / 2) of every motion are
//               stored as zeros (they are the next convolution's padding: the trailing one and, through the one-row shift, the next motion's leading one);
//   conv 2      the same over G1 [B][TP/2][512] with lda = 2 x 512, K = 4 x 512: TP/4 rows per motion, floor(T / 4) of them valid, the rest zeros;
//   linears     out_net, input_emb, then the input-side GRU products of both directions as one GEMM (N = 6 x 1024);
//   recurrence  one gru_step_kernel launch per step (max over the chunk of len / 4), state double buffered in vH0 / vH1 as [B][h_fwd | h_bwd] -- which IS the cat() the head reads;
//   head        Linear(2048 -> 1024), LayerNorm + LeakyReLU, Linear(1024 -> 512) straight into the caller's rows.
// Text tower: staging (word + Linear(15 -> 300)(pos) into K = 384 rows), input_emb, the GRU at H = 512 over L rows per caption, the same head at half the widths.
// Issued eagerly.  Part of libmldhip's single translation unit; include order: see mldhip.hip.
#pragma once

namespace {

int eval_tp(int T) { return (T + 4 + 3) / 4 * 4; }      // staging rows per motion (a multiple of 4: TP / 2 is even, so motion strides stay whole rows behind both convolutions)

// finalize: the tables the towers derive from their weights (tap-major convolution weights, the padded text input weight, the folded GRU input biases)
int build_eval_tables(Ctx& c) {
  E* e = c.e;
  if (!e->cfg.t2m_eval || (!e->group_ready[kGroupEvalMotion] && !e->group_ready[kGroupEvalText])) return MLDHIP_OK;
  const size_t n1 = (size_t)kEvalMove * 4 * kEvalConvC, n2 = (size_t)kEvalMove * 4 * kEvalMove, n3 = (size_t)kEvalTextH * kEvalTextK, n4 = 6 * kEvalMotionH, n5 = 6 * kEvalTextH;
  if (!e->eval_tabs && hipMalloc((void**)&e->eval_tabs, (n1 + n2 + n3 + n4 + n5) * sizeof(float)) != hipSuccess) return e->fail(MLDHIP_EHIP, "hipMalloc(evaluator tables)");
  e->ev_conv1_w = e->eval_tabs; e->ev_conv2_w = e->ev_conv1_w + n1; e->ev_text_in_w = e->ev_conv2_w + n2; e->ev_mbias = e->ev_text_in_w + n3; e->ev_tbias = e->ev_mbias + n4;
  auto bias = [&](float* out, const std::string& p, int H) {
    MLD_LAUNCH(gru_input_bias_kernel, dim3((6 * H + 255) / 256), dim3(256), 0, c.stream, out, P(e, p + ".gru.bias_ih_l0"), P(e, p + ".gru.bias_hh_l0"),
               P(e, p + ".gru.bias_ih_l0_reverse"), P(e, p + ".gru.bias_hh_l0_reverse"), H);
    check_launch(c, "gru_input_bias");
  };
  if (e->group_ready[kGroupEvalMotion]) {
    MLD_LAUNCH(conv_weight_relay_kernel, dim3(1024), dim3(256), 0, c.stream, P(e, "t2m_moveencoder.main.0.weight"), e->ev_conv1_w, kEvalMove, e->cfg.nfeats - 4, kEvalConvC);
    MLD_LAUNCH(conv_weight_relay_kernel, dim3(1024), dim3(256), 0, c.stream, P(e, "t2m_moveencoder.main.3.weight"), e->ev_conv2_w, kEvalMove, kEvalMove, kEvalMove);
    check_launch(c, "conv_weight_relay");
    bias(e->ev_mbias, "t2m_motionencoder", kEvalMotionH);
  }
  if (e->group_ready[kGroupEvalText]) {
    MLD_LAUNCH(pad_cols_kernel, dim3((kEvalTextH * kEvalTextK + 255) / 256), dim3(256), 0, c.stream, P(e, "t2m_textencoder.input_emb.weight"), e->ev_text_in_w, kEvalTextH, kEvalWord, kEvalTextK);
    check_launch(c, "pad_cols");
    bias(e->ev_tbias, "t2m_textencoder", kEvalTextH);
  }
  return c.rc;
}

bool eval_x3(const E* e) { return e->cfg.precision == MLDHIP_PREC_F16X3 && e->arena_x3 && e->probe[kProbeEval].ok; }      // the verdict of finalize's range probe

// the bidirectional recurrence of one chunk: `steps` launches in stream order; returns the buffer that holds the final state [B][2H]
template <int H>
const float* eval_gru(Ctx& c, bool x3, const std::string& p, const float* Gi, const int* d_lens, int B, int R, int steps) {
  E* e = c.e;
  MLD_LAUNCH(gru_init_kernel, dim3((unsigned)std::min(1024, (B * 2 * H + 255) / 256)), dim3(256), 0, c.stream, e->vH0, P(e, p + ".hidden"), B, 2 * H);
  check_launch(c, "gru_init");
  GruStepArgs a;
  const float* w[2] = {P(e, p + ".gru.weight_hh_l0"), P(e, p + ".gru.weight_hh_l0_reverse")};
  for (int d = 0; d < 2; ++d) a.Whh[d] = x3 ? e->arena_x3 + (w[d] - e->arena) : w[d];      // (tensors start on 64-float boundaries: whole groups of the split image)
  a.bhh[0] = P(e, p + ".gru.bias_hh_l0"); a.bhh[1] = P(e, p + ".gru.bias_hh_l0_reverse");
  a.Gi = Gi; a.lens = d_lens; a.B = B; a.R = R;
  const dim3 grid(H / 16, (B + 63) / 64, 2);
  for (int s = 0; s < steps && !c.rc; ++s) {
    a.s = s;
    a.h_prev = (s & 1) ? e->vH1 : e->vH0;
    a.h_next = (s & 1) ? e->vH0 : e->vH1;
    if (x3) { MLD_LAUNCH((gru_step_kernel<H, PREC_F16X3>), grid, dim3(256), 0, c.stream, a); }
    else { MLD_LAUNCH((gru_step_kernel<H, PREC_F32>), grid, dim3(256), 0, c.stream, a); }
    check_launch(c, "gru_step");
  }
  return (steps & 1) ? e->vH1 : e->vH0;
}

// cat(h_fwd, h_bwd) [B][2H] -> Linear(2H -> H), LayerNorm, LeakyReLU(0.2), Linear(H -> 512) into out [B][512]
void eval_head(Ctx& c, bool x3, const std::string& p, const float* hcat, int B, int H, float* out) {
  E* e = c.e;
  gemm_eval(c, lin_args(hcat, 2 * H, 2 * H, P(e, p + ".output_net.0.weight"), P(e, p + ".output_net.0.bias"), e->vHead, H, B, H), x3);
  MLD_LAUNCH(eval_ln_lrelu_kernel, dim3(B), dim3(256), 0, c.stream, e->vHead, P(e, p + ".output_net.1.weight"), P(e, p + ".output_net.1.bias"), H);
  check_launch(c, "eval_ln_lrelu");
  gemm_eval(c, lin_args(e->vHead, H, H, P(e, p + ".output_net.3.weight"), P(e, p + ".output_net.3.bias"), out, kEvalOut, B, kEvalOut), x3);
}

int eval_count_nonfinite(Ctx& c, const float* out, int B) {
  MLD_LAUNCH(count_nonfinite_kernel, dim3((unsigned)std::min(256, (B * kEvalOut + 255) / 256)), dim3(256), 0, c.stream, out, (long long)B * kEvalOut, c.e->nonfinite);
  return check_launch(c, "count_nonfinite");
}

// count: the call's non-finite output values go into the handle's sticky counter (the range probe's own calls do not: engine/probe.hpp)
int t2m_motion_embed_impl(E* e, const float* feats_dev, const int32_t* lens_host, int B, int T, int renorm, float* out_dev, hipStream_t stream, bool count = true) {
  const auto& cfg = e->cfg;
  if (!cfg.t2m_eval) return e->fail(MLDHIP_ESTATE, "mldhip_t2m_motion_embed: the handle was created without the evaluator towers (mldhip_config.t2m_eval = 0)");
  if (!e->finalized || !e->group_ready[kGroupEvalMotion]) return e->fail(MLDHIP_ESTATE, "mldhip_t2m_motion_embed before finalize / t2m_moveencoder.*, t2m_motionencoder.*, mean_eval, std_eval not loaded");
  if (!feats_dev || !lens_host || !out_dev) return e->fail(MLDHIP_EINVAL, "null pointer");
  if (renorm != 0 && renorm != 1) return e->fail(MLDHIP_EINVAL, "renorm=%d must be 0 or 1", renorm);
  if (renorm && !e->group_ready[kGroupStats]) return e->fail(MLDHIP_ESTATE, "mldhip_t2m_motion_embed with renorm = 1 needs mean / std");
  if (B < 1 || B > cfg.t2m_max_motions) return e->fail(MLDHIP_EINVAL, "B=%d must be in 1..t2m_max_motions=%d", B, cfg.t2m_max_motions);
  if (T < 1 || T > cfg.max_frames) return e->fail(MLDHIP_EINVAL, "T=%d must be in 1..max_frames=%d", T, cfg.max_frames);
  for (int b = 0; b < B; ++b)
    if (lens_host[b] < kEvalUnit || lens_host[b] > T) return e->fail(MLDHIP_EINVAL, "lengths[%d]=%d must be in %d..T=%d (a motion shorter than the unit length has no GRU step)", b, lens_host[b], kEvalUnit, T);
  CtxUse use(e, stream);
  if (use.rc) return use.rc;
  Ctx c{e, stream};
  const bool x3 = eval_x3(e);
  const int NF = cfg.nfeats, TP = eval_tp(T), R1 = TP / 2, R2 = TP / 4;
  const std::string mv = "t2m_moveencoder", me = "t2m_motionencoder";
  std::vector<int32_t>& tab = e->ctxs[e->cur_ctx].eval_tab_host;
  tab.assign((size_t)3 * B, 0);
  for (int b0 = 0, off = 0; b0 < B && !c.rc; b0 += kEvalChunk) {
    const int Bc = std::min(kEvalChunk, B - b0);
    int32_t* t = tab.data() + off;
    int steps = 0;
    for (int b = 0; b < Bc; ++b) {
      t[b] = T / 2; t[Bc + b] = T / 4; t[2 * Bc + b] = lens_host[b0 + b] / kEvalUnit;
      steps = std::max(steps, t[2 * Bc + b]);
    }
    off += 3 * Bc;
    int32_t* dtab = reinterpret_cast<int32_t*>(e->vTab);
    HIP_TRY(e, hipMemcpyAsync(dtab, t, (size_t)3 * Bc * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    MLD_LAUNCH(eval_stage_motion_kernel, dim3((unsigned)std::min<long long>(4096, ((long long)Bc * TP * (kEvalConvC / 4) + 255) / 256)), dim3(256), 0, stream,
               feats_dev + (size_t)b0 * T * NF, e->vG0, P(e, "mean"), P(e, "std"), P(e, "mean_eval"), P(e, "std_eval"), Bc, T, NF, TP, kEvalConvC, renorm);
    if (check_launch(c, "eval_stage_motion")) return c.rc;
    GemmArgs c1 = lin_args(e->vG0, 2 * kEvalConvC, 4 * kEvalConvC, e->ev_conv1_w, P(e, mv + ".main.0.bias"), e->vG1 + kEvalMove, kEvalMove, Bc * R1, kEvalMove);
    c1.act = ACT_LRELU; c1.lens = dtab; c1.rows_per_group = R1;
    gemm_eval(c, c1, x3);
    GemmArgs c2 = lin_args(e->vG1, 2 * kEvalMove, 4 * kEvalMove, e->ev_conv2_w, P(e, mv + ".main.3.bias"), e->vA, kEvalMove, Bc * R2, kEvalMove);
    c2.act = ACT_LRELU; c2.lens = dtab + Bc; c2.rows_per_group = R2;
    gemm_eval(c, c2, x3);
    const int rows = Bc * R2;
    gemm_eval(c, lin_args(e->vA, kEvalMove, kEvalMove, P(e, mv + ".out_net.weight"), P(e, mv + ".out_net.bias"), e->vB, kEvalMove, rows, kEvalMove), x3);
    gemm_eval(c, lin_args(e->vB, kEvalMove, kEvalMove, P(e, me + ".input_emb.weight"), P(e, me + ".input_emb.bias"), e->vA, kEvalMotionH, rows, kEvalMotionH), x3);
    gemm_eval(c, lin_args(e->vA, kEvalMotionH, kEvalMotionH, P(e, me + ".gru.weight_ih_l0"), e->ev_mbias, e->vGi, 6 * kEvalMotionH, rows, 6 * kEvalMotionH), x3);
    if (c.rc) return c.rc;
    const float* hcat = eval_gru<kEvalMotionH>(c, x3, me, e->vGi, dtab + 2 * Bc, Bc, R2, steps);
    eval_head(c, x3, me, hcat, Bc, kEvalMotionH, out_dev + (size_t)b0 * kEvalOut);
  }
  if (c.rc || !count) return c.rc;
  return eval_count_nonfinite(c, out_dev, B);
}

int t2m_text_embed_impl(E* e, const float* word_dev, const float* pos_dev, const int32_t* lens_host, int B, int L, float* out_dev, hipStream_t stream, bool count = true) {
  const auto& cfg = e->cfg;
  if (!cfg.t2m_eval) return e->fail(MLDHIP_ESTATE, "mldhip_t2m_text_embed: the handle was created without the evaluator towers (mldhip_config.t2m_eval = 0)");
  if (!e->finalized || !e->group_ready[kGroupEvalText]) return e->fail(MLDHIP_ESTATE, "mldhip_t2m_text_embed before finalize / t2m_textencoder.* not loaded");
  if (!word_dev || !pos_dev || !lens_host || !out_dev) return e->fail(MLDHIP_EINVAL, "null pointer");
  if (B < 1 || B > cfg.t2m_max_motions) return e->fail(MLDHIP_EINVAL, "B=%d must be in 1..t2m_max_motions=%d", B, cfg.t2m_max_motions);
  if (L < 1 || L > cfg.t2m_max_words) return e->fail(MLDHIP_EINVAL, "L=%d must be in 1..t2m_max_words=%d", L, cfg.t2m_max_words);
  for (int b = 0; b < B; ++b)
    if (lens_host[b] < 1 || lens_host[b] > L) return e->fail(MLDHIP_EINVAL, "text_lengths[%d]=%d must be in 1..L=%d", b, lens_host[b], L);
  CtxUse use(e, stream);
  if (use.rc) return use.rc;
  Ctx c{e, stream};
  const bool x3 = eval_x3(e);
  const std::string te = "t2m_textencoder";
  std::vector<int32_t>& tab = e->ctxs[e->cur_ctx].eval_tab_host;
  tab.assign(lens_host, lens_host + B);
  for (int b0 = 0; b0 < B && !c.rc; b0 += kEvalChunk) {
    const int Bc = std::min(kEvalChunk, B - b0), rows = Bc * L;
    int steps = 0;
    for (int b = 0; b < Bc; ++b) steps = std::max(steps, lens_host[b0 + b]);
    int32_t* dtab = reinterpret_cast<int32_t*>(e->vTab);
    HIP_TRY(e, hipMemcpyAsync(dtab, tab.data() + b0, (size_t)Bc * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    MLD_LAUNCH(eval_stage_text_kernel, dim3((unsigned)std::min<long long>(4096, ((long long)rows * kEvalTextK + 255) / 256)), dim3(256), 0, stream,
               word_dev + (size_t)b0 * L * kEvalWord, pos_dev + (size_t)b0 * L * kEvalPos, P(e, te + ".pos_emb.weight"), P(e, te + ".pos_emb.bias"), e->vB, rows, kEvalWord, kEvalPos, kEvalTextK);
    if (check_launch(c, "eval_stage_text")) return c.rc;
    gemm_eval(c, lin_args(e->vB, kEvalTextK, kEvalTextK, e->ev_text_in_w, P(e, te + ".input_emb.bias"), e->vA, kEvalTextH, rows, kEvalTextH), x3);
    gemm_eval(c, lin_args(e->vA, kEvalTextH, kEvalTextH, P(e, te + ".gru.weight_ih_l0"), e->ev_tbias, e->vGi, 6 * kEvalTextH, rows, 6 * kEvalTextH), x3);
    if (c.rc) return c.rc;
    const float* hcat = eval_gru<kEvalTextH>(c, x3, te, e->vGi, dtab, Bc, L, steps);
    eval_head(c, x3, te, hcat, Bc, kEvalTextH, out_dev + (size_t)b0 * kEvalOut);
  }
  if (c.rc || !count) return c.rc;
  return eval_count_nonfinite(c, out_dev, B);
}

}  // namespace
