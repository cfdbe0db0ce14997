// The HumanAct12 action-recognition GRU (mldhip_a2m_recognize; config fields a2m_rec = 1, a2m_max_motions): joints [B][T][72] -> logits [B][12] and
// activations [B][30], the math of MotionDiscriminator / MotionDiscriminatorForFID as HUMANACTMetrics runs them (include/mldhip.h has the contract,
// the padded-frame rule and the h0 contract included; kernels/a2m_gru.hpp the kernel and its price).
//
// A call uploads the lengths and issues ONE a2m_gru_kernel launch: a workgroup per 16-motion tile runs both layers over the tile's steps and the head.
// No tables are derived at finalize: the kernel reads the a2m_rec.* tensors of the arena as they are.
// Issued eagerly.  Exact fp32 in every precision mode.  Part of libmldhip's single translation unit; include order: see mldhip.hip.
#pragma once

namespace {

int a2m_recognize_impl(E* e, const float* joints_dev, const int32_t* lens_host, const float* h0_dev, int B, int T, float* logits_dev, float* act_dev,
                       hipStream_t stream) {
  const auto& cfg = e->cfg;
  if (!cfg.a2m_rec) return e->fail(MLDHIP_ESTATE, "mldhip_a2m_recognize: the handle was created without the recognition GRU (mldhip_config.a2m_rec = 0)");
  if (!e->finalized || !e->group_ready[kGroupA2m]) return e->fail(MLDHIP_ESTATE, "mldhip_a2m_recognize before finalize / the a2m_rec.* tensors not loaded");
  if (!joints_dev || !lens_host) return e->fail(MLDHIP_EINVAL, "null pointer");
  if (!logits_dev && !act_dev) return e->fail(MLDHIP_EINVAL, "logits_out_dev and act_out_dev are both NULL: nothing to compute");
  if (B < 1 || B > cfg.a2m_max_motions) return e->fail(MLDHIP_EINVAL, "B=%d must be in 1..a2m_max_motions=%d", B, cfg.a2m_max_motions);
  if (T < 1 || T > cfg.max_frames) return e->fail(MLDHIP_EINVAL, "T=%d must be in 1..max_frames=%d", T, cfg.max_frames);
  for (int b = 0; b < B; ++b)
    if (lens_host[b] < 1 || lens_host[b] > T) return e->fail(MLDHIP_EINVAL, "lengths[%d]=%d must be in 1..T=%d", b, lens_host[b], T);
  CtxUse use(e, stream);
  if (use.rc) return use.rc;
  Ctx c{e, stream};
  std::vector<int32_t>& tab = e->ctxs[e->cur_ctx].a2m_tab_host;
  tab.assign(lens_host, lens_host + B);
  int32_t* dtab = reinterpret_cast<int32_t*>(e->rTab);
  HIP_TRY(e, hipMemcpyAsync(dtab, tab.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  A2mArgs a;
  a.x = joints_dev; a.lens = dtab; a.h0 = h0_dev;
  a.wih0 = P(e, "a2m_rec.recurrent.weight_ih_l0"); a.whh0 = P(e, "a2m_rec.recurrent.weight_hh_l0");
  a.wih1 = P(e, "a2m_rec.recurrent.weight_ih_l1"); a.whh1 = P(e, "a2m_rec.recurrent.weight_hh_l1");
  a.bih0 = P(e, "a2m_rec.recurrent.bias_ih_l0"); a.bhh0 = P(e, "a2m_rec.recurrent.bias_hh_l0");
  a.bih1 = P(e, "a2m_rec.recurrent.bias_ih_l1"); a.bhh1 = P(e, "a2m_rec.recurrent.bias_hh_l1");
  a.w1 = P(e, "a2m_rec.linear1.weight"); a.b1 = P(e, "a2m_rec.linear1.bias");
  a.w2 = P(e, "a2m_rec.linear2.weight"); a.b2 = P(e, "a2m_rec.linear2.bias");
  a.logits = logits_dev; a.act = act_dev; a.counter = e->nonfinite;
  a.B = B; a.T = T;
  MLD_LAUNCH(a2m_gru_kernel, dim3((unsigned)((B + kA2mTile - 1) / kA2mTile)), dim3(512), 0, stream, a);
  return check_launch(c, "a2m_gru");
}

}  // namespace
