// The text-to-motion metric kernels (mldhip_t2m_match / mldhip_act_stats / mldhip_pair_dist; config fields t2m_metrics = 1, metrics_max_rows): grouped
// retrieval, activation statistics and pair distances on device-resident embeddings [N][D] (include/mldhip.h has the contract; kernels/t2m_metrics.hpp
// the kernels).
//
// No weights and nothing derived at finalize: the calls work on any handle created with t2m_metrics = 1, finalized or not.  The only workspace is the
// index table of mldhip_pair_dist (2 x metrics_max_rows words), uploaded with the call like the length tables of the other entry points.
// Issued eagerly.  Exact fp32 in every precision mode.  Part of libmldhip's single translation unit; include order: see mldhip.hip.
#pragma once

namespace {

// the checks the three calls share; 0 when they pass
int metrics_check(E* e, const char* who, int N, int D, int minN) {
  const auto& cfg = e->cfg;
  if (!cfg.t2m_metrics) return e->fail(MLDHIP_ESTATE, "%s: the handle was created without the metric kernels (mldhip_config.t2m_metrics = 0)", who);
  if (D < 1 || D > kMetMaxD) return e->fail(MLDHIP_EINVAL, "%s: D=%d must be in 1..%d", who, D, kMetMaxD);
  if (N < minN || N > cfg.metrics_max_rows) return e->fail(MLDHIP_EINVAL, "%s: N=%d must be in %d..metrics_max_rows=%d", who, N, minN, cfg.metrics_max_rows);
  return MLDHIP_OK;
}

int t2m_match_impl(E* e, const float* text_dev, const float* motion_dev, int N, int D, int R, int32_t* rank_dev, float* diag_dev, hipStream_t stream) {
  if (int rc = metrics_check(e, "mldhip_t2m_match", N, D, 1)) return rc;
  if (!text_dev || !motion_dev) return e->fail(MLDHIP_EINVAL, "null pointer");
  if (!rank_dev && !diag_dev) return e->fail(MLDHIP_EINVAL, "rank_out_dev and diag_out_dev are both NULL: nothing to compute");
  if (R < 1 || R > kMetR) return e->fail(MLDHIP_EINVAL, "R=%d must be in 1..%d", R, kMetR);
  const int G = N / R;
  if (G == 0) return MLDHIP_OK;      // fewer rows than one group: every row is a tail row
  CtxUse use(e, stream);
  if (use.rc) return use.rc;
  Ctx c{e, stream};
  MatchArgs a;
  a.text = text_dev; a.motion = motion_dev; a.rank = rank_dev; a.diag = diag_dev; a.D = D; a.R = R;
  MLD_LAUNCH(t2m_match_kernel, dim3((unsigned)G), dim3(256), 0, stream, a);
  return check_launch(c, "t2m_match");
}

int act_stats_impl(E* e, const float* x_dev, int N, int D, float* mean_dev, float* cov_dev, hipStream_t stream) {
  if (int rc = metrics_check(e, "mldhip_act_stats", N, D, 2)) return rc;
  if (!x_dev || !mean_dev || !cov_dev) return e->fail(MLDHIP_EINVAL, "null pointer");
  CtxUse use(e, stream);
  if (use.rc) return use.rc;
  Ctx c{e, stream};
  StatArgs a;
  a.x = x_dev; a.mean = mean_dev; a.cov = cov_dev; a.N = N; a.D = D;
  MLD_LAUNCH(act_mean_kernel, dim3((unsigned)((D + 63) / 64)), dim3(256), 0, stream, a);
  if (int rc = check_launch(c, "act_mean")) return rc;
  const int nt = (D + 31) / 32;
  MLD_LAUNCH(act_cov_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, stream, a);
  return check_launch(c, "act_cov");
}

int pair_dist_impl(E* e, const float* x_dev, int N, int D, const int32_t* a_host, const int32_t* b_host, int P, float* dist_dev, hipStream_t stream) {
  if (int rc = metrics_check(e, "mldhip_pair_dist", N, D, 1)) return rc;
  if (!x_dev || !a_host || !b_host || !dist_dev) return e->fail(MLDHIP_EINVAL, "null pointer");
  if (P < 1 || P > e->cfg.metrics_max_rows) return e->fail(MLDHIP_EINVAL, "P=%d must be in 1..metrics_max_rows=%d", P, e->cfg.metrics_max_rows);
  for (int i = 0; i < P; ++i) {
    if (a_host[i] < 0 || a_host[i] >= N) return e->fail(MLDHIP_EINVAL, "a[%d]=%d must be in 0..N-1=%d", i, a_host[i], N - 1);
    if (b_host[i] < 0 || b_host[i] >= N) return e->fail(MLDHIP_EINVAL, "b[%d]=%d must be in 0..N-1=%d", i, b_host[i], N - 1);
  }
  CtxUse use(e, stream);
  if (use.rc) return use.rc;
  Ctx c{e, stream};
  std::vector<int32_t>& tab = e->ctxs[e->cur_ctx].met_tab_host;
  tab.assign(a_host, a_host + P);
  tab.insert(tab.end(), b_host, b_host + P);
  int32_t* dtab = reinterpret_cast<int32_t*>(e->mTab);
  HIP_TRY(e, hipMemcpyAsync(dtab, tab.data(), (size_t)2 * P * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  PairArgs a;
  a.x = x_dev; a.ab = dtab; a.out = dist_dev; a.D = D; a.P = P;
  MLD_LAUNCH(pair_dist_kernel, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, stream, a);
  return check_launch(c, "pair_dist");
}

}  // namespace
