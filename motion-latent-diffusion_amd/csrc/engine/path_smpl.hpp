// The SMPL body model (mldhip_smpl_forward; config field smpl_verts = V): rot6d features [B][T][150] -> joints [B][T][24][3] and vertices [B][T][V][3], the math
// of Rotation2xyz over smplx's SMPLLayer at betas = 0 as MLD's feats2joints / feats2joints_eval lambdas call it (include/mldhip.h has the contract, the
// padded-frame rule included; kernels/smpl.hpp the kernels).
//
// finalize   checks smpl.parents, computes the rest joints J = J_regressor v_template (host, accumulated in double) and re-lays posedirs, lbs_weights and
//            v_template per 16-vertex block (build_smpl_tables);
// a call     uploads the lengths, then per chunk of up to kSmplChunk frames: smpl_chain_kernel (joints, and the pose features / skinning matrices / per-frame
//            state of the chunk into the workspace) and, when vertices are asked for, smpl_verts_kernel.  A frame's numbers do not depend on the chunk or tile
//            it falls into: every product is a row of a matrix instruction whose other rows are other frames.
// Issued eagerly.  Exact fp32 in every precision mode.  Part of libmldhip's single translation unit; include order: see mldhip.hip.
#pragma once

namespace {

int smpl_blocks(const E* e) { return (e->cfg.smpl_verts + 15) / 16; }
// frames the workspace holds: whole pairs of 16-frame tiles
int smpl_chunk_frames(const E* e) { return (int)std::min<long long>(kSmplChunk, ((long long)e->cfg.max_batch * e->cfg.max_frames + 31) / 32 * 32); }

int build_smpl_tables(Ctx& c) {
  E* e = c.e;
  if (e->cfg.smpl_verts <= 0 || !e->group_ready[kGroupSmpl]) return MLDHIP_OK;
  const int V = e->cfg.smpl_verts, nblk = smpl_blocks(e);
  std::vector<float> par(kSmplJoints), vt((size_t)V * 3), jreg((size_t)kSmplJoints * V);
  HIP_TRY(e, hipMemcpy(par.data(), P(e, "smpl.parents"), par.size() * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(e, hipMemcpy(vt.data(), P(e, "smpl.v_template"), vt.size() * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(e, hipMemcpy(jreg.data(), P(e, "smpl.J_regressor"), jreg.size() * sizeof(float), hipMemcpyDeviceToHost));
  std::vector<float> small(kSmplJoints * 7, 0.f);      // J [24][3] | Jrel [24][3] | parents [24] (ints)
  int32_t* parents = reinterpret_cast<int32_t*>(small.data() + kSmplJoints * 6);
  parents[0] = -1;
  for (int i = 1; i < kSmplJoints; ++i) {
    const float pv = par[i];
    if (!(pv >= 0.f && pv < (float)i) || pv != std::floor(pv)) return e->fail(MLDHIP_EINVAL, "smpl.parents[%d] = %g must be an integer in [0, %d) (the chain runs parents first)", i, (double)pv, i);
    parents[i] = (int32_t)pv;
  }
  for (int j = 0; j < kSmplJoints; ++j)
    for (int cc = 0; cc < 3; ++cc) {
      double s = 0.0;
      for (int v = 0; v < V; ++v) s += (double)jreg[(size_t)j * V + v] * (double)vt[(size_t)v * 3 + cc];
      small[j * 3 + cc] = (float)s;
    }
  for (int j = 0; j < kSmplJoints; ++j)
    for (int cc = 0; cc < 3; ++cc) small[kSmplJoints * 3 + j * 3 + cc] = j == 0 ? small[cc] : small[j * 3 + cc] - small[parents[j] * 3 + cc];
  const size_t nP = (size_t)nblk * kSmplSteps * 3 * 64, nW = (size_t)nblk * kSmplJoints * 16, nT = (size_t)nblk * 48, nS = align_up(small.size());
  if (!e->smpl_tabs && hipMalloc((void**)&e->smpl_tabs, (nP + nW + nT + nS) * sizeof(float)) != hipSuccess) return e->fail(MLDHIP_EHIP, "hipMalloc(body model tables)");
  e->sm_P = e->smpl_tabs; e->sm_W = e->sm_P + nP; e->sm_vt = e->sm_W + nW; e->sm_small = e->sm_vt + nT;
  HIP_TRY(e, hipMemcpy(e->sm_small, small.data(), small.size() * sizeof(float), hipMemcpyHostToDevice));
  MLD_LAUNCH(smpl_relay_posedirs_kernel, dim3((unsigned)std::min<size_t>(4096, (nP + 255) / 256)), dim3(256), 0, c.stream, P(e, "smpl.posedirs"), e->sm_P, V, nblk);
  check_launch(c, "smpl_relay_posedirs");
  MLD_LAUNCH(smpl_relay_small_kernel, dim3((unsigned)std::min<size_t>(4096, (nW + nT + 255) / 256)), dim3(256), 0, c.stream, P(e, "smpl.lbs_weights"), P(e, "smpl.v_template"),
             e->sm_W, e->sm_vt, V, nblk);
  return check_launch(c, "smpl_relay_small");
}

int smpl_forward_impl(E* e, const float* feats_dev, const int32_t* lens_host, int B, int T, int flags, float* joints_dev, float* verts_dev, hipStream_t stream) {
  const auto& cfg = e->cfg;
  if (cfg.smpl_verts <= 0) return e->fail(MLDHIP_ESTATE, "mldhip_smpl_forward: the handle was created without the body model (mldhip_config.smpl_verts = 0)");
  if (!e->finalized || !e->group_ready[kGroupSmpl]) return e->fail(MLDHIP_ESTATE, "mldhip_smpl_forward before finalize / smpl.v_template, smpl.posedirs, smpl.J_regressor, smpl.lbs_weights, smpl.parents not loaded");
  if (!feats_dev || !lens_host) return e->fail(MLDHIP_EINVAL, "null pointer");
  if (!joints_dev && !verts_dev) return e->fail(MLDHIP_EINVAL, "joints_out_dev and verts_out_dev are both NULL: nothing to compute");
  if (flags & ~(MLDHIP_SMPL_TRANS_JOINTS | MLDHIP_SMPL_TRANS_VERTS)) return e->fail(MLDHIP_EINVAL, "flags=%d: unknown bits (MLDHIP_SMPL_TRANS_JOINTS | MLDHIP_SMPL_TRANS_VERTS)", flags);
  if (B < 1 || B > cfg.max_batch) return e->fail(MLDHIP_EINVAL, "B=%d must be in 1..max_batch=%d", B, cfg.max_batch);
  if (T < 1 || T > cfg.max_frames) return e->fail(MLDHIP_EINVAL, "T=%d must be in 1..max_frames=%d", T, cfg.max_frames);
  for (int b = 0; b < B; ++b)
    if (lens_host[b] < 1 || lens_host[b] > T) return e->fail(MLDHIP_EINVAL, "lengths[%d]=%d must be in 1..T=%d", b, lens_host[b], T);
  CtxUse use(e, stream);
  if (use.rc) return use.rc;
  Ctx c{e, stream};
  std::vector<int32_t>& tab = e->ctxs[e->cur_ctx].smpl_tab_host;
  tab.assign(lens_host, lens_host + B);
  int32_t* dtab = reinterpret_cast<int32_t*>(e->sTab);
  HIP_TRY(e, hipMemcpyAsync(dtab, tab.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  const int frames = B * T, chunk = smpl_chunk_frames(e), nblk = smpl_blocks(e);
  constexpr int FT = 2;
  for (int f0 = 0; f0 < frames && !c.rc; f0 += chunk) {
    const int n = std::min(chunk, frames - f0), tiles = (n + 15) / 16;
    SmplChainArgs a;
    a.feats = feats_dev; a.lens = dtab; a.J = e->sm_small; a.Jrel = e->sm_small + kSmplJoints * 3;
    a.parents = reinterpret_cast<const int*>(e->sm_small + kSmplJoints * 6);
    a.joints = joints_dev; a.pf = e->sPf; a.A = e->sA; a.aux = e->sAux; a.counter = e->nonfinite;
    a.T = T; a.frames = frames; a.f0 = f0; a.n = n; a.flags = flags;
    MLD_LAUNCH(smpl_chain_kernel, dim3((tiles * 16 + 63) / 64), dim3(64), 0, stream, a);
    if (check_launch(c, "smpl_chain")) return c.rc;
    if (!verts_dev) continue;
    SmplVertArgs v;
    v.pf = e->sPf; v.A = e->sA; v.aux = e->sAux; v.P = e->sm_P; v.W = e->sm_W; v.vt = e->sm_vt; v.verts = verts_dev; v.counter = e->nonfinite;
    v.V = cfg.smpl_verts; v.nblk = nblk; v.f0 = f0; v.tiles = tiles; v.flags = flags;
    // workgroups of one frame group walk the vertex blocks side by side (4 per step); enough groups x lanes to fill the chip twice, never more lanes than blocks
    const int groups = (tiles + FT - 1) / FT;
    const int lanes = std::max(1, std::min((nblk + 3) / 4, (kSmplLaneBudget + groups - 1) / groups));
    MLD_LAUNCH(smpl_verts_kernel<FT>, dim3(lanes, groups), dim3(256), 0, stream, v);
    check_launch(c, "smpl_verts");
  }
  return c.rc;
}

}  // namespace
