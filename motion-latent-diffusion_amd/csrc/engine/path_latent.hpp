// Latent-diffusion paths (configs 1-3, 5): what a sample call is made of -- condition rows, the reverse loop (path_loop.hpp), decode + joints (path_vae.hpp).
// Part of libmldhip's single translation unit; include order: see mldhip.hip.  Internal linkage throughout (anonymous namespace) except the handle type itself.
#pragma once

namespace {

// emb_proj = Sequential(ReLU, Linear) (mld_denoiser.py:65-68) for `rows` text rows -> dst[rows][D]; the
// bias already holds + pe[2] (token 2 of the sequence).
void text_projection(Ctx& c, const float* text_emb, int rows, float* dst) {
  E* e = c.e;
  const int D = e->cfg.latent_dim, TD = e->cfg.text_dim;
  GemmArgs g = lin_args(text_emb, TD, TD, P(e, "denoiser.emb_proj.1.weight"), e->text_bias, dst, D, rows, D);
  g.relu_in = 1;
  gemm(c, g);
}

// time-MLP rows for `n` timestep embeddings already in `temb0` -> out[n, D] (+pe[1] folded in the bias)
void time_mlp(Ctx& c, const float* temb0, float* mid, float* out, int n) {
  E* e = c.e;
  const int D = e->cfg.latent_dim, TD = time_width(e);
  GemmArgs a = lin_args(temb0, TD, TD, P(e, "denoiser.time_embedding.linear_1.weight"),
                        P(e, "denoiser.time_embedding.linear_1.bias"), mid, D, n, D);
  a.act = ACT_SILU;
  gemm(c, a);
  gemm(c, lin_args(mid, D, D, P(e, "denoiser.time_embedding.linear_2.weight"), e->time_b2pe, out, D, n, D));
}

// rows of token 2 for an action CFG batch of R rows -> dst[R][D] (labels already in labels_dev)
void action_rows(Ctx& c, int R, int nuncond, float* dst) {
  E* e = c.e;
  MLD_COUNTED(c, "action_rows", MLD_LAUNCH(action_rows_kernel, dim3(R), dim3(256), 0, c.stream, dst, P(e, "denoiser.emb_proj.action_embedding"),
         P(e, "denoiser.query_pos.pe") + 2 * e->cfg.latent_dim, e->labels_dev, nuncond));
}

// run-time part of the F16X3 range contract (mldhip.h): non-finite results are counted, mldhip_numeric_status reports them
void count_nonfinite(Ctx& c, const float* x, long long n) {
  E* e = c.e;
  if (e->cfg.precision != MLDHIP_PREC_F16X3 || !e->nonfinite || n <= 0) return;
  const unsigned blocks = (unsigned)std::min<long long>((n + 255) / 256, 2048);
  MLD_LAUNCH(count_nonfinite_kernel, dim3(blocks), dim3(256), 0, c.stream, x, n, e->nonfinite);
  check_launch(c, "count_nonfinite");
}

// the decode half of a sample call: MldVae.decode of the bound context's latents + feats2joints (mld.py:232-240,264), with the run-time non-finite count
void enqueue_decode(Ctx& c, int B, int T, float* feats_out, float* joints_out) {
  E* e = c.e;
  e->phase = 1;
  // feats_out == nullptr with joints_out set: nobody but feats2joints reads the features ("dec_lean": the narrow final stage)
  float* f = feats_out ? feats_out : e->feats_int;
  int pitch = 0;
  decode_body(c, e->lat, B, T, f, !feats_out && joints_out, &pitch);
  if (joints_out) {
    e->phase = 2;
    // "dec_lean": the joints kernel counts what it stores (the F16X3 range contract's run-time count, count_nonfinite)
    unsigned* counter = e->dec_lean && e->cfg.precision == MLDHIP_PREC_F16X3 ? e->nonfinite : nullptr;
    joints_body(c, f, B, T, joints_out, pitch, counter);
    if (!counter) count_nonfinite(c, joints_out, (long long)B * T * e->cfg.njoints * 3);
  } else {
    count_nonfinite(c, f, (long long)B * T * e->cfg.nfeats);      // feats-only call: the decoder's output is what the caller gets
  }
}

// Everything mld.py:232-240,264 does after the text encoder (enqueue_sample below).  The whole CFG batch runs as ONE
// chain of dependent launches (splitting a batch into sub-batch chains on parallel graph branches was measured: the
// sequential depth per chain is what costs, no gain -- profiles/r01_v3_chains*; removed).
// `text` == nullptr selects the action condition (labels_dev holds the 2B labels).
int enqueue_sample(E* e, hipStream_t stream, const float* text, const float* init_lat, int B, int T,
                   float* lat_out, float* feats_out, float* joints_out) {
  Ctx c{e, stream};
  const int D = e->cfg.latent_dim, n = e->cfg.num_inference_steps;
  // guidance_scale <= 1: the reference runs the conditional batch alone (mld.py:300,316-340); u + 1*(c-u) is that batch
  const float guidance = e->cfg.guidance_scale > 1.0f ? e->cfg.guidance_scale : 1.0f;
  e->launches[0] = e->launches[1] = e->launches[2] = 0;
  e->phase = 0;
  if (e->sample_part != 2) {
    if (text) text_projection(c, text, 2 * B, e->TP);
    else action_rows(c, 2 * B, B, e->TP);
  }
  if (use_cluster(e, B)) {
    launch_cluster_loop(c, init_lat, B, n, guidance);
    if (e->sample_part == 1) return c.rc;
  } else if (use_fused(e, B)) {
    launch_fused_loop(c, init_lat, B, n, guidance);
  } else {
    const DenView v = den_view(e, 2 * B);
    // mldhip_sample_many_from: every motion's own start state, then the steps from the call's smallest first step on; the from-form of the final-step kernels
    // holds the motions that start later
    const int s_first = e->from_on ? e->from_step0 : 0;
    if (e->from_on)
      MLD_COUNTED(c, "init_chain", MLD_LAUNCH(init_chain_from_kernel, dim3(B), dim3(256), 0, c.stream, init_lat, v.lat, v.X0, P(e, "denoiser.query_pos.pe"),
             (const float*)(e->T1 + (size_t)s_first * D), (const float*)e->TP, B, 1.0f /* init_noise_sigma */, (const StartRow*)e->starts_dev));
    else
    MLD_COUNTED(c, "init_chain", MLD_LAUNCH(init_chain_kernel, dim3(B), dim3(256), 0, c.stream, init_lat, v.lat, v.X0, P(e, "denoiser.query_pos.pe"), e->T1, e->TP, B, 0, B,
           1.0f /* init_noise_sigma */));
    for (int s = s_first; s < n && !c.rc; ++s) {
      denoiser_body(c, v);
      const float* t1n = (s + 1 < n) ? e->T1 + (size_t)(s + 1) * D : nullptr;
      if (e->from_on && eta_live(e))
        MLD_COUNTED(c, "den_final_step", MLD_LAUNCH(den_final_step_eta_from_kernel, dim3(B), dim3(256), 0, c.stream, den_final_args(e, v), v.lat, v.X0, P(e, "denoiser.query_pos.pe"), t1n, B,
               guidance, ddim_coef(e, e->timesteps[s]), e->keys_dev, s, ddim_eta(e, e->timesteps[s]), traj_table(e), (const StartRow*)e->starts_dev));
      else if (e->from_on)
        MLD_COUNTED(c, "den_final_step", MLD_LAUNCH(den_final_step_from_kernel, dim3(B), dim3(256), 0, c.stream, den_final_args(e, v), v.lat, v.X0, P(e, "denoiser.query_pos.pe"), t1n, B,
               guidance, ddim_coef(e, e->timesteps[s]), traj_table(e), s, (const StartRow*)e->starts_dev));
      else if (eta_live(e))
        MLD_COUNTED(c, "den_final_step", MLD_LAUNCH(den_final_step_eta_kernel, dim3(B), dim3(256), 0, c.stream, den_final_args(e, v), v.lat, v.X0, P(e, "denoiser.query_pos.pe"), t1n, B,
               guidance, ddim_coef(e, e->timesteps[s]), e->keys_dev, s, ddim_eta(e, e->timesteps[s]), traj_table(e)));
      else
        MLD_COUNTED(c, "den_final_step", MLD_LAUNCH(den_final_step_kernel, dim3(B), dim3(256), 0, c.stream, den_final_args(e, v), v.lat, v.X0, P(e, "denoiser.query_pos.pe"), t1n, B,
               guidance, ddim_coef(e, e->timesteps[s]), traj_table(e), s));
    }
  }
  if (c.rc || e->sample_part == 2) return c.rc;    // (part 2: the launch alone; the pipelined form counts non-finite latents on its side stream, in front of the decode)
  count_nonfinite(c, e->lat, (long long)B * D);
  if (lat_out) {
    hipError_t s = hipMemcpyAsync(lat_out, e->lat, (size_t)B * D * sizeof(float), hipMemcpyDeviceToDevice, stream);
    if (s != hipSuccess) return e->fail(MLDHIP_EHIP, "latents copy: %s", hipGetErrorString(s));
  }
  if (feats_out || joints_out) enqueue_decode(c, B, T, feats_out, joints_out);
  return c.rc;
}

int validate_lengths(E* e, const int32_t* lengths, int B, int* Tmax) {
  if (!lengths) return e->fail(MLDHIP_EINVAL, "lengths_host is NULL");
  if (B < 1 || B > e->cfg.max_batch) return e->fail(MLDHIP_EINVAL, "batch %d outside [1, max_batch=%d]", B, e->cfg.max_batch);
  int t = 0;
  for (int i = 0; i < B; ++i) {
    if (lengths[i] < 1 || lengths[i] > e->cfg.max_frames)
      return e->fail(MLDHIP_EINVAL, "lengths[%d]=%d outside [1, max_frames=%d]", i, lengths[i], e->cfg.max_frames);
    t = std::max(t, lengths[i]);
  }
  *Tmax = t;
  return 0;
}

}  // namespace
