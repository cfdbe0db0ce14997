// The sampling drivers behind the C ABI: the single call (sample_impl), the coalesced and the pipelined form of mldhip_sample_many, the one-step
// denoiser calls, the diffusion-only call, and the cluster loop's self-healing; the short host sequences they share are the helpers at the top.
// Part of libmldhip's single translation unit; include order: see mldhip.hip.  Internal linkage throughout (anonymous namespace).
#pragma once

namespace {

int range_probe(E* e, hipStream_t stream, const float* user_text = nullptr, const float* user_lat = nullptr, int user_B = 0);   // engine/probe.hpp

// ---------------------------------------------------------------------------------------------------------------- cluster loop: leaving it
// A cluster launch did not keep its workgroups resident together (a wait ran into its 200 ms bound): not an arithmetic verdict -- the handle stays on the
// other loop families from here on, and the captured graphs that hold the kernel are dropped (failure path: blocking).  mldhip_set_option("loop_kernel", 4) re-arms it.
void leave_cluster_loop(E* e) {
  e->cluster_failed = 1;
  if (e->cl_host_status) *e->cl_host_status = 0u;
  drop_graphs(e, true);      // (torch's streams are non-blocking: a device-wide sync in front of this does order it, the drain says so explicitly -- advisor r5)
}

// Self-healing of the cluster loop (advisor r5): the kernel sets a pinned host word next to its sticky status word when a wait runs into its bound.  Every sample call looks
// at it first -- a plain host read, no device synchronisation: a handle whose cluster launch timed out (its latents were poisoned with NaN and counted) serves the NEXT call
// on the other loop families already, without waiting for the caller to poll mldhip_numeric_status.
void heal_cluster(E* e) {
  if (!e->cl_host_status || e->cluster_failed || *reinterpret_cast<volatile unsigned*>(e->cl_host_status) == 0u) return;
  leave_cluster_loop(e);
  (void)cluster_timed_out(e);          // the device-side sticky words have been acted on: cleared (a later mldhip_numeric_status must not fail a re-armed handle for them)
}

// ---------------------------------------------------------------------------------------------------------------- shared host sequences
// action labels against nclasses; req >= 0 names the request of a mldhip_sample_many call in the message
int check_actions(E* e, const int32_t* actions, int n, int req = -1) {
  char where[32] = "";
  if (req >= 0) snprintf(where, sizeof where, "request %d: ", req);
  for (int i = 0; i < n; ++i)
    if (actions[i] < 0 || actions[i] >= e->cfg.nclasses)
      return e->fail(MLDHIP_EINVAL, "%sactions[%d]=%d outside [0, nclasses=%d)", where, i, actions[i], e->cfg.nclasses);
  return MLDHIP_OK;
}

// cond = cat(zeros_like(actions), actions) (mld.py:722-725) into the bound context's labels; the first half is never read (null embedding)
int stage_actions(E* e, const int32_t* actions_host, int B, hipStream_t s) {
  HIP_TRY(e, hipMemsetAsync(e->labels_dev, 0, (size_t)B * sizeof(int32_t), s));
  HIP_TRY(e, hipMemcpyAsync(e->labels_dev + B, actions_host, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s));
  return MLDHIP_OK;
}

// the caller's condition rows (text == nullptr: action labels, staged by stage_actions) and start latents into the bound context's staging buffers: what captured graphs read
int stage_inputs(E* e, const float* text, const float* init_lat, int B, hipStream_t s) {
  if (text) HIP_TRY(e, hipMemcpyAsync(e->text_in, text, (size_t)2 * B * e->cfg.text_dim * sizeof(float), hipMemcpyDeviceToDevice, s));
  HIP_TRY(e, hipMemcpyAsync(e->lat_in, init_lat, (size_t)B * e->cfg.latent_dim * sizeof(float), hipMemcpyDeviceToDevice, s));
  return MLDHIP_OK;
}

// ... and what a replay left in the bound context out to the caller's buffers (those that are asked for)
int copy_outputs(E* e, int B, int T, float* lat_out, float* feats_out, float* joints_out, hipStream_t s) {
  const size_t D = e->cfg.latent_dim, NF = e->cfg.nfeats, NJ = (size_t)e->cfg.njoints * 3;
  if (lat_out) HIP_TRY(e, hipMemcpyAsync(lat_out, e->lat, (size_t)B * D * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (feats_out) HIP_TRY(e, hipMemcpyAsync(feats_out, e->feats_int, (size_t)B * T * NF * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (joints_out) HIP_TRY(e, hipMemcpyAsync(joints_out, e->joints_int, (size_t)B * T * NJ * sizeof(float), hipMemcpyDeviceToDevice, s));
  return MLDHIP_OK;
}

// the time-MLP row of ONE timestep into t1_one (the one-step denoiser calls; sampling reads the rows finalize built for the schedule)
int single_timestep_row(Ctx& c, int timestep) {
  E* e = c.e;
  const int TD = time_width(e);
  std::vector<float> host(TD);
  timestep_sincos(float(timestep), TD, host.data());
  HIP_TRY(e, hipMemcpyAsync(e->temb0_one, host.data(), TD * sizeof(float), hipMemcpyHostToDevice, c.stream));
  HIP_TRY(e, hipStreamSynchronize(c.stream));   // `host` is a stack temporary
  time_mlp(c, e->temb0_one, e->temb0_one + TD, e->t1_one, 1);
  return MLDHIP_OK;
}

// calls served by a captured graph: all of them, except cluster-loop calls of a hooks build with "cluster_graph" 0 (and the simulator, which has no graphs)
bool replays(const E* e, int B) {
#if !defined(MLDHIP_SIM)
  return e->cfg.use_graph && (!use_cluster(e, B) || e->cluster_graph);    // cluster_graph: true outside the hooks build
#else
  (void)e; (void)B;
  return false;
#endif
}

// ---------------------------------------------------------------------------------------------------------------- one call
// shared body of mldhip_sample / mldhip_sample_action (text_emb_dev == nullptr <=> action labels given)
int sample_impl(E* e, const float* text_emb_dev, const int32_t* actions_host, const float* init_latents_dev,
                const int32_t* lengths_host, int32_t B, float* latents_out_dev, float* feats_out_dev, float* joints_out_dev,
                void* stream_) {
  if (!e->finalized) return e->fail(MLDHIP_ESTATE, "mldhip_sample before mldhip_finalize_weights");
  if (!e->group_ready[kGroupDenoiser] || !e->group_ready[kGroupVaeDecoder] || (joints_out_dev && !e->group_ready[kGroupStats]))
    return e->fail(MLDHIP_ESTATE, "mldhip_sample needs denoiser.*, vae.decoder.* (and mean/std for joints) loaded");
  if (!init_latents_dev) return e->fail(MLDHIP_EINVAL, "null input pointer");
  int T = 0;
  if (int rc = validate_lengths(e, lengths_host, B, &T)) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  heal_cluster(e);
  if (e->probe_first_call && text_emb_dev) {              // "range_probe" 2: the loop probe on THIS batch before it is sampled (one-off, synchronous)
    e->probe_first_call = false;
    if (e->probe[kProbeLoop].ok)
      if (int rc = range_probe(e, stream, text_emb_dev, init_latents_dev, B)) return rc;
  }
  CtxUse use(e, stream);                                  // picks + binds a workspace context (see WsContext)
  if (use.rc) return use.rc;
  ClusterLane lane(e, stream, e->cluster_lane && use_cluster(e, B));         // cluster launches never side by side (engine/params.hpp)
  HIP_TRY(e, hipMemcpyAsync(e->lens_dev, lengths_host, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  if (actions_host) {
    if (int rc = check_actions(e, actions_host, B)) return rc;
    if (int rc = stage_actions(e, actions_host, B, stream)) return rc;
  }
#if !defined(MLDHIP_SIM)
  // Calls served by the cluster loop replay a captured graph like the rest; its flags are cleared by a kernel, not a memset node: replays of
  // a hipMemsetAsync node in front of den_cluster_kernel left address-like words in the tail of the buffer on this runtime (r05).
  if (replays(e, B)) {
    // want_f = the caller wants features; with "dec_lean" 0 the joints need the full feature row as well (the parent's keys)
    const bool want_j = joints_out_dev != nullptr, want_f = feats_out_dev != nullptr || (want_j && !e->dec_lean);
    if (int rc = stage_inputs(e, text_emb_dev, init_latents_dev, B, stream)) return rc;
    hipGraphExec_t exec = nullptr;
    if (int rc = graph_for(e, GraphKey{B, T, want_f, want_j}, text_emb_dev != nullptr, &exec)) return rc;
    HIP_TRY(e, hipGraphLaunch(exec, stream));
    return copy_outputs(e, B, T, latents_out_dev, feats_out_dev, joints_out_dev, stream);
  }
#endif
  return enqueue_sample(e, stream, text_emb_dev, init_latents_dev, B, T, latents_out_dev, feats_out_dev, joints_out_dev);
}

// The noise keys of a request's motions into the bound context's key array (stochastic DDIM, include/mldhip.h "Noise contract"): motion k of request i
// gets {seed_i, first_index_i + k}; requests i0 .. i1 - 1 fill the array in chain order.  Stream-ordered like the lengths.
int upload_keys(E* e, const mldhip_request* rq, const mldhip_noise_key* keys, int i0, int i1, hipStream_t stream) {
  WsContext& x = e->ctxs[e->cur_ctx];
  int o = 0;
  for (int i = i0; i < i1; ++i)
    for (int k = 0; k < rq[i].B; ++k, ++o) x.keys_host[o] = NoiseKey{(unsigned long long)keys[i].seed, (long long)keys[i].first_index + k};
  HIP_TRY(e, hipMemcpyAsync(e->keys_dev, x.keys_host.data(), (size_t)o * sizeof(NoiseKey), hipMemcpyHostToDevice, stream));
  return MLDHIP_OK;
}

// The trajectory table of a coalesced call into the bound context's array (mldhip_sample_many_traj): motion k of request i gets {traj[i] + k * D, B_i * D} -- its row
// in step 0 of the request's [steps][B_i][D] buffer and the pitch between steps -- or {NULL, 0} when the request asked for none.  Built on the host into the context's
// stable copy and uploaded with every call, like the keys: the kernels never see a caller pointer as a launch argument, so a captured graph replays with fresh buffers.
int upload_traj(E* e, const mldhip_request* rq, float* const* traj, int nreq, hipStream_t stream) {
  WsContext& x = e->ctxs[e->cur_ctx];
  const long long D = (long long)e->cfg.latent_size * e->cfg.latent_dim;
  int o = 0;
  for (int i = 0; i < nreq; ++i)
    for (int k = 0; k < rq[i].B; ++k, ++o) x.traj_host[o] = traj[i] ? TrajRow{traj[i] + k * D, rq[i].B * D} : TrajRow{nullptr, 0ll};
  HIP_TRY(e, hipMemcpyAsync(e->traj_dev, x.traj_host.data(), (size_t)o * sizeof(TrajRow), hipMemcpyHostToDevice, stream));
  return MLDHIP_OK;
}

// The start table of a coalesced call into the bound context's array (mldhip_sample_many_from): motion k of request i gets {src_i + k * D, first_step_i, noised_i}
// and the two add_noise coefficients of its first step -- or the all-zero entry (start from noise at step 0) when the request has no source (`starts` == nullptr: none
// has one).  Every entry also carries the motion's guidance scale (mldhip_sample_many_guided): guid[i] where it is given and not negative, otherwise the value the plain
// forms get as their launch argument -- the from-forms read it here, so a call without `guid` computes the same expression on the same number as before.  Host copy +
// upload with every call, like the trajectory table: the kernels never see a caller pointer, a first step or a scale as a launch argument.  Returns the call's smallest
// first step.
int upload_starts(E* e, const mldhip_request* rq, const mldhip_start* starts, const float* guid, int nreq, hipStream_t stream, int* step0) {
  WsContext& x = e->ctxs[e->cur_ctx];
  const long long D = (long long)e->cfg.latent_size * e->cfg.latent_dim;
  const float g0 = e->cfg.guidance_scale > 1.0f ? e->cfg.guidance_scale : 1.0f;      // enqueue_sample's `guidance`
  int o = 0, lo = e->cfg.num_inference_steps - 1;
  for (int i = 0; i < nreq; ++i) {
    const mldhip_start s = starts ? starts[i] : mldhip_start{nullptr, 0, 0};
    const DdimCoef k = ddim_coef(e, e->timesteps[s.first_step]);
    const float g = guid && guid[i] >= 0.0f ? guid[i] : g0;
    lo = std::min(lo, (int)s.first_step);
    for (int m = 0; m < rq[i].B; ++m, ++o)
      x.starts_host[o] = s.src_latents_dev ? StartRow{s.src_latents_dev + m * D, s.first_step, s.noised, k.sqrt_at, k.sqrt_1mat, g, 0} : StartRow{nullptr, 0, 0, 0.f, 0.f, g, 0};
  }
  HIP_TRY(e, hipMemcpyAsync(e->starts_dev, x.starts_host.data(), (size_t)o * sizeof(StartRow), hipMemcpyHostToDevice, stream));
  *step0 = lo;
  return MLDHIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------- mldhip_sample_many, pipelined
// "many_pipeline": the requests of a mldhip_sample_many call ONE AFTER THE OTHER, each on the single-request path (the reverse loop of a request is one cluster
// launch, kernels/loop_cluster.hpp) -- the reference's own shape, batch after batch (mld.py:618-672, test.py:116-119) -- with the two halves of consecutive requests
// overlapped: the cluster launch holds 192 of 256 CUs at a few per cent of the matrix pipe for ~6.8 ms, the 44 decode launches of the previous request (one round
// of workgroups each on an idle chip) run beside it on the CUs it leaves free.
//   caller's stream S:  [wait ws(k) free] inputs(k) -> loop(k) -> record loop_done(k)                 ... after the last request: wait for every decode
//   side stream D:                                               wait loop_done(k) -> decode(k) -> outputs(k) -> record ws(k).done
// Two workspaces alternate (request k + 2 waits for decode k).  D has the lowest stream priority: a cluster launch needs its workgroups resident together, the
// decode's workgroups are short and independent of it -- they can only delay it, and they end.  The lane (ClusterLane) is held for the whole call; its event is
// recorded on S behind the join.  Every request gets exactly what mldhip_sample gives it (same kernels, same graphs' machine code): bit-identical, tested.
// Replayed calls whose requests are ONE cluster launch each (every bs-64 request) get the tighter schedule, `split` (three streams):
//   prep stream P:      [ws(k+1): loop k-1 and decode k-1 done] inputs(k+1) -> condition rows + flag clear (a graph, GraphKey.part 1) -> record pre_done(k+1)
//   caller's stream S:  wait pre_done(k) -> cluster launch(k) (issued directly) -> record loop_done(k)
//   side stream D:      wait loop_done(k) -> non-finite count, latents out, lengths -> decode(k) (a graph) -> outputs(k) -> record ws(k).done
// so on S the cluster kernels follow each other with two event packets between them, and the decode of request k (lowest priority) becomes ready at the same instant as
// the launch of request k + 1.  (First form of the round: everything but the decode on S -- 76 us between consecutive cluster kernels, in which the decode's first dozen
// kernels took the chip before the launch did: profiles/r06_trace_pipeline.log.)
struct ManyCall {
  E* e;
  const mldhip_request* rq;
  int nreq;
  const std::vector<int32_t>& tmax;
  const mldhip_noise_key* keys;
  hipStream_t stream;                  // S: the caller's
  hipStream_t side, prep;              // D and P (the simulator, and P of calls that are not split: S itself)
  bool replay = false, split = false;
  std::vector<int> ctx_of, used;       // workspace context of request i; the contexts the call has touched so far

  WsContext& ctx(int i) const { return e->ctxs[ctx_of[i]]; }
  const float* text(int i) const { return is_action(e) ? nullptr : rq[i].text_emb_dev; }
  void touch(int i, int k) {
    ctx_of[i] = k;
    if (std::find(used.begin(), used.end(), k) == used.end()) used.push_back(k);
  }
};

// The stream-ordering steps of a context inside the pipelined call.  The simulator runs everything in issue order: no events, nothing to do.
int wait_context_free(const ManyCall& m, WsContext& x, hipStream_t s) {      // behind the context's last decode (request i - 2, or an earlier call)
#if !defined(MLDHIP_SIM)
  if (x.used) HIP_TRY(m.e, hipStreamWaitEvent(s, x.done, 0));
#endif
  (void)m; (void)x; (void)s;
  return MLDHIP_OK;
}
int record_loop_done(const ManyCall& m, WsContext& x) {
#if !defined(MLDHIP_SIM)
  HIP_TRY(m.e, hipEventRecord(x.loop_done, m.stream));
#endif
  (void)m; (void)x;
  return MLDHIP_OK;
}
int side_waits_for_loop(const ManyCall& m, WsContext& x) {
#if !defined(MLDHIP_SIM)
  HIP_TRY(m.e, hipStreamWaitEvent(m.side, x.loop_done, 0));
#endif
  (void)m; (void)x;
  return MLDHIP_OK;
}
int record_done(const ManyCall& m, WsContext& x) {
#if !defined(MLDHIP_SIM)
  HIP_TRY(m.e, hipEventRecord(x.done, m.side));
  x.used = true;
#endif
  (void)m; (void)x;
  return MLDHIP_OK;
}

// The join, on every exit of the call: the caller's stream is ordered behind every decode of the call.  A call that fails half-way has issued work on P and D that
// nothing of the above waits for: then S additionally waits for both streams as they stand, and every context the call touched gets its completion event behind all of it.
struct ManyJoin {
  ManyCall& m;
  int& rc;
  ~ManyJoin() {
#if !defined(MLDHIP_SIM)
    E* e = m.e;
    if (rc && !m.used.empty()) {
      if (m.prep != m.stream && hipEventRecord(e->many_start, m.prep) == hipSuccess) (void)hipStreamWaitEvent(m.stream, e->many_start, 0);
      hipEvent_t ev = e->ctxs[m.used[0]].done;
      if (hipEventRecord(ev, m.side) == hipSuccess) (void)hipStreamWaitEvent(m.stream, ev, 0);
      for (int k : m.used)
        if (hipEventRecord(e->ctxs[k].done, m.stream) == hipSuccess) e->ctxs[k].used = true;
    }
    for (int k : m.used)
      if (e->ctxs[k].used) (void)hipStreamWaitEvent(m.stream, e->ctxs[k].done, 0);
#endif
  }
};

#if !defined(MLDHIP_SIM)
// the engine's side and prep streams (created on first use), the call's replay / split decision, P ordered behind what S held when the call came in
int many_open(ManyCall& m) {
  E* e = m.e;
  if (!e->side_stream) {
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    HIP_TRY(e, hipStreamCreateWithPriority(&e->side_stream, hipStreamNonBlocking, least));
  }
  m.side = e->side_stream;
  m.replay = m.split = e->cfg.use_graph && e->cluster_graph;
  for (int i = 0; i < m.nreq; ++i) m.split = m.split && use_cluster(e, m.rq[i].B) && m.rq[i].B <= e->cluster_chunk;
  if (m.split && !e->prep_stream) {
    HIP_TRY(e, hipStreamCreateWithFlags(&e->prep_stream, hipStreamNonBlocking));
    HIP_TRY(e, hipEventCreateWithFlags(&e->many_start, hipEventDisableTiming));
  }
  if (m.split) {
    m.prep = e->prep_stream;
    HIP_TRY(e, hipEventRecord(e->many_start, m.stream));
    HIP_TRY(e, hipStreamWaitEvent(m.prep, e->many_start, 0));          // the requests' inputs are the caller's stream's products
  }
  if (m.replay) for (int i = 0; i < m.nreq; ++i) m.touch(i, int(e->next_ctx++ % e->ctxs.size()));      // two contexts alternate
  return MLDHIP_OK;
}

// inputs of request i into its context + what precedes its cluster launch: on P beside the launch of request i - 1 (split), or behind it on S
int many_stage_pre(ManyCall& m, int i) {
  E* e = m.e;
  const mldhip_request& r = m.rq[i];
  WsContext& x = m.ctx(i);
  bind_context(e, m.ctx_of[i]);
  if (int rc = wait_context_free(m, x, m.prep)) return rc;
  if (m.split && i >= 2) HIP_TRY(e, hipStreamWaitEvent(m.prep, x.loop_done, 0));   // ... and its last cluster launch (on S; nothing to wait for when prep IS S)
  if (is_action(e))
    if (int rc = stage_actions(e, r.actions_host, r.B, m.prep)) return rc;
  if (int rc = stage_inputs(e, m.text(i), r.init_latents_dev, r.B, m.prep)) return rc;
  if (m.keys) if (int rc = upload_keys(e, m.rq, m.keys, i, i + 1, m.prep)) return rc;
  if (m.split) {
    hipGraphExec_t pre = nullptr;
    GraphKey kp{r.B, 0, false, false}; kp.part = 1;
    if (int rc = graph_for(e, kp, m.text(i) != nullptr, &pre)) return rc;
    HIP_TRY(e, hipGraphLaunch(pre, m.prep));
    HIP_TRY(e, hipEventRecord(x.pre_done, m.prep));
  }
  return MLDHIP_OK;
}

GraphKey many_decode_key(const ManyCall& m, int i) {
  const mldhip_request& r = m.rq[i];
  const bool want_j = r.joints_out_dev != nullptr;
  GraphKey kd{r.B, m.tmax[i], r.feats_out_dev != nullptr || (want_j && !m.e->dec_lean), want_j};
  kd.dec_only = true;
  return kd;
}

// the reverse loop of request i on S, loop_done(i) behind it
int many_issue_loop(ManyCall& m, int i) {
  E* e = m.e;
  const mldhip_request& r = m.rq[i];
  WsContext& x = m.ctx(i);
  if (m.split) {
    HIP_TRY(e, hipStreamWaitEvent(m.stream, x.pre_done, 0));
    // the launch itself is issued directly, not as a graph of one kernel (a graph launch puts its own packets in front of its first node)
    e->sample_part = 2;
    const int rc = enqueue_sample(e, m.stream, m.text(i) ? e->text_in : nullptr, e->lat_in, r.B, 0, nullptr, nullptr, nullptr);
    e->sample_part = 0;
    if (rc) return rc;
  } else {
    hipGraphExec_t loop = nullptr;
    if (int rc = graph_for(e, GraphKey{r.B, m.tmax[i], false, false}, m.text(i) != nullptr, &loop)) return rc;
    HIP_TRY(e, hipGraphLaunch(loop, m.stream));
    if (int rc = copy_outputs(e, r.B, m.tmax[i], r.latents_out_dev, nullptr, nullptr, m.stream)) return rc;
  }
  return record_loop_done(m, x);
}

// the decode of request i on D behind loop_done(i), its outputs, ws(i).done behind them
int many_issue_decode(ManyCall& m, int i, hipGraphExec_t dec) {
  E* e = m.e;
  const mldhip_request& r = m.rq[i];
  WsContext& x = m.ctx(i);
  bind_context(e, m.ctx_of[i]);
  if (int rc = side_waits_for_loop(m, x)) return rc;
  if (m.split) {
    Ctx cs{e, m.side};
    count_nonfinite(cs, e->lat, (long long)r.B * e->cfg.latent_dim);
    if (cs.rc) return cs.rc;
    if (int rc = copy_outputs(e, r.B, m.tmax[i], r.latents_out_dev, nullptr, nullptr, m.side)) return rc;
  }
  // the lengths are the decode's alone (the latent loop has no masks): copied on the side stream, in order behind the decode that used this context last
  HIP_TRY(e, hipMemcpyAsync(e->lens_dev, r.lengths_host, (size_t)r.B * sizeof(int32_t), hipMemcpyHostToDevice, m.side));
  HIP_TRY(e, hipGraphLaunch(dec, m.side));
  if (int rc = copy_outputs(e, r.B, m.tmax[i], nullptr, r.feats_out_dev, r.joints_out_dev, m.side)) return rc;
  return record_done(m, x);
}
#endif

// eager issue (no graphs: the simulator; hooks builds with "cluster_graph" 0): the two halves one behind the other per request, outputs straight into the caller's buffers
int many_issue_eager(ManyCall& m, int i) {
  E* e = m.e;
  const mldhip_request& r = m.rq[i];
  const int k = int(e->next_ctx++ % e->ctxs.size()), B = r.B, T = m.tmax[i];
  WsContext& x = e->ctxs[k];
  if (int rc = wait_context_free(m, x, m.stream)) return rc;
  bind_context(e, k);
  m.touch(i, k);
  HIP_TRY(e, hipMemcpyAsync(e->lens_dev, r.lengths_host, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, m.stream));
  if (m.keys) if (int rc = upload_keys(e, m.rq, m.keys, i, i + 1, m.stream)) return rc;
  if (is_action(e))
    if (int rc = stage_actions(e, r.actions_host, B, m.stream)) return rc;
  if (int rc = enqueue_sample(e, m.stream, m.text(i), r.init_latents_dev, B, T, r.latents_out_dev, nullptr, nullptr)) return rc;
  if (int rc = record_loop_done(m, x)) return rc;
  if (int rc = side_waits_for_loop(m, x)) return rc;
  Ctx cd{e, m.side};
  enqueue_decode(cd, B, T, r.feats_out_dev, r.joints_out_dev);
  if (cd.rc) return cd.rc;
  return record_done(m, x);
}

int sample_many_pipelined(E* e, const mldhip_request* rq, int nreq, const std::vector<int32_t>& tmax, hipStream_t stream, const mldhip_noise_key* keys) {
  ClusterLane lane(e, stream, e->cluster_lane);
  ManyCall m{e, rq, nreq, tmax, keys, stream, stream, stream};
  m.ctx_of.assign(nreq, 0);
  int rc = MLDHIP_OK;
  ManyJoin join{m, rc};                 // runs on every return below, in front of the lane's release
#if !defined(MLDHIP_SIM)
  if ((rc = many_open(m))) return rc;
  if (m.replay) {
    if ((rc = many_stage_pre(m, 0))) return rc;
    for (int i = 0; i < nreq; ++i) {
      bind_context(e, m.ctx_of[i]);
      hipGraphExec_t dec = nullptr;     // looked up (or captured) before anything of request i is issued
      if ((rc = graph_for(e, many_decode_key(m, i), m.text(i) != nullptr, &dec))) return rc;
      if ((rc = many_issue_loop(m, i))) return rc;
      if (i + 1 < nreq && (rc = many_stage_pre(m, i + 1))) return rc;
      if ((rc = many_issue_decode(m, i, dec))) return rc;
    }
    return rc;
  }
#endif
  for (int i = 0; i < nreq && !rc; ++i) rc = many_issue_eager(m, i);
  return rc;
}

// ---------------------------------------------------------------------------------------------------------------- mldhip_sample_many, coalesced
// Several independent requests as ONE reverse-diffusion chain + ONE decode (mldhip_sample_many): inputs are gathered into
// the engine's staging buffers (unconditional halves first, as one big CFG batch), outputs scattered per request with
// each request's own Tmax as its row pitch.  Motions never interact (attention is per sample), so results equal the
// per-request calls up to the summation order of the kernel family picked for the larger row count.
// lat_of (or nullptr: the requests' init_latents_dev): the [B_i][D] buffer gathered as request i's start latents
int gather_requests(Ctx& c, const mldhip_request* rq, int nreq, int Btot, const float* const* lat_of = nullptr) {
  E* e = c.e;
  const bool action = is_action(e);
  const long long D = e->cfg.latent_dim, TD = e->cfg.text_dim;
  GatherArgs ga;
  int o = 0, bmax = 0;
  for (int i = 0; i < kMaxRequests; ++i) { ga.text[i] = nullptr; ga.lat[i] = nullptr; ga.off[i] = 0; ga.nb[i] = 0; }
  for (int i = 0; i < nreq; ++i) {
    ga.text[i] = action ? nullptr : rq[i].text_emb_dev; ga.lat[i] = lat_of ? lat_of[i] : rq[i].init_latents_dev; ga.off[i] = o; ga.nb[i] = rq[i].B;
    o += rq[i].B; bmax = std::max(bmax, (int)rq[i].B);
  }
  ga.text_in = e->text_in; ga.lat_in = e->lat_in; ga.Btot = Btot; ga.TD = (int)TD; ga.D = (int)D;
  const long long per = (action ? 0 : 2LL * bmax * TD) + (long long)bmax * D;      // elements of the largest request
  const unsigned chunks = (unsigned)std::min<long long>(64, std::max<long long>(1, (per + 2047) / 2048));
  MLD_LAUNCH(gather_requests_kernel, dim3((unsigned)nreq, chunks), dim3(256), 0, c.stream, ga);
  return check_launch(c, "gather_requests");
}

int scatter_results(Ctx& c, const mldhip_request* rq, int nreq, const std::vector<int32_t>& tmax, int T) {
  E* e = c.e;
  ScatterArgs sa;
  int o = 0, bmax = 0;
  for (int i = 0; i < kMaxRequests; ++i) { sa.lat_out[i] = nullptr; sa.feats_out[i] = nullptr; sa.joints_out[i] = nullptr; sa.off[i] = 0; sa.nb[i] = 0; sa.tmax[i] = 0; }
  for (int i = 0; i < nreq; ++i) {
    sa.lat_out[i] = rq[i].latents_out_dev; sa.feats_out[i] = rq[i].feats_out_dev; sa.joints_out[i] = rq[i].joints_out_dev;
    sa.off[i] = o; sa.nb[i] = rq[i].B; sa.tmax[i] = tmax[i];
    o += rq[i].B; bmax = std::max(bmax, (int)rq[i].B);
  }
  sa.lat = e->lat; sa.feats = e->feats_int; sa.joints = e->joints_int; sa.T = T;
  sa.D = e->cfg.latent_dim; sa.NF = e->cfg.nfeats; sa.NJ = e->cfg.njoints * 3;
  MLD_LAUNCH(scatter_results_kernel, dim3((unsigned)nreq, (unsigned)bmax), dim3(256), 0, c.stream, sa);
  return check_launch(c, "scatter_results");
}

// `traj` (or nullptr): per request, the [steps][B_i][D] buffer that receives the latents after every scheduler step (mldhip_sample_many_traj); a call that asks
// for any runs as one chain, also under "many_pipeline" 1.  `starts` (or nullptr): per request, where its motions enter the loop (mldhip_sample_many_from; checked by
// the caller); a call with any source is one chain as well, on the from-forms of the loop kernels.  `guid` (or nullptr): per request, its guidance scale or a negative
// value for the handle's own (mldhip_sample_many_guided; the caller passes it only when some entry is not negative): the same from-forms, which take every motion's
// scale from its start entry -- a guided call without sources is a from-call whose starts are all trivial
int sample_many_impl(E* e, const mldhip_request* rq, int nreq, hipStream_t stream, const mldhip_noise_key* keys = nullptr, float* const* traj = nullptr,
                     const mldhip_start* starts = nullptr, const float* guid = nullptr) {
  if (!e->finalized) return e->fail(MLDHIP_ESTATE, "mldhip_sample_many before mldhip_finalize_weights");
  heal_cluster(e);
  const bool action = is_action(e);
  bool want_j = false, want_f = false;
  int Btot = 0, T = 0;
  std::vector<int32_t> lens, tmax(nreq, 0);
  for (int i = 0; i < nreq; ++i) {
    const mldhip_request& r = rq[i];
    const bool resumes = starts && starts[i].src_latents_dev && starts[i].noised;      // the loop state is the source as it is: init_latents is not read
    if ((!r.init_latents_dev && !resumes) || (action ? !r.actions_host : !r.text_emb_dev)) return e->fail(MLDHIP_EINVAL, "request %d: null input pointer", i);
    if (r.joints_out_dev && is_actor(e)) return e->fail(MLDHIP_ESTATE, "joints of the ActorVae feature layout need SMPL (out of scope)");
    if (int rc = validate_lengths(e, r.lengths_host, r.B, &tmax[i])) return rc;
    if (action)
      if (int rc = check_actions(e, r.actions_host, r.B, i)) return rc;
    lens.insert(lens.end(), r.lengths_host, r.lengths_host + r.B);
    Btot += r.B;
    T = std::max(T, tmax[i]);
    want_j = want_j || r.joints_out_dev;
    want_f = want_f || r.feats_out_dev || (r.joints_out_dev && !e->dec_lean);      // features for a caller (any request): the full [M][263] rows; joints alone do not need them ("dec_lean")
  }
  if (!e->group_ready[kGroupDenoiser] || !e->group_ready[kGroupVaeDecoder] || (want_j && !e->group_ready[kGroupStats]))
    return e->fail(MLDHIP_ESTATE, "mldhip_sample_many needs denoiser.*, vae.decoder.* (and mean/std for joints) loaded");
  bool want_t = false;
  for (int i = 0; traj && i < nreq; ++i) want_t = want_t || traj[i];
  bool want_s = guid != nullptr;
  for (int i = 0; starts && i < nreq; ++i) want_s = want_s || starts[i].src_latents_dev;
  if (e->many_pipeline && nreq >= 2 && e->ctxs.size() >= 2 && !want_t && !want_s) {
    bool ok = true;
    for (int i = 0; i < nreq; ++i) ok = ok && use_cluster(e, rq[i].B) && (rq[i].feats_out_dev || rq[i].joints_out_dev);
    if (ok) return sample_many_pipelined(e, rq, nreq, tmax, stream, keys);
  }
  if (Btot > e->cfg.max_batch) return e->fail(MLDHIP_EINVAL, "requests hold %d motions, max_batch is %d", Btot, e->cfg.max_batch);
  CtxUse use(e, stream);
  if (use.rc) return use.rc;
  ClusterLane lane(e, stream, e->cluster_lane && use_cluster(e, Btot));
  HIP_TRY(e, hipMemcpyAsync(e->lens_dev, lens.data(), (size_t)Btot * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  if (keys) if (int rc = upload_keys(e, rq, keys, 0, nreq, stream)) return rc;
  if (want_t) if (int rc = upload_traj(e, rq, traj, nreq, stream)) return rc;
  int step0 = 0;
  if (want_s) if (int rc = upload_starts(e, rq, starts, guid, nreq, stream, &step0)) return rc;
  if (action) {
    // stage_actions' layout for the gathered batch, built on the host (the requests' labels are not contiguous): one copy
    std::vector<int32_t> lab(2 * (size_t)Btot, 0);
    int o = 0;
    for (int i = 0; i < nreq; ++i) { std::copy(rq[i].actions_host, rq[i].actions_host + rq[i].B, lab.begin() + Btot + o); o += rq[i].B; }
    HIP_TRY(e, hipMemcpyAsync(e->labels_dev, lab.data(), lab.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  }
  Ctx cio{e, stream};
  std::vector<const float*> lat_of;
  if (want_s) {      // a resumed request may come without init_latents: its source stands in for the gather (same shape; the from-forms never read those rows)
    for (int i = 0; i < nreq; ++i) lat_of.push_back(rq[i].init_latents_dev || !starts ? rq[i].init_latents_dev : starts[i].src_latents_dev);
  }
  if (int rc = gather_requests(cio, rq, nreq, Btot, want_s ? lat_of.data() : nullptr)) return rc;
  const float* text = action ? nullptr : e->text_in;
#if !defined(MLDHIP_SIM)
  if (replays(e, Btot)) {
    hipGraphExec_t exec = nullptr;
    GraphKey key{Btot, T, want_f, want_j};
    key.traj = want_t;
    key.from = want_s;
    // the one-launch loops read the first steps from the table (one graph for all of them); the other families' host loop issues steps step0 .. n-1
    key.step0 = want_s && !(use_cluster(e, Btot) || use_fused(e, Btot)) ? step0 : 0;
    if (int rc = graph_for(e, key, text != nullptr, &exec)) return rc;
    HIP_TRY(e, hipGraphLaunch(exec, stream));
  } else
#endif
  {
    e->traj_on = want_t;
    e->from_on = want_s;
    e->from_step0 = step0;
    const int rc = enqueue_sample(e, stream, text, e->lat_in, Btot, T, nullptr, want_f ? e->feats_int : nullptr, want_j ? e->joints_int : nullptr);
    e->traj_on = false;
    e->from_on = false;
    if (rc) return rc;
  }
  return scatter_results(cio, rq, nreq, tmax, T);
}

// ---------------------------------------------------------------------------------------------------------------- one denoiser step; the diffusion-only call
int denoiser_forward_impl(E* e, const float* sample_dev, int32_t timestep, const float* text_emb_dev,
                          const int32_t* actions_host, int32_t R, float* out_dev, void* stream_) {
  if (!e->finalized || !e->group_ready[kGroupDenoiser]) return e->fail(MLDHIP_ESTATE, "denoiser_forward before finalize / denoiser.* not loaded");
  if (!sample_dev || !out_dev) return e->fail(MLDHIP_EINVAL, "null pointer");
  if (R < 1 || R > 2 * e->cfg.max_batch) return e->fail(MLDHIP_EINVAL, "R=%d outside [1, 2*max_batch]", R);
  if (timestep < 0 || timestep >= e->cfg.num_train_timesteps) return e->fail(MLDHIP_EINVAL, "timestep %d out of range", timestep);
  hipStream_t stream = (hipStream_t)stream_;
  CtxUse use(e, stream);                                  // picks + binds a workspace context (see WsContext)
  if (use.rc) return use.rc;
  Ctx c{e, stream};
  const int D = e->cfg.latent_dim;
  e->phase = 0;
  if (actions_host) {
    if (int rc = check_actions(e, actions_host, R)) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->labels_dev, actions_host, (size_t)R * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  }
  if (int rc = single_timestep_row(c, timestep)) return rc;
  const DenView v = den_view(e, R);
  if (text_emb_dev) text_projection(c, text_emb_dev, R, e->X0 + (size_t)2 * R * D);
  else action_rows(c, R, e->cfg.guidance_scale > 1.0f ? R / 2 : 0, e->X0 + (size_t)2 * R * D);   // mld_denoiser.py:253-257
  // token 0 rows: sample + pe[0]; token 1 rows: the time-MLP row (pe[1] already folded in)
  MLD_LAUNCH(add_rows_kernel, dim3((R * D + 255) / 256), dim3(256), 0, stream, e->X0, sample_dev, P(e, "denoiser.query_pos.pe"), R, D);
  MLD_LAUNCH(bcast_rows_kernel, dim3((R * D + 255) / 256), dim3(256), 0, stream, e->X0 + (size_t)R * D, (const float*)e->t1_one, R, D);
  check_launch(c, "assemble");
  denoiser_body(c, v);
  MLD_LAUNCH(den_final_rows_kernel, dim3(R), dim3(256), 0, stream, den_final_args(e, v), out_dev);
  check_launch(c, "final_norm");
  return c.rc;
}

int denoiser_forward_novae_impl(E* e, const float* sample_dev, int32_t timestep, const float* text_emb_dev,
                                const int32_t* lengths_host, int32_t R, int32_t T, float* out_dev, void* stream_) {
  if (!e->finalized || !e->group_ready[kGroupDenoiser]) return e->fail(MLDHIP_ESTATE, "denoiser_forward_novae before finalize / denoiser.* not loaded");
  if (!sample_dev || !text_emb_dev || !lengths_host || !out_dev) return e->fail(MLDHIP_EINVAL, "null pointer");
  if (R < 1 || R > 2 * e->cfg.max_batch) return e->fail(MLDHIP_EINVAL, "R=%d outside [1, 2*max_batch]", R);
  if (T < 1 || T > e->cfg.max_frames) return e->fail(MLDHIP_EINVAL, "T=%d outside [1, max_frames=%d]", T, e->cfg.max_frames);
  if (timestep < 0 || timestep >= e->cfg.num_train_timesteps) return e->fail(MLDHIP_EINVAL, "timestep %d out of range", timestep);
  for (int i = 0; i < R; ++i)
    if (lengths_host[i] < 0 || lengths_host[i] > T) return e->fail(MLDHIP_EINVAL, "lengths[%d]=%d outside [0, T=%d]", i, lengths_host[i], T);
  hipStream_t stream = (hipStream_t)stream_;
  CtxUse use(e, stream);                                  // picks + binds a workspace context (see WsContext)
  if (use.rc) return use.rc;
  Ctx c{e, stream};
  const int D = e->cfg.latent_dim;
  e->phase = 0;
  HIP_TRY(e, hipMemcpyAsync(e->lens_dev, lengths_host, (size_t)R * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  if (int rc = single_timestep_row(c, timestep)) return rc;
  novae_memory_kv(c, e->t1_one, 1, e->TKV_one, (long long)2 * D);
  novae_fold_memory(c, e->TKV_one, 1, (long long)2 * D, e->TKW_one, e->TKU_one, e->TKC_one);
  novae_text_memory(c, text_emb_dev, R);
  novae_pad_input(c, sample_dev, (long long)R * T, 1);
  novae_denoiser_body(c, R, T, e->TKV_one, (long long)2 * D, NovaeFold{e->TKW_one, e->TKU_one, e->TKC_one, 1}, out_dev);
  return c.rc;
}

int sample_novae_impl(E* e, const float* text_emb_dev, const float* init_latents_dev, const int32_t* lengths_host,
                      int32_t B, const float* step_noise_dev, uint64_t seed, float* feats_out_dev, float* joints_out_dev, void* stream_) {
  if (!e->finalized || !e->group_ready[kGroupDenoiser] || (joints_out_dev && !e->group_ready[kGroupStats]))
    return e->fail(MLDHIP_ESTATE, "mldhip_sample_novae needs finalize and denoiser.* (and mean/std for joints) loaded");
  if (!text_emb_dev || !init_latents_dev) return e->fail(MLDHIP_EINVAL, "null input pointer");
  int T = 0;
  if (int rc = validate_lengths(e, lengths_host, B, &T)) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  CtxUse use(e, stream);                                  // picks + binds a workspace context (see WsContext)
  if (use.rc) return use.rc;
  HIP_TRY(e, hipMemcpyAsync(e->lens_dev, lengths_host, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  HIP_TRY(e, hipMemcpyAsync(e->lens_dev + B, lengths_host, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, stream));   // lengths * 2 (mld.py:327-328)
  if (int rc = novae_prologue(e, stream, text_emb_dev, init_latents_dev, B, T)) return rc;
#if !defined(MLDHIP_SIM)
  if (e->cfg.use_graph && !step_noise_dev) {              // the steps as replays of captured chunks (engine/graphs.hpp); injected noise: eager
    if (int rc = replay_steps(e, stream, B, T, seed)) return rc;
  } else
#endif
  if (int rc = novae_steps(e, stream, B, T, 0, e->cfg.num_inference_steps, step_noise_dev, seed, nullptr)) return rc;
  return novae_epilogue(e, stream, B, T, feats_out_dev, joints_out_dev);
}

}  // namespace
