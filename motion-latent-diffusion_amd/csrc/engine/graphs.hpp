// Captured graphs: the one capture helper, the per-context cache of sample() graphs, the step-graph cache of the diffusion-only
// variant, and the one place that destroys a context's graphs.  Every hipGraphExecDestroy of the library is in this file.
// Part of libmldhip's single translation unit; include order: see mldhip.hip.  Internal linkage throughout (anonymous namespace).
#pragma once

namespace {

constexpr int kStepChunk = 20;                 // DDPM steps per captured graph (diffusion-only variant)
constexpr size_t kGraphCacheCapacity = 48;     // captured graphs kept per workspace context

// Destroys every captured graph of one workspace context.  Captured graphs bake in the kernel choice, the derived tables and the
// cluster kernel: whoever changes one of these (mldhip_set_option, finalize, a handle that leaves the cluster loop) or frees the
// buffers they use (destroy) calls this.  drain: an exec may still be replaying on the context's last stream -- wait for the context's
// completion event first (callers that have just synchronised the device pass false).
void drop_graphs(WsContext& x, bool drain) {
#if !defined(MLDHIP_SIM)
  if (drain) drain_context(x);
  for (auto& kv : x.graphs) (void)hipGraphExecDestroy(kv.second);
  x.graphs.clear();
  x.graph_lru.clear();
  for (auto& kv : x.step_graphs) (void)hipGraphExecDestroy(kv.second);
  x.step_graphs.clear();
#endif
  (void)x; (void)drain;
}

void drop_graphs(E* e, bool drain) {
  for (auto& x : e->ctxs) drop_graphs(x, drain);
}

#if !defined(MLDHIP_SIM)
// begin capture on the engine's capture stream -> body() enqueues on it -> end capture -> instantiate, with the error ladder; `what` tags the messages
template <class Body>
int capture(E* e, const char* what, hipGraphExec_t* out, Body body) {
  hipGraph_t graph = nullptr;
  HIP_TRY(e, hipStreamBeginCapture(e->cap_stream, hipStreamCaptureModeRelaxed));
  const int rc = body();
  hipError_t s = hipStreamEndCapture(e->cap_stream, &graph);
  if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
  if (s != hipSuccess) return e->fail(MLDHIP_EHIP, "hipStreamEndCapture%s: %s", what, hipGetErrorString(s));
  s = hipGraphInstantiate(out, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (s != hipSuccess) return e->fail(MLDHIP_EHIP, "hipGraphInstantiate%s: %s", what, hipGetErrorString(s));
  return MLDHIP_OK;
}

// The captured graph of (B, Tmax, requested outputs) on the bound workspace context: looked up, or captured now.  Graphs
// read the engine's staging buffers (text_in / lat_in / labels / lens) and write lat / feats_int / joints_int, so they
// are independent of the caller's buffers and of how many requests make up the B motions.
int graph_for(E* e, const GraphKey& key, bool text_condition, hipGraphExec_t* out) {
  auto& graphs = e->ctxs[e->cur_ctx].graphs;
  auto& lru = e->ctxs[e->cur_ctx].graph_lru;
  auto same = [&](const GraphKey& k) { return !(k < key) && !(key < k); };
  lru.erase(std::remove_if(lru.begin(), lru.end(), same), lru.end());
  lru.push_back(key);
  auto it = graphs.find(key);
  if (it == graphs.end()) {
    // one graph per (B, Tmax, outputs): a serving loop with ragged batches sees many Tmax values, so keep a generous
    // number (each exec holds ~2 100 kernel nodes, a few MB) and evict the least recently used one beyond it
    while (graphs.size() >= kGraphCacheCapacity) {
      auto victim = graphs.find(lru.front());
      lru.erase(lru.begin());
      if (victim == graphs.end()) continue;
      drain_context(e->ctxs[e->cur_ctx]);               // the victim may still be replaying on this context's last stream
      (void)hipGraphExecDestroy(victim->second);
      graphs.erase(victim);
    }
    hipGraphExec_t exec = nullptr;
    const int rc = capture(e, "", &exec, [&]() -> int {
      if (key.dec_only) {
        Ctx cd{e, e->cap_stream};
        enqueue_decode(cd, key.B, key.T, key.feats ? e->feats_int : nullptr, key.joints ? e->joints_int : nullptr);
        return cd.rc;
      }
      e->sample_part = key.part;
      e->traj_on = key.traj;
      e->from_on = key.from;
      e->from_step0 = key.step0;
      const int r = enqueue_sample(e, e->cap_stream, text_condition ? e->text_in : nullptr, e->lat_in, key.B, key.T, nullptr,
                                   key.feats ? e->feats_int : nullptr, key.joints ? e->joints_int : nullptr);
      e->sample_part = 0;
      e->traj_on = false;
      e->from_on = false;
      return r;
    });
    if (rc) return rc;
    it = graphs.emplace(key, exec).first;
  }
  *out = it->second;
  return MLDHIP_OK;
}

// Diffusion-only variant: the n DDPM steps of a call as replays of graphs captured once per (B, Tmax, chunk of kStepChunk steps).
// ~114 launches per step: a 1000-step call is 114 k launches.  Issued eagerly they keep one host thread busy for the
// whole call, so a second call on another stream cannot even be enqueued before the first is nearly done.  Everything a
// step needs is a constant of (weights, step index) except the Philox seed, which the step kernel reads from the workspace.
int replay_steps(E* e, hipStream_t stream, int B, int T, unsigned long long seed) {
  WsContext& x = e->ctxs[e->cur_ctx];
  const int n = e->cfg.num_inference_steps;
  x.seed_host = seed;
  HIP_TRY(e, hipMemcpyAsync(e->seed_slot, &x.seed_host, sizeof seed, hipMemcpyHostToDevice, stream));
  const int nchunks = (n + kStepChunk - 1) / kStepChunk;
  if (x.step_graphs.size() + nchunks > 512) drop_graphs(x, true);
  for (int ch = 0; ch < nchunks; ++ch) {
    auto key = std::make_tuple(B, T, ch);
    auto it = x.step_graphs.find(key);
    if (it == x.step_graphs.end()) {
      hipGraphExec_t exec = nullptr;
      if (int rc = capture(e, "(steps)", &exec, [&]() {
            return novae_steps(e, e->cap_stream, B, T, ch * kStepChunk, std::min(n, (ch + 1) * kStepChunk), nullptr, 0,
                               reinterpret_cast<const unsigned long long*>(e->seed_slot));
          })) return rc;
      it = x.step_graphs.emplace(key, exec).first;
    }
    HIP_TRY(e, hipGraphLaunch(it->second, stream));
  }
  return MLDHIP_OK;
}
#endif

}  // namespace
