// libmldhip: engine + C ABI (include/mldhip.h) for the MLD sampling hot path on MI355X (gfx950).
//
// Host-side structure (what the reference leaves to PyTorch/Lightning, rebuilt natively):
//   ParamTable   one HBM arena holding every weight the path reads, laid out per layer in execution
//                order with a uniform per-layer stride (lets one launch cover all 9 layers' tiny
//                cross-attention GEMMs via blockIdx.z);
//   Workspace    one HBM arena for activations, sized from (max_batch, max_frames) at create();
//   Schedule     DDIM tables (float32, as diffusers keeps them) + the time-MLP output for each of
//                the scheduler's timesteps, computed once at finalize (they depend on weights only);
//   sample()     ~2.1k kernel launches captured once per (B, Tmax, requested outputs) and workspace context into a
//                hipGraph and replayed: the 50-step loop has no host work and no host<->device sync.
//
// Source layout, in include order; then the C ABI below: each entry point is its argument checks and a call into the engine.  kernels/*.hpp hold the device code (no __global__ in this file).
//   engine/state.hpp         handle, contexts, weight groups, probe verdicts
//   engine/params.hpp        weight contract, schedules
//   engine/dispatch.hpp      kernel selection, the counted launch
//   engine/path_loop.hpp     the latent models' reverse loop
//   engine/streams.hpp       finalize-time weight images
//   engine/path_vae.hpp      VAE decode / encode, feats2joints
//   engine/path_latent.hpp   the latent models' sample calls
//   engine/path_novae.hpp    the diffusion-only variant's sample calls
//   engine/path_clip.hpp     the CLIP text tower
//   engine/path_eval.hpp     the T2M evaluator towers
//   engine/path_smpl.hpp     the SMPL body model
//   engine/path_a2m.hpp      the HumanAct12 recognition GRU
//   engine/path_uestc.hpp    the UESTC recognition ST-GCN
//   engine/path_metrics.hpp  the text-to-motion metric kernels
//   engine/graphs.hpp        graph capture and caches
//   engine/create.hpp        validation and defaults, workspace carve, LDS registration, teardown
//   engine/serve.hpp         the sampling drivers and their shared host sequences
//   engine/probe.hpp         range probe
// One translation unit: hipcc builds it in one pass for gfx950.
//
// Reference call stack being replaced: mld/models/modeltype/mld.py:216-265,290-360.
#include "../../include/mldhip.h"
#if defined(MLDHIP_HOOKS)
#include "../../include/mldhip_hooks.h"
#endif

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <tuple>
#include <vector>
#include "kernels/attention.hpp"
#include "kernels/elementwise.hpp"
#include "kernels/gemm.hpp"
#include "kernels/gemm_pipe.hpp"
#include "kernels/novae.hpp"
#include "kernels/rt.hpp"
#include "kernels/tile32.hpp"
#include "kernels/strip.hpp"
#include "kernels/loop_fused.hpp"
#include "kernels/loop_cluster.hpp"
#include "kernels/ffn_strip.hpp"
#include "kernels/gemm_strip_x3.hpp"
#include "kernels/final_strip.hpp"
#include "kernels/dec_half.hpp"
#include "kernels/clip_text.hpp"
#include "kernels/gru.hpp"
#include "kernels/smpl.hpp"
#include "kernels/a2m_gru.hpp"
#include "kernels/stgcn.hpp"
#include "kernels/t2m_metrics.hpp"

using namespace mld;

#include "engine/state.hpp"
#include "engine/params.hpp"
#include "engine/dispatch.hpp"
#include "engine/path_loop.hpp"
#include "engine/streams.hpp"
#include "engine/path_vae.hpp"
#include "engine/path_latent.hpp"
#include "engine/path_novae.hpp"
#include "engine/path_clip.hpp"
#include "engine/path_eval.hpp"
#include "engine/path_smpl.hpp"
#include "engine/path_a2m.hpp"
#include "engine/path_uestc.hpp"
#include "engine/path_metrics.hpp"
#include "engine/graphs.hpp"
#include "engine/create.hpp"
#include "engine/serve.hpp"
#include "engine/probe.hpp"
#include "kernels/ddim_step.hpp"   // (last on purpose: see the file)

// ======================================================================================= C ABI

// Struct sizes a caller may pass.  Fields were appended over time, some without a new ABI number: a caller built before an append passes the struct that ends
// behind the last field it knows, and what it does not cover keeps its default (the module is off; a numeric_info field is not written).
#define MLDHIP_ENDS_BEHIND(T, field) (int32_t)(offsetof(T, field) + sizeof(T::field))
template <size_t N>
static bool size_accepted(const int32_t (&sizes)[N], int32_t size) { return std::find(sizes, sizes + N, size) != sizes + N; }

extern "C" {

int mldhip_abi_version(void) { return MLDHIP_ABI_VERSION; }

void mldhip_default_config(mldhip_config* c) {
  std::memset(c, 0, sizeof *c);
  c->struct_size = sizeof(mldhip_config);
  c->latent_dim = 256; c->latent_size = 1; c->ff_size = 1024; c->num_layers = 9; c->num_heads = 4;
  c->nfeats = 263; c->njoints = 22; c->text_dim = 768; c->max_batch = 64; c->max_frames = 196;
  c->num_train_timesteps = 1000; c->num_inference_steps = 50; c->steps_offset = 1; c->set_alpha_to_one = 0;
  c->beta_start = 0.00085f; c->beta_end = 0.012f; c->guidance_scale = 7.5f;
  c->precision = MLDHIP_PREC_F32; c->use_graph = 1;
  c->condition = MLDHIP_COND_TEXT; c->nclasses = 0; c->vae_arch = MLDHIP_VAE_MLD; c->vae_num_layers = 0;
  c->denoiser_arch = MLDHIP_ARCH_TRANS_ENC; c->scheduler_type = MLDHIP_SCHED_DDIM;
  c->max_in_flight = 1;
  // no text tower by default (clip_layers 0); the other fields are CLIP ViT-L/14's, clip_max_prompts 0 = 2 x max_batch
  c->clip_layers = 0; c->clip_heads = 12; c->clip_ff = 3072; c->clip_vocab = 49408; c->clip_ctx = 77; c->clip_max_prompts = 0;
  // every other optional module is off by default and its capacities are 0 = the defaults of resolve_defaults (engine/create.hpp): all zero bits, as the memset left them
}

const char* mldhip_last_error(mldhip_handle* h) { return h ? h->err.c_str() : g_last_error.c_str(); }

int mldhip_create(const mldhip_config* cfg, int device, mldhip_handle** out) {
  auto bad = [&](const char* m) { g_last_error = m; return MLDHIP_EINVAL; };
  if (!cfg || !out) return bad("null argument");
  constexpr int32_t kConfigAbi5 = MLDHIP_ENDS_BEHIND(mldhip_config, max_in_flight);
  constexpr int32_t kConfigSizes[] = {
      kConfigAbi5,                                              // ABI 5 caller: no eta (it is 0 then, whatever the default)
      MLDHIP_ENDS_BEHIND(mldhip_config, eta),                   // ABI 6 caller: no text tower
      MLDHIP_ENDS_BEHIND(mldhip_config, clip_max_prompts),      // ABI 7 caller from before the t2m_* fields: no evaluators
      MLDHIP_ENDS_BEHIND(mldhip_config, t2m_max_words),         // ... from before smpl_verts: no body model
      MLDHIP_ENDS_BEHIND(mldhip_config, smpl_verts),            // ... from before the a2m_* fields: no recognition GRU
      MLDHIP_ENDS_BEHIND(mldhip_config, a2m_max_motions),       // ... from before the uestc_* fields: no recognition ST-GCN
      MLDHIP_ENDS_BEHIND(mldhip_config, uestc_classes),         // ... from before the two metric fields: no metric kernels
      (int32_t)sizeof(mldhip_config),                           // today's caller
  };
  if (!size_accepted(kConfigSizes, cfg->struct_size)) return bad("mldhip_config.struct_size mismatch (ABI skew)");
  mldhip_config full;
  mldhip_default_config(&full);                       // fields the caller's struct does not cover keep their defaults ...
  if (cfg->struct_size == kConfigAbi5) full.eta = 0.0f;
  std::memcpy(&full, cfg, (size_t)cfg->struct_size);  // ... every field it covers is the caller's
  full.struct_size = (int32_t)sizeof(mldhip_config);
  resolve_defaults(full);
  if (const char* what = config_error(&full)) return bad(what);
  int num_cus = 0;
  if (int rc = check_device(device, &num_cus)) return rc;
  return create_engine(full, device, num_cus, out);
}

void mldhip_destroy(mldhip_handle* e) {
  if (e) destroy_engine(e);
}

int mldhip_load_tensor(mldhip_handle* e, const char* key, const void* data, const int64_t* shape, int32_t ndim,
                       int32_t dtype, int32_t src_is_device) {
  if (!e || !key || !data || (!shape && ndim > 0)) return e ? e->fail(MLDHIP_EINVAL, "null argument") : MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  if (dtype != MLDHIP_F32) return e->fail(MLDHIP_EINVAL, "tensor %s: only float32 tensors are accepted", key);
  auto it = e->index.find(key);
  if (it == e->index.end()) return ignorable_key(key) ? 1 : e->fail(MLDHIP_EINVAL, "unexpected key %s", key);
  Param& p = e->params[it->second];
  size_t numel = 1;
  for (int i = 0; i < ndim; ++i) numel *= size_t(shape[i]);
  bool same = (size_t)ndim == p.shape.size();
  for (int i = 0; same && i < ndim; ++i) same = shape[i] == p.shape[i];
  if (!same && numel == p.numel && (ndim == 1 || p.shape.size() == 1)) same = true;   // tolerate squeezed vectors
  if (!same) return e->fail(MLDHIP_EINVAL, "shape mismatch for %s (expected %zu elements, got %zu)", key, p.numel, numel);
  HIP_TRY(e, hipMemcpy(e->arena + p.offset, data, p.numel * sizeof(float), src_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  p.loaded = true;
  e->finalized = false;
  return MLDHIP_OK;
}

int mldhip_set_option(mldhip_handle* e, const char* name, int64_t value) {
  if (!e || !name) return MLDHIP_EINVAL;
  const std::string n = name;
  if (n == "loop_kernel") {
    if (value < 0 || value > 4) return e->fail(MLDHIP_EINVAL, "loop_kernel must be 0 (auto), 1 (latency), 2 (throughput), 3 (sample-major persistent loop) or 4 (cluster loop)");
    if (value == 3 && e->finalized && !e->loop_ips) return e->fail(MLDHIP_EINVAL, "loop_kernel 3: the sample-major loop is built for fp32 loop arithmetic, ff_size 1024, 4 heads");
    if (value == 4 && e->finalized && !e->cl_stream) return e->fail(MLDHIP_EINVAL, "loop_kernel 4: the cluster loop is built for the split-f16 mode, latent_dim 256, ff_size 1024, 4 heads");
    e->loop_kernel = (int)value;
    if (value == 4) { e->cluster_failed = 0; if (e->cl_host_status) *e->cl_host_status = 0u; }
  } else if (n == "fused_x3") {
    if (value != 0 && value != 1) return e->fail(MLDHIP_EINVAL, "fused_x3 must be 0 or 1");
    e->fused_x3 = (int)value;
  } else if (n == "cluster_max_batch") {
    if (value < 0 || value > kClMaxCall) return e->fail(MLDHIP_EINVAL, "cluster_max_batch must be 0 .. %d", kClMaxCall);
    e->cluster_max_batch = (int)value;
  } else if (n == "cluster_wt") {
    if (value != 0 && value != 1) return e->fail(MLDHIP_EINVAL, "cluster_wt must be 0 (plain payload stores inside an XCD, write-through across) or 1 (write-through always)");
    e->cluster_wt = (int)value;
  } else if (n == "cluster_groups") {
    if (value != 0 && value != 4 && value != 8) return e->fail(MLDHIP_EINVAL, "cluster_groups must be 0 (auto: 8 up to 64 motions, 4 above), 4 or 8");
    e->cluster_groups = (int)value;
#if defined(MLDHIP_HOOKS)
  } else if (n == "cluster_inject") {
    // hooks build only: fault injection for the tests of the bounded waits -- member value - 1 of every cluster never raises its first flag and the wait bound shrinks to
    // 2 ms (GPU) / 1 500 polls (simulator); 0 = off
    if (value < 0 || value > kClMembersMax) return e->fail(MLDHIP_EINVAL, "cluster_inject must be 0 (off) or 1 + a member index");
    e->cluster_mute = (int)value - 1;
#if defined(MLDHIP_SIM)
    e->cluster_timeout = value ? 1500 : 0;
#else
    e->cluster_timeout = value ? 200000 : 0;
#endif
  } else if (n == "cluster_stale") {
    e->cluster_stale = value != 0;      // hooks build only: the next cluster launches find a stale epoch in a polled word (entry check)
  } else if (n == "cluster_chunk") {
    if (value < 8 || value > 8 * kClMaxClusters || value % 8) return e->fail(MLDHIP_EINVAL, "cluster_chunk must be a multiple of 8 in 8 .. %d", 8 * kClMaxClusters);
    e->cluster_chunk = (int)value;      // hooks build only: motions per cluster launch (tests of the several-launches path on a few motions)
  } else if (n == "cluster_lane") {
    e->cluster_lane = value != 0;       // hooks build only: 0 = cluster calls of different streams are NOT ordered behind each other (reproduces the co-residency starvation: tools/two_streams.py)
  } else if (n == "cluster_graph") {
    if (value != 0 && value != 1) return e->fail(MLDHIP_EINVAL, "cluster_graph must be 0 (eager issue) or 1 (graphs); 2 (the memset-node clear that reproduced the r05 replay fault) was removed in round 6: the kernel's entry check covers the case");
    e->cluster_graph = value != 0;      // hooks build only
  } else if (n == "fused_dbg") {
    if (value != 0 && value != 5) return e->fail(MLDHIP_EINVAL, "fused_dbg must be 0 or 5 (phase counters; the builds with wrong results live in tools/loopbench only)");
    if (value == 5 && !e->trace_buf && hipMalloc((void**)&e->trace_buf, (size_t)512 * 8 * 8 * sizeof(uint64_t)) != hipSuccess) return e->fail(MLDHIP_EHIP, "hipMalloc(trace)");
    e->fused_dbg = (int)value;
#endif
  } else if (n == "range_probe") {
    if (value < 0 || value > 2) return e->fail(MLDHIP_EINVAL, "range_probe must be 0 (off), 1 (seeded probe batch at finalize) or 2 (1 + the reverse-loop probe again on the caller's first batch)");
    e->range_probe = (int)value;
    e->finalized = false;            // the probe is part of finalize
  } else if (n == "loop_lean") {
    if (value != 0 && value != 1) return e->fail(MLDHIP_EINVAL, "loop_lean must be 0 or 1");
    e->loop_lean = (int)value;
  } else if (n == "fused_min_batch") {
    if (value < 0) return e->fail(MLDHIP_EINVAL, "fused_min_batch must be >= 0 (0 = automatic)");
    e->fused_min_batch = (int)std::min<int64_t>(value, 1 << 30);
  } else if (n == "strip_min_rows") {
    if (value < 1) return e->fail(MLDHIP_EINVAL, "strip_min_rows must be >= 1");
    e->strip_min_rows = (int)std::min<int64_t>(value, 1 << 30);
  } else if (n == "flash_attn") {
    if (value < 0 || value > 2) return e->fail(MLDHIP_EINVAL, "flash_attn must be 0 (never), 1 (auto) or 2 (always)");
    e->flash_attn = (int)value;
  } else if (n == "dec_tail") {
    if (value != 0 && value != 1) return e->fail(MLDHIP_EINVAL, "dec_tail must be 0 or 1");
    e->dec_tail = (int)value;
  } else if (n == "dec_l0_once") {
    if (value != 0 && value != 1) return e->fail(MLDHIP_EINVAL, "dec_l0_once must be 0 or 1");
    e->dec_l0_once = (int)value;
  } else if (n == "dec_lean") {
    if (value != 0 && value != 1) return e->fail(MLDHIP_EINVAL, "dec_lean must be 0 or 1");
    e->dec_lean = (int)value;
  } else if (n == "many_pipeline") {
    if (value != 0 && value != 1) return e->fail(MLDHIP_EINVAL, "many_pipeline must be 0 (one chain over all motions of a mldhip_sample_many call) or 1 (request after request, decodes on the side stream)");
    if (value && e->ctxs.size() < 2) return e->fail(MLDHIP_EINVAL, "many_pipeline needs two workspaces: create the handle with max_in_flight >= 2");
    e->many_pipeline = (int)value;
    return MLDHIP_OK;                   // (host-side orchestration only: nothing a captured graph bakes in changes -- the graphs stay)
  } else if (n == "dec_half") {
    if (value < 0 || value > 6 || value == 3 || value == 5) return e->fail(MLDHIP_EINVAL, "dec_half must be 0 (fp32 Q|K|V, split x3 products), 1 (half Q|K|V; strip height by launch size), 4 or 6 (1 with 64- / 96-row in-projection strips always) or 2 (1, but never overruled by finalize's probe)");
    // the probe's reading of the form is part of finalize: switching it on (with the veto in force) on a probed handle that has not read it asks for finalize again
    if (value != 0 && value != 2 && e->finalized && e->range_probe && e->cfg.precision == MLDHIP_PREC_F16X3 && e->probe[kProbeDecode].err >= 0.f && e->probe[kProbeDecodeHalf].err < 0.f) e->finalized = false;
    e->dec_half = (int)value;
  } else if (n == "tile_x3") {
    if (value != 0 && value != 1) return e->fail(MLDHIP_EINVAL, "tile_x3 must be 0 or 1");
    e->tile_x3 = (int)value;
  } else if (n == "cross_fold") {
    if (value != 0 && value != 1) return e->fail(MLDHIP_EINVAL, "cross_fold must be 0 or 1");
    e->cross_fold = (int)value;
  } else if (n == "gemm_pipe") {
    if (value < 0 || value > 2) return e->fail(MLDHIP_EINVAL, "gemm_pipe must be 0 (off), 1 (auto: launches of >= 2 048 rows) or 2 (always)");
    e->gemm_pipe = (int)value;
  } else if (n == "strip_gemm") {
    if (value != 0 && value != 1) return e->fail(MLDHIP_EINVAL, "strip_gemm must be 0 or 1");
    e->strip_gemm = (int)value;
  } else if (n == "ffn_strip") {
    if (value != 0 && value != 1 && value != 3 && value != 4 && value != 6) return e->fail(MLDHIP_EINVAL, "ffn_strip must be 0 (off), 1 (auto: 64- or 96-row strips by launch size), 3, 4 or 6");
    e->ffn_strip = (int)value;
  } else if (n == "gemm_small_m") {
    if (value < 0) return e->fail(MLDHIP_EINVAL, "gemm_small_m must be >= 0");
    e->small_m = (int)std::min<int64_t>(value, 1 << 30);
  } else {
    return e->fail(MLDHIP_EINVAL, "unknown option %s", name);
  }
  // captured graphs bake the kernel choice in: drop them (nothing may be in flight on a context while it is rebuilt)
  DeviceGuard dg(e->device);
  drop_graphs(e, true);
  return MLDHIP_OK;
}

int mldhip_missing_keys(mldhip_handle* e, char* buf, int64_t buflen) {
  if (!e) return MLDHIP_EINVAL;
  int missing = 0;
  int64_t pos = 0;
  for (auto& p : e->params)
    if (!p.loaded) {
      ++missing;
      if (buf && pos + (int64_t)p.key.size() + 1 < buflen) {
        std::memcpy(buf + pos, p.key.c_str(), p.key.size() + 1);
        pos += p.key.size() + 1;
      }
    }
  if (buf && pos < buflen) buf[pos] = 0;
  return missing;
}

int mldhip_finalize_weights(mldhip_handle* e, void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  // A weight group (engine/state.hpp) must be loaded completely or not at all; ops of an absent group fail with MLDHIP_ESTATE
  int have[kGroupCount] = {0}, total[kGroupCount] = {0}, any = 0;
  for (auto& p : e->params) { total[p.group]++; have[p.group] += p.loaded; any += p.loaded; }
  for (auto& p : e->params)
    if (!p.loaded && have[p.group] != 0) return e->fail(MLDHIP_ENOKEY, "missing tensor %s (strict load)", p.key.c_str());
  if (any == 0) return e->fail(MLDHIP_ENOKEY, "no tensors loaded");
  for (int g = 0; g < kGroupCount; ++g) e->group_ready[g] = total[g] > 0 && have[g] == total[g];
  hipStream_t stream = (hipStream_t)stream_;
  bind_layers(e);
  Ctx c{e, stream};
  const int D = e->cfg.latent_dim, TD = time_width(e), n = e->cfg.num_inference_steps;
  HIP_TRY(e, hipDeviceSynchronize());                   // no call may be in flight on any context while tables are rebuilt
  if (e->cfg.precision == MLDHIP_PREC_F16X3) {
    // the staged GEMMs of these modes run on split-f16 MFMAs: split the weights once, here, not in every workgroup
    if (!e->arena_x3 && hipMalloc((void**)&e->arena_x3, e->arena_floats * sizeof(float)) != hipSuccess) return e->fail(MLDHIP_EHIP, "hipMalloc(split weights)");
    const long long groups = (long long)((e->arena_floats + 31) / 32);   // arena_floats is a multiple of kAlign = 64
    MLD_LAUNCH(split_bf16_weights_kernel, dim3((unsigned)((groups + 15) / 16)), dim3(256), 0, stream, e->arena, e->arena_x3, groups);
    if (check_launch(c, "split_bf16_weights")) return c.rc;
  }
  if (int rc = build_loop_stream(c)) return rc;
  if (int rc = build_cluster_stream(c)) return rc;
  if (int rc = build_ffn_streams(c)) return rc;
  if (int rc = build_eval_tables(c)) return rc;
  if (int rc = build_smpl_tables(c)) return rc;
  if (int rc = build_uestc_tables(c)) return rc;
  for (int k = 0; k < (int)e->ctxs.size(); ++k) {       // the derived tables live in each context's workspace
  bind_context(e, k);
  if (e->group_ready[kGroupDenoiser]) {
    // PE-folded biases: token 1 (time) gets pe[1], token 2 (text) gets pe[2] (mld_denoiser.py:187,196)
    // (trans_dec: the memory tokens [time, text] get mem_pos.pe[0], pe[1] instead, mld_denoiser.py:213)
    const float* pe_time = is_novae(e) ? P(e, "denoiser.mem_pos.pe") : P(e, "denoiser.query_pos.pe") + D;
    const float* pe_text = pe_time + D;
    MLD_LAUNCH(add_rows_kernel, dim3((D + 255) / 256), dim3(256), 0, stream, e->time_b2pe, P(e, "denoiser.time_embedding.linear_2.bias"), pe_time, 1, D);
    if (!is_action(e)) MLD_LAUNCH(add_rows_kernel, dim3((D + 255) / 256), dim3(256), 0, stream, e->text_bias, P(e, "denoiser.emb_proj.1.bias"), pe_text, 1, D);
    if (check_launch(c, "add_rows")) return c.rc;
    // time-MLP output for every scheduler timestep (sample independent; embeddings.py:245-305)
    std::vector<float> host((size_t)n * TD);
    for (int s = 0; s < n; ++s) timestep_sincos(float(e->timesteps[s]), TD, host.data() + (size_t)s * TD);
    HIP_TRY(e, hipMemcpy(e->temb0, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    time_mlp(c, e->temb0, e->tmid, e->T1, n);
    if (c.rc) return c.rc;
    if (is_novae(e)) {
      // the time token's K|V for every (layer, scheduler step) depend on weights only; pose_embd.weight padded to KP
      novae_memory_kv(c, e->T1, n, e->TKV, (long long)n * 2 * D);
      novae_fold_memory(c, e->TKV, n, (long long)n * 2 * D, e->TKW, e->TKU, e->TKC);      // ... and so do their folded forms ("cross_fold")
      const int NF = e->cfg.nfeats, KP = novae_kp(e);
      MLD_LAUNCH(pad_cols_kernel, dim3((D * KP + 255) / 256), dim3(256), 0, stream, P(e, "denoiser.pose_embd.weight"), e->WskelP, D, NF, KP);
      if (check_launch(c, "pad_cols")) return c.rc;
    }
  }
  if (e->group_ready[kGroupVaeEncoder]) {
    const int NF = e->cfg.nfeats, KP = (NF + 31) / 32 * 32;
    MLD_LAUNCH(pad_cols_kernel, dim3((D * KP + 255) / 256), dim3(256), 0, stream,
               P(e, is_actor(e) ? "vae.encoder.skel_embedding.weight" : "vae.skel_embedding.weight"), e->WskelP, D, NF, KP);
    if (check_launch(c, "pad_cols")) return c.rc;
  }
  }
  HIP_TRY(e, hipStreamSynchronize(stream));
  drop_graphs(e, false);                                 // they hold the old tables (the stream and the device are idle here)
  for (auto& x : e->ctxs) x.used = false;
  bind_context(e, 0);
  e->next_ctx = 0;
  if (e->loop_kernel == 4 && !e->cl_stream)
    return e->fail(MLDHIP_EINVAL, "loop_kernel 4: the cluster loop is built for the split-f16 mode, latent_dim 256, ff_size 1024, 4 heads");
  if (e->loop_kernel == 3 && !e->loop_ips)      // (set before finalize: refused here, like mldhip_set_option refuses it afterwards)
    return e->fail(MLDHIP_EINVAL, "loop_kernel 3: the sample-major loop is built for fp32 / split-f16 loop arithmetic, latent_dim 256, ff_size 1024, 4 heads");
  e->finalized = true;
  for (ProbeVerdict& v : e->probe) v = ProbeVerdict{};
  if (e->cfg.precision == MLDHIP_PREC_F16X3 && e->range_probe) {
    if (int rc = range_probe(e, stream)) { e->finalized = false; return rc; }
    e->probe_first_call = e->range_probe == 2;
  }
  return MLDHIP_OK;
}

int mldhip_numeric_status(mldhip_handle* e, mldhip_numeric_info* out) {
  if (!e || !out) return MLDHIP_EINVAL;
  constexpr int32_t kInfoSizes[] = {
      MLDHIP_ENDS_BEHIND(mldhip_numeric_info, reserved),        // ABI 7 caller: no text tower fields
      MLDHIP_ENDS_BEHIND(mldhip_numeric_info, probe_err_text),  // ABI 8 caller from before the evaluator towers' two fields
      MLDHIP_ENDS_BEHIND(mldhip_numeric_info, probe_err_eval),  // ... from before the recognition ST-GCN's two
      (int32_t)sizeof(mldhip_numeric_info),                     // today's caller
  };
  if (!size_accepted(kInfoSizes, out->struct_size)) return e->fail(MLDHIP_EINVAL, "mldhip_numeric_info.struct_size mismatch (ABI)");
  DeviceGuard dg(e->device);
  HIP_TRY(e, hipDeviceSynchronize());
  unsigned n = 0;
  HIP_TRY(e, hipMemcpy(&n, e->nonfinite, sizeof n, hipMemcpyDeviceToHost));
  HIP_TRY(e, hipMemset(e->nonfinite, 0, sizeof n));
  // a cluster launch that ran into its wait bound poisoned its latents (counted above) and left its status word set: the handle stays off the cluster loop from here on
  // (the captured graphs that hold it are dropped); mldhip_set_option("loop_kernel", 4) re-arms it
  if (!e->cluster_failed && cluster_timed_out(e)) leave_cluster_loop(e);
  const bool x3 = e->cfg.precision == MLDHIP_PREC_F16X3;
  const ProbeVerdict* v = e->probe;
  mldhip_numeric_info full = {out->struct_size};
  for (int s = 0; s < kProbeStages; ++s) full.probed |= v[s].err >= 0.f;      // (kProbeDecodeHalf is read only where kProbeDecode is)
  full.loop_split_ok = x3 && v[kProbeLoop].ok;
  full.decode_split_ok = x3 && v[kProbeDecode].ok;
  full.probe_err_loop = v[kProbeLoop].err;
  full.probe_err_decode = v[kProbeDecode].err;
  full.nonfinite_values = (int64_t)n;
  full.cluster_loop = !e->cl_stream ? 0 : e->cluster_foreign ? 3 : e->cluster_failed ? 2 : 1;
  full.decode_half_ok = x3 && v[kProbeDecode].ok && e->dec_half && (v[kProbeDecodeHalf].ok || e->dec_half == 2);
  full.probe_err_decode_half = v[kProbeDecodeHalf].err;
  full.text_split_ok = e->cfg.clip_layers > 0 && x3 && e->arena_x3 && v[kProbeText].ok;
  full.probe_err_text = v[kProbeText].err;
  full.eval_split_ok = e->cfg.t2m_eval && x3 && e->arena_x3 && v[kProbeEval].ok;
  full.probe_err_eval = v[kProbeEval].err;
  full.uestc_split_ok = uestc_x3(e) && e->group_ready[kGroupUestc];
  full.probe_err_uestc = v[kProbeUestc].err;
  std::memcpy(out, &full, (size_t)out->struct_size);      // the caller gets the fields its struct covers
  return MLDHIP_OK;
}

// noise is never drawn from a fixed key behind the caller's back: an eta > 0 handle samples through the seeded entry point only
#define MLDHIP_REFUSE_UNSEEDED(e, fn) \
  if (eta_on(e)) return (e)->fail(MLDHIP_ESTATE, fn " on a handle with eta > 0 would draw its noise from a fixed key: use mldhip_sample_many_seeded (one mldhip_noise_key per request)")

int mldhip_sample_many(mldhip_handle* e, const mldhip_request* reqs, int32_t nreq, void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  if (is_novae(e)) return e->fail(MLDHIP_ESTATE, "mldhip_sample_many serves the latent models (text or action condition)");
  MLDHIP_REFUSE_UNSEEDED(e, "mldhip_sample_many");
  if (!reqs || nreq < 1 || nreq > 64) return e->fail(MLDHIP_EINVAL, "1..64 requests expected");
  return sample_many_impl(e, reqs, nreq, (hipStream_t)stream_);
}

int mldhip_sample_many_seeded(mldhip_handle* e, const mldhip_request* reqs, const mldhip_noise_key* keys, int32_t nreq, void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  if (is_novae(e)) return e->fail(MLDHIP_ESTATE, "mldhip_sample_many_seeded serves the latent models (text or action condition)");
  if (!reqs || nreq < 1 || nreq > 64) return e->fail(MLDHIP_EINVAL, "1..64 requests expected");
  if (!keys) return e->fail(MLDHIP_EINVAL, "keys is NULL (one mldhip_noise_key per request)");
  for (int i = 0; i < nreq; ++i)
    if (keys[i].first_index < 0) return e->fail(MLDHIP_EINVAL, "keys[%d].first_index %lld is negative", i, (long long)keys[i].first_index);
  // eta = 0: nothing is drawn -- the keys are ignored and the call IS mldhip_sample_many
  return sample_many_impl(e, reqs, nreq, (hipStream_t)stream_, eta_on(e) ? keys : nullptr);
}

int mldhip_sample_many_traj(mldhip_handle* e, const mldhip_request* reqs, const mldhip_noise_key* keys, float* const* traj_out_dev, int32_t nreq, void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  if (!reqs || nreq < 1 || nreq > 64) return e->fail(MLDHIP_EINVAL, "1..64 requests expected");
  bool any = false;
  for (int i = 0; traj_out_dev && i < nreq; ++i) {
    any = any || traj_out_dev[i];
    if (reinterpret_cast<uintptr_t>(traj_out_dev[i]) % 16) return e->fail(MLDHIP_EINVAL, "traj_out_dev[%d] is not 16-byte aligned (the rows are stored four floats at a time)", i);
  }
  if (is_novae(e)) {
    if (any) return e->fail(MLDHIP_EINVAL, "mldhip_sample_many_traj: the diffusion-only variant has no latent trajectory (its loop state is the raw motion [B, T, nfeats] over 1000 steps)");
    return e->fail(MLDHIP_ESTATE, "mldhip_sample_many_traj serves the latent models (text or action condition)");      // as mldhip_sample_many_seeded answers such a handle
  }
  // the keys: required where noise is drawn (as mldhip_sample_many_seeded requires them), optional and ignored on an eta = 0 handle
  if (eta_on(e) && !keys) return e->fail(MLDHIP_EINVAL, "keys is NULL on a handle with eta > 0 (one mldhip_noise_key per request)");
  for (int i = 0; keys && i < nreq; ++i)
    if (keys[i].first_index < 0) return e->fail(MLDHIP_EINVAL, "keys[%d].first_index %lld is negative", i, (long long)keys[i].first_index);
  return sample_many_impl(e, reqs, nreq, (hipStream_t)stream_, eta_on(e) ? keys : nullptr, any ? traj_out_dev : nullptr);
}

// shared body of mldhip_sample_many_from / mldhip_sample_many_guided behind their trivial cases: `starts` may be NULL (no request has a source), `guid` is non-NULL
// only when some request names a guidance scale of its own
static int sample_many_from_checked(mldhip_handle* e, const mldhip_request* reqs, const mldhip_noise_key* keys, const mldhip_start* starts, float* const* traj_out_dev,
                                    const float* guid, int32_t nreq, void* stream_) {
  const int n = e->cfg.num_inference_steps;
  bool traj = false;
  for (int i = 0; i < nreq; ++i) {
    const mldhip_start s = starts ? starts[i] : mldhip_start{nullptr, 0, 0};
    if (s.noised != 0 && s.noised != 1) return e->fail(MLDHIP_EINVAL, "starts[%d].noised = %d (0: a clean source, 1: the loop state at first_step)", i, (int)s.noised);
    if (s.first_step < 0 || s.first_step >= n) return e->fail(MLDHIP_EINVAL, "starts[%d].first_step = %d outside [0, num_inference_steps = %d)", i, (int)s.first_step, n);
    if (!s.src_latents_dev && s.first_step != 0) return e->fail(MLDHIP_EINVAL, "starts[%d]: first_step = %d without a source (a start from noise begins at step 0)", i, (int)s.first_step);
    if (!s.src_latents_dev && s.noised != 0) return e->fail(MLDHIP_EINVAL, "starts[%d]: noised = 1 without a source", i);
    if (reinterpret_cast<uintptr_t>(s.src_latents_dev) % 16) return e->fail(MLDHIP_EINVAL, "starts[%d].src_latents_dev is not 16-byte aligned (the rows are read four floats at a time)", i);
    if (traj_out_dev) {
      traj = traj || traj_out_dev[i];
      if (reinterpret_cast<uintptr_t>(traj_out_dev[i]) % 16) return e->fail(MLDHIP_EINVAL, "traj_out_dev[%d] is not 16-byte aligned (the rows are stored four floats at a time)", i);
    }
  }
  if (eta_on(e) && !keys) return e->fail(MLDHIP_EINVAL, "keys is NULL on a handle with eta > 0 (one mldhip_noise_key per request)");
  for (int i = 0; keys && i < nreq; ++i)
    if (keys[i].first_index < 0) return e->fail(MLDHIP_EINVAL, "keys[%d].first_index %lld is negative", i, (long long)keys[i].first_index);
  return sample_many_impl(e, reqs, nreq, (hipStream_t)stream_, eta_on(e) ? keys : nullptr, traj ? traj_out_dev : nullptr, starts, guid);
}

int mldhip_sample_many_from(mldhip_handle* e, const mldhip_request* reqs, const mldhip_noise_key* keys, const mldhip_start* starts, float* const* traj_out_dev,
                            int32_t nreq, void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  bool any = false;
  for (int i = 0; starts && nreq >= 1 && nreq <= 64 && i < nreq; ++i) any = any || starts[i].src_latents_dev || starts[i].first_step != 0 || starts[i].noised != 0;
  // no source anywhere (and nothing else set): the call IS mldhip_sample_many_traj -- same checks, same path, same captured graphs
  if (!any) return mldhip_sample_many_traj(e, reqs, keys, traj_out_dev, nreq, stream_);
  DeviceGuard dg(e->device);
  if (!reqs) return e->fail(MLDHIP_EINVAL, "1..64 requests expected");
  if (is_novae(e)) return e->fail(MLDHIP_EINVAL, "mldhip_sample_many_from: the diffusion-only variant has no latent to start from (its loop state is the raw motion [B, T, nfeats])");
  return sample_many_from_checked(e, reqs, keys, starts, traj_out_dev, nullptr, nreq, stream_);
}

int mldhip_sample_many_guided(mldhip_handle* e, const mldhip_request* reqs, const mldhip_noise_key* keys, const mldhip_start* starts, float* const* traj_out_dev,
                              const float* guidance_host, int32_t nreq, void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  bool any = false;
  for (int i = 0; guidance_host && nreq >= 1 && nreq <= 64 && i < nreq; ++i) {
    if (!std::isfinite(guidance_host[i])) {
      DeviceGuard dg(e->device);
      return e->fail(MLDHIP_EINVAL, "guidance_host[%d] is not finite", i);
    }
    any = any || guidance_host[i] >= 0.0f;
  }
  // no request names a scale: the call IS mldhip_sample_many_from -- same checks, same path, same captured graphs
  if (!any) return mldhip_sample_many_from(e, reqs, keys, starts, traj_out_dev, nreq, stream_);
  DeviceGuard dg(e->device);
  if (!reqs) return e->fail(MLDHIP_EINVAL, "1..64 requests expected");
  if (is_novae(e)) return e->fail(MLDHIP_EINVAL, "mldhip_sample_many_guided: per-request guidance serves the latent models (the diffusion-only variant is out of scope)");
  if (!(e->cfg.guidance_scale > 1.0f))
    return e->fail(MLDHIP_EINVAL, "mldhip_sample_many_guided: the handle's guidance_scale is %g (<= 1): such a model does no classifier-free guidance (an action engine builds no unconditional rows)",
                   (double)e->cfg.guidance_scale);
  return sample_many_from_checked(e, reqs, keys, starts, traj_out_dev, guidance_host, nreq, stream_);
}

int mldhip_sample(mldhip_handle* e, const float* text_emb_dev, const float* init_latents_dev, const int32_t* lengths_host,
                  int32_t B, float* latents_out_dev, float* feats_out_dev, float* joints_out_dev, void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  if (is_action(e)) return e->fail(MLDHIP_ESTATE, "engine was created with the action condition: use mldhip_sample_action");
  if (is_novae(e)) return e->fail(MLDHIP_ESTATE, "engine was created for the diffusion-only variant: use mldhip_sample_novae");
  MLDHIP_REFUSE_UNSEEDED(e, "mldhip_sample");
  if (joints_out_dev && is_actor(e)) return e->fail(MLDHIP_ESTATE, "joints of the ActorVae feature layout need SMPL (out of scope)");
  if (!text_emb_dev) return e->fail(MLDHIP_EINVAL, "null input pointer");
  return sample_impl(e, text_emb_dev, nullptr, init_latents_dev, lengths_host, B, latents_out_dev, feats_out_dev, joints_out_dev, stream_);
}

int mldhip_sample_action(mldhip_handle* e, const int32_t* actions_host, const float* init_latents_dev, const int32_t* lengths_host,
                         int32_t B, float* latents_out_dev, float* feats_out_dev, void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  if (!is_action(e)) return e->fail(MLDHIP_ESTATE, "engine was created with the text condition: use mldhip_sample");
  MLDHIP_REFUSE_UNSEEDED(e, "mldhip_sample_action");
  if (!actions_host) return e->fail(MLDHIP_EINVAL, "null input pointer");
  return sample_impl(e, nullptr, actions_host, init_latents_dev, lengths_host, B, latents_out_dev, feats_out_dev, nullptr, stream_);
}

int mldhip_denoiser_forward(mldhip_handle* e, const float* sample_dev, int32_t timestep, const float* text_emb_dev,
                            int32_t R, float* out_dev, void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  if (is_action(e)) return e->fail(MLDHIP_ESTATE, "engine was created with the action condition: use mldhip_denoiser_forward_action");
  if (is_novae(e)) return e->fail(MLDHIP_ESTATE, "engine was created for the diffusion-only variant: use mldhip_denoiser_forward_novae");
  if (!text_emb_dev) return e->fail(MLDHIP_EINVAL, "null pointer");
  return denoiser_forward_impl(e, sample_dev, timestep, text_emb_dev, nullptr, R, out_dev, stream_);
}

int mldhip_denoiser_forward_action(mldhip_handle* e, const float* sample_dev, int32_t timestep, const int32_t* actions_host,
                                   int32_t R, float* out_dev, void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  if (!is_action(e)) return e->fail(MLDHIP_ESTATE, "engine was created with the text condition: use mldhip_denoiser_forward");
  if (!actions_host) return e->fail(MLDHIP_EINVAL, "null pointer");
  return denoiser_forward_impl(e, sample_dev, timestep, nullptr, actions_host, R, out_dev, stream_);
}

int mldhip_sample_novae(mldhip_handle* e, const float* text_emb_dev, const float* init_latents_dev, const int32_t* lengths_host,
                        int32_t B, const float* step_noise_dev, uint64_t seed, float* feats_out_dev, float* joints_out_dev, void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  if (!is_novae(e)) return e->fail(MLDHIP_ESTATE, "engine was not created for the diffusion-only variant (vae_arch = MLDHIP_VAE_NONE)");
  return sample_novae_impl(e, text_emb_dev, init_latents_dev, lengths_host, B, step_noise_dev, seed, feats_out_dev, joints_out_dev, stream_);
}

int mldhip_denoiser_forward_novae(mldhip_handle* e, const float* sample_dev, int32_t timestep, const float* text_emb_dev,
                                  const int32_t* lengths_host, int32_t R, int32_t T, float* out_dev, void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  if (!is_novae(e)) return e->fail(MLDHIP_ESTATE, "engine was not created for the diffusion-only variant (vae_arch = MLDHIP_VAE_NONE)");
  return denoiser_forward_novae_impl(e, sample_dev, timestep, text_emb_dev, lengths_host, R, T, out_dev, stream_);
}

int mldhip_ddpm_step(mldhip_handle* e, const float* eps_dev, int32_t timestep, const float* sample_dev, const float* noise_dev,
                     uint64_t seed, int32_t step_index, float* prev_dev, int64_t n, void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  if (!is_ddpm(e)) return e->fail(MLDHIP_ESTATE, "engine was created with the DDIM scheduler: use mldhip_ddim_step");
  if (!eps_dev || !sample_dev || !prev_dev || n < 1) return e->fail(MLDHIP_EINVAL, "null pointer / n < 1");
  if (timestep < 0 || timestep >= e->cfg.num_train_timesteps) return e->fail(MLDHIP_EINVAL, "timestep %d out of range", timestep);
  Ctx c{e, (hipStream_t)stream_};
  MLD_LAUNCH(cfg_ddpm_step_kernel, dim3((unsigned)std::min<long long>(4096, (n / 4 + 256) / 256)), dim3(256), 0, c.stream, eps_dev,
             (const float*)nullptr, sample_dev, noise_dev, prev_dev, (long long)n, 1.0f, ddpm_coef(e, timestep), (unsigned long long)seed,
             (unsigned)step_index);
  return check_launch(c, "ddpm_step");
}

int mldhip_philox_normal(mldhip_handle* e, float* out_dev, int64_t n, uint64_t seed, int32_t step_index, void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  if (!out_dev || n < 1) return e->fail(MLDHIP_EINVAL, "null pointer / n < 1");
  Ctx c{e, (hipStream_t)stream_};
  MLD_LAUNCH(philox_normal_kernel, dim3((unsigned)std::min<long long>(4096, (n / 4 + 256) / 256)), dim3(256), 0, c.stream, out_dev, (long long)n,
             (unsigned long long)seed, (unsigned)step_index);
  return check_launch(c, "philox_normal");
}

int mldhip_vae_decode(mldhip_handle* e, const float* z_dev, const int32_t* lengths_host, int32_t B, float* feats_out_dev,
                      void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  if (!e->finalized || !e->group_ready[kGroupVaeDecoder]) return e->fail(MLDHIP_ESTATE, "vae_decode before finalize / vae.* not loaded");
  if (!z_dev || !feats_out_dev) return e->fail(MLDHIP_EINVAL, "null pointer");
  int T = 0;
  if (int rc = validate_lengths(e, lengths_host, B, &T)) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  CtxUse use(e, stream);                                  // picks + binds a workspace context (see WsContext)
  if (use.rc) return use.rc;
  HIP_TRY(e, hipMemcpyAsync(e->lens_dev, lengths_host, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  Ctx c{e, stream};
  e->phase = 1;
  decode_body(c, z_dev, B, T, feats_out_dev);
  return c.rc;
}

int mldhip_vae_encode(mldhip_handle* e, const float* feats_dev, const int32_t* lengths_host, int32_t B, int32_t T,
                      const float* eps_dev, float* latent_out_dev, float* mu_out_dev, float* logvar_out_dev, void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  if (!e->finalized || !e->group_ready[kGroupVaeEncoder]) return e->fail(MLDHIP_ESTATE, "vae_encode before finalize / vae.encoder.* not loaded");
  if (!feats_dev || !mu_out_dev || !logvar_out_dev) return e->fail(MLDHIP_EINVAL, "null pointer");
  if (eps_dev && !latent_out_dev) return e->fail(MLDHIP_EINVAL, "eps given but latent_out is NULL");
  int Tm = 0;
  if (int rc = validate_lengths(e, lengths_host, B, &Tm)) return rc;
  if (T < Tm || T > e->cfg.max_frames || T + 2 > 288) return e->fail(MLDHIP_EINVAL, "T=%d must satisfy max(lengths) <= T <= min(max_frames, 286)", T);
  hipStream_t stream = (hipStream_t)stream_;
  CtxUse use(e, stream);                                  // picks + binds a workspace context (see WsContext)
  if (use.rc) return use.rc;
  e->lens2_host.assign(lengths_host, lengths_host + B);
  for (auto& v : e->lens2_host) v += 2;                       // the two distribution tokens are always attended to
  HIP_TRY(e, hipMemcpyAsync(e->lens2_dev, e->lens2_host.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  Ctx c{e, stream};
  e->phase = 1;
  encode_body(c, feats_dev, B, T, eps_dev, latent_out_dev, mu_out_dev, logvar_out_dev);
  return c.rc;
}

int mldhip_ddim_step(mldhip_handle* e, const float* eps_dev, int32_t timestep, const float* sample_dev, float* prev_dev,
                     int64_t n, void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  if (!eps_dev || !sample_dev || !prev_dev || n < 0) return e->fail(MLDHIP_EINVAL, "bad argument");
  if (timestep < 0 || timestep >= e->cfg.num_train_timesteps) return e->fail(MLDHIP_EINVAL, "timestep %d out of range", timestep);
  if (n == 0) return MLDHIP_OK;
  Ctx c{e, (hipStream_t)stream_};
  MLD_LAUNCH(ddim_step_kernel, dim3((unsigned)std::min<int64_t>(1024, (n + 255) / 256)), dim3(256), 0, c.stream, eps_dev, sample_dev,
             prev_dev, (long long)n, ddim_coef(e, timestep));
  return check_launch(c, "ddim_step");
}

int mldhip_ddim_step_eta(mldhip_handle* e, const float* eps_dev, int32_t timestep, const float* sample_dev, const float* noise_dev,
                         uint64_t seed, int32_t step_index, float* prev_dev, int64_t n, void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  if (is_ddpm(e)) return e->fail(MLDHIP_ESTATE, "engine was created with the DDPM scheduler: use mldhip_ddpm_step");
  if (!eps_dev || !sample_dev || !prev_dev || n < 0 || step_index < 0) return e->fail(MLDHIP_EINVAL, "bad argument");
  if (timestep < 0 || timestep >= e->cfg.num_train_timesteps) return e->fail(MLDHIP_EINVAL, "timestep %d out of range", timestep);
  if (n == 0) return MLDHIP_OK;
  Ctx c{e, (hipStream_t)stream_};
  MLD_LAUNCH(ddim_step_eta_kernel, dim3((unsigned)std::min<int64_t>(1024, (n / 4 + 256) / 256)), dim3(256), 0, c.stream, eps_dev, sample_dev,
             noise_dev, prev_dev, (long long)n, ddim_coef(e, timestep), ddim_eta(e, timestep), (unsigned long long)seed, (unsigned)step_index);
  return check_launch(c, "ddim_step_eta");
}

int mldhip_text_encode(mldhip_handle* e, const int32_t* ids_host, const int32_t* eos_pos_host, int32_t P, float* text_emb_out_dev, void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  return text_encode_impl(e, ids_host, eos_pos_host, P, text_emb_out_dev, (hipStream_t)stream_);
}

int mldhip_t2m_motion_embed(mldhip_handle* e, const float* feats_dev, const int32_t* lengths_host, int32_t B, int32_t T, int32_t renorm, float* emb_out_dev, void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  return t2m_motion_embed_impl(e, feats_dev, lengths_host, B, T, renorm, emb_out_dev, (hipStream_t)stream_);
}

int mldhip_t2m_text_embed(mldhip_handle* e, const float* word_embs_dev, const float* pos_ohot_dev, const int32_t* text_lengths_host, int32_t B, int32_t L,
                          float* emb_out_dev, void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  return t2m_text_embed_impl(e, word_embs_dev, pos_ohot_dev, text_lengths_host, B, L, emb_out_dev, (hipStream_t)stream_);
}

int mldhip_smpl_forward(mldhip_handle* e, const float* feats_dev, const int32_t* lengths_host, int32_t B, int32_t T, int32_t flags, float* joints_out_dev,
                        float* verts_out_dev, void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  return smpl_forward_impl(e, feats_dev, lengths_host, B, T, flags, joints_out_dev, verts_out_dev, (hipStream_t)stream_);
}

int mldhip_a2m_recognize(mldhip_handle* e, const float* joints_dev, const int32_t* lengths_host, const float* h0_dev, int32_t B, int32_t T, float* logits_out_dev,
                         float* act_out_dev, void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  return a2m_recognize_impl(e, joints_dev, lengths_host, h0_dev, B, T, logits_out_dev, act_out_dev, (hipStream_t)stream_);
}

int mldhip_uestc_recognize(mldhip_handle* e, const float* x_dev, const int64_t* strides, int32_t B, int32_t T, float* logits_out_dev, float* feat_out_dev, void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  return uestc_recognize_impl(e, x_dev, strides, B, T, logits_out_dev, feat_out_dev, (hipStream_t)stream_);
}

int mldhip_t2m_match(mldhip_handle* e, const float* text_dev, const float* motion_dev, int32_t N, int32_t D, int32_t R, int32_t* rank_out_dev, float* diag_out_dev,
                     void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  return t2m_match_impl(e, text_dev, motion_dev, N, D, R, rank_out_dev, diag_out_dev, (hipStream_t)stream_);
}

int mldhip_act_stats(mldhip_handle* e, const float* x_dev, int32_t N, int32_t D, float* mean_out_dev, float* cov_out_dev, void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  return act_stats_impl(e, x_dev, N, D, mean_out_dev, cov_out_dev, (hipStream_t)stream_);
}

int mldhip_pair_dist(mldhip_handle* e, const float* x_dev, int32_t N, int32_t D, const int32_t* a_host, const int32_t* b_host, int32_t P, float* dist_out_dev,
                     void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  return pair_dist_impl(e, x_dev, N, D, a_host, b_host, P, dist_out_dev, (hipStream_t)stream_);
}

int mldhip_feats2joints(mldhip_handle* e, const float* feats_dev, int32_t B, int32_t T, float* joints_out_dev, void* stream_) {
  if (!e) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  if (is_actor(e) || e->cfg.nfeats < joint_feat_cols(e)) return e->fail(MLDHIP_ESTATE, "feats2joints implements the HumanML3D / KIT-ML layout (recover_from_ric) only (SMPL-based layouts are out of scope)");
  if (!e->finalized || !e->group_ready[kGroupStats]) return e->fail(MLDHIP_ESTATE, "feats2joints before finalize / mean,std not loaded");
  if (!feats_dev || !joints_out_dev) return e->fail(MLDHIP_EINVAL, "null pointer");
  if (B < 1 || T < 1 || T > 512) return e->fail(MLDHIP_EINVAL, "B >= 1 and 1 <= T <= 512 required");
  Ctx c{e, (hipStream_t)stream_};
  e->phase = 2;
  joints_body(c, feats_dev, B, T, joints_out_dev);
  return c.rc;
}


// Measurement hooks: only in the hooks build (make hooks -> libmldhip_hooks.so, include/mldhip_hooks.h); the production library exports the sampling surface only.
#if defined(MLDHIP_HOOKS)
int mldhip_profile_kernel(mldhip_handle* e, const char* name, int32_t B, int32_t T, int32_t iters, double* flops_per_launch,
                          void* stream_) {
  // Launches ONE kernel of the sampling path `iters` times back-to-back on `stream` at its production
  // shape, on the engine's own buffers (call after a sample() so they hold real activations).  The
  // caller brackets the call with events on the same stream (bench.py does) -- no timing happens here.
  if (!e || !name || !flops_per_launch) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  if (!e->finalized || !e->group_ready[kGroupDenoiser] || !e->group_ready[kGroupVaeDecoder]) return e->fail(MLDHIP_ESTATE, "profile before finalize");
  if (B < 1 || B > e->cfg.max_batch || T < 1 || T > e->cfg.max_frames || iters < 1) return e->fail(MLDHIP_EINVAL, "bad B/T/iters");
  CtxUse use(e, (hipStream_t)stream_);
  if (use.rc) return use.rc;
  Ctx c{e, (hipStream_t)stream_};
  const int D = e->cfg.latent_dim, F = e->cfg.ff_size, H = e->cfg.num_heads;
  const std::string n = name;
  const bool dec = n.rfind("dec_", 0) == 0;
  const int R = 2 * B;
  const long long M = dec ? (long long)B * T : 3LL * R;
  const int mid = (e->cfg.num_layers - 1) / 2;
  int saved_phase = e->phase;
  e->phase = dec ? 1 : 0;
  const EncLayerP& DL = e->den[mid];
  const DenView v = den_view(e, R);
  for (int it = 0; it < iters && !c.rc; ++it) {
    if (n == "den_qkv") {            // with the LN2-on-load prologue of a typical layer (sums the 4 FFN2 slabs)
      den_qkv(c, v, DL, den_layer_output(e, v, e->den[mid - 1], v.S[mid - 1]));
      *flops_per_launch = 2.0 * M * D * 3 * D;
    } else if (n == "den_outproj") {
      den_outproj(c, v, DL);
      *flops_per_launch = 2.0 * M * D * D + 4.0 * M * 3 * D;
    } else if (n == "den_ffn1") {
      den_ffn1(c, v, DL, v.S[mid - 1]);
      *flops_per_launch = 2.0 * M * D * F;
    } else if (n == "den_ffn2") {
      den_ffn2(c, v, DL);
      *flops_per_launch = 2.0 * M * D * F;
    } else if (n == "den_final") {
      MLD_LAUNCH(den_final_step_kernel, dim3(B), dim3(256), 0, c.stream, den_final_args(e, v), e->zbuf, e->LNO,
                 P(e, "denoiser.query_pos.pe"), (const float*)e->T1, B, e->cfg.guidance_scale, ddim_coef(e, e->timesteps[0]), (const TrajRow*)nullptr, 0);
      check_launch(c, "den_final_step");
      *flops_per_launch = 0.0;
    } else if (n == "dec_qkv") {
      gemm(c, lin_args(e->S[0], D, D, e->dec[mid].in_w, e->dec[mid].in_b, e->QKV, 3 * D, (int)M, 3 * D));
      *flops_per_launch = 2.0 * M * D * 3 * D;
    } else if (n == "dec_ffn1") {
      GemmArgs f1 = lin_args(e->H1, D, D, e->dec[mid].l1_w, e->dec[mid].l1_b, e->FF, F, (int)M, F);
      f1.act = ACT_GELU;
      gemm(c, f1);
      *flops_per_launch = 2.0 * M * D * F;
    } else if (n == "dec_ffn") {      // the whole feed-forward block as the layer runs it (one fused launch in the split-f16 mode)
      ffn_block(c, e->H1, e->Hb, (int)M, e->dec[mid].l1_w, e->dec[mid].l1_b, e->dec[mid].l2_w, e->dec[mid].l2_b, e->dec[mid].n3_w, e->dec[mid].n3_b, 0);
      *flops_per_launch = 4.0 * M * D * F;
    } else if (n == "dec_ffn2_ln") {
      GemmArgs f2 = lin_args(e->FF, F, F, e->dec[mid].l2_w, e->dec[mid].l2_b, e->Hb, D, (int)M, D);
      f2.res = e->H1; f2.ldres = D; f2.g1 = e->dec[mid].n3_w; f2.b1 = e->dec[mid].n3_b;
      gemm_ln(c, f2);
      *flops_per_launch = 2.0 * M * D * F;
    } else if (n == "dec_outproj_ln") {
      GemmArgs o = lin_args(e->AO, D, D, e->dec[mid].out_w, e->dec[mid].out_b, e->Hb, D, (int)M, D);
      o.res = e->S[0]; o.ldres = D; o.g1 = e->dec[mid].n1_w; o.b1 = e->dec[mid].n1_b;
      o.cvec = e->cvec; o.ldcvec = D; o.rows_per_group = T; o.g2 = e->dec[mid].n2_w; o.b2 = e->dec[mid].n2_b;
      gemm_ln(c, o);
      *flops_per_launch = 2.0 * M * D * D;
    } else if (n == "dec_attn") {
      dec_attention(c, B, T);
      *flops_per_launch = 4.0 * B * H * (double)T * T * 64;
    } else {
      e->phase = saved_phase;
      return e->fail(MLDHIP_EINVAL, "unknown kernel name %s", name);
    }
  }
  e->phase = saved_phase;
  return c.rc;
}

int mldhip_profile_trace(mldhip_handle* e, const char* name, int32_t B, int32_t T, uint64_t* out_host, int64_t cap_u64, void* stream_) {
  // Runs ONE traced launch of a den_* kernel (after 3 untraced warm-ups) and copies back 8 timestamps per
  // wave: [0] start [1] loads landed + prologue [2] LDS written [3] barrier passed [4] MFMAs done
  // [5] stores drained (shader clock), [6]/[7] start/end on the 100 MHz realtime counter.
  if (!e || !name || !out_host) return MLDHIP_EINVAL;
  DeviceGuard dg(e->device);
  constexpr int64_t kMax = 512 * 8 * 8;
  if (!e->trace_buf && hipMalloc((void**)&e->trace_buf, kMax * sizeof(uint64_t)) != hipSuccess) return e->fail(MLDHIP_EHIP, "hipMalloc(trace)");
  if (std::string(name) == "den_loop_phases") {
    // the persistent loop's own phase counters ("fused_dbg" 5): written by the last sample call, 16 values per wave of the first 64 workgroups
    HIP_TRY(e, hipStreamSynchronize((hipStream_t)stream_));
    const int64_t n = std::min<int64_t>(cap_u64, 64 * 8 * 16);      // 16 counters per wave: two 8-value records
    HIP_TRY(e, hipMemcpy(out_host, e->trace_buf, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return (int)(n / 64);
  }
  if (std::string(name) == "den_cluster_status") {
    // the cluster loop's status words of the last call: [0] timeout flag, [1] clusters that span XCDs, then per workgroup (first 256) its XCC id + 1 (debug builds of the kernel)
    if (!e->cl_flags) return e->fail(MLDHIP_ESTATE, "no cluster loop on this handle");
    HIP_TRY(e, hipStreamSynchronize((hipStream_t)stream_));
    const size_t ncl = std::min<size_t>(kClMaxClusters, (e->cfg.max_batch + 7) / 8);
    const int64_t n = std::min<int64_t>(cap_u64, 8);
    HIP_TRY(e, hipMemcpy(out_host, reinterpret_cast<unsigned*>(e->cl_flags) + ncl * kClFlagWords, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 1;
  }
  if (std::string(name) == "den_cluster_xbuf") {
    // the exchange region of cluster 0 as the last cluster-loop call left it (kernels/loop_cluster.hpp: AO, h1, Y, Z, H of the last two layers) + its flags:
    // what tests compare between the simulator and the GPU
    if (!e->cl_xbuf) return e->fail(MLDHIP_ESTATE, "no cluster loop on this handle");
    HIP_TRY(e, hipStreamSynchronize((hipStream_t)stream_));
    const int64_t n = std::min<int64_t>(cap_u64, (int64_t)kClXFloats / 2);
    const int cl = std::max(0, std::min<int>(B, (int)std::min<size_t>(kClMaxClusters, (e->cfg.max_batch + 7) / 8) - 1));      // B = cluster index here
    HIP_TRY(e, hipMemcpy(out_host, e->cl_xbuf + (size_t)cl * kClXFloats, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return (int)(n / 64);
  }
  double fl = 0;
  if (int rc = mldhip_profile_kernel(e, name, B, T, 3, &fl, stream_)) return rc;
  // the traced build is its own kernel: two launches of it first (code fetched, instruction cache warm), then the one that is kept
  e->trace_on = e->trace_buf;
  int rc = mldhip_profile_kernel(e, name, B, T, 2, &fl, stream_);
  if (!rc && hipMemsetAsync(e->trace_buf, 0, kMax * sizeof(uint64_t), (hipStream_t)stream_) != hipSuccess) rc = e->fail(MLDHIP_EHIP, "hipMemsetAsync(trace)");
  if (!rc) rc = mldhip_profile_kernel(e, name, B, T, 1, &fl, stream_);
  e->trace_on = nullptr;
  if (rc) return rc;
  HIP_TRY(e, hipStreamSynchronize((hipStream_t)stream_));
  const int64_t n = std::min<int64_t>(cap_u64, kMax);
  HIP_TRY(e, hipMemcpy(out_host, e->trace_buf, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return (int)(n / 64);
}

#endif  // MLDHIP_HOOKS

int mldhip_get_timesteps(mldhip_handle* e, int32_t* out, int32_t n) {
  if (!e || !out) return MLDHIP_EINVAL;
  int m = std::min<int>(n, (int)e->timesteps.size());
  std::memcpy(out, e->timesteps.data(), m * sizeof(int32_t));
  return m;
}

int mldhip_get_alphas_cumprod(mldhip_handle* e, float* out, int32_t n) {
  if (!e || !out) return MLDHIP_EINVAL;
  int m = std::min<int>(n, (int)e->alphas_cumprod.size());
  std::memcpy(out, e->alphas_cumprod.data(), m * sizeof(float));
  return m;
}

int mldhip_get_launch_counts(mldhip_handle* e, int32_t* out) {
  if (!e || !out) return MLDHIP_EINVAL;
  for (int i = 0; i < 3; ++i) out[i] = e->launches[i];
  return MLDHIP_OK;
}

}  // extern "C"
