// Range probe of the F16X3 mode (include/mldhip.h "Range contract"): the split-f16 kernels against the exact-fp32 ones of the SAME
// handle on one seeded probe batch; a stage that disagrees (or is not finite) is switched to the fp32 kernels.  Six stages, each run only where the handle has its weights: 1 the
// reverse loop, 2 the decoder, 3 the diffusion-only denoiser (in place of 1 and 2), 4 the CLIP text tower, 5 the T2M evaluator towers, 6 the UESTC recognition ST-GCN.  They share ONE
// seeded generator (a draw more or less in one stage moves the inputs of every later one) and the helpers at the top; verdicts go to the handle's probe[] (engine/state.hpp ProbeStage).
// Part of libmldhip's single translation unit; include order: see mldhip.hip.  Internal linkage throughout (anonymous namespace).
#pragma once

namespace {

// sets an option of the handle for a scope; the value it had comes back on every exit
template <class T>
struct Scoped {
  T& ref;
  T saved;
  Scoped(T& r, T v) : ref(r), saved(r) { ref = v; }
  ~Scoped() { ref = saved; }
  Scoped(const Scoped&) = delete;
  Scoped& operator=(const Scoped&) = delete;
};

// The probe must run the kernels production calls run.  The row-strip GEMMs, the fused decoder tail, the final strip and (diffusion-only
// variant) the pipelined 128 x 256 tile are selected by row count ("gemm_small_m", gemm_pipe_min_rows) and the two attention forms by
// the number of (sample, head) pairs -- a probe batch is far below all of these (advisor r4: at 4 x 64 = 256 rows both arms of the decoder
// probe ran the SAME fp32 small-M kernel for every GEMM but two).  For the duration of a stage the thresholds are lifted, and the stage
// is probed once per attention form (flash_attn is the stage's to set); what stays unprobed is listed in include/mldhip.h "Range contract".
struct ProbeLift {
  Scoped<int> small_m, pipe_rows, flash;
  explicit ProbeLift(E* e) : small_m(e->small_m, 0), pipe_rows(e->gemm_pipe_min_rows, 0), flash(e->flash_attn, e->flash_attn) {}
};

struct ProbeRng {      // Box-Muller, seeded: the probe is a function of the weights only
  unsigned long long st = 0x9E3779B97F4A7C15ull;
  unsigned bits() { st = st * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(st >> 40); }      // 24 bits
  float uni() { st = st * 6364136223846793005ull + 1442695040888963407ull; return (float)((st >> 40) + 1) * (1.0f / 16777217.0f); }
  void fill(std::vector<float>& v, float scale) {
    for (size_t i = 0; i + 1 < v.size(); i += 2) {
      const float r = std::sqrt(-2.0f * std::log(uni())), a = 6.283185307179586f * uni();
      v[i] = scale * r * std::cos(a); v[i + 1] = scale * r * std::sin(a);
    }
  }
};

struct ProbeDev {      // a device buffer of the probe's own
  float* p = nullptr;
  ~ProbeDev() { if (p) (void)hipFree(p); }
  int up(const std::vector<float>& h) { return hipMalloc((void**)&p, h.size() * sizeof(float)) == hipSuccess && hipMemcpy(p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess ? 0 : 1; }
  int make(size_t n) { return hipMalloc((void**)&p, n * sizeof(float)) == hipSuccess && hipMemset(p, 0, n * sizeof(float)) == hipSuccess ? 0 : 1; }
};

int probe_down(E* e, hipStream_t stream, const float* dev, size_t n, std::vector<float>& h) {
  h.resize(n);
  if (hipStreamSynchronize(stream) != hipSuccess || hipMemcpy(h.data(), dev, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return e->fail(MLDHIP_EHIP, "range probe: copy");
  return MLDHIP_OK;
}

// One pair of runs of a stage: run(split) with the stage's flag on split arithmetic, then on exact fp32 (the stage's verdict overwrites the flag afterwards); after each
// run n floats at `dev` come down into ha (split) / hb (fp32).  The first error ends the pair.
template <class Run>
int probe_pair(E* e, hipStream_t stream, ProbeStage stage, const float* dev, size_t n, std::vector<float>& ha, std::vector<float>& hb, Run run) {
  for (int split = 1; split >= 0; --split) {
    e->probe[stage].ok = split != 0;
    if (int rc = run(split != 0)) return rc;
    if (int rc = probe_down(e, stream, dev, n, split ? ha : hb)) return rc;
  }
  return MLDHIP_OK;
}

void probe_verdict(E* e, ProbeStage stage, float err) { e->probe[stage] = {err <= MLDHIP_PROBE_TOL, err}; }

// max difference d over reference magnitude m (over an amplification the stage allows for); inf when anything was not finite, or differs from an all-zero reference
float probe_ratio(bool finite, float d, float m, float amp = 1.0f) {
  const float inf = std::numeric_limits<float>::infinity();
  return !finite ? inf : (m > 0.f ? d / m / amp : (d > 0.f ? inf : 0.f));
}

float rel_err(const std::vector<float>& a, const std::vector<float>& b) {       // max|a - b| / max|b|
  float d = 0.f, m = 0.f;
  bool finite = true;
  for (size_t i = 0; i < a.size(); ++i) {
    finite = finite && std::isfinite(a[i]) && std::isfinite(b[i]);
    d = std::max(d, std::fabs(a[i] - b[i])); m = std::max(m, std::fabs(b[i]));
  }
  return probe_ratio(finite, d, m);
}

// ---------------------------------------------------------------------------------------------------------------- stage 1: the reverse loop
struct LoopProbe {
  E* e;
  hipStream_t stream;
  int Bp;                               // motions of the probe batch
  std::vector<float> hs, ht;            // start latents [2 Bp][D] (both CFG halves the same), text rows [2 Bp][TD]
  std::vector<int32_t> act;             // action labels [2 Bp]
  ProbeDev sample, text, out;
  float worst = 0.f;
};

// (a) one denoiser call of the latency kernels at the first and the last timestep of the schedule
int probe_loop_denoiser(LoopProbe& p) {
  E* e = p.e;
  const int D = e->cfg.latent_dim, n = e->cfg.num_inference_steps;
  std::vector<float> ha, hb;
  for (int which = 0; which < 2; ++which) {
    const int t = e->timesteps[which == 0 ? 0 : n - 1];
    auto run = [&](bool) { return denoiser_forward_impl(e, p.sample.p, t, is_action(e) ? nullptr : p.text.p, is_action(e) ? p.act.data() : nullptr, 2 * p.Bp, p.out.p, p.stream); };
    if (int rc = probe_pair(e, p.stream, kProbeLoop, p.out.p, (size_t)2 * p.Bp * D, ha, hb, run)) return rc;
    p.worst = std::max(p.worst, rel_err(ha, hb));
  }
  return MLDHIP_OK;
}

// (c) the cluster loop (kernels/loop_cluster.hpp: split-f16 only, unclamped images like the persistent loop's) on the same two steps, against the exact-fp32 result `hb`;
// m, amp: the reference magnitude and amplification of (b)
int probe_loop_cluster(LoopProbe& p, Ctx& c, const std::vector<float>& hb, float m, float amp, float guidance) {
  E* e = p.e;
  const int D = e->cfg.latent_dim, n = e->cfg.num_inference_steps, Bp = p.Bp;
  e->probe[kProbeLoop].ok = true;
  // both forms (advisor r5): 8 column groups per token (24 workgroups per cluster: calls of up to 64 motions -- what a probe batch of 8 picks by itself) and 4 (12 workgroups:
  // calls of 65 .. 256 motions); they differ in how linear1 / linear2 / the skip linear are split over members and waves, i.e. in the order of sums
  Scoped<int> restore_cg(e->cluster_groups, e->cluster_groups);
  const int first = cluster_groups(e, Bp);      // what the handle picks for the probe batch: 8 unless the device is small or the option says 4
  for (int form = 0; form < 2 && !e->cluster_failed; ++form) {
    if (form == 1) {
      e->cluster_groups = first == 8 ? 4 : 8;
      if (cluster_groups(e, Bp) == first) break;      // the other form is not available on this device: nothing new to run
    }
    std::vector<float> hc;
    {
      ClusterLane lane(e, c.stream, true);
      launch_cluster_loop(c, p.sample.p, Bp, std::min(2, n), guidance);
    }
    if (c.rc) return c.rc;
    if (int rc = probe_down(e, p.stream, e->lat, (size_t)Bp * D, hc)) return rc;
    if (cluster_timed_out(e)) { leave_cluster_loop(e); continue; }      // not an arithmetic verdict (engine/serve.hpp)
    float d = 0.f;
    bool finite = true;
    for (size_t i = 0; i < hc.size(); ++i) { finite = finite && std::isfinite(hc[i]); d = std::max(d, std::fabs(hc[i] - hb[i])); }
    p.worst = std::max(p.worst, probe_ratio(finite, d, m, amp));
  }
  return MLDHIP_OK;
}

// (b) two reverse steps of the persistent loop (its operand images are not clamped: an overflow shows up as NaN here), then (c)
// (run whenever the split stream exists: "fused_x3" / "tile_x3" / "loop_kernel" may be changed after finalize, and the verdict must cover them)
int probe_loop_steps(LoopProbe& p) {
  E* e = p.e;
  const int D = e->cfg.latent_dim, n = e->cfg.num_inference_steps, Bp = p.Bp;
  Scoped<int> x3(e->fused_x3, 1);
  CtxUse use(e, p.stream);
  if (use.rc) return use.rc;
  Ctx c{e, p.stream};
  e->phase = 0;
  const float guidance = e->cfg.guidance_scale > 1.0f ? e->cfg.guidance_scale : 1.0f;
  std::vector<float> ha, hb;
  if (int rc = probe_pair(e, p.stream, kProbeLoop, e->lat, (size_t)Bp * D, ha, hb, [&](bool) -> int {
        if (is_action(e)) {
          HIP_TRY(e, hipMemcpyAsync(e->labels_dev, p.act.data(), p.act.size() * sizeof(int32_t), hipMemcpyHostToDevice, p.stream));
          action_rows(c, 2 * Bp, Bp, e->TP);
        } else {
          text_projection(c, p.text.p, 2 * Bp, e->TP);
        }
        launch_fused_loop(c, p.sample.p, Bp, std::min(2, n), guidance);
        return c.rc;
      })) return rc;
  // measured against the UPDATE the two steps made (latents - start noise), not against the latents: near t = T a DDIM step moves
  // x by a few per cent, and how much depends on the schedule; the update is (guided eps) x (step coefficients), so this reads
  // like (a) times the guidance amplification (2 g - 1 at worst) -- hence the factor on the tolerance
  float d = 0.f, m = 0.f;
  bool finite = true;
  for (size_t i = 0; i < ha.size(); ++i) {
    finite = finite && std::isfinite(ha[i]) && std::isfinite(hb[i]);
    d = std::max(d, std::fabs(ha[i] - hb[i]));
    m = std::max(m, std::fabs(hb[i] - p.hs[i]));
  }
  const float amp = std::max(1.0f, 2.0f * guidance - 1.0f);
  p.worst = std::max(p.worst, probe_ratio(finite, d, m, amp));
#if defined(MLDHIP_SIM)
  const bool probe_cluster = e->cl_stream && (e->loop_kernel == 4 || e->cluster_max_batch > 0);      // (the simulator's handles never pick it by themselves: 20 s per probe saved)
#else
  const bool probe_cluster = e->cl_stream != nullptr;
#endif
  return probe_cluster ? probe_loop_cluster(p, c, hb, m, amp, guidance) : MLDHIP_OK;
}

// user_text / user_lat: "range_probe" 2 -- the stage once more on the first min(8, B) motions of the caller's first batch (device pointers of
// a text-conditioned mldhip_sample call: [2B][TD] embeddings, unconditional half first, and [B][D] start latents)
int probe_loop(E* e, hipStream_t stream, ProbeRng& rng, const float* user_text, const float* user_lat, int user_B) {
  const int D = e->cfg.latent_dim, TD = e->cfg.text_dim;
  const bool user = user_B > 0;
  LoopProbe p{e, stream, std::min(8, user ? user_B : e->cfg.max_batch)};
  const int Bp = p.Bp;
  p.hs.resize((size_t)2 * Bp * D); p.ht.resize((size_t)2 * Bp * TD);
  rng.fill(p.hs, 1.0f); rng.fill(p.ht, 0.5f);
  if (user) {
    if (hipStreamSynchronize(stream) != hipSuccess ||
        hipMemcpy(p.hs.data(), user_lat, (size_t)Bp * D * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(p.ht.data(), user_text, (size_t)Bp * TD * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(p.ht.data() + (size_t)Bp * TD, user_text + (size_t)user_B * TD, (size_t)Bp * TD * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
      return e->fail(MLDHIP_EHIP, "range probe: copy of the caller's batch");
  }
  for (int i = 0; i < Bp * D; ++i) p.hs[(size_t)Bp * D + i] = p.hs[i];                      // both CFG halves see the same latents
  p.act.resize((size_t)2 * Bp);
  for (int i = 0; i < 2 * Bp; ++i) p.act[i] = i % std::max(1, e->cfg.nclasses);
  if (p.sample.up(p.hs) || p.text.up(p.ht) || p.out.make((size_t)2 * Bp * D)) return e->fail(MLDHIP_EHIP, "range probe: hipMalloc");
  if (int rc = probe_loop_denoiser(p)) return rc;
  if (e->loop_ips > 0 && e->loop_stream_x3)
    if (int rc = probe_loop_steps(p)) return rc;
  if (user) p.worst = std::max(p.worst, e->probe[kProbeLoop].err);          // the verdict covers the seeded batch AND the caller's
  probe_verdict(e, kProbeLoop, p.worst);
  return MLDHIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------- stage 2: the decoder
// decodes of 4 motions x min(64, max_frames) frames (two full, two ragged), key-blocked and whole-K/V attention
int probe_decoder(E* e, hipStream_t stream, ProbeRng& rng) {
  ProbeLift lift(e);
  const int D = e->cfg.latent_dim, NF = e->cfg.nfeats;
  const int B = std::min(4, e->cfg.max_batch), T = std::min(64, e->cfg.max_frames);
  std::vector<float> hz((size_t)B * D);
  rng.fill(hz, 4.0f);
  std::vector<int32_t> lens(B, T);
  if (B > 1) lens[1] = std::max(1, T - 7);
  if (B > 3) lens[3] = std::max(1, T / 2 + 1);
  ProbeDev z, feats;
  if (z.up(hz) || feats.make((size_t)B * T * NF)) return e->fail(MLDHIP_EHIP, "range probe: hipMalloc");
  std::vector<float> ha, hb;
  auto run = [&](std::vector<float>& h) -> int {
    CtxUse use(e, stream);
    if (use.rc) return use.rc;
    HIP_TRY(e, hipMemcpyAsync(e->lens_dev, lens.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    Ctx c{e, stream};
    e->phase = 1;
    decode_body(c, z.p, B, T, feats.p);
    if (c.rc) return c.rc;
    return probe_down(e, stream, feats.p, (size_t)B * T * NF, h);
  };
  const int dh = e->dec_half;
  Scoped<int> restore_dh(e->dec_half, dh);
  bool& split = e->probe[kProbeDecode].ok;
  split = false;                                 // the exact-fp32 decode: the reference of every form below
  if (int rc = run(hb)) return rc;
  split = true;
  float worst = 0.f;
  for (int form = 0; form < 2; ++form) {         // fp32 Q | K | V, split x3 products: key-blocked and whole-K/V attention
    e->dec_half = 0;
    e->flash_attn = form == 0 ? 2 : 0;
    if (int rc = run(ha)) return rc;
    worst = std::max(worst, rel_err(ha, hb));
  }
  float half_err = -1.f;
  if (dh) {
    // the opt-in self-attention block on half Q | K | V (kernels/dec_half.hpp): its own bound, read on UNIT-normal latents -- with large latents the per-sample
    // cross-attention vector drowns the frame-to-frame signal the self-attention carries and the form looks 10-30x better than it is (profiles/r06_decoder_precision.json)
    std::vector<float> hz1((size_t)B * D);
    rng.fill(hz1, 1.0f);
    HIP_TRY(e, hipMemcpy(z.p, hz1.data(), hz1.size() * sizeof(float), hipMemcpyHostToDevice));
    e->dec_half = 0;
    split = false;
    if (int rc = run(hb)) return rc;
    split = true;
    e->dec_half = 2;
    if (int rc = run(ha)) return rc;
    half_err = rel_err(ha, hb);
  }
  probe_verdict(e, kProbeDecode, worst);
  e->probe[kProbeDecodeHalf] = {!dh || (half_err >= 0.f && half_err <= MLDHIP_PROBE_TOL_HALF), half_err};      // (option off: nothing to veto; switching it on later un-finalizes the handle, mldhip_set_option)
  return MLDHIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------- stage 3: the diffusion-only variant
// one denoiser call (every GEMM and the frame-level attention run split in this mode) on 4 CFG rows x 128 frames, on the pipelined tile +
// key-blocked head-dim-128 attention and on the staged tile + two-phase attention
int probe_novae(E* e, hipStream_t stream, ProbeRng& rng) {
  ProbeLift lift(e);
  const int NF = e->cfg.nfeats, TD = e->cfg.text_dim;
  const int R = 2 * std::min(2, e->cfg.max_batch), T = std::min(128, e->cfg.max_frames);
  std::vector<float> hx((size_t)R * T * NF), ht((size_t)R * TD);
  rng.fill(hx, 1.0f); rng.fill(ht, 0.5f);
  std::vector<int32_t> lens(R, T);
  lens[1] = std::max(1, T - 5); lens[R - 1] = std::max(1, T - 5);
  ProbeDev x, text, out;
  if (x.up(hx) || text.up(ht) || out.make((size_t)R * T * NF)) return e->fail(MLDHIP_EHIP, "range probe: hipMalloc");
  std::vector<float> ha, hb;
  float worst = 0.f;
  Scoped<int> pipe(e->gemm_pipe, e->gemm_pipe);
  for (int form = 0; form < 2; ++form) {
    e->flash_attn = form == 0 ? 2 : 0;
    e->gemm_pipe = form == 0 ? pipe.saved : 0;
    auto run = [&](bool) { return denoiser_forward_novae_impl(e, x.p, e->timesteps[0], text.p, lens.data(), R, T, out.p, stream); };
    if (int rc = probe_pair(e, stream, kProbeDecode, out.p, (size_t)R * T * NF, ha, hb, run)) return rc;
    worst = std::max(worst, rel_err(ha, hb));
  }
  probe_verdict(e, kProbeDecode, worst);
  return MLDHIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------- stage 4: the CLIP text tower
// one mldhip_text_encode of four seeded prompts (2, 17, 33 and clip_ctx token rows: a short prompt, both sides of the x3 attention's 32-key
// block edge, the full context) on the split-f16 tower and on the exact-fp32 tower of the same handle.  The tower picks its kernels by the
// arithmetic alone (one GEMM tile and one attention kernel per mode at every row count, engine/dispatch.hpp gemm_clip): nothing to lift.
int probe_text(E* e, hipStream_t stream, ProbeRng& rng) {
  const int ctx = e->cfg.clip_ctx, W = e->cfg.text_dim;
  const int lens[4] = {2, 17, 33, ctx};
  const int NP = std::min(4, e->cfg.clip_max_prompts);
  std::vector<int32_t> ids((size_t)NP * ctx), eos(NP);
  for (auto& id : ids) id = (int32_t)(rng.bits() % (unsigned)e->cfg.clip_vocab);
  for (int p = 0; p < NP; ++p) eos[p] = std::min(lens[4 - NP + p], ctx) - 1;      // (fewer than 4 prompts of capacity: the longest ones)
  ProbeDev out;
  if (out.make((size_t)NP * W)) return e->fail(MLDHIP_EHIP, "range probe: hipMalloc");
  std::vector<float> ha, hb;
  if (int rc = probe_pair(e, stream, kProbeText, out.p, (size_t)NP * W, ha, hb, [&](bool) { return text_encode_impl(e, ids.data(), eos.data(), NP, out.p, stream, false); })) return rc;
  probe_verdict(e, kProbeText, rel_err(ha, hb));
  return MLDHIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------- stage 5: the T2M evaluator towers
// four seeded motions (T = min(64, max_frames), lengths 64 / 37 / 20 / 4 clipped to T: full, len % 4 = 1, a short one, a single GRU step; unit-normal rows in the
// evaluators' normalisation, no renorm) and four seeded captions (the longest t2m_max_words allows, 3, 2 and 1 words) on the split-f16 towers and on the exact-fp32
// towers of the same handle, then the recurrent products h . W_hh^T by themselves (below).  One tile shape and one recurrence kernel per mode at every row count: nothing to lift.
int probe_eval(E* e, hipStream_t stream, ProbeRng& rng) {
  const int NF = e->cfg.nfeats, NB = std::min(4, e->cfg.t2m_max_motions);
  float worst = -1.f;
  ProbeDev out;
  if (out.make((size_t)NB * kEvalOut)) return e->fail(MLDHIP_EHIP, "range probe: hipMalloc");
  std::vector<float> ha, hb;
  if (e->group_ready[kGroupEvalMotion] && e->cfg.max_frames >= kEvalUnit) {
    const int T = std::min(64, e->cfg.max_frames);
    const int want[4] = {64, 37, 20, 4};
    std::vector<int32_t> lens(NB);
    for (int b = 0; b < NB; ++b) lens[b] = std::max(kEvalUnit, std::min(want[b], T));
    std::vector<float> hf((size_t)NB * T * NF + 1);
    rng.fill(hf, 1.0f);
    for (int b = 0; b < NB; ++b)
      for (size_t i = ((size_t)b * T + lens[b]) * NF; i < (size_t)(b + 1) * T * NF; ++i) hf[i] = 0.f;      // padded frames hold zeros, as the decoder leaves them
    ProbeDev feats;
    if (feats.up(hf)) return e->fail(MLDHIP_EHIP, "range probe: hipMalloc");
    if (int rc = probe_pair(e, stream, kProbeEval, out.p, (size_t)NB * kEvalOut, ha, hb, [&](bool) { return t2m_motion_embed_impl(e, feats.p, lens.data(), NB, T, 0, out.p, stream, false); })) return rc;
    worst = std::max(worst, rel_err(ha, hb));
  }
  if (e->group_ready[kGroupEvalText]) {
    const int L = std::min(20, e->cfg.t2m_max_words);
    const int want[4] = {L, 3, 2, 1};
    std::vector<int32_t> lens(NB);
    for (int b = 0; b < NB; ++b) lens[b] = std::min(want[b], L);
    std::vector<float> hw((size_t)NB * L * kEvalWord + 1), hp((size_t)NB * L * kEvalPos, 0.f);
    rng.fill(hw, 1.0f);
    for (int i = 0; i < NB * L; ++i) hp[(size_t)i * kEvalPos + rng.bits() % kEvalPos] = 1.f;
    ProbeDev word, pos;
    if (word.up(hw) || pos.up(hp)) return e->fail(MLDHIP_EHIP, "range probe: hipMalloc");
    if (int rc = probe_pair(e, stream, kProbeEval, out.p, (size_t)NB * kEvalOut, ha, hb, [&](bool) { return t2m_text_embed_impl(e, word.p, pos.p, lens.data(), NB, L, out.p, stream, false); })) return rc;
    worst = std::max(worst, rel_err(ha, hb));
  }
  // (c) the recurrent products by themselves: 16 seeded state rows (uniform in (-1, 1), where a GRU state lives) times W_hh^T of every loaded tower and direction,
  // split image against fp32, on the towers' own GEMM tile.  The embeddings above cannot see this operand on the probe's inputs: unit-normal rows make the input-side
  // gate terms O(1), and a W_hh whose split image has lost its precision (weights near 1e-5: both halves are half subnormals, ~4e-3 relative) then moves an embedding
  // by 1e-7 -- on a caller's rows whose input-side terms are as small as the recurrent ones it would not.  The product is held to the same bound as the outputs.
  for (int tower = 0; tower < 2; ++tower) {
    if (!e->group_ready[tower == 0 ? kGroupEvalMotion : kGroupEvalText]) continue;
    const int H = tower == 0 ? kEvalMotionH : kEvalTextH, M = 16;
    const std::string p = tower == 0 ? "t2m_motionencoder" : "t2m_textencoder";
    std::vector<float> hx((size_t)M * H);
    for (auto& v : hx) v = 2.0f * rng.uni() - 1.0f;
    ProbeDev x, y;
    if (x.up(hx) || y.make((size_t)M * 3 * H)) return e->fail(MLDHIP_EHIP, "range probe: hipMalloc");
    for (int dir = 0; dir < 2; ++dir) {
      const float* W = P(e, p + (dir ? ".gru.weight_hh_l0_reverse" : ".gru.weight_hh_l0"));
      auto run = [&](bool split) { Ctx c{e, stream}; gemm_eval(c, lin_args(x.p, H, H, W, nullptr, y.p, 3 * H, M, 3 * H), split); return c.rc; };      // (this GEMM takes its arithmetic as an argument, not from the flag)
      if (int rc = probe_pair(e, stream, kProbeEval, y.p, (size_t)M * 3 * H, ha, hb, run)) return rc;
      worst = std::max(worst, rel_err(ha, hb));
    }
  }
  e->probe[kProbeEval] = {worst < 0.f || worst <= MLDHIP_PROBE_TOL, worst};
  return MLDHIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------- stage 6: the UESTC recognition ST-GCN
// four seeded motions of 16 frames (unit-normal rot6d values, what data_bn was fitted to) on the split-f16 net and on the exact-fp32 net of the same handle;
// err = max |split - fp32| / max |fp32| over features and logits.  One tile shape per mode at every row count: nothing to lift.
int probe_uestc(E* e, hipStream_t stream, ProbeRng& rng) {
  const int NB = std::min(4, e->cfg.uestc_max_motions), T = std::min(16, e->cfg.max_frames), NC = e->cfg.uestc_classes;
  std::vector<float> hx((size_t)NB * kStgJoints * kStgIn * T);
  rng.fill(hx, 1.0f);
  ProbeDev x, out;
  if (x.up(hx) || out.make((size_t)NB * (kStgFeat + NC))) return e->fail(MLDHIP_EHIP, "range probe: hipMalloc");
  const int64_t strides[4] = {(int64_t)kStgJoints * kStgIn * T, (int64_t)kStgIn * T, T, 1};
  std::vector<float> ha, hb;
  if (int rc = probe_pair(e, stream, kProbeUestc, out.p, (size_t)NB * (kStgFeat + NC), ha, hb, [&](bool) { return uestc_recognize_impl(e, x.p, strides, NB, T, out.p + (size_t)NB * kStgFeat, out.p, stream, false); })) return rc;
  probe_verdict(e, kProbeUestc, rel_err(ha, hb));
  return MLDHIP_OK;
}

int range_probe(E* e, hipStream_t stream, const float* user_text, const float* user_lat, int user_B) {
  Scoped<bool> noise_off(e->noise_off, true);      // deterministic on every handle: the probe compares arithmetic on the eta = 0 step (include/mldhip.h "range_probe")
  ProbeRng rng;
  const bool user = user_text != nullptr && user_lat != nullptr && user_B > 0;      // "range_probe" 2: the reverse-loop stage alone, on the caller's batch
  if (e->group_ready[kGroupDenoiser] && !is_novae(e))
    if (int rc = probe_loop(e, stream, rng, user_text, user_lat, user ? user_B : 0)) return rc;
  if (user) { e->phase = 0; return MLDHIP_OK; }
  if (e->group_ready[kGroupVaeDecoder] && !is_novae(e))
    if (int rc = probe_decoder(e, stream, rng)) return rc;
  if (e->group_ready[kGroupDenoiser] && is_novae(e))
    if (int rc = probe_novae(e, stream, rng)) return rc;
  if (e->cfg.clip_layers > 0 && e->group_ready[kGroupClip] && e->arena_x3)
    if (int rc = probe_text(e, stream, rng)) return rc;
  if (e->cfg.t2m_eval && (e->group_ready[kGroupEvalMotion] || e->group_ready[kGroupEvalText]) && e->arena_x3)
    if (int rc = probe_eval(e, stream, rng)) return rc;
  if (e->cfg.uestc_rec && e->group_ready[kGroupUestc] && e->uestc_tabs_x3)
    if (int rc = probe_uestc(e, stream, rng)) return rc;
  e->phase = 0;
  return MLDHIP_OK;
}

}  // namespace
