// Handle construction and teardown: the cluster-lane lock of a device, config validation, the workspace carve of the two variants,
// the dynamic-LDS registration list, create_engine / destroy_engine.
// Part of libmldhip's single translation unit; include order: see mldhip.hip.  Internal linkage throughout (anonymous namespace).
#pragma once
#if !defined(MLDHIP_SIM)
#include <fcntl.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <unistd.h>
#endif

namespace {

// One PROCESS per device may launch the cluster loop (kernels/loop_cluster.hpp): its launches need their workgroups resident together, ClusterLane orders them inside a
// process, and two processes interleaving such launches on one GPU would each end partly resident -- every wait runs into its 200 ms bound (advisor r5).  The first
// process that creates a handle on a device takes an advisory lock on a per-device file and keeps it until it exits (released by the kernel on any exit); a process that
// finds it taken -- and is not the owner itself or one of its descendants -- runs every call on the other loop families (mldhip_numeric_info.cluster_loop says so).
// One process per GPU -- torch.distributed ranks -- is unaffected; two ranks sharing a GPU are siblings: the second one is foreign.
bool cluster_lane_owned(int device) {
#if !defined(MLDHIP_SIM)
  static std::mutex mu;
  static int state[64] = {0};     // 0 unknown, 1 owned by this process, 2 foreign
  std::lock_guard<std::mutex> lk(mu);
  int& st = state[device & 63];
  if (st) return st == 1;
  char bus[64] = {0};
  if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, device) != hipSuccess) { (void)hipGetLastError(); st = 1; return true; }
  for (char* c = bus; *c; ++c) if (*c == ':' || *c == '.') *c = '_';
  const std::string path = std::string("/tmp/mldhip_cluster_lane_") + bus + ".lock";      // (a fixed directory: processes with different TMPDIRs must meet at one file)
  // O_NOFOLLOW + regular-file check: /tmp is shared, the name is predictable -- never write through somebody's symlink.  Another user's file (created under their umask) may
  // not be writable: flock works on a read-only descriptor too, only the pid note is skipped then.
  int fd = open(path.c_str(), O_CREAT | O_RDWR | O_CLOEXEC | O_NOFOLLOW, 0666);
  bool writable = fd >= 0;
  if (fd >= 0) (void)fchmod(fd, 0666);                        // (ours if we created it; EPERM otherwise: ignored)
  else fd = open(path.c_str(), O_RDONLY | O_CLOEXEC | O_NOFOLLOW);
  struct stat sb;
  if (fd < 0 || fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) {      // no lock file possible (read-only /tmp, a symlink in its place): no coordination, behave as before
    if (fd >= 0) close(fd);
    st = 1;
    return true;
  }
  if (flock(fd, LOCK_EX | LOCK_NB) == 0) {                    // fd stays open for the life of the process; the owner's pid goes into the file
    char buf[32];
    const int n = snprintf(buf, sizeof buf, "%ld\n", (long)getpid());
    if (writable && ftruncate(fd, 0) == 0 && pwrite(fd, buf, (size_t)n, 0) == n) {}
    st = 1;
    return true;
  }
  // taken.  One tenant = the owner's process TREE: a second instance of the library inside the owner (the hooks build beside the production one) and the owner's
  // supervised children (bench.py's rocprofv3 child runs while the parent sits idle) are the owner's business; anybody else is foreign
  long owner = -1;
  {
    char buf[32] = {0};
    if (pread(fd, buf, sizeof buf - 1, 0) > 0) owner = strtol(buf, nullptr, 10);
  }
  close(fd);
  long pid = (long)getpid();
  for (int depth = 0; depth < 32 && pid > 1 && owner > 1; ++depth) {
    if (pid == owner) { st = 1; return true; }
    char sp[64];
    snprintf(sp, sizeof sp, "/proc/%ld/stat", pid);
    FILE* f = fopen(sp, "r");
    if (!f) break;
    char line[512] = {0};
    const bool got = fgets(line, sizeof line, f) != nullptr;
    fclose(f);
    if (!got) break;
    const char* rp = strrchr(line, ')');                      // pid (comm) state ppid ...: comm may hold spaces and parentheses
    long ppid = -1;
    char state = 0;
    if (!rp || sscanf(rp + 1, " %c %ld", &state, &ppid) != 2) break;
    pid = ppid;
  }
  st = 2;
  return false;
#else
  (void)device;
  return true;
#endif
}

// "0 = default" capacities of the optional modules (include/mldhip.h "mldhip_config"): resolved before config_error reads them; the handle stores the resolved values
void resolve_defaults(mldhip_config& c) {
  if (c.clip_layers > 0 && c.clip_max_prompts == 0) c.clip_max_prompts = 2 * c.max_batch;
  if (c.t2m_eval && c.t2m_max_motions == 0) c.t2m_max_motions = 2 * c.max_batch;
  if (c.t2m_eval && c.t2m_max_words == 0) c.t2m_max_words = 32;
  if (c.a2m_rec && c.a2m_max_motions == 0) c.a2m_max_motions = 4 * c.max_batch;
  if (c.uestc_rec && c.uestc_max_motions == 0) c.uestc_max_motions = 2 * c.max_batch;
  if (c.uestc_rec && c.uestc_classes == 0) c.uestc_classes = 40;
  if (c.t2m_metrics && c.metrics_max_rows == 0) c.metrics_max_rows = 8192;
}

// What is wrong with a (full-size, resolved) config, or nullptr: the combinations the library is built for (include/mldhip.h "mldhip_config")
const char* config_error(const mldhip_config* cfg) {
  if (!(cfg->eta >= 0.0f && cfg->eta <= 1.0f)) return "eta must be in [0, 1] (DDIMScheduler.step; NaN refused)";
  if (cfg->eta != 0.0f && cfg->scheduler_type != MLDHIP_SCHED_DDIM) return "eta != 0 needs the DDIM scheduler (DDPMScheduler.step has no eta)";
  if (cfg->eta != 0.0f && (cfg->latent_size * cfg->latent_dim) % 4 != 0) return "eta != 0: latent_size x latent_dim must be a multiple of 4 (one Philox call = 4 draws)";
  const bool novae = cfg->vae_arch == MLDHIP_VAE_NONE;
  if (cfg->vae_arch != MLDHIP_VAE_MLD && cfg->vae_arch != MLDHIP_VAE_ACTOR && !novae) return "vae_arch must be mld, actor or none";
  if (cfg->denoiser_arch != MLDHIP_ARCH_TRANS_ENC && cfg->denoiser_arch != MLDHIP_ARCH_TRANS_DEC) return "denoiser_arch must be trans_enc or trans_dec";
  if (cfg->scheduler_type != MLDHIP_SCHED_DDIM && cfg->scheduler_type != MLDHIP_SCHED_DDPM) return "scheduler_type must be ddim or ddpm";
  if (novae != (cfg->denoiser_arch == MLDHIP_ARCH_TRANS_DEC) || novae != (cfg->scheduler_type == MLDHIP_SCHED_DDPM))
    return "supported combinations: (vae mld|actor, trans_enc, ddim) as in config_mld_*.yaml, or (vae none, trans_dec, ddpm) as in config_novae_humanml3d.yaml";
  if (novae) {
    if (cfg->latent_dim != 512 || cfg->latent_size != 1 || cfg->num_heads * 128 != 512) return "diffusion-only variant: latent_dim [1, 512], 4 heads of 128";
    if (cfg->condition != MLDHIP_COND_TEXT) return "diffusion-only variant: text condition only";
    if (cfg->num_layers < 1 || cfg->num_layers > 24) return "num_layers must be 1..24";
  } else {
    if (cfg->latent_dim != 256 || cfg->latent_size != 1)
      return "mldhip_config.latent_size / latent_dim (model.latent_dim in the YAML): only [1, 256] is built; the reference's [N, 256] ablations "
                 "(N = 2, 5, 7, 10: N + 2 denoiser tokens, mld_denoiser.py:171,187; 2N global / N memory tokens, mld_vae.py:150-163) are not";
    if (cfg->num_heads * 64 != cfg->latent_dim) return "head_dim must be 64";
    if (cfg->num_layers < 3 || cfg->num_layers % 2 == 0 || cfg->num_layers > 17) return "num_layers must be odd, 3..17 (SkipTransformer)";
  }
  if ((cfg->ff_size != 256 && cfg->ff_size != 512 && cfg->ff_size != 1024) || cfg->text_dim % 32) return "ff_size must be 256, 512 or 1024 and text_dim % 32 == 0";
  if (cfg->max_batch < 1 || cfg->max_frames < 1 || cfg->max_frames > 288) return "max_batch >= 1, 1 <= max_frames <= 288";
  if (cfg->condition != MLDHIP_COND_TEXT && cfg->condition != MLDHIP_COND_ACTION) return "condition must be text or action";
  if (cfg->condition == MLDHIP_COND_ACTION && (cfg->nclasses < 1 || cfg->nclasses > 4096)) return "action condition needs 1 <= nclasses <= 4096";
  if (cfg->vae_num_layers < 0 || cfg->vae_num_layers > 17) return "vae_num_layers must be 0..17";
  // MldVae / diffusion-only: joints by recover_from_ric, which reads feature columns 0 .. 4 + 3 (njoints - 1) - 1 (HumanML3D: 22 joints, 263 features; KIT-ML: 21, 251)
  if (cfg->vae_arch != MLDHIP_VAE_ACTOR && (cfg->njoints < 1 || cfg->njoints > 64 || cfg->nfeats < 4 + 3 * (cfg->njoints - 1)))
    return "skeleton: 1 <= njoints <= 64 and nfeats >= 4 + 3 (njoints - 1), the feature columns feats2joints reads (HumanML3D 22 / 263, KIT-ML 21 / 251)";
  if (cfg->nfeats < 1 || cfg->nfeats > 1024) return "nfeats must be 1..1024";
  if (cfg->num_inference_steps < 1 || cfg->num_train_timesteps % cfg->num_inference_steps) return "num_train_timesteps must be a multiple of num_inference_steps";
  if (cfg->scheduler_type == MLDHIP_SCHED_DDIM &&
      (cfg->num_inference_steps - 1) * (cfg->num_train_timesteps / cfg->num_inference_steps) + cfg->steps_offset >= cfg->num_train_timesteps)
    return "steps_offset pushes the first timestep past num_train_timesteps";
  if (cfg->precision == 3) return "precision 3 (MLDHIP_PREC_FP8_DENOISER of ABI <= 4) was retired in ABI 5: it met no tolerance and was slower than MLDHIP_PREC_F16X3 (include/mldhip.h)";
  if (cfg->precision < MLDHIP_PREC_F32 || cfg->precision > MLDHIP_PREC_BF16) return "unsupported precision";
  if (cfg->max_in_flight < 1 || cfg->max_in_flight > 8) return "max_in_flight must be 1..8";
  if (cfg->clip_layers < 0 || cfg->clip_layers > 48) return "clip_layers must be 0 (no text tower) .. 48";
  if (cfg->clip_layers > 0) {      // the CLIP text tower (mldhip_text_encode)
    if (cfg->clip_heads < 1 || cfg->clip_ff < 1 || cfg->clip_vocab < 1 || cfg->clip_ctx < 1 || cfg->clip_max_prompts < 1) return "text tower: clip_heads, clip_ff, clip_vocab, clip_ctx and clip_max_prompts must be positive";
    if (cfg->text_dim % cfg->clip_heads || cfg->text_dim / cfg->clip_heads != 64) return "text tower: text_dim / clip_heads must be 64 (head dim of the attention kernel)";
    if (cfg->clip_ctx > 80) return "text tower: clip_ctx must be <= 80 (five key tiles of 16)";
    if (cfg->text_dim != 768 || cfg->clip_ff != 3072) return "text tower: the GEMMs are built for text_dim 768 and clip_ff 3072 (CLIP ViT-L/14)";
    if (cfg->precision == MLDHIP_PREC_BF16) return "text tower: MLDHIP_PREC_BF16 is refused (exact fp32 or split-f16 only)";
    if ((long long)cfg->clip_max_prompts * cfg->clip_ctx > (1 << 20)) return "text tower: clip_max_prompts x clip_ctx must be <= 2^20 rows";
  }
  if (cfg->t2m_eval != 0 && cfg->t2m_eval != 1) return "t2m_eval must be 0 (no evaluators) or 1 (both T2M evaluator towers)";
  if (cfg->t2m_eval) {             // the T2M evaluator towers (mldhip_t2m_motion_embed / mldhip_t2m_text_embed)
    if (cfg->precision == MLDHIP_PREC_BF16) return "evaluator towers: MLDHIP_PREC_BF16 is refused (exact fp32 or split-f16 only)";
    if (cfg->nfeats < 8 || cfg->nfeats - 4 > kEvalConvC) return "evaluator towers: nfeats must be 8 .. 292 (the first convolution's GEMM is built for up to 288 input channels)";
    if (cfg->t2m_max_motions < 1 || cfg->t2m_max_motions > (1 << 20)) return "evaluator towers: t2m_max_motions must be 1 .. 2^20";
    if (cfg->t2m_max_words < 1 || cfg->t2m_max_words > 1024) return "evaluator towers: t2m_max_words must be 1 .. 1024";
  }
  if (cfg->smpl_verts < 0 || cfg->smpl_verts > 16384) return "smpl_verts must be 0 (no body model) .. 16384";
  if (cfg->smpl_verts > 0 && cfg->nfeats != 150) return "body model: nfeats must be 150 (25 slots x 6: rot6d of 24 joints + the translation slot)";
  if (cfg->a2m_rec != 0 && cfg->a2m_rec != 1) return "a2m_rec must be 0 (no recognizer) or 1 (the HumanAct12 recognition GRU)";
  if (cfg->a2m_rec && (cfg->a2m_max_motions < 1 || cfg->a2m_max_motions > (1 << 20))) return "recognition GRU: a2m_max_motions must be 1 .. 2^20";
  if (cfg->uestc_rec != 0 && cfg->uestc_rec != 1) return "uestc_rec must be 0 (no recognizer) or 1 (the UESTC recognition ST-GCN)";
  if (cfg->uestc_rec) {            // the UESTC recognition ST-GCN (mldhip_uestc_recognize)
    if (cfg->precision == MLDHIP_PREC_BF16) return "recognition ST-GCN: MLDHIP_PREC_BF16 is refused (exact fp32 or split-f16 only)";
    if (cfg->uestc_max_motions < 1 || cfg->uestc_max_motions > (1 << 20)) return "recognition ST-GCN: uestc_max_motions must be 1 .. 2^20";
    if (cfg->uestc_classes < 1 || cfg->uestc_classes > 256) return "recognition ST-GCN: uestc_classes must be 1 .. 256";
  }
  if (cfg->t2m_metrics != 0 && cfg->t2m_metrics != 1) return "t2m_metrics must be 0 (no metric kernels) or 1 (mldhip_t2m_match / mldhip_act_stats / mldhip_pair_dist)";
  if (cfg->t2m_metrics && (cfg->metrics_max_rows < 2 || cfg->metrics_max_rows > (1 << 20))) return "metric kernels: metrics_max_rows must be 2 .. 2^20";
  return nullptr;
}

// The workspace carve: one HBM arena per context, the handle's buffer members are offsets into it (bind_context).  want(&member, floats) appends a buffer.
struct Carver {
  E* e;
  size_t off = 0;
  void operator()(float** p, size_t nfl) { e->carve.push_back({p, off}); off += align_up(nfl); }
};
struct CarveDims { size_t D, F, TD, NF, Bm, Tm, n, L; };
CarveDims carve_dims(const mldhip_config& c) {
  return {(size_t)c.latent_dim, (size_t)c.ff_size, (size_t)std::max(c.text_dim, c.latent_dim), (size_t)c.nfeats, (size_t)c.max_batch, (size_t)c.max_frames,
          (size_t)c.num_inference_steps, (size_t)c.num_layers};
}

void carve_novae(E* e, Carver& want) {
  const mldhip_config* cfg = &e->cfg;
  const auto [D, F, TD, NF, Bm, Tm, n, L] = carve_dims(e->cfg);
  // diffusion-only: M = 2*B*T rows of width 512; raw-motion latents [B][T][NF]; eps of the CFG batch [2B][T][NF]
  const size_t r2 = 2 * Bm * Tm, KPn = novae_kp(e);
  want(&e->X0, r2 * D); want(&e->Ha, r2 * D); want(&e->Hb, r2 * D); want(&e->H1, r2 * D); want(&e->LNO, 0);
  for (int i = 0; i < 8; ++i) want(&e->S[i], 0);
  want(&e->QKV, r2 * 3 * D); want(&e->AO, r2 * D); want(&e->FF, r2 * std::max(F, KPn));
  want(&e->lat, Bm * Tm * NF); want(&e->zbuf, 0);
  want(&e->Po, 0); want(&e->Pf, 0); want(&e->Ps, 0); want(&e->TP, 2 * Bm * D);
  want(&e->T1, n * D); want(&e->temb0, n * TD); want(&e->tmid, n * D);
  want(&e->text_bias, D); want(&e->time_b2pe, D); want(&e->t1_one, D); want(&e->temb0_one, TD + D);
  want(&e->cv1, 0); want(&e->cvec, 0);
  want(&e->WskelP, D * KPn);
  want(&e->feats_int, 2 * Bm * Tm * NF); want(&e->joints_int, Bm * Tm * cfg->njoints * 3);
  want(&e->TKV, L * n * 2 * D); want(&e->XKV, L * 2 * Bm * 2 * D); want(&e->TKV_one, L * 2 * D);
  {
    const size_t Hn = (size_t)cfg->num_heads;      // folded memory tokens ("cross_fold"): w, u [L][tokens][H][D], c [L][tokens][H]
    want(&e->TKW, L * n * Hn * D); want(&e->TKU, L * n * Hn * D); want(&e->TKC, L * n * Hn);
    want(&e->XKW, L * 2 * Bm * Hn * D); want(&e->XKU, L * 2 * Bm * Hn * D); want(&e->XKC, L * 2 * Bm * Hn);
    want(&e->TKW_one, L * Hn * D); want(&e->TKU_one, L * Hn * D); want(&e->TKC_one, L * Hn);
  }
  want(&e->seed_slot, 2);
}

void carve_latent(E* e, Carver& want) {
  const mldhip_config* cfg = &e->cfg;
  const auto [D, F, TD, NF, Bm, Tm, n, L] = carve_dims(e->cfg);
  const size_t Lv = std::max<size_t>(L, vae_layers(e));
  const size_t rows = std::max(Bm * (Tm + 2), 6 * Bm);   // decoder: B*T frame rows; encoder: B*(T+2) token rows
  const size_t KP = (NF + 31) / 32 * 32;                 // feature width padded to the MFMA K chunk
  want(&e->X0, rows * D); want(&e->Ha, rows * D); want(&e->Hb, rows * D); want(&e->H1, rows * D); want(&e->LNO, rows * D);
  for (int i = 0; i < 8; ++i) want(&e->S[i], (i < (int)(L - 1) / 2) ? rows * D : 0);
  want(&e->QKV, rows * 3 * D); want(&e->AO, rows * D); want(&e->FF, rows * std::max(F, KP));   // FF: the FFN hidden rows, and encode_body's padded features [B*T][KP]
  want(&e->lat, Bm * D); want(&e->zbuf, Bm * D);
  want(&e->FS, (Bm + 7) / 8 * ((L - 1) / 2) * 48 * D);
  {
    // cluster loop (kernels/loop_cluster.hpp): at most kClMaxClusters clusters of 8 motions, 12 workgroups each, launched in rows of 8 XCD slots
    const size_t ncl = D == 256 ? std::min<size_t>(kClMaxClusters, (Bm + 7) / 8) : 0, wgs = std::max<size_t>(8 * kClMembers * ((ncl + 7) / 8), 8 * kClMembersMax);
    want(&e->cl_xbuf, ncl * kClXFloats); want(&e->cl_park, wgs * ((L - 1) / 2) * 16 * 256); want(&e->cl_flags, ncl ? ncl * kClFlagWords + 16 : 0);
  }
  want(&e->Po, 6 * Bm * D); want(&e->Pf, 8 * 6 * Bm * D); want(&e->Ps, 2 * 6 * Bm * D); want(&e->TP, 2 * Bm * D);
  want(&e->T1, n * D); want(&e->temb0, n * TD); want(&e->tmid, n * D);
  want(&e->text_bias, D); want(&e->time_b2pe, D); want(&e->t1_one, D); want(&e->temb0_one, TD + D);
  want(&e->cv1, Lv * Bm * D); want(&e->cvec, Lv * Bm * D);
  want(&e->WskelP, D * KP);
  want(&e->feats_int, Bm * Tm * NF); want(&e->joints_int, Bm * Tm * cfg->njoints * 3);
  want(&e->len_rep, Bm);
  want(&e->text_in, 2 * Bm * TD); want(&e->lat_in, Bm * D);
}

// workspace of the CLIP text tower (engine/path_clip.hpp), carved only when clip_layers > 0: sized for clip_max_prompts x clip_ctx token rows
void carve_clip(E* e, Carver& want) {
  const auto& c = e->cfg;
  if (c.clip_layers <= 0) return;
  const size_t Pm = (size_t)c.clip_max_prompts, R = Pm * (size_t)c.clip_ctx, W = (size_t)c.text_dim, F = (size_t)c.clip_ff;
  want(&e->cX, R * W); want(&e->cLN, R * W); want(&e->cQKV, R * 3 * W); want(&e->cAO, R * W); want(&e->cFF, R * F);
  want(&e->cE0, Pm * W); want(&e->cE1, Pm * W);
  want(&e->cTab, 2 * R + 4 * Pm);      // ints: token id and position per row; row offset, row count and EOS row per unique prompt; unique index per prompt
}

// workspace of the T2M evaluator towers (engine/path_eval.hpp), carved only when t2m_eval = 1: sized for one chunk of kEvalChunk motions x max_frames frames /
// captions x t2m_max_words words
void carve_eval(E* e, Carver& want) {
  const auto& c = e->cfg;
  if (!c.t2m_eval) return;
  const size_t Bc = (size_t)std::min(c.t2m_max_motions, kEvalChunk), TP = (size_t)eval_tp(c.max_frames), R1 = TP / 2, R2 = TP / 4;
  const size_t rows = Bc * std::max<size_t>(R2, (size_t)c.t2m_max_words);
  want(&e->vG0, (Bc * TP + 2) * kEvalConvC); want(&e->vG1, (Bc * R1 + 2) * kEvalMove);
  want(&e->vA, rows * kEvalMotionH); want(&e->vB, rows * kEvalMove);
  want(&e->vGi, std::max<size_t>(Bc * R2 * 6 * kEvalMotionH, Bc * (size_t)c.t2m_max_words * 6 * kEvalTextH));
  want(&e->vH0, Bc * 2 * kEvalMotionH); want(&e->vH1, Bc * 2 * kEvalMotionH); want(&e->vHead, Bc * kEvalMotionH);
  want(&e->vTab, 3 * Bc);      // ints: rows per motion behind each convolution, GRU steps per motion
}

// workspace of the SMPL body model (engine/path_smpl.hpp), carved only when smpl_verts > 0: one chunk of frames
void carve_smpl(E* e, Carver& want) {
  if (e->cfg.smpl_verts <= 0) return;
  const size_t F = (size_t)smpl_chunk_frames(e), tiles = F / 16;
  want(&e->sPf, tiles * kSmplPfTile); want(&e->sA, tiles * kSmplATile); want(&e->sAux, F * 4);
  want(&e->sTab, (size_t)e->cfg.max_batch);      // ints: the call's lengths
}

// workspace of the HumanAct12 recognition GRU (engine/path_a2m.hpp), carved only when a2m_rec = 1: the call's lengths
void carve_a2m(E* e, Carver& want) {
  if (!e->cfg.a2m_rec) return;
  want(&e->rTab, (size_t)e->cfg.a2m_max_motions);      // ints
}

// workspace of the UESTC recognition ST-GCN (engine/path_uestc.hpp), carved only when uestc_rec = 1: one chunk of up to kUestcChunk motions at max_frames frames (kUestcWsCap floats at the most)
void carve_uestc(E* e, Carver& want) {
  if (!e->cfg.uestc_rec) return;
  const size_t T = (size_t)e->cfg.max_frames, per = uestc_z_floats((int)T) + 4 * uestc_pad_floats((int)T);
  const size_t n = std::max<size_t>(1, std::min<size_t>((size_t)std::min(e->cfg.uestc_max_motions, kUestcChunk), kUestcWsCap / per));
  e->uestc_ws_floats = n * per;
  want(&e->uZ, e->uestc_ws_floats + 4 * kUestcSlack + 5 * kAlign);      // + the slack rows behind each padded buffer and the five buffers' alignment
}

// workspace of the text-to-motion metric kernels (engine/path_metrics.hpp), carved only when t2m_metrics = 1: the a | b index tables of mldhip_pair_dist
void carve_metrics(E* e, Carver& want) {
  if (!e->cfg.t2m_metrics) return;
  want(&e->mTab, 2 * (size_t)e->cfg.metrics_max_rows);      // ints
}

// Kernels launched with more dynamic LDS than the default limit register their size once per process and device (tests/test_cabi.py compares this list
// with the MLD_LAUNCH sites of engine/*.hpp)
void register_dynamic_lds() {
#if !defined(MLDHIP_SIM)
  // the decoder attention keeps K and V of one (sample, head) in LDS: up to 2*18*16*68*4 = 153 KiB
  const int big = 2 * 18 * 16 * 68 * 4;
  (void)hipFuncSetAttribute((const void*)attn_decode_kernel<13>, hipFuncAttributeMaxDynamicSharedMemorySize, big);
  (void)hipFuncSetAttribute((const void*)attn_decode_kernel<18>, hipFuncAttributeMaxDynamicSharedMemorySize, big);
  (void)hipFuncSetAttribute((const void*)attn_decode_kernel<7>, hipFuncAttributeMaxDynamicSharedMemorySize, big);
  (void)hipFuncSetAttribute((const void*)attn_decode_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, big);
  (void)hipFuncSetAttribute((const void*)attn_decode_x3_kernel<7>, hipFuncAttributeMaxDynamicSharedMemorySize, attn_x3_lds_bytes<7>());
  (void)hipFuncSetAttribute((const void*)attn_decode_x3_kernel<13>, hipFuncAttributeMaxDynamicSharedMemorySize, attn_x3_lds_bytes<13>());
  (void)hipFuncSetAttribute((const void*)attn_decode_x3_kernel<18>, hipFuncAttributeMaxDynamicSharedMemorySize, attn_x3_lds_bytes<18>());
  const int big128 = 18 * 16 * 132 * 4;   // attn_seq_kernel<*,128>: one operand (K, then V) of up to 288 keys x 132 floats = 148.5 KiB
  (void)hipFuncSetAttribute((const void*)attn_seq_kernel<4, 128>, hipFuncAttributeMaxDynamicSharedMemorySize, big128);
  (void)hipFuncSetAttribute((const void*)attn_seq_kernel<7, 128>, hipFuncAttributeMaxDynamicSharedMemorySize, big128);
  (void)hipFuncSetAttribute((const void*)attn_seq_kernel<13, 128>, hipFuncAttributeMaxDynamicSharedMemorySize, big128);
  (void)hipFuncSetAttribute((const void*)attn_seq_kernel<18, 128>, hipFuncAttributeMaxDynamicSharedMemorySize, big128);
  (void)hipFuncSetAttribute((const void*)attn_seq_x3_kernel<4, 128>, hipFuncAttributeMaxDynamicSharedMemorySize, (attn_seq_x3_lds_bytes<4, 128>()));
  (void)hipFuncSetAttribute((const void*)attn_seq_x3_kernel<7, 128>, hipFuncAttributeMaxDynamicSharedMemorySize, (attn_seq_x3_lds_bytes<7, 128>()));
  (void)hipFuncSetAttribute((const void*)attn_seq_x3_kernel<13, 128>, hipFuncAttributeMaxDynamicSharedMemorySize, (attn_seq_x3_lds_bytes<13, 128>()));
  (void)hipFuncSetAttribute((const void*)attn_seq_x3_kernel<18, 128>, hipFuncAttributeMaxDynamicSharedMemorySize, (attn_seq_x3_lds_bytes<18, 128>()));
  (void)hipFuncSetAttribute((const void*)strip_gemm_x3_kernel<6, 1, false, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (strip_gemm_lds_bytes<6, 1, true>()));
  (void)hipFuncSetAttribute((const void*)strip_gemm_x3_kernel<4, 1, false, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (strip_gemm_lds_bytes<4, 1, true>()));
  (void)hipFuncSetAttribute((const void*)strip_gemm_x3_kernel<4, 2, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (strip_gemm_lds_bytes<4, 2, false>()));
  (void)hipFuncSetAttribute((const void*)strip_gemm_x3_kernel<6, 1, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (strip_gemm_lds_bytes<6, 1, false>()));
  (void)hipFuncSetAttribute((const void*)strip_gemm_x3_kernel<4, 1, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (strip_gemm_lds_bytes<4, 1, false>()));
  (void)hipFuncSetAttribute((const void*)ffn_strip_x3_kernel<6>, hipFuncAttributeMaxDynamicSharedMemorySize, ffn_strip_lds_bytes<6>());
  (void)hipFuncSetAttribute((const void*)ffn_strip_x3_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, ffn_strip_lds_bytes<4>());
  (void)hipFuncSetAttribute((const void*)ffn_strip_x3_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize, ffn_strip_lds_bytes<3>());
  (void)hipFuncSetAttribute((const void*)ffn_strip_x3_kernel<3, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, ffn_strip_lds_bytes<3>());
  (void)hipFuncSetAttribute((const void*)dec_tail_l0_x3_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, ffn_strip_lds_bytes<3>());
  (void)hipFuncSetAttribute((const void*)final_strip_x3_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, final_strip_lds_bytes());
  (void)hipFuncSetAttribute((const void*)final_strip2_x3_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, final_strip_lds_bytes());
  (void)hipFuncSetAttribute((const void*)final_joints_x3_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, final_strip_lds_bytes());
  (void)hipFuncSetAttribute((const void*)attn_flash_x3_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kFlashLdsBytes);
  (void)hipFuncSetAttribute((const void*)attn_flash_h_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kFlashHLdsBytes);
  (void)hipFuncSetAttribute((const void*)strip_inproj_h_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, inproj_h_lds_bytes<4>());
  (void)hipFuncSetAttribute((const void*)strip_inproj_h_kernel<6>, hipFuncAttributeMaxDynamicSharedMemorySize, inproj_h_lds_bytes<6>());
  (void)hipFuncSetAttribute((const void*)attn_flash128_x3_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kFlash128LdsBytes);
  (void)hipFuncSetAttribute((const void*)cross2_fold_ln_kernel<512, 128>, hipFuncAttributeMaxDynamicSharedMemorySize, kC2LdsBytes);
  (void)hipFuncSetAttribute((const void*)cross_fold_kernel<512, 128>, hipFuncAttributeMaxDynamicSharedMemorySize, kCrossFoldLdsBytes);
  (void)hipFuncSetAttribute((const void*)attn_decode_x3_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, attn_x3_lds_bytes<4>());
  (void)hipFuncSetAttribute((const void*)clip_attn_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kClipAttnLdsBytes);
  (void)hipFuncSetAttribute((const void*)clip_attn_x3_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kClipAttnX3LdsBytes);
  (void)hipFuncSetAttribute((const void*)gemm_pipe_x3_kernel<2, 4, 4, 4, 16, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, (gemm_pipe_lds_bytes<2, 4, 4, 4>()));
  (void)hipFuncSetAttribute((const void*)gemm_pipe_x3_kernel<2, 4, 4, 4, 32, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, (gemm_pipe_lds_bytes<2, 4, 4, 4>()));
  (void)hipFuncSetAttribute((const void*)den_loop_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, kLoopLdsBytes);
  (void)hipFuncSetAttribute((const void*)den_loop_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, kLoopLdsBytes);
  (void)hipFuncSetAttribute((const void*)den_loop_kernel<false, kLoopEta>, hipFuncAttributeMaxDynamicSharedMemorySize, kLoopLdsBytes);
  (void)hipFuncSetAttribute((const void*)den_loop_kernel<true, kLoopEta>, hipFuncAttributeMaxDynamicSharedMemorySize, kLoopLdsBytes);
  (void)hipFuncSetAttribute((const void*)den_loop_kernel<false, kLoopFrom>, hipFuncAttributeMaxDynamicSharedMemorySize, kLoopLdsBytes);
  (void)hipFuncSetAttribute((const void*)den_loop_kernel<true, kLoopFrom>, hipFuncAttributeMaxDynamicSharedMemorySize, kLoopLdsBytes);
  (void)hipFuncSetAttribute((const void*)den_loop_kernel<false, kLoopFromEta>, hipFuncAttributeMaxDynamicSharedMemorySize, kLoopLdsBytes);
  (void)hipFuncSetAttribute((const void*)den_loop_kernel<true, kLoopFromEta>, hipFuncAttributeMaxDynamicSharedMemorySize, kLoopLdsBytes);
#if defined(MLDHIP_HOOKS)
  (void)hipFuncSetAttribute((const void*)den_loop_kernel<true, 5>, hipFuncAttributeMaxDynamicSharedMemorySize, kLoopLdsBytes);
#endif
  (void)hipFuncSetAttribute((const void*)den_cluster_kernel<true, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, kClLdsBytes);
  (void)hipFuncSetAttribute((const void*)den_cluster_kernel<false, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, kClLdsBytes);
  (void)hipFuncSetAttribute((const void*)den_cluster_kernel<true, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, kClLdsBytes);
  (void)hipFuncSetAttribute((const void*)den_cluster_kernel<false, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, kClLdsBytes);
  (void)hipFuncSetAttribute((const void*)den_cluster_eta_kernel<true, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, kClLdsBytes);
  (void)hipFuncSetAttribute((const void*)den_cluster_eta_kernel<false, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, kClLdsBytes);
  (void)hipFuncSetAttribute((const void*)den_cluster_eta_kernel<true, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, kClLdsBytes);
  (void)hipFuncSetAttribute((const void*)den_cluster_eta_kernel<false, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, kClLdsBytes);
  (void)hipFuncSetAttribute((const void*)den_cluster_from_kernel<true, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, kClLdsBytes);
  (void)hipFuncSetAttribute((const void*)den_cluster_from_kernel<false, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, kClLdsBytes);
  (void)hipFuncSetAttribute((const void*)den_cluster_from_kernel<true, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, kClLdsBytes);
  (void)hipFuncSetAttribute((const void*)den_cluster_from_kernel<false, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, kClLdsBytes);
  (void)hipFuncSetAttribute((const void*)den_cluster_from_eta_kernel<true, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, kClLdsBytes);
  (void)hipFuncSetAttribute((const void*)den_cluster_from_eta_kernel<false, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, kClLdsBytes);
  (void)hipFuncSetAttribute((const void*)den_cluster_from_eta_kernel<true, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, kClLdsBytes);
  (void)hipFuncSetAttribute((const void*)den_cluster_from_eta_kernel<false, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, kClLdsBytes);
#define MLD_T32_ATTR1(MT, NS, TR, PR) \
  (void)hipFuncSetAttribute((const void*)gemm_tile32_kernel<MT, NS, TR, PR, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, kT32LdsBytes); \
  (void)hipFuncSetAttribute((const void*)gemm_tile32_kernel<MT, NS, TR, PR, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, kT32LdsBytes);
#define MLD_T32_ATTR(NS)                                                                                                    \
  MLD_T32_ATTR1(32, NS, false, PREC_F32) MLD_T32_ATTR1(32, NS, true, PREC_F32) MLD_T32_ATTR1(16, NS, false, PREC_F32) MLD_T32_ATTR1(16, NS, true, PREC_F32) \
  MLD_T32_ATTR1(32, NS, false, PREC_BF16) MLD_T32_ATTR1(16, NS, false, PREC_BF16)                                             \
  MLD_T32_ATTR1(32, NS, false, PREC_F16X3) MLD_T32_ATTR1(16, NS, false, PREC_F16X3)                                         \
  MLD_T32_ATTR1(32, NS, true, PREC_F16X3) MLD_T32_ATTR1(16, NS, true, PREC_F16X3)
  MLD_T32_ATTR(0) MLD_T32_ATTR(1) MLD_T32_ATTR(2) MLD_T32_ATTR(4)
#undef MLD_T32_ATTR
#undef MLD_T32_ATTR1
#define MLD_STRIP_ATTR8(NS, ACT)                                                                                            \
  (void)hipFuncSetAttribute((const void*)gemm_strip_kernel<NS, 1, false, PREC_F32, ACT, 2, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, (strip_lds_bytes<1, 2>())); \
  (void)hipFuncSetAttribute((const void*)gemm_strip_kernel<NS, 1, false, PREC_BF16, ACT, 2, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, (strip_lds_bytes<1, 2>()));;
  MLD_STRIP_ATTR8(0, 0) MLD_STRIP_ATTR8(1, 0) MLD_STRIP_ATTR8(1, 1) MLD_STRIP_ATTR8(2, 0)
#undef MLD_STRIP_ATTR8
#define MLD_STRIP_ATTR8S(NS)                                                                                                \
  (void)hipFuncSetAttribute((const void*)gemm_strip_kernel<NS, 2, false, PREC_F32, 0, 1, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, (strip_lds_bytes<2, 1>())); \
  (void)hipFuncSetAttribute((const void*)gemm_strip_kernel<NS, 2, false, PREC_BF16, 0, 1, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, (strip_lds_bytes<2, 1>()));;
  MLD_STRIP_ATTR8S(1) MLD_STRIP_ATTR8S(2)
  (void)hipFuncSetAttribute((const void*)gemm_strip_kernel<1, 1, false, PREC_F32, 1, 2, 8, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (strip_lds_bytes<1, 2>()));
  (void)hipFuncSetAttribute((const void*)gemm_strip_kernel<2, 1, false, PREC_F32, 0, 2, 8, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (strip_lds_bytes<1, 2>()));
#undef MLD_STRIP_ATTR8S
  (void)hipFuncSetAttribute((const void*)gemm_strip_kernel<0, 1, true, PREC_F32, 0, 1, 8, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (strip_lds_bytes<1, 1>()));
  (void)hipGetLastError();
#endif
}

// mldhip_create's device checks: a gfx950 device at this index; its CU count (a partitioned or masked device has fewer than 256)
int check_device(int device, int* num_cus) {
#if !defined(MLDHIP_SIM)
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_last_error = "no HIP device visible (libmldhip has no CPU path)"; return MLDHIP_ENODEV; }
  if (device < 0 || device >= ndev) { g_last_error = "device index out of range"; return MLDHIP_EINVAL; }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
      g_last_error = std::string("libmldhip is built for gfx950 only; device is ") + prop.gcnArchName;
      return MLDHIP_ENODEV;
    }
    *num_cus = prop.multiProcessorCount;
  }
#endif
  (void)device; (void)num_cus;
  return MLDHIP_OK;
}

// Teardown, also of a partly constructed handle (create_engine's failures come through here): everything the handle and its contexts list as owned
// (engine/state.hpp: device_buffers / events / streams) is released by the loops below -- a new buffer is added to its list beside its declaration, not here.
void destroy_engine(E* e) {
  DeviceGuard dg(e->device);
#if !defined(MLDHIP_SIM)
  (void)hipDeviceSynchronize();      // calls may still be in flight on other streams; their buffers are freed below
  drop_graphs(e, false);
  for (auto& x : e->ctxs)
    for (hipEvent_t* ev : x.events()) if (*ev) (void)hipEventDestroy(*ev);
  for (hipStream_t* s : e->streams()) if (*s) (void)hipStreamDestroy(*s);
  for (hipEvent_t* ev : e->events()) if (*ev) (void)hipEventDestroy(*ev);
#endif
  for (void** p : e->device_buffers()) if (*p) (void)hipFree(*p);
  for (auto& x : e->ctxs)
    for (void** p : x.device_buffers()) if (*p) (void)hipFree(*p);
#if !defined(MLDHIP_SIM)
  if (e->cl_host_status) (void)hipHostFree(e->cl_host_status);
#else
  delete e->cl_host_status;
#endif
  delete e;
}

// The handle of a validated config on a checked device: weight arena, max_in_flight workspace contexts, the capture stream
int create_engine(const mldhip_config& cfg, int device, int num_cus, mldhip_handle** out) {
  DeviceGuard dg(device);      // allocations below land on `device`; the caller's current device is restored on return
  auto* e = new mldhip_engine();
  e->cfg = cfg;
  e->device = device;
#if !defined(MLDHIP_SIM)
  e->num_cus = num_cus;
  e->cluster_foreign = !cluster_lane_owned(device);
  if (hipHostMalloc((void**)&e->cl_host_status, sizeof(unsigned), hipHostMallocMapped) == hipSuccess) *e->cl_host_status = 0u;
  else { e->cl_host_status = nullptr; (void)hipGetLastError(); }
#else
  (void)num_cus;
  e->cl_host_status = new unsigned(0u);
#endif
  declare_params(e);
  build_schedule(e);
  auto fail_create = [&](const char* what) { g_last_error = e->err = what; destroy_engine(e); return MLDHIP_EHIP; };
  if (hipMalloc((void**)&e->arena, e->arena_floats * sizeof(float)) != hipSuccess) return fail_create("hipMalloc(weights) failed");
  Carver want{e};
  if (is_novae(e)) carve_novae(e, want);
  else carve_latent(e, want);
  carve_clip(e, want);
  carve_eval(e, want);
  carve_smpl(e, want);
  carve_a2m(e, want);
  carve_uestc(e, want);
  carve_metrics(e, want);
  const size_t Bm = cfg.max_batch;
  e->ws_floats = want.off;
  e->ctxs.resize(cfg.max_in_flight);
  for (auto& x : e->ctxs) {
    if (hipMalloc((void**)&x.ws, want.off * sizeof(float)) != hipSuccess) return fail_create("hipMalloc(workspace) failed");
    if (hipMemset(x.ws, 0, want.off * sizeof(float)) != hipSuccess) return fail_create("hipMemset(workspace) failed");
    if (hipMalloc((void**)&x.lens, 2 * Bm * sizeof(int32_t)) != hipSuccess || hipMalloc((void**)&x.lens2, Bm * sizeof(int32_t)) != hipSuccess ||
        hipMalloc((void**)&x.labels, 2 * Bm * sizeof(int32_t)) != hipSuccess || hipMalloc((void**)&x.keys, Bm * sizeof(NoiseKey)) != hipSuccess ||
        hipMemset(x.keys, 0, Bm * sizeof(NoiseKey)) != hipSuccess || hipMalloc((void**)&x.traj, Bm * sizeof(TrajRow)) != hipSuccess ||
        hipMemset(x.traj, 0, Bm * sizeof(TrajRow)) != hipSuccess || hipMalloc((void**)&x.starts, Bm * sizeof(StartRow)) != hipSuccess ||
        hipMemset(x.starts, 0, Bm * sizeof(StartRow)) != hipSuccess) return fail_create("hipMalloc(lens) failed");
    x.keys_host.assign(Bm, NoiseKey{0ull, 0ll});
    x.traj_host.assign(Bm, TrajRow{nullptr, 0ll});
    x.starts_host.assign(Bm, StartRow{nullptr, 0, 0, 0.f, 0.f, 0.f, 0});
#if !defined(MLDHIP_SIM)
    for (hipEvent_t* ev : x.events())
      if (hipEventCreateWithFlags(ev, hipEventDisableTiming) != hipSuccess) return fail_create("event create failed");
#endif
  }
  bind_context(e, 0);
  if (hipMalloc((void**)&e->nonfinite, sizeof(unsigned)) != hipSuccess || hipMemset(e->nonfinite, 0, sizeof(unsigned)) != hipSuccess)
    return fail_create("hipMalloc(non-finite counter) failed");
#if !defined(MLDHIP_SIM)
  if (hipStreamCreateWithFlags(&e->cap_stream, hipStreamNonBlocking) != hipSuccess) return fail_create("hipStreamCreate failed");
#endif
  register_dynamic_lds();
  *out = e;
  return MLDHIP_OK;
}

}  // namespace
