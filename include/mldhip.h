/* mldhip.h -- C ABI of libmldhip.so, the MI355X (gfx950) engine for the Motion-Latent-Diffusion
 * sampling hot path:  text embedding -> 50-step DDIM latent sampling with classifier-free
 * guidance -> motion-VAE decode -> (nframe, 22, 3) joints.
 *
 * Every entry point names the reference interface it replaces (paths relative to the
 * ChenFengYe/motion-latent-diffusion tree).  The reference has no FFI of its own (it is pure
 * Python/PyTorch), so "what its FFI for this path would bind" is its plugin surface:
 * instantiate_from_config targets (mld/config.py:16-31) for denoiser / motion_vae / scheduler
 * and the MLD.forward / _diffusion_reverse orchestration (mld/models/modeltype/mld.py:216-360).
 * INTEGRATION.md shows the ctypes binding and the YAML `target:` swap.
 *
 * Conventions
 *   - plain pointers and sizes only; `*_dev` pointers are device (HBM) addresses, `*_host` host.
 *   - all tensors are contiguous row-major float32 unless stated; int32 for lengths.
 *   - every call returns 0 on success or a negative MLDHIP_E* code; nothing throws across the ABI;
 *     mldhip_last_error() gives the message of the last failure on that handle (or globally for
 *     a failed create).
 *   - work is enqueued on the caller's `stream` (a hipStream_t passed as void*, NULL = the null
 *     stream) and is stream-ordered: no implicit device synchronisation.
 *   - the caller owns every I/O buffer; the engine owns weights, workspaces and the captured hipGraphs.
 *   - the request, key, start, guidance and trajectory tables of a call are read on the host before it returns.  actions_host and lengths_host are
 *     handed to hipMemcpyAsync as they are: in pageable memory they are consumed when the call returns (the runtime stages or completes such a copy
 *     before it returns); in page-locked memory (hipHostMalloc, hipHostRegister) they must stay unchanged until the stream has passed the call.
 *   - one handle per device and model variant; a handle is not thread-safe (issue its calls from one host thread).
 *     Calls on DIFFERENT streams overlap on the GPU when the handle was created with max_in_flight > 1.
 */
#ifndef MLDHIP_H_
#define MLDHIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: the declarations of this header are its only exports */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define MLDHIP_ABI_VERSION 8

enum {
  MLDHIP_OK = 0,
  MLDHIP_EINVAL = -1,      /* bad argument / shape / unsupported configuration */
  MLDHIP_ENOKEY = -2,      /* finalize: a required tensor was never loaded */
  MLDHIP_ESTATE = -3,      /* call order violated (e.g. sample before finalize) */
  MLDHIP_EHIP = -4,        /* a HIP runtime call failed (message has the hipError string) */
  MLDHIP_ENODEV = -5       /* no gfx950 device visible */
};

enum { MLDHIP_F32 = 0 };   /* dtype codes for mldhip_load_tensor */

enum {                     /* arithmetic mode of the matrix kernels.  In EVERY mode accumulation, bias, residual,
                              LayerNorm, softmax, the 3-token attention of the reverse loop, the scheduler step and all
                              stored activations are fp32; the modes differ in the operand format fed to the MFMAs of the
                              GEMMs -- and modes 1..3 also run the frame-level self-attention (VAE decoder / encoder,
                              diffusion-only denoiser) on split-f16 products (QK^T and PV as hi + lo halves, fp32 softmax). */
  MLDHIP_PREC_F32 = 0,            /* exact-fp32 MFMA (v_mfma_f32_16x16x4_f32) everywhere: the parity mode */
  MLDHIP_PREC_F16X3 = 1,          /* split-f16: every GEMM operand x = hi + lo with hi = half(x), lo = half(x - hi) (22 mantissa bits),
                                     lo*hi + hi*lo + hi*hi as 3 x v_mfma_f32_16x16x32_f16 with fp32 accumulation, ~5e-7 relative per
                                     product.  VAE decoder / encoder, every GEMM of the diffusion-only variant, and the reverse loop
                                     of the latent models -- both in calls served by the sample-major persistent loop
                                     ("loop_kernel" = 3 / auto from "fused_min_batch" motions) and, since ABI 3, in the latency kernels
                                     that serve ONE bs-64 request ("tile_x3": rounds 1-2 ran that loop in fp32 under the same enum
                                     value); only the column-split loop kernels of 128-319-motion calls stay fp32.  Guarded by the
                                     "Range contract" below (probe at finalize, fp32 fallback per stage, run-time counter).  Meets the 1e-3 joint contract with a 5x margin (tests: every motion of a
                                     2 048-motion call).  Rounds 1-2 split into bf16 halves (16 mantissa bits, 30x the error: the
                                     reverse loop could not use it); ABI value and behaviour of the other entry points unchanged. */
  MLDHIP_PREC_BF16X3_DECODE = 1,  /* the name rounds 1-2 gave mode 1 (kept for source compatibility) */
  MLDHIP_PREC_BF16 = 2            /* operands of EVERY GEMM rounded to bf16 (one v_mfma_f32_16x16x32_bf16 per tile and K chunk):
                                     the "bf16" of BASELINE.json configs[1].  Does NOT meet the 1e-3 joint contract on the
                                     synthetic weights; bench.py reports its measured error next to its throughput, and
                                     profiles/r03_precision_ab.json attributes it per GEMM class. */
  /* 3 was MLDHIP_PREC_FP8_DENOISER (BASELINE.json configs[4]: the reverse-loop GEMMs on v_mfma_f32_16x16x32_fp8_fp8) through ABI 4.  Retired in ABI 5 (VERDICT r5
     item 7: "faster than split-f16 or gone"): measured latents off by 11.9 on |x| ~ 73 AND slower than split-f16 (profiles/r03_precision_ab.json attributes the error
     per GEMM class: e4m3's 3-bit mantissa costs 2^-4 per operand whatever the scaling -- an fp8 reverse loop cannot meet a 1e-3 joint contract under guidance 7.5 x 50
     steps).  mldhip_create refuses the value; config 5 runs in F16X3. */
};

/* Mirrors the keys of configs/config_mld_humanml3d.yaml + configs/modules/{denoiser,motion_vae,
 * scheduler}.yaml that the hot path consumes.
 *
 * Which fields select which kernels.  mldhip_create accepts a family of models (num_layers odd 3..17, or 1..24 for the diffusion-only variant;
 * ff_size 256 / 512 / 1024; text_dim a multiple of 32; nfeats up to 1024; on MldVae and diffusion-only handles a skeleton of 1 <= njoints <= 64 joints with
 * nfeats >= 4 + 3 (njoints - 1), the columns recover_from_ric reads -- HumanML3D 22 / 263, KIT-ML 21 / 251 -- while ActorVae handles take any njoints: their joints need SMPL; any guidance_scale; any num_inference_steps that divides num_train_timesteps;
 * steps_offset, set_alpha_to_one, beta_start, beta_end; nclasses 1..4096 and vae_num_layers 0..17 on action engines), but only some of them get every
 * kernel family:
 *   - the persistent loop ("loop_kernel" 3), the cluster loop ("loop_kernel" 4), the weight streams and the row-strip decoder / encoder kernels
 *     ("ffn_strip", "dec_tail", "dec_lean") are built for latent_dim 256, ff_size 1024, 4 heads only.  With ff_size 256 or 512 the reverse loop runs on the
 *     latency or column-split kernels at every batch size ("loop_kernel" 3 and 4 are refused) and the decoder / encoder layers on the staged GEMMs;
 *   - the one-launch final stage of the decoder (final norm + final_layer, and its joints-only form where 4 + 3 (njoints - 1) <= 128) is built for
 *     256 < nfeats <= 264 (three column blocks: HumanML3D) and for 128 < nfeats < 256 (two column blocks: KIT-ML); every other width, 128 and 256
 *     included, ends in a row LayerNorm and a staged GEMM.  The encoder pads the features to a multiple of 32 columns;
 *   - guidance_scale <= 1 runs the same kernels with guidance 1.0 (the conditional half of the [2B] batch, which the entry points still take); on an
 *     action engine mldhip_denoiser_forward_action then gives no row the zero embedding.
 * All of them compute the same model.  The whole accepted envelope is tested against a float64 reference, on the MI355X and on the functional simulator
 * (tests/test_gpu_config_envelope.py, tests/test_config_envelope_sim.py; measured errors in profiles/config_envelope.json); the action-conditioned
 * models on every loop family, serving entry and ActorVae frame length in tests/test_gpu_action_edges.py and tests/test_action_edges_sim.py
 * (profiles/action_edges.json). */
typedef struct mldhip_config {
  int32_t struct_size;          /* sizeof(mldhip_config), for ABI evolution */
  int32_t latent_dim;           /* model.latent_dim[1]  = 256 */
  int32_t latent_size;          /* model.latent_dim[0]  = 1   */
  int32_t ff_size;              /* 1024 */
  int32_t num_layers;           /* 9 (odd: SkipTransformer, cross_attention.py:26) */
  int32_t num_heads;            /* 4 */
  int32_t nfeats;               /* DATASET.NFEATS = 263 (KIT-ML: 251) */
  int32_t njoints;              /* DATASET.NJOINTS = 22 (KIT-ML: 21); MldVae / diffusion-only: 1..64 with nfeats >= 4 + 3 (njoints - 1) */
  int32_t text_dim;             /* denoiser.params.text_encoded_dim = 768 */
  int32_t max_batch;            /* capacity: motions per sample() call */
  int32_t max_frames;           /* capacity: frames per motion (<= 288 in this release) */
  int32_t num_train_timesteps;  /* scheduler.params.num_train_timesteps = 1000 */
  int32_t num_inference_steps;  /* scheduler.num_inference_timesteps = 50 */
  int32_t steps_offset;         /* 1 */
  int32_t set_alpha_to_one;     /* 0 */
  float beta_start;             /* 0.00085 (scaled_linear) */
  float beta_end;               /* 0.012 */
  float guidance_scale;         /* model.guidance_scale = 7.5 */
  int32_t precision;            /* MLDHIP_PREC_* */
  int32_t use_graph;            /* 1: capture sample() into a hipGraph and replay it */
  /* ---- ABI 2: the action-conditioned variant (configs/config_mld_humanact12.yaml, modules_humanact12/) */
  int32_t condition;            /* MLDHIP_COND_TEXT | MLDHIP_COND_ACTION (denoiser.params.condition) */
  int32_t nclasses;             /* rows of emb_proj.action_embedding (12 HumanAct12, 40 UESTC); action only */
  int32_t vae_arch;             /* MLDHIP_VAE_MLD (MldVae, skip enc-dec) | MLDHIP_VAE_ACTOR (ActorVae decoder) */
  int32_t vae_num_layers;       /* ActorVae: layers of seqTransDecoder (6); 0 = num_layers */
  /* ---- the diffusion-only variant (configs/config_novae_humanml3d.yaml, modules_novae/): latent_dim 512,
   * vae_arch NONE, denoiser_arch TRANS_DEC, scheduler_type DDPM with num_inference_steps 1000, steps_offset 0 */
  int32_t denoiser_arch;        /* MLDHIP_ARCH_TRANS_ENC (skip encoder, mld_denoiser.py:98-119) | MLDHIP_ARCH_TRANS_DEC (:120-133) */
  int32_t scheduler_type;       /* MLDHIP_SCHED_DDIM | MLDHIP_SCHED_DDPM (variance_type fixed_small) */
  /* ---- serving */
  int32_t max_in_flight;        /* 1..8 activation workspaces sharing the weights.  Consecutive calls rotate through them, so
                                 * calls issued on DIFFERENT streams overlap on the GPU (a workspace is reused only after the
                                 * new call's stream has waited for its previous user).  1 = calls serialise as before. */
  /* ---- ABI 6: stochastic DDIM (configs/modules/scheduler.yaml `eta`, passed to DDIMScheduler.step at mld.py:316-320,345-346) */
  float eta;                    /* 0 (default) .. 1: sigma_t = eta * sqrt((1 - ab_p) / (1 - ab_t) * (1 - ab_t / ab_p)), fresh N(0,1) noise every step
                                 * (the "Noise contract" below).  Read only when struct_size covers it (an ABI-5 caller's smaller struct means 0).
                                 * mldhip_create refuses eta < 0, eta > 1, NaN, and eta != 0 with MLDHIP_SCHED_DDPM.  A handle with eta > 0 samples
                                 * through mldhip_sample_many_seeded only: mldhip_sample / _action / _many fail with MLDHIP_ESTATE. */
  /* ---- ABI 7: the optional CLIP text tower (mldhip_text_encode below; transformers CLIPTextConfig of the model at configs/assets.yaml model.clip_path).
   * Read only when struct_size covers them (an ABI-6 caller's smaller struct means no tower).  The tower's width is text_dim.  With clip_layers > 0
   * mldhip_create refuses text_dim / clip_heads != 64, clip_ctx > 80, non-positive sizes, widths other than text_dim 768 / clip_ff 3072 (what the
   * GEMMs are built for) and MLDHIP_PREC_BF16. */
  int32_t clip_layers;          /* num_hidden_layers = 12; 0 (default) = no tower: no weights, no workspace, every text_encoder.* key ignored */
  int32_t clip_heads;           /* num_attention_heads = 12 */
  int32_t clip_ff;              /* intermediate_size = 3072 */
  int32_t clip_vocab;           /* vocab_size = 49408 */
  int32_t clip_ctx;             /* max_position_embeddings = 77 */
  int32_t clip_max_prompts;     /* capacity: prompts per mldhip_text_encode call; 0 (default) = 2 x max_batch (one classifier-free-guidance batch) */
  /* ---- the optional T2M evaluator towers (mldhip_t2m_motion_embed / mldhip_t2m_text_embed below; MLDHIP_ABI_VERSION stays 8: callers detect the feature by
   * the presence of the two symbols).  Read only when struct_size covers them (a caller's struct that ends behind clip_max_prompts means no evaluators).
   * With t2m_eval = 1 mldhip_create refuses MLDHIP_PREC_BF16, nfeats < 8 and nfeats > 292 (the first convolution's GEMM is built for up to 288 input channels). */
  int32_t t2m_eval;             /* 0 (default) = no evaluators: no weights, no workspace, every t2m_* key ignored; 1 = both towers */
  int32_t t2m_max_motions;      /* capacity: motions per mldhip_t2m_motion_embed call and captions per mldhip_t2m_text_embed call; 0 (default) = 2 x max_batch
                                 * (a batch's generated and ground-truth motions in one call) */
  int32_t t2m_max_words;        /* capacity: words per caption (L of mldhip_t2m_text_embed); 0 (default) = 32 */
  /* ---- the optional SMPL body model (mldhip_smpl_forward below; MLDHIP_ABI_VERSION stays 8: callers detect the feature by the presence of the symbol).  Read only
   * when struct_size covers it (a caller's struct that ends behind t2m_max_words means no body model).  With smpl_verts > 0 mldhip_create refuses nfeats != 150;
   * the field is otherwise independent of vae_arch / condition. */
  int32_t smpl_verts;           /* 0 (default) = no body model: no weights, no workspace, every smpl.* key accepted and ignored, mis-shaped ones included;
                                 * 1 .. 16384 = V, the vertex count of the body (SMPL: 6890) */
  /* ---- the optional HumanAct12 action-recognition GRU (mldhip_a2m_recognize below; MLDHIP_ABI_VERSION stays 8: callers detect the feature by the presence of
   * the symbol).  Read only when struct_size covers them (a caller's struct that ends behind smpl_verts means no recognizer).  Independent of condition / vae_arch. */
  int32_t a2m_rec;              /* 0 (default) = no recognizer: no weights, no workspace, every a2m_rec.* key accepted and ignored, mis-shaped ones included;
                                 * 1 = the recognition GRU */
  int32_t a2m_max_motions;      /* capacity: motions per mldhip_a2m_recognize call; 0 (default) = 4 x max_batch (one metric update's four passes -- the classifier
                                 * and the FID net on the generated and the ground-truth motions -- in one call) */
  /* ---- the optional UESTC recognition ST-GCN (mldhip_uestc_recognize below; MLDHIP_ABI_VERSION stays 8: callers detect the feature by the presence of the symbol).
   * Read only when struct_size covers them (a caller's struct that ends behind a2m_max_motions means no net).  Independent of condition / vae_arch / nfeats.
   * With uestc_rec = 1 mldhip_create refuses MLDHIP_PREC_BF16. */
  int32_t uestc_rec;            /* 0 (default) = no net: no weights, no workspace, every uestc_rec.* key accepted and ignored, mis-shaped ones included; 1 = the ST-GCN */
  int32_t uestc_max_motions;    /* capacity: motions per mldhip_uestc_recognize call; 0 (default) = 2 x max_batch (generated + ground truth in one call) */
  int32_t uestc_classes;        /* NC, the width of fcn; 0 (default) = 40 (UESTC); 1 .. 256 */
  /* ---- the optional text-to-motion metric kernels (mldhip_t2m_match / mldhip_act_stats / mldhip_pair_dist below; MLDHIP_ABI_VERSION stays 8: callers detect the
   * feature by the presence of the symbols).  Read only when struct_size covers them (a caller's struct that ends behind uestc_classes means no metrics).
   * Independent of every other field (condition, vae_arch, nfeats, precision); there are no weights, and the calls work before and after mldhip_finalize_weights. */
  int32_t t2m_metrics;          /* 0 (default) = none: no workspace; 1 = the three calls */
  int32_t metrics_max_rows;     /* capacity: N (rows) and P (pairs) of a call; 0 (default) = 8192; 2 .. 2^20.
                                 * WORKSPACE: 2 x metrics_max_rows 32-bit words per context (the a | b index tables of mldhip_pair_dist) and nothing else:
                                 * the statistics keep their chunk sums in registers. */
} mldhip_config;

enum { MLDHIP_COND_TEXT = 0, MLDHIP_COND_ACTION = 1 };
enum { MLDHIP_VAE_MLD = 0, MLDHIP_VAE_ACTOR = 1, MLDHIP_VAE_NONE = 2 /* model.vae_type 'no': latents are raw motion */ };
enum { MLDHIP_ARCH_TRANS_ENC = 0, MLDHIP_ARCH_TRANS_DEC = 1 };
enum { MLDHIP_SCHED_DDIM = 0, MLDHIP_SCHED_DDPM = 1 };

typedef struct mldhip_engine mldhip_handle;

/* Fill *cfg with the config_mld_humanml3d.yaml defaults (max_batch 64, max_frames 196). */
void mldhip_default_config(mldhip_config* cfg);

/* Replaces: get_model(cfg, datamodule) -> MLD.__init__ instantiating denoiser / vae / scheduler
 * (mld/models/get_model.py:4-17, mld/models/modeltype/mld.py:56-83). */
int mldhip_create(const mldhip_config* cfg, int device, mldhip_handle** out);
void mldhip_destroy(mldhip_handle* h);

/* Replaces: model.load_state_dict(ckpt["state_dict"], strict=True) (demo.py:129-150) plus the
 * datamodule's Mean.npy/Std.npy (mld/data/get_data.py:38-40).  `key` is the checkpoint key
 * ("denoiser.encoder.input_blocks.0.self_attn.in_proj_weight", "vae.final_layer.bias", ...) or
 * "mean" / "std".  Keys the engine never reads (denoiser.mem_pos.pe, text_encoder.*, t2m_*) are accepted
 * and ignored (returns 1).  Weight groups (denoiser.*, VAE decoder, VAE encoder, mean/std) are each
 * all-or-nothing; ops of an absent group return MLDHIP_ESTATE.  `src_is_device` != 0 when `data` is a device pointer.
 * With clip_layers > 0 the text tower's tensors form one more optional group (all-or-nothing, like vae.encoder.*):
 *   text_encoder.text_model.text_model.embeddings.{token,position}_embedding.weight, ...encoder.layers.{i}.{layer_norm1,layer_norm2}.{weight,bias},
 *   ...self_attn.{q,k,v,out}_proj.{weight,bias}, ...mlp.{fc1,fc2}.{weight,bias}, ...final_layer_norm.{weight,bias}, text_encoder.text_model.text_projection.weight;
 * every other text_encoder.* key (vision_model.*, visual_projection, logit_scale, position_ids) stays accepted and ignored. */
int mldhip_load_tensor(mldhip_handle* h, const char* key, const void* data, const int64_t* shape,
                       int32_t ndim, int32_t dtype, int32_t src_is_device);

/* Checks every required key arrived, derives step-invariant tables (DDIM coefficients,
 * time-MLP outputs for the scheduler's timesteps, PE-folded biases).  Runs on `stream`. */
int mldhip_finalize_weights(mldhip_handle* h, void* stream);

/* Per-handle tuning options (ABI 3; no reference counterpart, no process-wide environment knobs).  Changing one drops the
 * handle's captured graphs.  Round 4 retired the knobs whose A/B is settled -- each is now simply how the engine works: row-swizzled LDS
 * images in the persistent loop and in the decoder tail ("fused_swz", "ffn_swz"), 4 / 8 weight items in flight ("fused_ring", "strip_ring"),
 * decoder.norm + final_layer as one row-strip launch ("final_strip"), V through the gfx950 transpose read ("attn_tr"), streaming hints on
 * the in-projection's strips ("nt_hints"), pre-split weight images ("split_weights"); round 2's LDS-staged feed-forward kernel
 * ("fused_ffn", kernels/ffn_fused.hpp) is gone.  Names:
 *   "loop_kernel"     reverse loop of the latent models: 0 = auto (default: by motions per call: F16X3 mode -- cluster loop up to
 *                     "cluster_max_batch" = 256 motions, persistent loop above), 1 = latency kernels
 *                     (kernels/tile32.hpp: one request of <= ~128 motions, 41 launches per step), 2 = column-split throughput kernels
 *                     (kernels/strip.hpp: a few hundred motions per call), 3 = the sample-major persistent loop
 *                     (kernels/loop_fused.hpp: ONE launch for all steps of the call, a workgroup per 8 motions, weights streamed in
 *                     consumption order; built for latent_dim 256 / ff_size 1024 / 4 heads in the F32 and F16X3 modes -- refused
 *                     elsewhere).  Its run time does not depend on the batch up to 8 x #CUs = 2 048 motions.  4 = the cluster loop
 *                     (kernels/loop_cluster.hpp, ABI 4 / round 5: ONE launch for all steps of ONE request of up to 128 motions -- 24 (up to 64 motions)
 *                     or 12 workgroups per 8 motions (3 tokens x 8 / 4 column groups) hand partial products to each other inside the launch; F16X3 mode,
 *                     latent_dim 256 / ff_size 1024 / 4 heads, refused elsewhere; 6.8 / 7.6 ms per 50-step loop at 64 / 128 motions against 11.2 / 15.2 ms
 *                     of the latency kernels).  The launch needs its workgroups resident together: it is sized to the chip, every wait inside it is
 *                     bounded (200 ms: the latents of the call are then NaN and counted, and the handle leaves the cluster loop by itself: the kernel also
 *                     sets a pinned host word that the NEXT sample call reads first -- round 6; mldhip_numeric_status / finalize's probe as before), the launch
 *                     is only chosen where its workgroups fit the device in total AND per XCD (round 6: a partitioned device), and calls served by it on
 *                     different streams of this PROCESS are ordered behind each other (one lane per device: two such launches side by side could starve
 *                     each other of CUs).  Across processes (round 6): the first process that creates a handle on a device holds an advisory lock
 *                     (/tmp/mldhip_cluster_lane_<pci bus id>.lock) for its lifetime; any other process on that device never launches the cluster loop
 *                     (mldhip_numeric_info.cluster_loop = 3) and runs the other loop families.  A foreign tenant that fills the GPU with long-running
 *                     workgroups of its own can still delay a launch into its bound: set "cluster_max_batch" 0 there
 *   "many_pipeline"   (round 6) 1 = mldhip_sample_many runs its requests ONE AFTER THE OTHER, each exactly as mldhip_sample would (bit-identical results), with the
 *                     decode of request k on the engine's low-priority side stream beside the reverse loop of request k + 1: the cluster launch leaves 64 of
 *                     256 CUs free and the matrix pipe of the others nearly idle, the decode's 44 launches are one round of workgroups each.  Needs
 *                     max_in_flight >= 2 (two workspaces alternate) and requests the cluster loop serves with a decode asked for; otherwise, and with
 *                     0 (default), the call is one chain over all its motions.  The caller's stream is ordered behind every decode when the call returns
 *                     (requests of one cluster launch each -- up to 128 motions -- also get their inputs and condition rows staged on a third engine stream
 *                     beside the previous request's launch; the request buffers must be the caller's stream's products, as for every entry point)
 *   "cluster_max_batch" auto runs the cluster loop for calls of up to this many motions (default 256: one launch up to 128 = two clusters per XCD, two launches one
 *                     after the other up to 256 -- 2 x 7.6 ms against the persistent loop's flat 18.7 ms; 0 = never)
 *   "cluster_wt"      cluster loop, payload stores of the in-launch hand-offs: 0 (default) = plain where the twelve workgroups of a cluster report one
 *                     XCC id (served by the shared L2), write-through (sc1) for a cluster that spans XCDs; 1 = write-through always (+3.5 % per call)
 *   "cluster_groups"  cluster loop, column groups per token: 0 (default) = 8 (24 workgroups per cluster: the feed-forward block on twice the CUs) for calls
 *                     of up to 64 motions -- every cluster still has an XCD's 32 CUs to itself -- and 4 (12 workgroups) above; 4 / 8 = forced (8 only up to 64)
 *   "fused_min_batch" auto picks the persistent loop from this many motions per call up; 0 (default) = by operand format, from the measured
 *                     crossover table (tools/ab_crossover.py, profiles/r04_loop_crossover.json): 192 on split-f16 MFMAs (19 ms per call
 *                     whatever the batch; the split-f16 latency kernels take 19.0 ms at 192 motions), 1 280 on exact-fp32 MFMAs (73 ms)
 *   "loop_lean"       persistent loop ("loop_kernel" 3 / auto), both operand formats, every entry point: 1 (default) = the LAST denoiser layer of a step works
 *                     on the latent token's rows only -- nothing behind it reads the time and condition rows -- except in its K and V products, which the
 *                     latent query attends to (kernels/loop_fused.hpp `full`; latents equal to the bit); 0 = all three tokens in every layer
 *   "fused_x3"        F16X3 mode: 1 (default) = the persistent loop multiplies on split-f16 MFMAs (row-swizzled operand images, 4 weight
 *                     items in flight per lane: the settled forms of round 3's "fused_swz" / "fused_ring" knobs), 0 = on exact-fp32 MFMAs
 *   "cluster_inject"  (hooks build only) fault injection: 1 + the index of a cluster member that never raises its first flag (the wait bound shrinks to 2 ms): the members
 *                     waiting for it run into the bound, the call returns NaN latents (counted) and the handle leaves the cluster loop at the next mldhip_numeric_status; 0 = off
 *   "cluster_stale"   (hooks build only) 1 = a cluster launch finds an epoch of an earlier launch in one of its polled words (what the r05 memset-node replay fault left
 *                     behind): member 0's entry check must fail the launch (NaN latents, counted; the handle leaves the cluster loop) instead of consuming it as "ready"
 *   "cluster_chunk"   (hooks build only) motions per cluster launch (default 128, a multiple of 8): lets the tests drive the several-launches path of calls above 128
 *                     motions with a few motions
 *   "cluster_lane"    (hooks build only) 0 = calls served by the cluster loop on different streams are not ordered behind each other: two cluster launches side by side
 *                     starve each other of CUs until the 200 ms wait bound fails both (tools/two_streams.py shows it); 1 (default, and always in the production library):
 *                     one lane per device and process
 *   "cluster_graph"   (hooks build only) 1 (default) = calls served by the cluster loop replay captured graphs like every other call; 0 = eager issue.  (Round 5's value 2 --
 *                     flags cleared by a captured hipMemsetAsync node, which reproduced that round's replay fault -- is gone: "cluster_stale" exercises what it led to.)
 *   "fused_dbg"       (hooks build only, include/mldhip_hooks.h; unknown to the production library) 5 = the F16X3 persistent loop with per-phase cycle counters of the first 64 workgroups (same arithmetic, same
 *                     results), read back with mldhip_profile_trace("den_loop_phases") (tools/trace_loop.py); 0 (default) = off.  The
 *                     measurement builds that compute WRONG results (no weight stream, no MFMAs, ...) are not in the library any
 *                     more: tools/loopbench builds them stand-alone
 *   "range_probe"     F16X3 mode: 1 (default) = mldhip_finalize_weights runs the range probe of the "Range contract" below, 0 = skips it
 *                     (the split kernels are used unconditionally), 2 = as 1, and the first text-conditioned mldhip_sample after finalize
 *                     repeats the reverse-loop part on the first 8 motions of ITS batch (the caller's embeddings and start noise) before
 *                     it samples: the verdict then covers a real prompt batch, not only the seeded one.  Setting it un-finalizes the handle.
 *                     The probe is deterministic on every handle, eta > 0 ones included: it runs the eta = 0 step (it measures the
 *                     arithmetic of the kernels, not sampling)
 *   "ffn_strip"       F16X3 mode, decoder / encoder layers: strip height of the register-direct kernels (kernels/ffn_strip.hpp,
 *                     kernels/gemm_strip_x3.hpp): 1 (default) = by launch size -- more than 512 strips of 64 rows: 96-row strips for the
 *                     GEMMs, 48-row strips at two workgroups per CU for the feed-forward block; else 64 rows (one bs-64 request: 196
 *                     strips on 256 CUs instead of 131 longer ones); 6 / 4 = 96 / 64 rows always, 3 = 48 rows for the feed-forward
 *                     block (96 for the GEMMs); 0 = feed-forward block as the two staged GEMMs of kernels/gemm.hpp
 *   "dec_tail"        F16X3 mode, chip-filling launches: 1 (default) = a decoder layer's out-projection + residual + norm1 +
 *                     cross-attention vector + norm2 + feed-forward block as ONE launch (kernels/ffn_strip.hpp TAIL form: the block
 *                     input never goes to HBM), 0 = two launches
 *   "dec_l0_once"     every mode: 1 (default) = the first decoder layer's in-projection runs over ONE sample's rows: its input is
 *                     zeros + the positional rows (mld_vae.py:216-222, actor_vae.py:221-222), the same for every sample, so Q, K, V of
 *                     layer 0 are computed for [T] rows and every (sample, head) attention workgroup reads them (exact: same numbers,
 *                     B times less work and no [B T][3 D] round trip through HBM for that layer); 0 = per sample like the other layers
 *   "dec_lean"        F16X3 mode, chip-filling launches: 1 (default) = the decoder does not compute what the joints never read (results equal
 *                     0 to the bit): a call in which no request asks for features ends in a 67-column final stage (the columns feats2joints
 *                     reads; [M][68] staging rows instead of [M][263]); layer 0 takes its residual from the positional table and its
 *                     attention output from ONE sample per distinct length (no per-sample copy of the positional rows, the other attention
 *                     workgroups return at once); feats2joints counts the non-finite joints while it stores them (no separate pass).
 *                     0 = the full feature row always, per-sample layer 0, the separate counting pass
 *   "dec_half"        F16X3 mode, decoder self-attention block, OPT-IN: 0 (default) = fp32 Q | K | V and split x3 products
 *                     (kernels/gemm_strip_x3.hpp, attention.hpp); 1 = in-projection on half rows x split weights, Q | K | V stored as halves
 *                     (q pre-scaled), attention on plain half operands (kernels/dec_half.hpp) -- kept only if finalize's probe reads the form below
 *                     MLDHIP_PROBE_TOL_HALF on the handle's own weights ("Range contract" below: it is NOT safe in general); 4 / 6 = 1 with
 *                     64- / 96-row in-projection strips; 2 = 1 without the probe's veto (A/B tools)
 *   "tile_x3"         F16X3 mode: 1 (default) = the latency kernels of the reverse loop (kernels/tile32.hpp, one request at a time) multiply
 *                     on split-f16 MFMAs reading the pre-split weight image, 0 = on exact-fp32 MFMAs
 *   "strip_gemm"      F16X3 mode, decoder / encoder in-projection, out-projection (+ residual + LayerNorms) and skip linears:
 *                     1 (default) = row-strip kernels with register-direct weights (kernels/gemm_strip_x3.hpp), 0 = staged tiles
 *   "cross_fold"      diffusion-only variant (latent width 512, 4 heads), every mode: 1 (default) = LayerNorm 1 + the cross-attention sub-layer + LayerNorm 2 of a trans_dec layer
 *                     run as ONE launch (kernels/novae.hpp cross2_fold_ln_kernel).  The memory is two tokens per sample, so (x Wq^T + bq) . k = x . (Wq^T k) + bq . k and
 *                     Wo (p1 v1 + p2 v2) = p1 (Wo v1) + p2 (Wo v2): the query and out-projection GEMMs become 16 dot products / axpys of length 512 per row against vectors
 *                     folded from the memory tokens (time token: per layer and scheduler step at finalize; text tokens: once per call) -- exact algebra, fp32; 0 = the five
 *                     launches (LayerNorm, query GEMM, two-key attention, out-projection GEMM, LayerNorm)
 *   "gemm_pipe"       F16X3 mode, diffusion-only variant (latent width 512): 1 (default) = its K >= 512 GEMMs at >= 2 048 rows run on the
 *                     software-pipelined 128 x 256 tile (kernels/gemm_pipe.hpp: fragments of chunk c + 1 are read while chunk c is
 *                     multiplied, one barrier per 32-wide K chunk; same products in the same order as the 64 x 128 staged tile,
 *                     results identical to the bit), 2 = at any row count (tests), 0 = the 64 x 128 staged tile of kernels/gemm.hpp
 *   "strip_min_rows"  auto picks the column-split throughput kernels when the reverse loop has >= this many token rows (6 x batch; default
 *                     768 = 128 motions) -- in the modes whose latency kernels run fp32 / bf16; in the F16X3 mode the split-f16
 *                     latency kernels serve every call below the persistent loop's threshold (15.2 vs 18.4 ms at 128 motions)
 *   "flash_attn"      split-f16 modes, frame-level self-attention of the decoder / encoder: key-blocked online-softmax kernel with
 *                     two workgroups per CU (kernels/attention.hpp attn_flash_x3_kernel): 0 = never, 1 = auto (default: calls
 *                     with >= 512 (sample, head) pairs), 2 = always.  The diffusion-only variant (head dim 128) has its own form of
 *                     the kernel (attn_flash128_x3_kernel, one workgroup per CU) under the same rule
 *   "gemm_small_m"    row count up to which one-off GEMMs use the register-direct 16x64 shape (default 256; tests set 0
 *                     to drive the LDS-staged kernels at simulator-sized shapes) */
int mldhip_set_option(mldhip_handle* h, const char* name, int64_t value);

/* Range contract of MLDHIP_PREC_F16X3 (ABI 4; ABI 5 adds the decoder's half Q | K | V form, ABI 8 the text tower's stage).  A split operand x = hi + lo keeps 22 mantissa bits only while x sits inside the
 * half format's comfortable range: |x| > 65 504 has no high half (operands produced inside a kernel -- LayerNorm / GELU /
 * attention outputs -- are not clamped: they become inf, then NaN; weights and caller inputs saturate), and the low half of
 * |x| < 2^-3 is a half subnormal (absolute error <= 3e-8 -- harmless for an O(1) tensor, NOT for one that lives at 1e-4: a
 * LayerNorm further down rescales the relative error).  Released checkpoints are unreachable offline, so instead of evidence
 * there is a guard, in three parts:
 *  1. PROBE (mldhip_finalize_weights, option "range_probe"): the handle runs its own split-f16 kernels and its exact-fp32
 *     kernels on one probe batch built from the loaded weights (8 motions, seeded unit-normal latents / condition rows: two
 *     reverse steps of the persistent loop and of the cluster loop (both of its forms since round 6: 24 workgroups per cluster, what calls of up to 64 motions
 *     run, and 12, what calls of 65 .. 256 motions run) and one denoiser call of the latency kernels at the first and last timestep; one
 *     decode of 4 x 64 frames) and compares: err = max|split - fp32| / max|fp32| (for the two loop steps: max|split - fp32| of the
 *     latents / max|latents - start noise| / (2 guidance_scale - 1), i.e. relative to the update the steps made, whatever the schedule).
 *     Diffusion-only variant: one denoiser call on 4 CFG rows x 128 frames, reported as probe_err_decode / decode_split_ok (all of its
 *     GEMMs and its frame-level attention follow that switch).
 *  2. FALLBACK: a stage whose err exceeds MLDHIP_PROBE_TOL (or is not finite) runs on the exact-fp32 kernels from then on --
 *     loop_split_ok = 0: reverse loop (persistent loop and latency kernels on v_mfma_f32_16x16x4_f32, ~3x slower);
 *     decode_split_ok = 0: decoder / encoder / diffusion-only GEMMs and attention.  Results then equal MLDHIP_PREC_F32's.
 *  3. RUN TIME: every sample call counts the non-finite values of the latents and joints it produced into a sticky device
 *     counter (two small launches); mldhip_numeric_status reads it.  A prompt that drives an activation out of range although
 *     the probe passed is therefore reported, not hidden.
 * MLDHIP_PROBE_TOL: on the seeded synthetic weights the probe reads 1.4e-6 .. 1.7e-6 (loop) and 5e-7 (decoder) and the joints of a
 * full-length call end 1.9e-4 from the reference, i.e. ~100x the probe; 6e-6 keeps a 5x margin under the 1e-3 joint contract.  Measured
 * on MI355X (tests/test_gpu_parity.py::test_split_f16_range_contract_out_of_comfort_zone, profiles/r04_range_contract_test.log):
 * LayerNorm gains x 2^+-10 read 1.4e-6 and stay split; weight matrices x 2^-12 read 1.2e-5 and fall back (joints 9e-5 off if forced to
 * stay split); a feed-forward layer whose hidden activation passes 65 504 reads 2.2e-3 / 5e-5 and falls back in both stages (joints 1e-2
 * off without the guard, finite: the conversions saturate before the matrix instructions see an inf).
 * Round 6 (ABI 5): an OPT-IN cheaper form of the decoder's self-attention block inside this mode (option "dec_half", kernels/dec_half.hpp):
 * in-projection with its input rows rounded to ONE half and the weights kept split (2 matrix instructions per product), Q | K | V stored as halves,
 * Q K^T and P V on plain half operands.  The decode is not amplified by guidance x 50 steps, so the question was worth asking per GEMM class
 * (tools/precision_attribution_decoder.py -> profiles/r06_decoder_precision.json): on the committed fixtures' latents (|z| ~ 75) the form costs
 * <= 2e-5 on the joints; on unit-normal latents -- where the per-sample cross-attention vector no longer drowns the frame-to-frame signal -- 3.1e-4
 * (first weight family) and 6.7e-4 .. 8.8e-4 (heavy-tailed second family: rounding Q and K alone costs 5.7e-4), and ANY rounded operand in the
 * feed-forward block / out-projection / skip / final linears costs 1e-3 .. 4e-3 there.  So nothing in the decoder leaves 22-bit products by default;
 * the half form exists for weights that pass the probe: same 4 x 64 frames on UNIT-normal latents, against the exact-fp32 decode of the same latents,
 * bound MLDHIP_PROBE_TOL_HALF = 3e-5 (a decode error of e ends ~ 7.5 e x max|feats| on the joints: 2.5e-4 at most); above it, or with the option
 * off, the block runs on fp32 Q | K | V and x3 products (decode_half_ok = 0).
 * ABI 8: the CLIP text tower (mldhip_text_encode) is a fourth stage.  PROBE: when the handle is F16X3, carries a tower (clip_layers > 0) and its weight group
 * is loaded, finalize encodes four seeded prompts (ids drawn mod clip_vocab; 2, 17, 33 and clip_ctx token rows) on the split-f16 tower and on the exact-fp32
 * tower of the same handle: probe_err_text = max|split - fp32| / max|fp32| over the four embeddings.  FALLBACK: above MLDHIP_PROBE_TOL (or not finite)
 * text_split_ok = 0 and every mldhip_text_encode runs the fp32 GEMMs and attention: results equal MLDHIP_PREC_F32's to the bit.  RUN TIME: the rows the tower's
 * GEMMs read are all produced by its own kernels and are split without a range clamp, so with the probe off a hidden activation beyond 65 504 ends as NaN
 * embeddings in the non-finite counter, not as a saturated finite row.  Readings (two random-init layers at the real widths, MI355X,
 * tests/test_gpu_text_tower_rows.py -> profiles/text_tower_rows.json; every row of the tower against transformers in float64, in units of e32 = the float32-CPU
 * error of the same model): plain weights read 2.3e-6 and stay split (worst row 3.4 x e32); q / k x 4 4.4e-6 (2.0 x), the same with an attention sink on key 0
 * 3.9e-6 (2.5 x), outlier embedding channels 1.0e-6 (1.5 x), fc1 x 8 / x 32 2.7e-6 / 2.4e-6 (3.7 x / 2.7 x): all stay split.  fc1 x 64 with fc2 x 1/64 -- the
 * small-weights limit above: fc2's weights sit at 3e-4, where the low half is a subnormal -- reads 6.1e-5 (4.4e-5 on the one-layer simulator tower, where plain
 * reads 2.8e-6) and falls back; left split it ends 63 x e32 from fp64 with finite outputs and a silent counter.  fc1 x 2^16 (hidden activation 2.4e5) reads inf and
 * falls back; with "range_probe" 0 it returns NaN rows, all of them counted.
 * The T2M evaluator towers (t2m_eval = 1) are a fifth stage.  PROBE: on an F16X3 handle whose evaluator groups are loaded, finalize embeds four seeded motions
 * (T = min(64, max_frames), lengths 64 / 37 / 20 / 4 clipped to T, unit-normal features, no renorm) and four seeded captions (t2m_max_words words at most) on the
 * split-f16 towers and on the exact-fp32 towers of the same handle, and multiplies 16 seeded state rows (uniform in (-1, 1)) with W_hh^T of every tower and direction,
 * split image against fp32 (the embeddings of unit-normal probe rows cannot see a W_hh whose split image lost its precision -- weights near 1e-5, both halves half subnormals
 * -- because the input-side gate terms are O(1) there; a caller's rows may differ): probe_err_eval = the largest max|split - fp32| / max|fp32| of these readings.  FALLBACK: above
 * MLDHIP_PROBE_TOL (or not finite) eval_split_ok = 0 and both towers run their fp32 kernels: results equal MLDHIP_PREC_F32's to the bit.
 * The UESTC recognition ST-GCN (uestc_rec = 1) is a sixth stage.  PROBE: on an F16X3 handle whose uestc_rec.* group is loaded, finalize runs four seeded motions of
 * min(16, max_frames) frames (unit-normal rot6d values) on the split-f16 net and on the exact-fp32 net of the same handle: probe_err_uestc = max|split - fp32| / max|fp32|
 * over features and logits.  FALLBACK: above MLDHIP_PROBE_TOL (or not finite) uestc_split_ok = 0 and the net runs its fp32 GEMMs: results equal MLDHIP_PREC_F32's to the bit.
 * The other modes: F32 has no such limits; BF16 is a reported-only mode whose errors bench.py prints. */
#define MLDHIP_PROBE_TOL 6e-6f
#define MLDHIP_PROBE_TOL_HALF 3e-5f
typedef struct mldhip_numeric_info {
  int32_t struct_size;        /* sizeof(mldhip_numeric_info), set by the caller */
  int32_t probed;             /* 1: finalize ran the probe (F16X3 mode, "range_probe" 1) */
  int32_t loop_split_ok;      /* 1: the reverse loop multiplies on split-f16 MFMAs; 0: fell back to exact fp32 */
  int32_t decode_split_ok;    /* the same for decoder / encoder / diffusion-only GEMMs and attention */
  float probe_err_loop;       /* err of part 1 (-1: not probed) */
  float probe_err_decode;
  int64_t nonfinite_values;   /* non-finite latents / joints elements counted since the previous mldhip_numeric_status call */
  int32_t decode_half_ok;     /* ABI 5.  1: the decoder's self-attention block runs on half Q | K | V ("dec_half"); 0: fp32 Q | K | V, x3 products */
  float probe_err_decode_half; /* the probe's reading of that form (-1: not probed / option off) */
  int32_t cluster_loop;       /* ABI 5.  The one-launch reverse loop of small calls (kernels/loop_cluster.hpp): 0 not built for this handle (mode / shape), 1 available,
                                 2 left after a launch ran into its wait bound (the next sample call already runs on the other loop families; "loop_kernel" 4 re-arms it),
                                 3 another PROCESS holds this device's cluster lane (/tmp/mldhip_cluster_lane_<pci bus id>.lock): never launched by this process */
  int32_t reserved;
  /* ---- ABI 8: the CLIP text tower's stage.  Written only when struct_size covers them (an ABI-7 caller's smaller struct is accepted and gets the fields above). */
  int32_t text_split_ok;      /* 1: mldhip_text_encode multiplies on split-f16 MFMAs; 0: fell back to exact fp32, or no tower / another mode */
  float probe_err_text;       /* the tower stage's err (-1: not probed / no tower) */
  /* ---- the T2M evaluator towers' stage.  Written only when struct_size covers them (the struct that ends behind probe_err_text is accepted). */
  int32_t eval_split_ok;      /* 1: the evaluator towers multiply on split-f16 MFMAs; 0: fell back to exact fp32, or no evaluators / another mode */
  float probe_err_eval;       /* the evaluator stage's err: the larger of the two towers' (-1: not probed / no evaluators) */
  /* ---- the UESTC recognition ST-GCN's stage.  Written only when struct_size covers them (the struct that ends behind probe_err_eval is accepted). */
  int32_t uestc_split_ok;     /* 1: mldhip_uestc_recognize multiplies on split-f16 MFMAs; 0: fell back to exact fp32, or no net / another mode */
  float probe_err_uestc;      /* that stage's err (-1: not probed / no net) */
} mldhip_numeric_info;
/* Synchronises the device (it reads the counter), fills *out and resets nonfinite_values.  No reference counterpart. */
int mldhip_numeric_status(mldhip_handle* h, mldhip_numeric_info* out);

/* Number of tensors the engine requires / names of those still missing (NUL-separated list
 * written to buf, returns the count missing). */
int mldhip_missing_keys(mldhip_handle* h, char* buf, int64_t buflen);

/* Replaces: MLD.forward after the text encoder = _diffusion_reverse + vae.decode + feats2joints
 * (mld/models/modeltype/mld.py:232-240,264; 290-360).
 *   text_emb_dev      [2B, 1, text_dim]  unconditional half first (mld.py:224-231)
 *   init_latents_dev  [B, latent_size, latent_dim]  the torch.randn of mld.py:303 (injected)
 *   lengths_host      [B] int32
 *   latents_out_dev   [B, latent_size, latent_dim]  final latents (may be NULL)
 *   feats_out_dev     [B, Tmax, nfeats]   Tmax = max(lengths); zeros at padded frames (may be NULL)
 *   joints_out_dev    [B, Tmax, njoints, 3]  (may be NULL) */
int mldhip_sample(mldhip_handle* h, const float* text_emb_dev, const float* init_latents_dev,
                  const int32_t* lengths_host, int32_t B, float* latents_out_dev, float* feats_out_dev,
                  float* joints_out_dev, void* stream);

/* Serving entry (ABI 3): several independent requests as ONE reverse-diffusion chain and ONE decode.  Replaces: a loop
 * of MLD.forward calls, one per batch (demo.py:171-186 iterates the batches of a prompt file; test.py does the same over
 * the dataloader).  The reverse loop at bs 64 is a chain of ~2 000 launches with a few hundred rows each; a few requests
 * coalesced run the same chain once at more rows on the throughput kernels (kernels/strip.hpp), and from "fused_min_batch"
 * motions up (default: 320 in the F16X3 mode; the serving shape is 32 x 64 = 2 048 motions) the whole reverse loop of the call is ONE
 * persistent launch, a workgroup per 8 motions (kernels/loop_fused.hpp): one call on one stream fills the chip -- no calls
 * in flight, no stream / hardware-queue placement for the caller to get right.  Motions never interact, so every request
 * gets what mldhip_sample / mldhip_sample_action would have given it (up to fp32 summation order / the mode's operand
 * format).  Sum of B <= max_batch.  Output shapes are those of mldhip_sample with Tmax = max(lengths) of THAT request. */
typedef struct mldhip_request {
  const float* text_emb_dev;      /* [2B, 1, text_dim], unconditional half first (NULL on action engines) */
  const int32_t* actions_host;    /* [B] class labels (action engines; NULL otherwise) */
  const float* init_latents_dev;  /* [B, latent_size, latent_dim] */
  const int32_t* lengths_host;    /* [B] */
  int32_t B;
  float* latents_out_dev;         /* [B, latent_size, latent_dim] or NULL */
  float* feats_out_dev;           /* [B, Tmax, nfeats] or NULL */
  float* joints_out_dev;          /* [B, Tmax, njoints, 3] or NULL */
} mldhip_request;
int mldhip_sample_many(mldhip_handle* h, const mldhip_request* reqs, int32_t nreq, void* stream);

/* Stochastic DDIM (ABI 6).  Noise contract -- one definition for every reverse-loop path of the latent models:
 *   inside one request, motion m (0-based) and latent element e (flat over latent_size x latent_dim, latent_elems of them) draw
 *   at scheduler step i (0-based, in loop order)  z = element (first_index + m) * latent_elems + e  of the stream
 *   mldhip_philox_normal(seed, step_index = i).
 * A motion's noise is therefore a function of (seed, first_index + m, i) alone: not of the loop family or launch that serves it,
 * its position in a coalesced chain, or how a data-parallel run sharded the prompts (pass each shard's global start index as
 * first_index).  The step is diffusers' DDIMScheduler.step(eta) with the CFG-combined eps, z added at every step including the last:
 *   x' = sqrt(ab_p) x0 + sqrt(1 - ab_p - sigma^2) eps + sigma z,   x0 = (x - sqrt(1 - ab_t) eps) / sqrt(ab_t).
 * (A modular loop that draws z from torch's generator cannot reproduce these draws bit for bit; handed the Philox draws it agrees
 * with the fused paths up to the mode's tolerance.) */
typedef struct mldhip_noise_key {
  uint64_t seed;
  int64_t first_index;            /* global index of the request's motion 0 */
} mldhip_noise_key;

/* mldhip_sample_many with one noise key per request (keys[nreq]).  Serves text and action engines on the same path rules as
 * mldhip_sample_many, "many_pipeline" 1 included (there every request is bit-identical to a one-request seeded call with the
 * same key).  On an eta = 0 handle the keys are ignored and the results are bit-identical to mldhip_sample_many.  The keys are
 * uploaded with every call: a new seed replays the already-captured graph. */
int mldhip_sample_many_seeded(mldhip_handle* h, const mldhip_request* reqs, const mldhip_noise_key* keys, int32_t nreq,
                              void* stream);

/* Per-step latent trajectories (added at ABI 8 WITHOUT a version bump: one more symbol, no struct changed -- callers detect it by
 * its presence, dlsym / hasattr).  Replaces: MLD._diffusion_reverse_tsne (mld/models/modeltype/mld.py:362-424), the reverse loop that
 * returns the latents after every scheduler step -- here read out of the loop that serves the call, whichever family that is (one
 * 1 KB row store per motion and step from the registers that hold the step's result; no extra launch).
 *   traj_out_dev      [nreq] device pointers; entry i: [num_inference_steps][B_i][latent_size * latent_dim] floats, or NULL (no trajectory
 *                     for request i).  Row s holds the latents of request i's motions after scheduler step s (0-based, loop order), i.e.
 *                     prev_sample of step s: row num_inference_steps - 1 equals latents_out to the bit (also behind a cluster launch that ran
 *                     into its wait bound: NaN in both).  Every non-NULL entry must be 16-byte aligned (the kernels store a row four floats at
 *                     a time, straight into the caller's buffer; any hipMalloc / torch allocation is): MLDHIP_EINVAL otherwise.
 *   keys              one mldhip_noise_key per request, as for mldhip_sample_many_seeded; may be NULL on an eta = 0 handle (nothing is drawn),
 *                     MLDHIP_EINVAL on an eta > 0 one.
 * traj_out_dev NULL, or every entry NULL: the call IS mldhip_sample_many_seeded -- same path, same captured graphs, same bits.  Otherwise the
 * path rules of mldhip_sample_many apply (text and action engines, eta = 0 and eta > 0, every loop family) with one exception: a call that
 * asks for any trajectory runs as ONE chain over all its motions even under "many_pipeline" 1 (sum of B <= max_batch).  Latents, features and
 * joints of such a call are bit-identical to the same call without trajectories on that path.  The buffers are reached through an engine-owned
 * table uploaded with every call, so the captured graph of the shape is replayed whatever buffers the caller passes.
 * The diffusion-only variant (MLDHIP_VAE_NONE) refuses a non-NULL trajectory with MLDHIP_EINVAL. */
int mldhip_sample_many_traj(mldhip_handle* h, const mldhip_request* reqs, const mldhip_noise_key* keys /* NULL on an eta = 0 handle */,
                            float* const* traj_out_dev /* [nreq]; entry i: [num_inference_steps][B_i][latent_size * latent_dim] or NULL */,
                            int32_t nreq, void* stream);

/* Start the reverse loop from a source latent at a chosen step (added at ABI 8 WITHOUT a version bump, as mldhip_sample_many_traj was: one more symbol and one
 * more struct, nothing existing changed -- callers detect it by its presence).  n = num_inference_steps, t_i = timesteps[i]; every motion of request i starts as
 * starts[i] says:
 *   src_latents_dev NULL (first_step 0, noised 0)   x = init_latents * init_noise_sigma,                                     steps 0 .. n-1, as mldhip_sample_many
 *   src given, 0 <= f < n, noised = 0               x = sqrt(ab_{t_f}) src + sqrt(1 - ab_{t_f}) init_latents,                steps f .. n-1
 *                                                   (diffusers' add_noise at the first timestep that is run, as its image-to-image pipelines do)
 *   src given, 0 <= f < n, noised = 1               x = src as it is -- the loop state in front of step f, e.g. row f-1 of a trajectory --
 *                                                   steps f .. n-1; the request's init_latents_dev is not read and may be NULL
 * Steps below f are not applied to the motion.  With eta > 0 the Noise contract is unchanged: step i draws with the absolute step index i.  With a trajectory
 * buffer, rows s < f of the motion are left untouched, rows f .. n-1 are written and row n-1 equals latents_out to the bit.  Decode, feats2joints, the
 * non-finite counter and the range contract are those of any other call.  Requests of one call may start differently; motions never interact, so a motion's
 * results do not depend on where its neighbours start.
 *   starts            [nreq], or NULL.  NULL, or every entry {NULL, 0, 0}: the call IS mldhip_sample_many_traj -- same path, same captured graphs, same bits.
 *                     A source must be 16-byte aligned ([B_i, latent_size, latent_dim] floats; the kernels read a row four floats at a time).
 *   keys, traj_out_dev  as for mldhip_sample_many_traj.
 * Serves text and action engines, eta = 0 and eta > 0, and every loop family (new forms of the loop kernels beside the plain ones, which keep their machine code).
 * MLDHIP_EINVAL: first_step outside [0, n); first_step != 0 or noised != 0 with a NULL source; noised not 0 or 1; init_latents_dev NULL on a request that is not
 * resumed; a misaligned source; any non-trivial start on a MLDHIP_VAE_NONE handle.  A call with any source runs as ONE chain over all its motions, also under
 * "many_pipeline" 1 (sum of B <= max_batch), which is the trajectory rule.  Sources, first steps and the noised flags reach the kernels through an engine-owned
 * per-motion table uploaded with every call: the captured graph of a shape is replayed with fresh buffers and, on the one-launch loops (persistent and cluster),
 * with different first steps; the launch-per-GEMM families issue steps min f .. n-1 and keep one graph per (shape, min f).  A workgroup / cluster of a one-launch
 * loop runs steps min f .. n-1 of ITS motions: a call whose motions all start at f costs about (n - f) / n of a full one. */
typedef struct mldhip_start {
  const float* src_latents_dev;   /* [B, latent_size, latent_dim], or NULL = start from noise at step 0 */
  int32_t first_step;             /* 0 .. num_inference_steps - 1; must be 0 when src_latents_dev is NULL */
  int32_t noised;                 /* 0: src is a clean latent, mixed with init_latents at t_f; 1: src already is x at step f */
} mldhip_start;
int mldhip_sample_many_from(mldhip_handle* h, const mldhip_request* reqs, const mldhip_noise_key* keys /* NULL ok at eta = 0 */,
                            const mldhip_start* starts /* [nreq] */, float* const* traj_out_dev /* NULL ok */, int32_t nreq, void* stream);

/* Per-request classifier-free-guidance scale (added at ABI 8 WITHOUT a version bump, as the two entries above were: one more symbol, no struct changed -- callers
 * detect it by its presence).  mldhip_config.guidance_scale is fixed when the handle is created; here every request of a call may name its own, so one handle (one
 * set of weight images and workspaces) serves callers who choose guidance, and their requests share a chain.
 *   guidance_host     [nreq] host floats, or NULL.
 *                     g_i >= 0 and finite: every motion of request i combines eps = eps_u + g_i * (eps_c - eps_u) with that g_i.  The formula is applied as it stands
 *                       for every such value: g = 0 is the unconditional prediction, g = 1 the conditional one up to a rounding.  (The reference switches CFG off per
 *                       MODEL at guidance_scale <= 1 -- mld.py:300 -- not per sample: there is no per-sample switch to reproduce.)
 *                     g_i < 0 (write -1): the handle's own guidance_scale.
 *                     NULL, or every entry negative: the call IS mldhip_sample_many_from -- same path, same captured graphs, same launch counts, same bits.
 *   starts, keys, traj_out_dev   as for mldhip_sample_many_from; starts may be NULL (no request has a source).
 * MLDHIP_EINVAL: a NaN or infinite entry; a non-negative entry on a handle whose guidance_scale <= 1 (such a model does no CFG, and an action engine then builds no
 * unconditional rows); a non-negative entry on a MLDHIP_VAE_NONE handle (the diffusion-only variant is out of scope, as it is for trajectories).
 * A call with any non-negative entry runs as ONE chain over all its motions, also under "many_pipeline" 1 (sum of B <= max_batch): the trajectory rule.  It serves text
 * and action engines, eta = 0 and eta > 0, with or without trajectories and sources, on every loop family, on the from-forms of the loop kernels: the scale is a field
 * of the per-motion start table that is uploaded with every call, so on the one-launch loops (persistent and cluster) the captured graph of a shape is replayed with
 * different values, and the launch-per-GEMM families keep their graph keys (the values are no part of them).  Motions never interact: a motion's result depends on its
 * own g and not on its neighbours'.
 * Range contract: the verdict of the finalize probe (mldhip_numeric_info) is for the handle's guidance_scale g_0.  The probe models the amplification of the split-f16
 * error by guidance as 2 g - 1, so a request above the handle's value scales that error by (2 g_i - 1) / (2 g_0 - 1).  The engine does not refuse such a request;
 * the non-finite counter (mldhip_numeric_status) applies as ever. */
int mldhip_sample_many_guided(mldhip_handle* h, const mldhip_request* reqs, const mldhip_noise_key* keys /* NULL ok at eta = 0 */,
                              const mldhip_start* starts /* NULL ok */, float* const* traj_out_dev /* NULL ok */,
                              const float* guidance_host /* [nreq] or NULL */, int32_t nreq, void* stream);

/* Replaces: MldDenoiser.forward(sample, timestep, encoder_hidden_states)[0]
 * (mld/models/architectures/mld_denoiser.py:135-228).  sample [R,1,D], text [R,1,text_dim],
 * out [R,1,D]; any integer timestep in [0, num_train_timesteps). */
int mldhip_denoiser_forward(mldhip_handle* h, const float* sample_dev, int32_t timestep,
                            const float* text_emb_dev, int32_t R, float* out_dev, void* stream);

/* Action-conditioned sampling (BASELINE config 5).  Replaces: the sampling core of MLD.a2m_eval
 * (mld/models/modeltype/mld.py:716-735: cond = cat(zeros_like(actions), actions); _diffusion_reverse;
 * vae.decode) for an engine created with condition = MLDHIP_COND_ACTION.
 *   actions_host      [B] int32 class labels in [0, nclasses)
 *   feats_out_dev     [B, Tmax, nfeats]  (rot6d features; mldhip_smpl_forward below turns them into joints and vertices on a handle with smpl_verts > 0) */
int mldhip_sample_action(mldhip_handle* h, const int32_t* actions_host, const float* init_latents_dev,
                         const int32_t* lengths_host, int32_t B, float* latents_out_dev, float* feats_out_dev,
                         void* stream);

/* Replaces: MldDenoiser.forward with condition 'action' (mld_denoiser.py:69-77,171-178 -> EmbedAction,
 * mld_denoiser.py:249-260).  actions_host [R] labels; as in the reference's eval mode with
 * guidance_scale > 1 the FIRST R/2 rows get the zero (unconditional) embedding whatever their label. */
int mldhip_denoiser_forward_action(mldhip_handle* h, const float* sample_dev, int32_t timestep,
                                   const int32_t* actions_host, int32_t R, float* out_dev, void* stream);

/* Diffusion-only sampling (BASELINE config 4).  Replaces: MLD.forward after the text encoder with vae_type 'no'
 * (mld/models/modeltype/mld.py:232-242,264; _diffusion_reverse :290-360 with latents = raw motion [B,Tmax,nfeats]):
 * num_inference_steps x (trans_dec denoiser on the 2B-row CFG batch, guidance, DDPM ancestral step), identity
 * "decode", feats2joints.
 *   text_emb_dev      [2B, 1, text_dim]   unconditional half first
 *   init_latents_dev  [B, Tmax, nfeats]   the torch.randn of mld.py:296-301 (injected), Tmax = max(lengths)
 *   step_noise_dev    [steps, B, Tmax, nfeats] the N(0,1) draw of every scheduler.step (injected; the reference takes
 *                     it from torch's global generator), or NULL: drawn in-kernel from Philox4x32-10(seed, step, element)
 *   feats_out_dev     [B, Tmax, nfeats] (padded frames hold the scheduler's noise, as in the reference; may be NULL)
 *   joints_out_dev    [B, Tmax, njoints, 3] (may be NULL) */
int mldhip_sample_novae(mldhip_handle* h, const float* text_emb_dev, const float* init_latents_dev,
                        const int32_t* lengths_host, int32_t B, const float* step_noise_dev, uint64_t seed,
                        float* feats_out_dev, float* joints_out_dev, void* stream);

/* Replaces: MldDenoiser.forward, diffusion_only + arch trans_dec (mld_denoiser.py:144-146,208-221).
 * sample [R, T, nfeats], text [R, 1, text_dim], lengths_host [R] (rows t >= len of the output are zero; all T frames
 * are attended to, the reference passes no key-padding mask here) -> out [R, T, nfeats]. */
int mldhip_denoiser_forward_novae(mldhip_handle* h, const float* sample_dev, int32_t timestep, const float* text_emb_dev,
                                  const int32_t* lengths_host, int32_t R, int32_t T, float* out_dev, void* stream);

/* Replaces: DDPMScheduler.step(model_output, t, sample).prev_sample (call site mld.py:345-346), variance_type
 * fixed_small.  noise_dev [n] = the step's N(0,1) draw, or NULL for the Philox stream (seed, step_index).
 * n elements, in/out may alias. */
int mldhip_ddpm_step(mldhip_handle* h, const float* eps_dev, int32_t timestep, const float* sample_dev,
                     const float* noise_dev, uint64_t seed, int32_t step_index, float* prev_sample_dev, int64_t n,
                     void* stream);

/* The engine's counter-based Gaussian stream: out[i] = N(0,1) of (seed, step_index, i) -- what mldhip_sample_novae
 * uses when step_noise_dev is NULL (Philox4x32-10 + Box-Muller; restated in numpy in oracle/mld_oracle.py). */
int mldhip_philox_normal(mldhip_handle* h, float* out_dev, int64_t n, uint64_t seed, int32_t step_index, void* stream);

/* Replaces: MldVae.decode(z, lengths) (mld/models/architectures/mld_vae.py:186-248); with
 * vae_arch = MLDHIP_VAE_ACTOR: ActorVae.decode (mld/models/architectures/actor_vae.py:72-74,209-235).
 * z [latent_size, B, D] (== [B, D] for latent_size 1) -> feats [B, Tmax, nfeats]. */
int mldhip_vae_decode(mldhip_handle* h, const float* z_dev, const int32_t* lengths_host, int32_t B,
                      float* feats_out_dev, void* stream);

/* Replaces: MldVae.encode(features, lengths) (mld/models/architectures/mld_vae.py:124-184) -- scope row 8f.1.
 * feats [B, T, nfeats] zero padded (T >= max(lengths)); mu / logvar [B, D] are the Normal's parameters
 * (dist.loc, log of dist.scale^2); when eps_dev [B, D] (the N(0,1) draw of rsample) is given,
 * latent_out = mu + exp(logvar)^0.5 * eps.  Needs the optional weight group vae.encoder.*, vae.skel_embedding.*,
 * vae.global_motion_token, vae.query_pos_encoder.pe. */
int mldhip_vae_encode(mldhip_handle* h, const float* feats_dev, const int32_t* lengths_host, int32_t B, int32_t T,
                      const float* eps_dev, float* latent_out_dev, float* mu_out_dev, float* logvar_out_dev, void* stream);

/* Replaces: DDIMScheduler.step(model_output, t, sample, eta=0).prev_sample (call site
 * mld.py:345-346).  n elements, in/out may alias. */
int mldhip_ddim_step(mldhip_handle* h, const float* eps_dev, int32_t timestep, const float* sample_dev,
                     float* prev_sample_dev, int64_t n, void* stream);

/* Replaces: DDIMScheduler.step(model_output, t, sample, eta=cfg.eta, variance_noise=z).prev_sample with the HANDLE's eta
 * (ABI 6; DDIM handles only).  noise_dev [n] = the step's N(0,1) draw, or NULL: element i of mldhip_philox_normal(seed, step_index)
 * (the Noise contract with first_index 0).  n elements, in/out may alias. */
int mldhip_ddim_step_eta(mldhip_handle* h, const float* eps_dev, int32_t timestep, const float* sample_dev, const float* noise_dev,
                         uint64_t seed, int32_t step_index, float* prev_sample_dev, int64_t n, void* stream);

/* The CLIP text tower (ABI 7; handles created with clip_layers > 0).  Replaces: the text branch of MldTextEncoder.forward behind the tokenizer
 * (mld/models/architectures/mld_clip.py:53-78: text_model.get_text_features(input_ids) -> unsqueeze(1)), i.e. transformers' CLIPModel.get_text_features:
 * token + position embedding, clip_layers pre-LN layers (layer_norm1, causal self-attention with q scaled by head_dim^-0.5, residual, layer_norm2, fc1,
 * quick-GELU x * sigmoid(1.702 x), fc2, residual), final_layer_norm, the EOS row, text_projection (no bias).
 *   ids_host          [P][clip_ctx] token ids as the tokenizer pads them (every id in [0, clip_vocab))
 *   eos_pos_host      [P] position of the EOS token in [0, clip_ctx) (CLIPTextTransformer's pooling rule; the tokenizer stays on the CPU)
 *   text_emb_out_dev  [P][1][text_dim]
 * Exactness rules -- each computes the numbers of the padded [P][clip_ctx] tower, on less work:
 *   1. causality: the attention is causal and the output is read at the EOS row, so ids behind eos_pos never reach it -- they are not read, and prompt p
 *      runs as eos_pos[p] + 1 token rows (all prompts of a call packed into one ragged activation; no padding rows exist);
 *   2. duplicates: identical (ids[0 .. eos_pos], eos_pos) rows of a call -- the B copies of "" of a classifier-free-guidance batch -- are computed once
 *      and stored to every duplicate's output row (deduplicated on the host, on the id rows);
 *   3. the last stage: final_layer_norm and the projection run on the EOS rows only.
 * A prompt's output row is bit-identical whatever else is in the call.  Arithmetic: the handle's mode (MLDHIP_PREC_F32 exact-fp32 MFMAs,
 * MLDHIP_PREC_F16X3 split-f16 GEMMs and attention products -- unless finalize's range probe moved the tower to fp32: "Range contract", text_split_ok; fp32 LayerNorm, softmax, residuals).  Issued eagerly (no hipGraph: the row total changes
 * per call), stream-ordered like every other call; non-finite output values are counted into mldhip_numeric_status like latents and joints.
 * Returns MLDHIP_EINVAL for P > clip_max_prompts, an id outside [0, clip_vocab) or eos_pos outside [0, clip_ctx); MLDHIP_ESTATE when the handle has no
 * tower (clip_layers = 0), the tower's weight group is absent, or the handle is not finalized. */
int mldhip_text_encode(mldhip_handle* h, const int32_t* ids_host, const int32_t* eos_pos_host, int32_t P, float* text_emb_out_dev, void* stream);

/* The T2M evaluator towers (handles created with t2m_eval = 1).  Replaces: the evaluator half of MLD.t2m_eval (mld/models/modeltype/mld.py:675-697):
 * renorm4t2m, MovementConvEncoder -> MotionEncoderBiGRUCo for motions, TextEncoderBiGRUCo for captions (mld/models/architectures/t2m_motionenc.py,
 * t2m_textenc.py), at the released evaluators' widths (configs/base.yaml: movement 512 / 512, motion GRU 1024 -> 512, word 300, POS one-hot 15, text GRU
 * 512 -> 512, unit length 4) -- the only widths the kernels are built for.
 *
 * WEIGHTS.  Two more optional all-or-nothing groups under their checkpoint key names (a wrong shape is MLDHIP_EINVAL, mldhip_missing_keys reports a half-loaded
 * group; with t2m_eval = 0 every t2m_* key stays accepted and ignored, mis-shaped ones included):
 *   motion group: t2m_moveencoder.main.{0,3}.{weight,bias} ([512][nfeats - 4][4], [512][512][4]), t2m_moveencoder.out_net.{weight,bias},
 *                 t2m_motionencoder.input_emb.{weight,bias}, t2m_motionencoder.gru.{weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0} and their four
 *                 *_reverse tensors, t2m_motionencoder.hidden [2][1][1024], t2m_motionencoder.output_net.{0,1,3}.{weight,bias}, mean_eval, std_eval [nfeats];
 *   text group:   t2m_textencoder.pos_emb.{weight,bias}, .input_emb.{weight,bias}, .gru.* (the same eight), .hidden [2][1][512], .output_net.{0,1,3}.{weight,bias}.
 *
 * MATH, motion tower.  feats [B][T][nfeats], lengths [B].
 *   renorm (renorm = 1; needs mean / std): g = (f std + mean - mean_eval) / std_eval on ALL T frames.  PADDED-FRAME RULE: a padded frame (t >= len) holds 0 in f
 *     and therefore a non-zero constant in g; the convolutions of the last valid steps read those rows; before frame 0 and beyond frame T - 1 the convolutions pad
 *     with true zeros.  So a motion's embedding depends on T exactly as it does in the reference (equal for any two T >= len + 7).  renorm = 0: the rows already are in
 *     the evaluators' normalisation (eval_gt).
 *   columns 0 .. nfeats - 5; Conv1d(nfeats - 4 -> 512, k 4, s 2, p 1), LeakyReLU(0.2), Conv1d(512 -> 512, 4, 2, 1), LeakyReLU(0.2), Linear(512, 512): floor(T / 4) rows
 *     per motion (dropout is identity);
 *   Linear(512 -> 1024); a bidirectional one-layer GRU, H = 1024, initial state hidden[dir] for every motion, packed-sequence semantics with m_len = len / 4
 *     (floor): the forward direction runs rows 0 .. m_len - 1, the backward direction m_len - 1 .. 0; a motion's state is untouched outside its own steps;
 *   cat(h_fwd, h_bwd) -> Linear(2048 -> 1024), LayerNorm, LeakyReLU(0.2), Linear(1024 -> 512).
 *   GRU cell (PyTorch's; gate order r | z | n in the stacked weights): r = s(W_ir x + b_ir + W_hr h + b_hr), z likewise, n = tanh(W_in x + b_in + r (W_hn h + b_hn)),
 *     h' = (1 - z) n + z h.
 * MATH, text tower.  word_embs [B][L][300], pos_ohot [B][L][15], text_lengths [B]: x = word + Linear(15 -> 300)(pos); Linear(300 -> 512); the same GRU at H = 512
 *   with packed lengths text_lengths; the same head (1024 -> 512, LayerNorm, LeakyReLU, 512 -> 512).
 * Any order of lengths is taken and rows come back in the caller's order (the reference sorts only because pack_padded_sequence demands it).  A motion's or
 * caption's embedding is bit-identical alone and inside any batch (at the same T / L): one GEMM tile shape and one recurrence kernel at every row count.
 *
 * KERNELS.  kernels/gru.hpp: the staging kernels (renorm + the convolution's zero rows; word + POS linear), the recurrence -- ONE launch per time step (at most 49
 * for 196 frames), both directions and all motions, h W_hh^T on MFMAs with the gate math, the per-motion step mask and the state update fused, state double
 * buffered -- and LayerNorm + LeakyReLU.  Every linear and both convolutions (as GEMMs over tap-major re-laid weights: lda = 2 C, K = 4 C) and the input-side GRU
 * products of both directions (one GEMM, b_hr / b_hz folded into its bias) run on the staged 64 x 128 GEMM tile of kernels/gemm.hpp with its EPI = 2 epilogue.
 * MLDHIP_PREC_F32: exact fp32 MFMAs; MLDHIP_PREC_F16X3: split-f16 products (pre-split weight image) unless finalize's probe moved the towers to fp32 ("Range
 * contract", eval_split_ok).  More than 256 motions are processed in chunks of 256 (workspace bound; the numbers do not depend on it).
 *
 * Both calls are stream-ordered and issued eagerly (no hipGraph), lengths reach the kernels through an engine-owned table uploaded with the call, non-finite
 * outputs go into the sticky counter.  MLDHIP_EINVAL: B outside 1 .. t2m_max_motions, T > max_frames, a length < 4 (m_len 0: PyTorch refuses an empty packed
 * sequence) or > T, a text length outside 1 .. L, L > t2m_max_words, null pointers, renorm outside {0, 1}.  MLDHIP_ESTATE: no evaluators on the handle, the
 * group (renorm = 1: or mean / std) not loaded, the handle not finalized. */
int mldhip_t2m_motion_embed(mldhip_handle* h, const float* feats_dev /*[B,T,nfeats]*/, const int32_t* lengths_host, int32_t B, int32_t T,
                            int32_t renorm /* 1: renorm4t2m first (needs mean/std); 0: already in evaluator normalisation (eval_gt's switch) */,
                            float* emb_out_dev /*[B,512]*/, void* stream);
int mldhip_t2m_text_embed(mldhip_handle* h, const float* word_embs_dev /*[B,L,300]*/, const float* pos_ohot_dev /*[B,L,15]*/,
                          const int32_t* text_lengths_host, int32_t B, int32_t L, float* emb_out_dev /*[B,512]*/, void* stream);

/* The SMPL body model (handles created with smpl_verts = V > 0).  Replaces: Rotation2xyz (mld/transforms/rotation2xyz.py:10-114) over smplx.SMPLLayer as the two
 * lambdas of MLD.__init__ call it on the action path (mld/models/modeltype/mld.py:118-143: feats2joints_eval with jointstype 'smpl', feats2joints with
 * jointstype 'vertices').  A restatement of the published SMPL / linear-blend-skinning algorithm.
 *
 * WEIGHTS.  One more optional all-or-nothing group, float32 (a wrong shape is MLDHIP_EINVAL, mldhip_missing_keys reports a half-loaded group; with
 * smpl_verts = 0 every smpl.* key stays accepted and ignored, mis-shaped ones included):
 *   smpl.v_template [V][3];  smpl.posedirs [207][3V], column 3 v + c (smplx's buffer: the file's [V][3][207] reshaped to [3V][207] and transposed);
 *   smpl.J_regressor [24][V];  smpl.lbs_weights [V][24] (dense: rows need not be sparse);  smpl.parents [24], integers stored as float32, parents[0] = -1.
 * Finalize refuses a parents[i] that is not an integer in [0, i) for i >= 1.  The SHAPE IS FIXED: v_shaped = v_template (the reference always passes betas = 0:
 * rotation2xyz.py:74-79, beta = 0 at both call sites); a caller who wants a body shape adds shapedirs . betas to v_template on the host, which is exact because the
 * joints are regressed from v_shaped.  The rest joints J = J_regressor v_template [24][3] are computed once at finalize.
 *
 * FEATURES (sample.view(..., 6, 25).permute(0, 3, 2, 1), mld.py:121,133).  Feature c 25 + j is component c (0 .. 5) of slot j; slots 0 .. 23 are the rot6d of the
 * global orientation and the 23 body joints; slot 24, components 0 .. 2, is the translation.  Features are used as they are: no mean / std.
 * rot6d -> matrix (pytorch3d's rotation_6d_to_matrix), a1 = components 0 .. 2, a2 = components 3 .. 5:
 *   b1 = a1 / max(|a1|, 1e-12);  u = a2 - (b1 . a2) b1;  b2 = u / max(|u|, 1e-12);  b3 = b1 x b2;  R has ROWS b1, b2, b3.
 * CHAIN AND SKINNING.  G_0 = [R_0 | J_0];  G_i = G_parent(i) . [R_i | J_i - J_parent(i)];  posed joint i = the translation of G_i;  A_i = [G_i.R | G_i.t - G_i.R J_i];
 *   pose feature pf = flatten(R_1 - I, ..., R_23 - I) in joint, row, column order (207 values);  vp[v] = v_template[v] + sum_k pf[k] posedirs[k][3 v + c];
 *   vert[v] = sum_j W[v][j] (A_j.R vp[v] + A_j.t).
 *
 * OUTPUTS AND THE PADDED-FRAME RULE.  trans[b][t] = slot 24 of frame t, read as it is, also from padded frames.
 *   joints [B][T][24][3]: a valid frame (t < len) holds joint_j - joint_0, a padded frame 0; with MLDHIP_SMPL_TRANS_JOINTS (the reference's vertstrans = True)
 *     trans[b][t] - trans[b][0] is added to EVERY frame, padded ones included -- what rotation2xyz.py:94-109 does: the mask is applied before the translation, so
 *     zero-padded features give -trans[b][0] on padded frames;
 *   vertices [B][T][V][3]: a valid frame holds vert (not root-centred), a padded frame 0; with MLDHIP_SMPL_TRANS_VERTS the same term is added to every frame (the
 *     model's own call sites leave this off).
 * Not served (mld_hip.smpl.HipSmpl.rot2xyz raises, naming each): the vertex-regressed joint sets 'a2m' / 'a2mpl' / 'vibe' (no call site in mld.py; they need
 * J_regressor_extra.npy and smplx's vertex-id table), pose_rep other than 'rot6d', glob = False, betas.
 *
 * KERNELS (kernels/smpl.hpp).  The chain kernel: one lane per frame -- rot6d -> R, the 24-joint chain, the joints output, pf (K padded to 208 with a zero) and A
 * (24 x 12 floats), laid out as the vertex kernel's matrix operands.  The vertex kernel (one launch: the [frames][3V] offsets never go to memory): 16 frames x 16
 * vertices per MFMA tile; three accumulators take pf . posedirs (posedirs re-laid coordinate-planar per 16-vertex block at finalize), twelve more the blended matrix
 * sum_j W[v][j] A_j as a [16 x 24] x [24 x 16] product per entry -- all fifteen in one lane layout, so the skinning of a (frame, vertex) is 12 FMAs in registers --
 * then the store; a workgroup stages the pf / A tiles of 32 frames in LDS once and walks the vertex blocks.
 * ARITHMETIC: exact-fp32 MFMAs (v_mfma_f32_16x16x4_f32) and fp32 VALU in EVERY precision mode -- no stage of the range contract; an MLDHIP_PREC_F16X3 handle gives
 * the same bits as an MLDHIP_PREC_F32 one.  Reasoning (an ESTIMATE, see profiles/smpl_ab.json for what was measured): 8.6 MFLOP of blend products and 83 KB of
 * output per frame, i.e. 33 GFLOP for HumanAct12's 64 x 60 frames = 0.2 ms at the fp32 matrix peak against a reverse loop of about 7 ms; and posedirs lives at
 * 1e-3 .. 1e-2, where the low half of a split-f16 image is a half subnormal (see the range contract above).
 *
 * The call is stream-ordered and issued eagerly (no hipGraph); lengths reach the kernels through an engine-owned table uploaded with the call; non-finite output
 * values are counted into the sticky counter of mldhip_numeric_status WHILE they are stored (no separate pass over the vertices).  verts_out_dev == NULL runs the
 * chain kernel only; its joints are bit-identical to those of a call that also asks for vertices.  More than 4 096 frames are processed in chunks (workspace
 * bound); a frame's numbers do not depend on the chunk, the tile or the batch it is in.
 * MLDHIP_EINVAL: B outside 1 .. max_batch, T outside 1 .. max_frames, a length outside 1 .. T, both outputs NULL, unknown flag bits, a null input.
 * MLDHIP_ESTATE: no body model on the handle, the group not loaded, the handle not finalized. */
enum { MLDHIP_SMPL_TRANS_JOINTS = 1, MLDHIP_SMPL_TRANS_VERTS = 2 };
int mldhip_smpl_forward(mldhip_handle* h, const float* feats_dev /*[B,T,150]*/, const int32_t* lengths_host, int32_t B, int32_t T,
                        int32_t flags, float* joints_out_dev /*[B,T,24,3] or NULL*/, float* verts_out_dev /*[B,T,V,3] or NULL*/, void* stream);

/* The HumanAct12 action-recognition GRU (handles created with a2m_rec = 1).  Replaces: MotionDiscriminator / MotionDiscriminatorForFID
 * (mld/models/architectures/humanact12_gru.py) with input_size 72, hidden_size 128, hidden_layer 2, output_size 12, as HUMANACTMetrics (mld/models/metrics/gru.py)
 * runs them on the joints of mldhip_smpl_forward.
 *
 * WEIGHTS.  One more optional all-or-nothing group, float32, under the names of humanact12_gru.tar's "model" prefixed a2m_rec. (a wrong shape is
 * MLDHIP_EINVAL, mldhip_missing_keys reports a half-loaded group; with a2m_rec = 0 every a2m_rec.* key is accepted and ignored):
 *   a2m_rec.recurrent.weight_ih_l0 [384][72];  a2m_rec.recurrent.weight_hh_l0, weight_ih_l1, weight_hh_l1 [384][128];
 *   a2m_rec.recurrent.bias_ih_l0, bias_hh_l0, bias_ih_l1, bias_hh_l1 [384];  a2m_rec.linear1.weight [30][128], .bias [30];  a2m_rec.linear2.weight [12][30], .bias [12].
 *
 * INPUT.  joints [B][T][72]: mldhip_smpl_forward's joints [B][T][24][3] as they are; feature 3 joint + coord (the reference's [B, 24, 3, T] reshaped to
 * [B, 72, T] and permuted to [T, B, 72]).
 * MATH.  A 2-layer unidirectional GRU over steps t = 0 .. len - 1 of each motion, PyTorch's cell, gate rows r | z | n of each [384] weight:
 *   r = sigmoid(W_ir x + b_ir + W_hr h + b_hr);  z = sigmoid(W_iz x + b_iz + W_hz h + b_hz);  n = tanh(W_in x + b_in + r (W_hn h + b_hn));  h' = (1 - z) n + z h;
 *   layer 1's x is layer 0's h' of the same step.  out = layer 1's state after step len - 1;  act = tanh(linear1(out)) [30];  logits = linear2(act) [12].
 * THE PADDED-FRAME RULE.  The GRU is causal and the reference reads its output at step len - 1, so frames t >= len never affect the outputs: they are never
 *   read (NaN there gives the same bits), and a motion's outputs are bit-identical alone, inside any batch and for any T >= len.
 * THE h0 CONTRACT.  h0_dev [2][B][128] is the initial state of layer 0 ([0][b]) and layer 1 ([1][b]); NULL means zeros.  The reference draws
 *   h0 = torch.randn(2, B, 128) on the CPU default generator at EVERY forward call (initHidden); the caller draws it the same way and passes it (HUMANACTMetrics
 *   .update makes four draws -- classifier on the generated motions, on the ground truth, then the FID net on each -- mld_hip.metrics.HipHUMANACTMetrics stacks
 *   them along B and makes one call of 4B motions).  Logits and activations of a call row come from the same h0 row.
 *
 * KERNEL (kernels/a2m_gru.hpp): ONE launch; a workgroup per tile of 16 motions runs both layers over the tile's steps (layer 1 one step behind layer 0, one
 * barrier per step, both states in LDS), each motion stopping at its own length, then the head on the tile's final states.  ARITHMETIC: exact-fp32 MFMAs
 * (v_mfma_f32_16x16x4_f32) for the recurrence and fp32 VALU for the head in EVERY precision mode -- no stage of the range contract; an MLDHIP_PREC_F16X3
 * handle gives the same bits as an MLDHIP_PREC_F32 one.  Reasoning: the work is tiny and latency-bound, and the predicted classes are argmaxes.
 * The call is stream-ordered and issued eagerly (no hipGraph); lengths reach the kernel through an engine-owned table uploaded with the call; non-finite
 * output values are counted into the sticky counter of mldhip_numeric_status.
 * MLDHIP_EINVAL: B outside 1 .. a2m_max_motions, T outside 1 .. max_frames, a length outside 1 .. T, both outputs NULL, a null input.
 * MLDHIP_ESTATE: no recognizer on the handle, the group not loaded, the handle not finalized. */
int mldhip_a2m_recognize(mldhip_handle* h, const float* joints_dev /*[B,T,72]*/, const int32_t* lengths_host, const float* h0_dev /*[2,B,128] or NULL = zeros*/,
                         int32_t B, int32_t T, float* logits_out_dev /*[B,12] or NULL*/, float* act_out_dev /*[B,30] or NULL*/, void* stream);

/* The UESTC recognition ST-GCN (handles created with uestc_rec = 1).  Replaces: STGCN(in_channels 6, num_class NC, layout 'smpl', strategy 'spatial',
 * edge_importance_weighting) of mld/models/architectures/uestc_stgcn.py in eval mode, as UESTCMetrics (mld/models/metrics/stgcn.py) runs it.
 *
 * WEIGHTS.  One more optional all-or-nothing group of 149 float32 tensors under the names of uestc_rot6d_stgcn.tar's state dict prefixed uestc_rec. (a wrong shape is
 * MLDHIP_EINVAL, mldhip_missing_keys reports a half-loaded group; with uestc_rec = 0 every uestc_rec.* key is accepted and ignored; num_batches_tracked is not a tensor
 * of the group):
 *   uestc_rec.A [3][24][24] (the checkpoint's registered buffer: no kinematic tree is read at run time);  uestc_rec.data_bn.{weight, bias, running_mean, running_var} [144];
 *   per block i = 0 .. 9, (Cin -> Cout, stride) = 6 -> 64, 1; 64 -> 64, 1 (x3); 64 -> 128, 2; 128 -> 128, 1 (x2); 128 -> 256, 2; 256 -> 256, 1 (x2):
 *     uestc_rec.st_gcn_networks.i.gcn.conv.{weight [3 Cout][Cin][1][1], bias [3 Cout]};  .tcn.0.* and .tcn.3.* (BatchNorm: weight, bias, running_mean, running_var [Cout]);
 *     .tcn.2.{weight [Cout][Cout][9][1], bias [Cout]};  for i = 4, 7 also .residual.0.{weight [Cout][Cin][1][1], bias} and .residual.1.* (BatchNorm);
 *   uestc_rec.edge_importance.i [3][24][24];  uestc_rec.fcn.{weight [NC][256][1][1], bias [NC]}.
 *
 * INPUT.  Element (n, v, c, t) -- motion, joint 0 .. 23, rot6d component 0 .. 5, frame -- is x_dev[n strides[0] + v strides[1] + c strides[2] + t strides[3]]
 * (elements, all four positive).  MLD's view of feature rows [B][T][150], m.view(B, T, 6, 25).permute(0, 3, 2, 1)[:, :-1], is strides (150 T, 1, 25, 150); a
 * contiguous [B][24][6][T] tensor is (144 T, 6 T, T, 1).  Neither needs a copy, and both give the same bits.
 * MATH (eval mode; BatchNorm = the affine of its running statistics, eps 1e-5; dropout = identity).  x <- data_bn over channel v 6 + c.  Then per block:
 *   y = conv1x1(x) [n][k][Cout][t][v], k = 0 .. 2;  g[n][c][t][w] = sum_k sum_v y[n][k][c][t][v] (A edge_importance[i])[k][v][w];
 *   h = BN(conv9x1(relu(BN(g)), stride s, padding 4));  out = relu(h + res), res = 0 (block 0), x (Cin = Cout, s = 1) or BN(conv1x1 stride s (x)) (blocks 4, 7);
 *   T_out = (T - 1) / 2 + 1 at each stride-2 block.  features [256] = the mean of the last block over all (t, v);  logits [NC] = fcn(features).
 * THERE ARE NO LENGTHS.  The reference has none (it leaves a "TODO: use mask"): all T frames of a motion, padded ones included, enter the convolutions and the
 * pool.  The engine reproduces that: a caller who wants the reference's numbers passes the padded batch as the reference does.
 * A motion's outputs do not depend on what else is in the call: bit-identical alone and in any batch (one tile shape, fixed summation orders).  NaN in one
 * motion stays in that motion.
 *
 * KERNELS (kernels/stgcn.hpp; engine/path_uestc.hpp has the folds and the launch order).  ARITHMETIC: MLDHIP_PREC_F32 handles multiply on exact-fp32 MFMAs;
 * MLDHIP_PREC_F16X3 handles run the GEMMs on split-f16 products while the graph mix, the pool and the head stay fp32 -- the sixth stage of the range contract
 * above (uestc_split_ok, probe_err_uestc).  Large B runs in chunks sized to the workspace (the numbers do not depend on it).  Stream-ordered, issued eagerly (no
 * hipGraph); non-finite output values are counted into the sticky counter of mldhip_numeric_status.
 * MLDHIP_EINVAL: a null input or strides, both outputs NULL, B outside 1 .. uestc_max_motions, T outside 1 .. max_frames, a stride < 1.
 * MLDHIP_ESTATE: no net on the handle, the group not loaded, the handle not finalized. */
int mldhip_uestc_recognize(mldhip_handle* h, const float* x_dev, const int64_t strides[4] /* n, v, c, t in elements */, int32_t B, int32_t T,
                           float* logits_out_dev /*[B,NC] or NULL*/, float* feat_out_dev /*[B,256] or NULL*/, void* stream);

/* The text-to-motion metric kernels (handles created with t2m_metrics = 1): the device-shaped parts of TM2TMetrics (mld/models/metrics/tm2t.py) and MMMetrics
 * (mm.py) -- grouped retrieval, activation statistics, pair distances -- on embeddings that stay on the device.  The matrix square root of the FID and
 * the random draws stay with the caller (mld_hip.metrics.HipTM2TMetrics / HipMMMetrics).
 *
 * COMMON RULES.  1 <= D <= 1024; rows are dense (row stride D).  Stream-ordered, issued eagerly (no hipGraph).  ARITHMETIC: exact fp32 in EVERY precision mode
 * (v_mfma_f32_16x16x4_f32 for the products, fp32 VALU elsewhere; no stage of the range contract): an MLDHIP_PREC_F16X3 or MLDHIP_PREC_BF16 handle gives the
 * bits of an MLDHIP_PREC_F32 one -- ranks are discrete and the FID goes through a matrix square root.  Summation order is fixed and there are no atomics:
 * results are bit-identical from call to call and do not depend on metrics_max_rows, on the grid or on what else runs.
 * MLDHIP_EINVAL: a null required pointer, a size out of range, N > metrics_max_rows, P outside 1 .. metrics_max_rows, an index outside 0 .. N - 1 (checked on
 * the host before anything is launched), both outputs NULL in mldhip_t2m_match.  MLDHIP_ESTATE: the handle was created with t2m_metrics = 0.
 *
 * mldhip_t2m_match.  Replaces one pass of the group loop of TM2TMetrics.compute (tm2t.py:100-113, :122-134: euclidean_distance_matrix, .nan_to_num(), .trace(),
 * argsort, calculate_top_k).  1 <= R <= 32, G = N / R (integer division; the last N - G R rows are ignored and their outputs left untouched, as in the
 * reference).  For group g and rows i, j of it:  d[i][j] = sqrt((-2 t_i.m_j + |t_i|^2) + |m_j|^2)  (the reference's expansion, in its order); a negative or NaN
 * argument of the root gives 0 (what nan_to_num makes of it), +inf becomes FLT_MAX.  diag[g R + i] = d[i][i];  rank[g R + i] = #{j : d[i][j] < d[i][i]} +
 * #{j < i : d[i][j] == d[i][i]}, the position a stable ascending sort gives column i.  The caller derives the top-k hit as rank < k and the matching score
 * as the sum of diag.  KERNEL (kernels/t2m_metrics.hpp): one workgroup per group; the group is one 32 x 32 accumulator tile (four 16 x 16 MFMA tiles, one
 * per wave), rows behind R and columns behind D are zeros (K is padded to the instruction's 4).
 *
 * mldhip_act_stats.  Replaces calculate_activation_statistics_np (np.mean(axis=0), np.cov(rowvar=False)).  N >= 2.  mean[d] = column mean;
 * cov = (X - mean)^T (X - mean) / (N - 1): rows are centred BEFORE they are multiplied (two passes; no E[xx] - E[x]E[x] form).  The row sum is two-level:
 * chunks of MLDHIP_ACT_STATS_CHUNK rows (the last one shorter), each summed from zero, the chunk sums added in ascending order.  cov is exactly symmetric:
 * only elements i <= j are computed, each is stored to [i][j] and [j][i].
 *
 * mldhip_pair_dist.  Replaces the distance part of calculate_diversity_np / calculate_multimodality_np: dist[p] = sqrt(sum_d (x[a[p]][d] - x[b[p]][d])^2), the
 * difference form (a == b gives exactly 0).  One wave per pair.  The index tables reach the kernel through an engine-owned table uploaded with the call. */
#define MLDHIP_ACT_STATS_CHUNK 256
int mldhip_t2m_match(mldhip_handle* h, const float* text_dev /*[N][D]*/, const float* motion_dev /*[N][D]*/, int32_t N, int32_t D, int32_t R,
                     int32_t* rank_out_dev /*[G*R] or NULL*/, float* diag_out_dev /*[G*R] or NULL*/, void* stream);
int mldhip_act_stats(mldhip_handle* h, const float* x_dev /*[N][D]*/, int32_t N, int32_t D, float* mean_out_dev /*[D]*/, float* cov_out_dev /*[D][D]*/,
                     void* stream);
int mldhip_pair_dist(mldhip_handle* h, const float* x_dev /*[N][D]*/, int32_t N, int32_t D, const int32_t* a_host /*[P]*/, const int32_t* b_host /*[P]*/,
                     int32_t P, float* dist_out_dev /*[P]*/, void* stream);

/* Replaces: HumanML3DDataModule.feats2joints (mld/data/HumanML3D.py:41-45 -> recover_from_ric,
 * mld/data/humanml/scripts/motion_process.py:415-432).  feats [B,T,nfeats] -> joints [B,T,njoints,3]. */
int mldhip_feats2joints(mldhip_handle* h, const float* feats_dev, int32_t B, int32_t T,
                        float* joints_out_dev, void* stream);

/* Scheduler introspection (DDIMScheduler.timesteps / alphas_cumprod): copies min(n, available). */
int mldhip_get_timesteps(mldhip_handle* h, int32_t* out_host, int32_t n);
int mldhip_get_alphas_cumprod(mldhip_handle* h, float* out_host, int32_t n);

/* (The measurement hooks of rounds 1-4 -- mldhip_profile_kernel, mldhip_profile_trace, option "fused_dbg" -- are not part of this library any more:
 * include/mldhip_hooks.h, built into libmldhip_hooks.so by `make hooks`.) */

/* Per-phase kernel launch counts of the last sample() (denoise loop, decode, joints). */
int mldhip_get_launch_counts(mldhip_handle* h, int32_t* out_host /*[3]*/);

const char* mldhip_last_error(mldhip_handle* h /* may be NULL */);
int mldhip_abi_version(void);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* MLDHIP_H_ */
