"""``MLD`` -- the orchestrator of the sampling path with the reference's call surface
(mld/models/modeltype/mld.py:33-143 construct, :216-265 forward, :267-275 gen_from_latent,
:290-360 _diffusion_reverse, :362-424 _diffusion_reverse_tsne), minus Lightning/training/metrics (out of scope).

Two execution paths, same results:
  fused   -- every network part is a Hip* drop-in: ONE ``mldhip_sample`` call (hipGraph replay of the
             50-step loop + decode + joints); this is what bench.py measures.
  modular -- the reference's own Python loop over ``denoiser`` / ``scheduler.step`` / ``vae.decode``; used
             when a part was swapped for something else, and by the parity tests of the per-op entry points.
"""
from __future__ import annotations

import inspect
from collections import OrderedDict
from typing import List, Optional

import torch
from torch import nn

from . import engine as _engine
from .config import instantiate_from_config
from .denoiser import HipMldDenoiser
from .scheduler import HipDDIMScheduler, HipDDPMScheduler
from .vae import HipActorVae, HipMldVae


def remove_padding(tensors, lengths):
    """mld/utils/temos_utils.py:24-28."""
    return [t[:n] for t, n in zip(tensors, lengths)]


class MLD(nn.Module):
    def __init__(self, cfg, datamodule, text_encoder: Optional[nn.Module] = None, engine_key: Optional[str] = None, **kwargs):
        super().__init__()
        self.cfg = cfg
        self.stage = cfg.TRAIN.get("STAGE", "diffusion")
        self.condition = cfg.model.condition
        self.nfeats = cfg.DATASET.NFEATS
        self.njoints = cfg.DATASET.NJOINTS
        self.latent_dim = cfg.model.latent_dim
        self.guidance_scale = cfg.model.guidance_scale
        self.datamodule = datamodule
        try:                                                                     # mld.py:50-54
            self.vae_type = cfg.model.vae_type
        except (KeyError, AttributeError):
            self.vae_type = cfg.model.motion_vae.target.split(".")[-1].lower().replace("hip", "").replace("vae", "")
        if self.condition not in ("text", "text_uncond", "action") or self.stage not in ("diffusion", "vae_diffusion"):
            raise NotImplementedError(f"mld_hip.MLD covers text-/action-to-motion sampling (condition={self.condition!r}, stage={self.stage!r})")
        self._engine_key = engine_key
        # engine registry variant ("text_uncond" is the text network fed with empty prompts on both CFG halves, mld.py:228-229)
        self.variant = "novae" if self.vae_type == "no" else ("action" if self.condition == "action" else "text")
        if hasattr(datamodule, "variant") and datamodule.variant is None:
            datamodule.variant = self.variant
        # the reference builds CLIP for every condition (mld.py:60); the action path never calls it, so it is skipped there
        self.text_encoder = text_encoder if (text_encoder is not None or self.condition == "action") \
            else instantiate_from_config(cfg.model.text_encoder)
        self.vae = instantiate_from_config(cfg.model.motion_vae) if self.vae_type != "no" else None      # mld.py:58-59
        self.denoiser = instantiate_from_config(cfg.model.denoiser)
        self.scheduler = instantiate_from_config(cfg.model.scheduler)
        # the T2M evaluator nets (mld.py:110-140) are opt-in: cfg.model.t2m_evaluator.target = mld_hip.evaluators.HipT2MEvaluator; without it t2m_* keys are dropped
        ev = cfg.model.get("t2m_evaluator") if hasattr(cfg.model, "get") else None
        self.t2m_evaluator = instantiate_from_config(ev) if ev and ev.get("target") else None
        # the SMPL body model (mld.py:118-143: Rotation2xyz) is opt-in too: cfg.model.smpl.target = mld_hip.smpl.HipSmpl, on action models
        sm = cfg.model.get("smpl") if hasattr(cfg.model, "get") else None
        self.smpl = instantiate_from_config(sm) if sm and sm.get("target") and self.condition == "action" else None
        # the metric kernels (grouped retrieval, activation statistics, pair distances behind mld_hip.metrics.HipTM2TMetrics / HipMMMetrics) are opt-in as well:
        # cfg.model.metric_ops.target = mld_hip.evaluators.HipMetricOps; the module has no weights and shares this model's handle
        mo = cfg.model.get("metric_ops") if hasattr(cfg.model, "get") else None
        self.metric_ops = instantiate_from_config(mo) if mo and mo.get("target") else None
        for m in (self.vae, self.denoiser, self.text_encoder, self.t2m_evaluator, self.smpl, self.metric_ops):
            if engine_key is not None and m is not None and hasattr(m, "use_engine"):
                m.use_engine(engine_key)
        # ONE engine for all parts of this model: every part asks the registry for the union of the architecture fields
        # (the fused sample() needs every weight group in one handle); another model with other fields gets its own engine
        shared = {}
        # (the datamodule first: its skeleton -- njoints, the feature width -- then the networks'; a HipMldTextEncoder adds the tower's fields: its weights live in the same handle)
        for m in (datamodule, self.denoiser, self.vae, self.text_encoder, self.t2m_evaluator, self.smpl, self.metric_ops):
            shared.update(getattr(m, "_arch", {}) or {})
        if hasattr(self.scheduler, "engine_config"):
            shared.update(self.scheduler.engine_config(cfg.model.scheduler.num_inference_timesteps))
        shared["guidance_scale"] = float(self.guidance_scale)
        # scheduler.eta (configs/modules/scheduler.yaml:4): stochastic DDIM in the engine (include/mldhip.h "Noise contract")
        try:
            self.eta = float(cfg.model.scheduler.eta)
        except (KeyError, AttributeError, TypeError):
            self.eta = 0.0
        if self.vae_type != "no":
            shared["eta"] = self.eta
        for m in (self.denoiser, self.vae, datamodule, self.scheduler, self.text_encoder, self.t2m_evaluator, self.smpl, self.metric_ops):
            if m is not None and hasattr(m, "_shared_arch") and engine_key is None:
                m._shared_arch = shared
        if self.metric_ops is not None:
            self.metric_ops._variant = self.variant
        if hasattr(self.text_encoder, "_shared_arch"):
            self.text_encoder._variant = self.variant
        if hasattr(self.scheduler, "_variant"):
            self.scheduler._variant = self.variant
        if self.t2m_evaluator is not None:
            self.t2m_evaluator._variant = self.variant
            if hasattr(datamodule, "mean_eval"):
                self.t2m_evaluator.stats_eval = (datamodule.mean_eval, datamodule.std_eval)
        self.sample_mean = False
        self.fact = None
        self.do_classifier_free_guidance = self.guidance_scale > 1.0
        self.feats2joints = datamodule.feats2joints
        if self.smpl is not None:                                               # mld.py:118-143
            self.smpl._variant = self.variant
            self.rot2xyz = self.smpl.rot2xyz
            self.feats2joints_eval = lambda sample, mask: self.rot2xyz(
                sample.view(*sample.shape[:-1], 6, 25).permute(0, 3, 2, 1), mask=mask, pose_rep='rot6d', glob=True, translation=True,
                jointstype='smpl', vertstrans=True, betas=None, beta=0, glob_rot=None, get_rotations_back=False)
            self.feats2joints = lambda sample, mask: self.rot2xyz(
                sample.view(*sample.shape[:-1], 6, 25).permute(0, 3, 2, 1), mask=mask, pose_rep='rot6d', glob=True, translation=True,
                jointstype='vertices', vertstrans=False, betas=None, beta=0, glob_rot=None, get_rotations_back=False)
        self.times: List[float] = []

    # ------------------------------------------------------------------ checkpoint contract (base.py:96-127)
    def load_state_dict(self, state_dict, strict: bool = True):
        te = self.text_encoder.state_dict() if self.text_encoder is not None else {}
        new = OrderedDict(("text_encoder." + k, v) for k, v in te.items())
        if self.smpl is not None:      # the body model is an asset of its own (SMPL_PATH), never part of a checkpoint: it keeps what it holds
            new.update(("smpl." + k, v) for k, v in self.smpl.state_dict().items())
        for k, v in state_dict.items():
            if k.startswith("rot2xyz.") or k.startswith("smpl."):
                continue
            if k.startswith("t2m_"):      # evaluator nets: loaded (strictly) when the model carries a HipT2MEvaluator, dropped otherwise -- they are not part of sampling
                if self.t2m_evaluator is not None:
                    new["t2m_evaluator." + k] = v
            elif "text_encoder" not in k:
                new[k] = v
        return super().load_state_dict(new, strict)

    # ------------------------------------------------------------------ helpers
    @property
    def fused(self) -> bool:
        if self.vae_type == "no":
            return (isinstance(self.denoiser, HipMldDenoiser) and isinstance(self.scheduler, HipDDPMScheduler)
                    and self.do_classifier_free_guidance)
        return (isinstance(self.denoiser, HipMldDenoiser) and isinstance(self.vae, (HipMldVae, HipActorVae))
                and isinstance(self.scheduler, HipDDIMScheduler) and self.do_classifier_free_guidance)

    def _engine(self):
        eng = self.denoiser.sync_weights()
        if self.vae is not None:
            self.vae.sync_weights()
        if self.t2m_evaluator is not None:
            self.t2m_evaluator.sync_weights()
        if self.smpl is not None:
            self.smpl.sync_weights()
        want = self.scheduler.engine_config(self.cfg.model.scheduler.num_inference_timesteps)
        for k in ("num_train_timesteps", "num_inference_steps", "steps_offset", "set_alpha_to_one"):
            if getattr(eng.cfg, k) != want[k]:
                raise RuntimeError(f"engine/scheduler mismatch on {k}: engine {getattr(eng.cfg, k)}, scheduler {want[k]}; "
                                   "create the engine with mld_hip.engine.configure(**scheduler.engine_config(n)) first")
        if abs(eng.cfg.guidance_scale - self.guidance_scale) > 1e-6:
            raise RuntimeError("engine guidance_scale differs from cfg.model.guidance_scale")
        if self.vae_type != "no" and abs(eng.cfg.eta - self.eta) > 1e-6:
            raise RuntimeError(f"engine/scheduler mismatch on eta: engine {eng.cfg.eta}, scheduler {self.eta}; "
                               "create the engine with mld_hip.engine.configure(eta=cfg.model.scheduler.eta) first")
        return eng

    def _noise_seed(self, seed: Optional[int]) -> Optional[int]:
        """The Philox seed of a fused stochastic-DDIM call (eta > 0): `seed`, or one drawn from torch's default CPU generator -- so
        torch.manual_seed makes a run reproducible, as it does for the reference.  None at eta = 0 (nothing is drawn, the generator is untouched)."""
        if self.eta == 0.0:
            return None
        return int(seed) if seed is not None else int(torch.randint(0, 2 ** 62, (1,)).item())

    # ------------------------------------------------------------------ fused path
    @torch.no_grad()
    def sample(self, text_emb: torch.Tensor, lengths: List[int], init_latents: Optional[torch.Tensor] = None, seed: Optional[int] = None,
               first_index: int = 0, return_trajectory: bool = False, src_latents: Optional[torch.Tensor] = None, first_step: int = 0,
               noised: bool = False, guidance_scale: Optional[float] = None):
        """text_emb [2B, 1, 768] (uncond half first) -> (joints [B,T,njoints,3], feats [B,T,nfeats], latents [B,1,D]) on device.
        src_latents [B, 1, D] (mldhip_sample_many_from): the loop starts at scheduler step `first_step` from the source noised with init_latents to
        that step's timestep (`noised` False), or from the source as it is (`noised` True: it already is the loop state there); trajectory rows
        below first_step are left as allocated.
        eta > 0: the step noise of motion m is the engine's Philox stream keyed (seed, first_index + m); `seed` None = drawn from torch's
        generator.  return_trajectory: a fourth result, the latents after every scheduler step [steps, B, D] (mldhip_sample_many_traj; its last
        row is `latents`).  guidance_scale: this call's classifier-free-guidance scale instead of cfg.model.guidance_scale (mldhip_sample_many_guided:
        eps_u + g (eps_c - eps_u) for any g >= 0); None = the model's own, on the call sites of a model without the keyword."""
        lengths = [int(x) for x in lengths]
        B, T = len(lengths), max(lengths)
        dev = text_emb.device
        text_emb = text_emb.float().contiguous()
        if init_latents is None:
            init_latents = torch.randn((B, self.latent_dim[0], self.latent_dim[-1]), device=dev, dtype=torch.float)   # mld.py:303
        init_latents = init_latents.float().contiguous()
        eng = self._engine()
        dm_eng = self.datamodule._engine(dev) if hasattr(self.datamodule, "_engine") else eng
        if dm_eng is not eng:
            raise RuntimeError("datamodule and network parts are bound to different engines")
        _engine.finalize_if_dirty(eng, _engine.current_stream_handle(text_emb))
        lat = torch.empty(B, self.latent_dim[0], self.latent_dim[-1], device=dev)
        feats = torch.empty(B, T, self.nfeats, device=dev)
        joints = torch.empty(B, T, self.njoints, 3, device=dev)
        seed = self._noise_seed(seed)
        if src_latents is not None or guidance_scale is not None:
            req = dict(text_emb=text_emb, init_latents=init_latents, lengths=lengths, latents_out=lat, feats_out=feats, joints_out=joints)
            if src_latents is not None:
                req.update(src_latents=src_latents.to(dev).float().contiguous(), first_step=int(first_step), noised=int(bool(noised)))
            if return_trajectory:
                req["traj_out"] = self._traj_buffer(eng, B, dev)
            keys = None if seed is None else [(seed, int(first_index))]
            if guidance_scale is not None:
                req["guidance"] = float(guidance_scale)
                eng.sample_many_guided([req], keys, _engine.current_stream_handle(text_emb))
            else:
                eng.sample_many_from([req], keys, _engine.current_stream_handle(text_emb))
            return (joints, feats, lat, req["traj_out"]) if return_trajectory else (joints, feats, lat)
        if return_trajectory:
            traj = self._traj_buffer(eng, B, dev)
            eng.sample_many_traj([dict(text_emb=text_emb, init_latents=init_latents, lengths=lengths, latents_out=lat, feats_out=feats,
                                       joints_out=joints, traj_out=traj)], None if seed is None else [(seed, int(first_index))],
                                 _engine.current_stream_handle(text_emb))
            return joints, feats, lat, traj
        if seed is None:
            eng.sample(text_emb, init_latents, lengths, lat, feats, joints, _engine.current_stream_handle(text_emb))
        else:
            eng.sample_many_seeded([dict(text_emb=text_emb, init_latents=init_latents, lengths=lengths, latents_out=lat, feats_out=feats,
                                         joints_out=joints)], [(seed, int(first_index))], _engine.current_stream_handle(text_emb))
        return joints, feats, lat

    @torch.no_grad()
    def sample_many(self, requests, init_latents=None, pipeline: bool = False, seed: Optional[int] = None, first_index: int = 0,
                    return_trajectory: bool = False, src_latents=None, first_step=None, noised=None, guidance=None):
        """Several independent text-to-motion requests as ONE engine call (``mldhip_sample_many``: one reverse-diffusion chain +
        one decode over all of them; the engine needs ``max_batch >= total motions``).  `requests` = [(text_emb [2B_i,1,768],
        lengths_i), ...]; returns [(joints_i, feats_i, latents_i), ...] on device, each shaped as ``sample`` would return it.

        ``pipeline=True`` (engine option "many_pipeline"; ``mld_hip.engine.configure("text", max_in_flight=2)`` before the first use): the
        requests run ONE AFTER THE OTHER -- the reference's own loop, batch after batch (mld.py:618-672) -- each exactly what ``sample`` returns
        for it, with the decode of request k overlapped with the reverse loop of request k + 1 (bs-64 requests: 7.0 instead of 8.0 ms each).

        ``return_trajectory=True``: every result tuple gets a fourth entry, the request's latents after every scheduler step [steps, B_i, D]
        (mldhip_sample_many_traj; such a call runs as one chain, also with ``pipeline=True``).

        ``src_latents`` / ``first_step`` / ``noised``: one entry per request (a tensor [B_i, 1, D] or None; an int; a bool) -- where each request
        enters the reverse loop (mldhip_sample_many_from, see ``sample``); such a call runs as one chain as well.

        ``guidance``: one entry per request, a float >= 0 or None (the model's own scale) -- requests with different classifier-free-guidance scales
        in one chain on one engine (mldhip_sample_many_guided).  None: the call sites above, unchanged."""
        if self.vae_type == "no" or self.condition == "action":
            raise NotImplementedError("sample_many serves the text-to-motion latent model")
        eng = self._engine()
        dev = requests[0][0].device
        dm_eng = self.datamodule._engine(dev) if hasattr(self.datamodule, "_engine") else eng
        if dm_eng is not eng:
            raise RuntimeError("datamodule and network parts are bound to different engines")
        stream = _engine.current_stream_handle(requests[0][0])
        _engine.finalize_if_dirty(eng, stream)
        reqs, outs, keep = [], [], []
        for i, (text_emb, lengths) in enumerate(requests):
            lengths = [int(x) for x in lengths]
            B, T = len(lengths), max(lengths)
            text_emb = text_emb.float().contiguous()
            lat0 = init_latents[i] if init_latents is not None else torch.randn((B, self.latent_dim[0], self.latent_dim[-1]), device=dev)
            lat0 = lat0.float().contiguous()
            lat = torch.empty(B, self.latent_dim[0], self.latent_dim[-1], device=dev)
            feats = torch.empty(B, T, self.nfeats, device=dev)
            joints = torch.empty(B, T, self.njoints, 3, device=dev)
            keep.append((text_emb, lat0))
            reqs.append(dict(text_emb=text_emb, init_latents=lat0, lengths=lengths, latents_out=lat, feats_out=feats, joints_out=joints))
            if src_latents is not None and src_latents[i] is not None:
                reqs[-1].update(src_latents=src_latents[i].to(dev).float().contiguous(), first_step=int(first_step[i]) if first_step is not None else 0,
                                noised=int(bool(noised[i])) if noised is not None else 0)
            if guidance is not None and guidance[i] is not None:
                reqs[-1]["guidance"] = float(guidance[i])
            if return_trajectory:
                reqs[-1]["traj_out"] = self._traj_buffer(eng, B, dev)
                outs.append((joints, feats, lat, reqs[-1]["traj_out"]))
                continue
            outs.append((joints, feats, lat))
        if pipeline:
            eng.set_option("many_pipeline", 1)
        seed = self._noise_seed(seed)
        try:
            if any("guidance" in q for q in reqs):
                eng.sample_many_guided(reqs, None if seed is None else self._keys(seed, reqs, first_index), stream)
            elif any("src_latents" in q for q in reqs):
                eng.sample_many_from(reqs, None if seed is None else self._keys(seed, reqs, first_index), stream)
            elif return_trajectory:
                eng.sample_many_traj(reqs, None if seed is None else self._keys(seed, reqs, first_index), stream)
            elif seed is None:
                eng.sample_many(reqs, stream)
            else:       # motion k of request i is motion sum(B_<i) + k of the call: the same noise however the call is split
                eng.sample_many_seeded(reqs, self._keys(seed, reqs, first_index), stream)
        finally:
            if pipeline:
                eng.set_option("many_pipeline", 0)
        return outs

    def _traj_buffer(self, eng, B: int, dev) -> torch.Tensor:
        """[steps, B, latent_size * D]: what mldhip_sample_many_traj fills for a request of B motions (the shape the reference's torch.cat gives)"""
        return torch.empty(int(eng.cfg.num_inference_steps), B, self.latent_dim[0] * self.latent_dim[-1], device=dev, dtype=torch.float)

    @staticmethod
    def _keys(seed: int, reqs, first_index: int = 0):
        out, o = [], int(first_index)
        for q in reqs:
            out.append((seed, o))
            o += len(q["lengths"])
        return out

    @torch.no_grad()
    def sample_novae(self, text_emb: torch.Tensor, lengths: List[int], init_latents: Optional[torch.Tensor] = None,
                     step_noise: Optional[torch.Tensor] = None, seed: Optional[int] = None):
        """Diffusion-only sampling in ONE mldhip_sample_novae call: text_emb [2B, 1, 768] -> (joints [B,T,njoints,3], feats [B,T,nfeats]).
        step_noise [steps, B, T, nfeats] injects the scheduler's per-step draws (parity runs); otherwise they come from the
        engine's Philox stream keyed by `seed` (default: drawn from torch's generator, so torch.manual_seed governs it)."""
        lengths = [int(x) for x in lengths]
        B, T = len(lengths), max(lengths)
        dev = text_emb.device
        text_emb = text_emb.float().contiguous()
        if init_latents is None:
            init_latents = torch.randn((B, T, self.nfeats), device=dev, dtype=torch.float)            # mld.py:296-301
        init_latents = init_latents.float().contiguous()
        if step_noise is not None:
            step_noise = step_noise.float().contiguous()
            if tuple(step_noise.shape) != (self.cfg.model.scheduler.num_inference_timesteps, B, T, self.nfeats):
                raise ValueError(f"step_noise must be [steps, B, T, nfeats], got {tuple(step_noise.shape)}")
        elif seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        eng = self._engine()
        if hasattr(self.datamodule, "_engine") and self.datamodule._engine(dev) is not eng:
            raise RuntimeError("datamodule and denoiser are bound to different engines")
        _engine.finalize_if_dirty(eng, _engine.current_stream_handle(text_emb))
        feats = torch.empty(B, T, self.nfeats, device=dev)
        joints = torch.empty(B, T, self.njoints, 3, device=dev)
        eng.sample_novae(text_emb, init_latents, lengths, step_noise, seed or 0, feats, joints, _engine.current_stream_handle(text_emb))
        return joints, feats

    @torch.no_grad()
    def sample_action(self, actions, lengths: List[int], init_latents: Optional[torch.Tensor] = None, device=None, seed: Optional[int] = None,
                      first_index: int = 0, return_trajectory: bool = False, guidance_scale: Optional[float] = None):
        """Action labels [B] / [B, 1] -> (feats [B, T, nfeats], latents [B, 1, D]) on device: ONE mldhip_sample_action call.
        return_trajectory: a third result, the latents after every scheduler step [steps, B, D] (mldhip_sample_many_traj).
        guidance_scale: this call's classifier-free-guidance scale (mldhip_sample_many_guided); None = the model's own."""
        lengths = [int(x) for x in lengths]
        acts = [int(a) for a in (actions.reshape(-1).tolist() if torch.is_tensor(actions) else list(actions))]
        B, T = len(lengths), max(lengths)
        dev = init_latents.device if init_latents is not None else (device or next(self.denoiser.parameters()).device)
        if init_latents is None:
            init_latents = torch.randn((B, self.latent_dim[0], self.latent_dim[-1]), device=dev, dtype=torch.float)   # mld.py:303
        init_latents = init_latents.float().contiguous()
        eng = self._engine()
        lat = torch.empty(B, self.latent_dim[0], self.latent_dim[-1], device=dev)
        feats = torch.empty(B, T, self.nfeats, device=dev)
        seed = self._noise_seed(seed)
        if guidance_scale is not None:
            req = dict(actions=acts, init_latents=init_latents, lengths=lengths, latents_out=lat, feats_out=feats, guidance=float(guidance_scale))
            if return_trajectory:
                req["traj_out"] = self._traj_buffer(eng, B, dev)
            eng.sample_many_guided([req], None if seed is None else [(seed, int(first_index))], _engine.current_stream_handle(init_latents))
            return (feats, lat, req["traj_out"]) if return_trajectory else (feats, lat)
        if return_trajectory:
            traj = self._traj_buffer(eng, B, dev)
            eng.sample_many_traj([dict(actions=acts, init_latents=init_latents, lengths=lengths, latents_out=lat, feats_out=feats, traj_out=traj)],
                                 None if seed is None else [(seed, int(first_index))], _engine.current_stream_handle(init_latents))
            return feats, lat, traj
        if seed is None:
            eng.sample_action(acts, init_latents, lengths, lat, feats, _engine.current_stream_handle(init_latents))
        else:
            eng.sample_many_seeded([dict(actions=acts, init_latents=init_latents, lengths=lengths, latents_out=lat, feats_out=feats)], [(seed, int(first_index))],
                                   _engine.current_stream_handle(init_latents))
        return feats, lat

    @torch.no_grad()
    def sample_many_action(self, requests, init_latents=None, device=None, seed: Optional[int] = None, first_index: int = 0, guidance=None):
        """Several action-to-motion requests as ONE engine call (``mldhip_sample_many`` with ``actions_host``): `requests` =
        [(actions_i, lengths_i), ...] -> [(feats_i [B_i, T_i, nfeats], latents_i), ...] on device; the engine needs
        ``max_batch >= total motions`` (four bs-256 requests per call: 30.0 k motions/s against 5.9 k one call at a time, bench.py).
        ``guidance``: one classifier-free-guidance scale per request or None, as for ``sample_many``."""
        if self.condition != "action":
            raise NotImplementedError("sample_many_action serves the action-conditioned model")
        eng = self._engine()
        dev = device or (init_latents[0].device if init_latents is not None else next(self.denoiser.parameters()).device)
        _engine.finalize_if_dirty(eng)
        reqs, outs, keep = [], [], []
        for i, (actions, lengths) in enumerate(requests):
            lengths = [int(x) for x in lengths]
            acts = [int(a) for a in (actions.reshape(-1).tolist() if torch.is_tensor(actions) else list(actions))]
            B, T = len(lengths), max(lengths)
            lat0 = init_latents[i] if init_latents is not None else torch.randn((B, self.latent_dim[0], self.latent_dim[-1]), device=dev)
            lat0 = lat0.to(dev).float().contiguous()
            lat = torch.empty(B, self.latent_dim[0], self.latent_dim[-1], device=dev)
            feats = torch.empty(B, T, self.nfeats, device=dev)
            keep.append(lat0)
            reqs.append(dict(actions=acts, init_latents=lat0, lengths=lengths, latents_out=lat, feats_out=feats))
            if guidance is not None and guidance[i] is not None:
                reqs[-1]["guidance"] = float(guidance[i])
            outs.append((feats, lat))
        seed = self._noise_seed(seed)
        if any("guidance" in q for q in reqs):
            eng.sample_many_guided(reqs, None if seed is None else self._keys(seed, reqs, first_index), _engine.current_stream_handle(keep[0]))
        elif seed is None:
            eng.sample_many(reqs, _engine.current_stream_handle(keep[0]))
        else:
            eng.sample_many_seeded(reqs, self._keys(seed, reqs, first_index), _engine.current_stream_handle(keep[0]))
        return outs

    @torch.no_grad()
    def a2m_eval(self, batch, init_latents: Optional[torch.Tensor] = None, seed: Optional[int] = None, first_index: int = 0):
        """Sampling core of MLD.a2m_eval (mld.py:710-735): batch["action"] [B, 1] labels, batch["length"] -> rs_set with
        ``m_action`` / ``m_rst`` (features [B, T, nfeats]) / ``m_lens``.  The joints entries of the reference's rs_set go through the SMPL body model:
        with a ``HipSmpl`` on the model (cfg.model.smpl.target, opt-in) the set also holds ``joints_rst`` [B, V, 3, T] (vertices, no translation) and
        ``joints_eval_rst`` [B, 24, 3, T] (joints, translation), and -- when the batch carries ``"motion"`` -- ``m_ref`` / ``joints_ref`` / ``joints_eval_ref``
        (mld.py:735-750; the mask is batch["mask"], or the prefix mask of the lengths).  Without it they are not produced."""
        actions, lengths = batch["action"], list(batch["length"])
        if self.fused:
            noise_kw = {} if self.eta == 0.0 else {"seed": seed, "first_index": first_index}
            feats, _ = self.sample_action(actions, lengths, init_latents,
                                          device=actions.device if torch.is_tensor(actions) and actions.is_cuda else None, **noise_kw)
        else:
            a = actions if torch.is_tensor(actions) else torch.tensor(actions)
            cond = torch.cat((torch.zeros_like(a), a)) if self.do_classifier_free_guidance else a      # mld.py:716-717
            z = self._diffusion_reverse(cond.reshape(-1, 1), lengths, init_latents)
            feats = self.vae.decode(z.contiguous(), lengths)
        rs = {"m_action": actions, "m_rst": feats, "m_lens": lengths}
        if self.smpl is None:
            return rs
        mask = batch["mask"] if "mask" in batch else torch.arange(feats.shape[1])[None, :] < torch.tensor([int(n) for n in lengths])[:, None]
        rs["joints_rst"] = self.feats2joints(feats, mask)                       # mld.py:735-739
        rs["joints_eval_rst"] = self.feats2joints_eval(feats, mask)
        if "motion" in batch:
            motions = batch["motion"].detach().clone().float().to(feats.device)
            rs["m_ref"] = motions
            rs["joints_ref"] = self.feats2joints(motions, mask)
            rs["joints_eval_ref"] = self.feats2joints_eval(motions, mask)
        return rs

    @torch.no_grad()
    def t2m_eval(self, batch, init_latents: Optional[torch.Tensor] = None, seed: Optional[int] = None):
        """MLD.t2m_eval for the diffusion stages (mld.py:618-708): batch {"text", "motion" [B, T, nfeats], "length", "word_embs" [B, L, 300], "pos_ohot" [B, L, 15],
        "text_len"} -> rs_set {"m_ref", "m_rst", "lat_t", "lat_m", "lat_rm"} in the reference's align_idx order (lengths descending) and {"joints_ref", "joints_rst"} in
        the batch's order, as there.  Generated and ground-truth motions go through ONE mldhip_t2m_motion_embed call of 2B rows (two when their frame counts differ:
        an embedding depends on T).  Repeating prompts for the multimodality pass (MM_NUM_REPEATS) is the caller's loop."""
        if self.t2m_evaluator is None:
            raise RuntimeError("t2m_eval needs the evaluator nets: load_config(overrides={'model.t2m_evaluator.target': 'mld_hip.evaluators.HipT2MEvaluator'})")
        import numpy as np
        texts, lengths = list(batch["text"]), [int(x) for x in batch["length"]]
        motions = batch["motion"].detach().clone().float()
        B = len(lengths)
        if self.do_classifier_free_guidance:                                    # mld.py:643-649: uncond half first
            texts = [""] * len(texts) + ([""] * len(texts) if self.condition == "text_uncond" else texts)
        text_emb = self.text_encoder(texts)
        if self.fused and self.vae_type != "no":
            noise_kw = {} if self.eta == 0.0 else {"seed": seed}
            joints_rst, feats_rst, _ = self.sample(text_emb.to(motions.device), lengths, init_latents, **noise_kw)
        else:
            z = self._diffusion_reverse(text_emb, lengths, init_latents)
            feats_rst = self.vae.decode(z, lengths) if self.vae_type != "no" else z.permute(1, 0, 2).contiguous()
            joints_rst = self.feats2joints(feats_rst.detach())
        motions = motions.to(feats_rst.device)
        joints_ref = self.feats2joints(motions.contiguous())
        m_rst, m_ref = self.datamodule.renorm4t2m(feats_rst), self.datamodule.renorm4t2m(motions)      # mld.py:675-677
        align_idx = np.argsort(lengths)[::-1].copy()                            # mld.py:682
        idx = torch.from_numpy(align_idx).to(feats_rst.device)
        ev = self.t2m_evaluator
        if m_rst.shape[1] == m_ref.shape[1] and 2 * B <= ev.capacity(ev.engine):
            emb = ev.motion_embed(torch.cat([m_rst, m_ref]).contiguous(), lengths * 2, renorm=False)
            recons_emb, motion_emb = emb[:B], emb[B:]
        else:
            recons_emb, motion_emb = ev.motion_embed(m_rst.contiguous(), lengths, renorm=False), ev.motion_embed(m_ref.contiguous(), lengths, renorm=False)
        dev = feats_rst.device
        lat_t = ev.text_embed(batch["word_embs"].detach().float().to(dev), batch["pos_ohot"].detach().float().to(dev), [int(x) for x in batch["text_len"]])
        return {"m_ref": m_ref[idx], "m_rst": m_rst[idx], "lat_t": lat_t[idx], "lat_m": motion_emb[idx], "lat_rm": recons_emb[idx],
                "joints_ref": joints_ref, "joints_rst": joints_rst}

    # ------------------------------------------------------------------ reference surface
    @torch.no_grad()
    def forward(self, batch, init_latents: Optional[torch.Tensor] = None, step_noise: Optional[torch.Tensor] = None, seed: Optional[int] = None,
                first_index: int = 0, guidance_scale=None):
        """mld.py:216-265.  Stochastic DDIM (cfg.model.scheduler.eta > 0): the fused path draws the engine's Philox stream keyed (seed,
        first_index + m) -- `seed` None = drawn from torch's generator; the modular path draws torch.randn, or takes step_noise [steps, B, 1, D]
        (the fused path's draws reproduce it: include/mldhip.h "Noise contract").
        guidance_scale (None: batch["guidance_scale"] if the batch has one): a float for the whole batch or a sequence with one value per prompt
        (fused latent models; mldhip_sample_many_guided).  A sequence becomes ONE engine call of one request per maximal run of equal values; the
        noise keys follow the motions (``_keys``), so a motion's draws do not depend on how the batch is split."""
        texts, lengths = list(batch["text"]), list(batch["length"])
        if guidance_scale is None:
            guidance_scale = batch.get("guidance_scale") if hasattr(batch, "get") else None
        if self.do_classifier_free_guidance:                                    # mld.py:224-230: uncond half first
            texts = [""] * len(texts) + ([""] * len(texts) if self.condition == "text_uncond" else texts)
        text_emb = self.text_encoder(texts)
        if self.vae_type == "no":
            if self.fused:
                joints, _ = self.sample_novae(text_emb, lengths, init_latents, step_noise)
            else:
                z = self._diffusion_reverse(text_emb, lengths, init_latents, step_noise)
                joints = self.feats2joints(z.permute(1, 0, 2).contiguous())     # mld.py:241-242: "decode" is a permute
            return remove_padding(joints.detach().cpu(), lengths)
        if guidance_scale is not None and not self.fused:
            raise NotImplementedError("guidance_scale per call serves the fused latent models")
        if self.fused and guidance_scale is not None:
            joints = self._forward_guided(text_emb, lengths, init_latents, seed, first_index, guidance_scale)
        elif self.fused:
            noise_kw = {} if self.eta == 0.0 else {"seed": seed, "first_index": first_index}      # (eta = 0: the call of the deterministic path, unchanged)
            joints, _, _ = self.sample(text_emb, lengths, init_latents, **noise_kw)
        else:
            z = self._diffusion_reverse(text_emb, lengths, init_latents, step_noise)
            feats = self.vae.decode(z, lengths)
            joints = self.feats2joints(feats.detach())
        return remove_padding(joints.detach().cpu(), lengths)                   # mld.py:264-265

    def _forward_guided(self, text_emb, lengths, init_latents, seed, first_index, guidance_scale):
        """forward's fused call under a guidance scale of the call's own -> joints [B, Tmax, njoints, 3]: a float is one ``sample``; a per-prompt
        sequence one ``sample_many`` of one request per maximal run of equal values (motion order kept, so ``_keys`` gives every motion its own key)."""
        noise_kw = {} if self.eta == 0.0 else {"seed": seed, "first_index": first_index}
        if isinstance(guidance_scale, (int, float)) or (torch.is_tensor(guidance_scale) and guidance_scale.dim() == 0):
            return self.sample(text_emb, lengths, init_latents, guidance_scale=float(guidance_scale), **noise_kw)[0]
        gs = [float(g) for g in guidance_scale]
        B = len(lengths)
        if len(gs) != B:
            raise ValueError(f"guidance_scale has {len(gs)} entries for {B} prompts")
        runs, a = [], 0
        for m in range(1, B + 1):
            if m == B or gs[m] != gs[a]:
                runs.append((a, m))
                a = m
        reqs = [(torch.cat([text_emb[a:b], text_emb[B + a:B + b]]), lengths[a:b]) for a, b in runs]
        lat0 = None if init_latents is None else [init_latents[a:b] for a, b in runs]
        outs = self.sample_many(reqs, lat0, guidance=[gs[a] for a, _ in runs], **noise_kw)
        joints = outs[0][0].new_zeros(B, max(int(x) for x in lengths), self.njoints, 3)
        for (a, b), o in zip(runs, outs):
            joints[a:b, :o[0].shape[1]] = o[0]
        return joints

    @torch.no_grad()
    def gen_from_latent(self, batch):
        feats = self.vae.decode(batch["latent"], batch["length"])
        return remove_padding(self.feats2joints(feats.detach()).cpu(), batch["length"])

    @torch.no_grad()
    def recon_from_motion(self, batch):
        """mld.py:277-288: encode -> decode -> joints for the reconstruction and the reference motion."""
        feats_ref, length = batch["motion"], list(batch["length"])
        z, _ = self.vae.encode(feats_ref, length)
        feats_rst = self.vae.decode(z.contiguous(), length)
        joints = self.feats2joints(feats_rst.detach())
        joints_ref = self.feats2joints(feats_ref.detach().contiguous())
        return remove_padding(joints.cpu(), length), remove_padding(joints_ref.cpu(), length)

    @torch.no_grad()
    def edit(self, batch, strength: float, init_latents: Optional[torch.Tensor] = None, seed: Optional[int] = None, sample_mean: bool = True,
             guidance_scale: Optional[float] = None):
        """Motion-to-motion under a new prompt, as diffusers' image-to-image pipelines do it: batch {"motion" [B, T, nfeats], "text", "length"} ->
        joints per motion (as ``forward`` returns them).  The motion is encoded (``HipMldVae.encode``; the distribution's mean, or its sample with
        ``sample_mean=False``), noised to scheduler step ``first_step = n - min(int(n * strength), n)`` with ``init_latents`` (default: torch.randn) and
        denoised from there under batch["text"] in ONE mldhip_sample_many_from call: strength 1 runs every step, strength 0.3 the last 30 % of them,
        strength 0 (first_step == n) returns the reconstruction without a loop.  ``guidance_scale``: passed on to ``sample``."""
        if not self.fused or self.vae_type == "no" or self.condition == "action":
            raise NotImplementedError("edit serves the fused text-to-motion latent model")
        motion, texts, lengths = batch["motion"], list(batch["text"]), [int(x) for x in batch["length"]]
        z, dist = self.vae.encode(motion, lengths)
        src = (dist.loc if sample_mean else z).permute(1, 0, 2).contiguous()            # [B, latent_size, D]
        n = int(self.cfg.model.scheduler.num_inference_timesteps)
        first_step = n - min(int(n * float(strength)), n)
        if first_step == n:
            feats = self.vae.decode(src.permute(1, 0, 2).contiguous(), lengths)
            return remove_padding(self.feats2joints(feats.detach()).cpu(), lengths)
        if self.do_classifier_free_guidance:                                    # mld.py:224-230: uncond half first
            texts = [""] * len(texts) + ([""] * len(texts) if self.condition == "text_uncond" else texts)
        text_emb = self.text_encoder(texts).to(src.device)
        noise_kw = {} if self.eta == 0.0 else {"seed": seed}
        if guidance_scale is not None:
            noise_kw["guidance_scale"] = float(guidance_scale)
        joints, _, _ = self.sample(text_emb, lengths, init_latents, src_latents=src, first_step=first_step, **noise_kw)
        return remove_padding(joints.detach().cpu(), lengths)

    @torch.no_grad()
    def _diffusion_reverse(self, encoder_hidden_states, lengths=None, init_latents: Optional[torch.Tensor] = None,
                           step_noise: Optional[torch.Tensor] = None, trace: Optional[list] = None):
        """The reference's Python loop (mld.py:290-360) over the drop-in parts -> [latent_size, B, D]
        ([T, B, nfeats] for vae_type 'no').  `trace`: a list that receives prev_sample of every step, permuted like the result (mld.py:418-421)."""
        bsz = encoder_hidden_states.shape[0] // (2 if self.do_classifier_free_guidance else 1)
        dev = init_latents.device if init_latents is not None else encoder_hidden_states.device
        if self.vae_type == "no":
            assert lengths is not None, "no vae (diffusion only) need lengths for diffusion"          # mld.py:295
            shape = (bsz, max(lengths), self.nfeats)
        else:
            shape = (bsz, self.latent_dim[0], self.latent_dim[-1])
        latents = init_latents if init_latents is not None else torch.randn(shape, device=dev, dtype=torch.float)
        latents = latents * self.scheduler.init_noise_sigma
        self.scheduler.set_timesteps(self.cfg.model.scheduler.num_inference_timesteps)
        extra = {}
        if "eta" in set(inspect.signature(self.scheduler.step).parameters.keys()):
            extra["eta"] = self.cfg.model.scheduler.eta
        params = set(inspect.signature(self.scheduler.step).parameters.keys())
        # injected per-step draws: DDPM's `noise=`, DDIM's `variance_noise=` (eta > 0; diffusers draws torch.randn otherwise)
        noise_kw = "noise" if "noise" in params else ("variance_noise" if "variance_noise" in params else None)
        for i, t in enumerate(self.scheduler.timesteps.tolist()):
            if step_noise is not None and noise_kw:
                extra[noise_kw] = step_noise[i]
            x = torch.cat([latents] * 2) if self.do_classifier_free_guidance else latents
            noise_pred = self.denoiser(sample=x, timestep=t, encoder_hidden_states=encoder_hidden_states,
                                       lengths=(list(lengths) * 2 if lengths is not None else None))[0]
            if self.do_classifier_free_guidance:
                u, c = noise_pred.chunk(2)
                noise_pred = u + self.guidance_scale * (c - u)
            latents = self.scheduler.step(noise_pred, t, latents, **extra).prev_sample
            if trace is not None:
                trace.append(latents.permute(1, 0, 2))
        return latents.permute(1, 0, 2)

    @torch.no_grad()
    def _diffusion_reverse_tsne(self, encoder_hidden_states, lengths=None, init_latents: Optional[torch.Tensor] = None, seed: Optional[int] = None):
        """mld.py:362-424: the reverse loop that keeps the latents after every scheduler step -> [steps, B, D], the shape the reference's
        torch.cat gives for latent_size 1 (what its denoising-process figures and t-SNE plots read).  Fused latent models: ONE
        mldhip_sample_many_traj call -- the trajectory of the loop that serves sampling, not of a different one; otherwise (a swapped part, the
        diffusion-only variant) the modular Python loop, collecting prev_sample per step.  `lengths` is only needed by the diffusion-only variant,
        as in the reference; eta > 0: `seed` keys the fused path's Philox stream (None = drawn from torch's generator)."""
        if not self.fused or self.vae_type == "no":
            steps: list = []
            self._diffusion_reverse(encoder_hidden_states, lengths, init_latents, trace=steps)
            return torch.cat(steps)
        bsz = encoder_hidden_states.shape[0] // 2
        lengths = [int(x) for x in lengths] if lengths is not None else [1] * bsz      # (the latent loop has no masks: the lengths only size a decode nobody asks for)
        dev = init_latents.device if init_latents is not None else encoder_hidden_states.device
        if init_latents is None:
            init_latents = torch.randn((bsz, self.latent_dim[0], self.latent_dim[-1]), device=dev, dtype=torch.float)
        init_latents = init_latents.float().contiguous()
        eng = self._engine()
        stream = _engine.current_stream_handle(init_latents)
        _engine.finalize_if_dirty(eng, stream)
        traj = self._traj_buffer(eng, bsz, dev)
        req = dict(init_latents=init_latents, lengths=lengths, traj_out=traj)
        if self.condition == "action":
            req["actions"] = [int(a) for a in encoder_hidden_states.reshape(-1).tolist()[bsz:]]      # cond = cat(zeros_like(actions), actions) (mld.py:716-717)
        else:
            req["text_emb"] = encoder_hidden_states.float().contiguous()
        seed = self._noise_seed(seed)
        eng.sample_many_traj([req], None if seed is None else [(seed, 0)], stream)
        return traj
