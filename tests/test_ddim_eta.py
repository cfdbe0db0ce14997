"""Stochastic DDIM (scheduler eta > 0, include/mldhip.h "Noise contract") without a GPU: the scheduler's formula against a numpy
restatement and against the DDPM ancestral step (the eta = 1 identity), mldhip_ddim_step_eta and every reverse-loop family on the
functional simulator against a numpy loop (oracle denoiser + the formula + oracle.philox_normal), the noise keys, the error paths."""
import numpy as np
import pytest
import torch

from mld_hip import _lib
from mld_hip import synthetic as syn
from mld_hip.scheduler import HipDDIMScheduler, HipDDPMScheduler
from oracle import mld_oracle as O

import simlib

SCHED_KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False,
                set_alpha_to_one=False, steps_offset=1)
f32 = np.float32


def eta_coeffs_np(acp, final, t, prev, eta):
    """(sqrt(ab_t), sqrt(1 - ab_t), sqrt(ab_p), sqrt(1 - ab_p - sigma^2), sigma) in float32, as diffusers computes them"""
    a_t = f32(acp[t])
    a_p = f32(acp[prev]) if prev >= 0 else f32(final)
    var = f32(f32(f32(1) - a_p) / f32(f32(1) - a_t)) * f32(f32(1) - f32(a_t / a_p))
    sigma = f32(f32(eta) * np.sqrt(var, dtype=f32))
    return (np.sqrt(a_t, dtype=f32), np.sqrt(f32(1) - a_t, dtype=f32), np.sqrt(a_p, dtype=f32),
            np.sqrt(max(f32(f32(f32(1) - a_p) - f32(sigma * sigma)), f32(0)), dtype=f32), sigma)


def ddim_eta_step_np(eps, t, x, z, eta, sch):
    prev = int(t) - sch.num_train_timesteps // sch.num_inference_steps
    sa, sb, pa, ce, sg = eta_coeffs_np(sch.alphas_cumprod, sch.final_alpha_cumprod, int(t), prev, eta)
    x0 = (x - sb * eps) / sa
    return (pa * x0 + ce * eps + sg * z).astype(f32)


def keyed_noise(seed, first, B, step):
    """z of motions first .. first + B - 1 at scheduler step `step` (the Noise contract): [B, 1, 256]"""
    return O.philox_normal(B * 256, seed, step, first=first * 256).reshape(B, 1, 256)


def reverse_eta_np(sdd, text_emb, init_latents, steps, eta, keys_per_motion, guidance=7.5):
    """MLD._diffusion_reverse with DDIMScheduler.step(eta) fed the Philox draws of the Noise contract; keys_per_motion [(seed, index)]"""
    ops = O.NumpyOps(f32)
    sd = O.to_backend(ops, sdd)
    sch = O.DDIMSchedule()
    lat = init_latents.astype(f32)
    B = lat.shape[0]
    for i, t in enumerate(sch.set_timesteps(steps)):
        e = np.asarray(O.denoiser_forward(ops, sd, np.concatenate([lat, lat], 0), t, text_emb, 4))
        u, c = e[:B], e[B:]
        eps = u + f32(guidance) * (c - u)
        z = np.stack([keyed_noise(s, k, 1, i)[0] for s, k in keys_per_motion])
        lat = ddim_eta_step_np(eps, t, lat, z, eta, sch)
    return lat


# ------------------------------------------------------------------------------------------------ scheduler (host)
def test_scheduler_step_eta_matches_numpy():
    sch = HipDDIMScheduler(**SCHED_KW)
    sch.set_timesteps(50)
    ref = O.DDIMSchedule()
    ref.set_timesteps(50)
    g = np.random.default_rng(3)
    for t in (981, 501, 21, 1):
        eps, x, z = (g.standard_normal((4, 1, 256)).astype(f32) for _ in range(3))
        out = sch.step(torch.from_numpy(eps), t, torch.from_numpy(x), eta=0.5, variance_noise=torch.from_numpy(z)).prev_sample.numpy()
        assert np.abs(out - ddim_eta_step_np(eps, t, x, z, 0.5, ref)).max() < 1e-6, t
    # eta = 0 is the deterministic step; eta > 0 without variance_noise draws from the generator
    eps, x = torch.randn(2, 1, 256), torch.randn(2, 1, 256)
    a = sch.step(eps, 501, x, eta=0.5, generator=torch.Generator().manual_seed(7)).prev_sample
    b = sch.step(eps, 501, x, eta=0.5, generator=torch.Generator().manual_seed(7)).prev_sample
    c = sch.step(eps, 501, x, eta=0.5, generator=torch.Generator().manual_seed(8)).prev_sample
    assert torch.equal(a, b) and not torch.equal(a, c)
    with pytest.raises(ValueError):
        sch.step(eps, 501, x, eta=1.5)


def test_eta_one_is_the_ddpm_ancestral_step():
    """At eta = 1, DDIM's sigma is DDPM's fixed_small sigma on the same (t, p) pair and the whole step is the ancestral step (writing eps through
    x and x0 makes both coefficients equal).  Every step of the 50-step grid with p >= 0 -- the last step differs by design (DDIM: ab_0, DDPM: 1)."""
    ddim = HipDDIMScheduler(**SCHED_KW)
    ddim.set_timesteps(50)
    ddpm = HipDDPMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                            variance_type="fixed_small", clip_sample=False)
    ddpm.set_timesteps(50)
    g = np.random.default_rng(5)
    n = 0
    for t in ddim.timesteps.tolist():
        if t - 20 < 0:
            continue
        _, _, _, _, sg_ddpm = ddpm.coeffs(t)
        _, sg_ddim = ddim.eta_coeffs(t, 1.0)
        assert abs(sg_ddim - sg_ddpm) <= 1e-5 * sg_ddpm, (t, sg_ddim, sg_ddpm)
        eps, x, z = (torch.from_numpy(g.standard_normal((3, 1, 256)).astype(f32)) for _ in range(3))
        a = ddim.step(eps, t, x, eta=1.0, variance_noise=z).prev_sample
        b = ddpm.step(eps, t, x, noise=z).prev_sample
        assert ((a - b).abs().max() / b.abs().max()).item() < 1e-5, t
        n += 1
    assert n == 49


# ------------------------------------------------------------------------------------------------ C ABI on the simulator
def test_ddim_step_eta_sim():
    e = _lib.Engine(lib=simlib.sim_library(), use_graph=0, max_batch=4, max_frames=8, num_layers=3, eta=0.5)
    ref = O.DDIMSchedule()
    ref.set_timesteps(50)
    g = np.random.default_rng(11)
    n = 3 * 256 + 2                                      # a partial Philox quad at the end
    eps, x, z = (g.standard_normal(n).astype(f32) for _ in range(3))
    for t, step in ((981, 0), (1, 49)):
        out = np.full(n, np.nan, f32)
        e.ddim_step_eta(eps, t, x, z, out, n)
        assert np.abs(out - ddim_eta_step_np(eps, t, x, z, 0.5, ref)).max() < 1e-5
        out2 = np.full(n, np.nan, f32)
        e.ddim_step_eta(eps, t, x, None, out2, n, seed=1234, step_index=step)
        assert np.abs(out2 - ddim_eta_step_np(eps, t, x, O.philox_normal(n, 1234, step), 0.5, ref)).max() < 1e-5
    e.close()


def _text_engine(**cfg):
    e = _lib.Engine(lib=simlib.sim_library(), use_graph=0, max_frames=8, num_inference_steps=2, num_layers=3, **cfg)
    sdd, sdv = simlib.text_weights(3)
    e.load_state_dict(sdd, "denoiser.")
    e.load_state_dict(sdv, "vae.")
    e.finalize()
    return e, sdd


def _seeded(e, b, keys, B=None):
    """one request per key over consecutive slices of the batch; returns the latents [B, 1, 256]"""
    B = B or b.init_latents.shape[0]
    per = B // len(keys)
    lat = np.full((B, 1, 256), np.nan, f32)
    reqs = []
    for k in range(len(keys)):
        s = slice(k * per, (k + 1) * per)
        te = np.concatenate([b.text_emb[:B][s], b.text_emb[B:][s]], 0)
        reqs.append(dict(text_emb=np.ascontiguousarray(te), init_latents=np.ascontiguousarray(b.init_latents[s]), lengths=b.lengths[s],
                         latents_out=lat[s]))
    e.sample_many_seeded(reqs, keys)
    return lat


@pytest.mark.parametrize("family", ["latency", "strip", "persistent", "cluster4", "cluster8"])
def test_every_loop_family_samples_eta(family):
    """eta = 0.5 on every reverse-loop family (loop_kernel 1 latency, 2 strip, 3 persistent with and without fused_x3, 4 cluster with 4 and 8
    column groups): B = 11 ragged, a 3-layer skip stack, 2 steps, against the numpy loop with the same Philox draws; and far from the eta = 0 result."""
    prec = 0 if family in ("latency", "strip") else 1
    e, sdd = _text_engine(max_batch=12, precision=prec, eta=0.5)
    b = syn.make_batch(11, [8, 5, 3, 8, 1, 7, 2, 6, 8, 4, 8], seed=9)
    seed = 0x1234_5678_9ABC
    ref = reverse_eta_np(sdd, b.text_emb, b.init_latents, 2, 0.5, [(seed, 5 + m) for m in range(11)])
    ops = O.NumpyOps(f32)
    ref0 = np.asarray(O.diffusion_reverse(ops, O.to_backend(ops, sdd), b.text_emb, b.init_latents, 7.5, 2, 4))
    runs = {"latency": [("loop_kernel", 1)], "strip": [("loop_kernel", 2)], "persistent": [("loop_kernel", 3), ("fused_x3", 1)],
            "cluster4": [("loop_kernel", 4), ("cluster_groups", 4)], "cluster8": [("loop_kernel", 4), ("cluster_groups", 8)]}[family]
    for k, v in runs:
        e.set_option(k, v)
    variants = [None, ("fused_x3", 0)] if family == "persistent" else [None]
    for var in variants:
        if var:
            e.set_option(*var)
        lat = _seeded(e, b, [(seed, 5)])
        err = np.abs(lat - ref).max()
        assert err < (5e-4 if family == "strip" else 2e-4), (family, var, err)
        assert np.abs(lat - ref0).max() > 1e-2, (family, var)
    e.close()


def test_noise_keys_sim():
    """Keys: one request of 16 with {s, 0} == two requests of 8 with {s, 0} and {s, 8} (bit for bit); the same key twice is reproducible; another seed
    differs; on an eta = 0 handle the keys are ignored (== mldhip_sample_many, bit for bit)."""
    b = syn.make_batch(16, [4] * 16, seed=21)
    e, _ = _text_engine(max_batch=16, precision=1, eta=0.5)
    e.set_option("loop_kernel", 1)
    a = _seeded(e, b, [(77, 0)])
    c = _seeded(e, b, [(77, 0), (77, 8)])
    d = _seeded(e, b, [(77, 0)])
    x = _seeded(e, b, [(78, 0)])
    assert np.array_equal(a, c) and np.array_equal(a, d)
    assert np.abs(a - x).max() > 1e-2
    e.close()
    e0, _ = _text_engine(max_batch=16, precision=1)
    e0.set_option("loop_kernel", 1)
    s0 = _seeded(e0, b, [(77, 0), (99, 8)])
    lat = np.full((16, 1, 256), np.nan, f32)
    e0.sample_many([dict(text_emb=b.text_emb, init_latents=b.init_latents, lengths=b.lengths, latents_out=lat)])
    assert np.array_equal(s0, lat)
    e0.close()


def test_eta_error_paths_sim():
    lib = simlib.sim_library()
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(_lib.MldHipError) as ei:
            _lib.Engine(lib=lib, use_graph=0, max_batch=2, max_frames=8, num_layers=3, eta=bad)
        assert ei.value.code == -1
    with pytest.raises(_lib.MldHipError) as ei:
        _lib.Engine(lib=lib, use_graph=0, num_layers=3, max_batch=2, **{**simlib.NOVAE_CFG, "eta": 0.5})
    assert ei.value.code == -1 and "DDIM" in str(ei.value)
    e, _ = _text_engine(max_batch=4, eta=0.5)
    b = syn.make_batch(2, [4, 4], seed=1)
    lat = np.zeros((2, 1, 256), f32)
    for call in (lambda: e.sample(b.text_emb, b.init_latents, b.lengths, latents_out=lat),
                 lambda: e.sample_many([dict(text_emb=b.text_emb, init_latents=b.init_latents, lengths=b.lengths, latents_out=lat)])):
        with pytest.raises(_lib.MldHipError) as ei:
            call()
        assert ei.value.code == -3 and "mldhip_sample_many_seeded" in str(ei.value)
    with pytest.raises(_lib.MldHipError) as ei:
        e.sample_many_seeded([dict(text_emb=b.text_emb, init_latents=b.init_latents, lengths=b.lengths, latents_out=lat)], [(1, -1)])
    assert ei.value.code == -1
    e.close()
    ea = _lib.Engine(lib=lib, use_graph=0, max_batch=2, max_frames=8, **{**simlib.SIM_ACTION_CFG, "eta": 0.5})
    with pytest.raises(_lib.MldHipError) as ei:
        ea.sample_action([1, 2], b.init_latents, b.lengths)
    assert ei.value.code == -3 and "mldhip_sample_many_seeded" in str(ei.value)
    ea.close()
