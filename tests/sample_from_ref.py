"""numpy reference of mldhip_sample_many_from for tests/test_sample_from_sim.py and tests/test_gpu_sample_from.py (not a test module): the reverse loop of
oracle.mld_oracle with a per-motion start -- O.denoiser_forward, O.DDIMSchedule and the stepping of tests/test_trajectory_sim.py::trace_ref /
tests/test_ddim_eta.py::ddim_eta_step_np; the oracle's own diffusion_reverse has no start step."""
import numpy as np

from oracle import mld_oracle as O

from test_ddim_eta import ddim_eta_step_np, keyed_noise

f32 = np.float32
NONE, SOURCE, RESUME = "none", "source", "resume"


def start_state(sch, n, kind, f, src, init):
    """the loop state of one motion in front of step f ([1, 256] rows): include/mldhip.h mldhip_start"""
    if kind == NONE:
        return (init * f32(sch.init_noise_sigma)).astype(f32)
    if kind == RESUME:
        return src.astype(f32)
    sa, sb, _, _ = sch.coeffs(sch.timesteps[f])              # diffusers' add_noise at the first timestep that is run
    return (sa * src + sb * init).astype(f32)


def reverse_from_np(sd, text_emb, init, starts, n, eta=0.0, keys_per_motion=None, guidance=7.5, nhead=4, denoise=None):
    """starts: per motion (kind, first_step, src [1, 256] or None).  -> (traj [n, B, 256], NaN where a row is not written; latents [B, 256]).
    `sd` is the oracle-backend denoiser state dict; `denoise(x2, t)` replaces O.denoiser_forward on the text condition (the action engine's call)."""
    ops = O.NumpyOps(f32)
    sch = O.DDIMSchedule()
    ts = sch.set_timesteps(n)
    B = init.shape[0]
    lat = np.stack([start_state(sch, n, k, f, s, init[m]) for m, (k, f, s) in enumerate(starts)]).astype(f32)      # [B, 1, 256]
    first = np.array([f for _, f, _ in starts])
    traj = np.full((n, B, 256), np.nan, f32)
    for i in range(int(first.min()), n):
        t = ts[i]
        x2 = np.concatenate([lat, lat], 0)
        e = np.asarray(denoise(x2, t) if denoise else O.denoiser_forward(ops, sd, x2, t, text_emb, nhead))
        u, c = e[:B], e[B:]
        eps = u + f32(guidance) * (c - u)
        if eta == 0.0:
            new = np.asarray(sch.step(eps, t, lat), f32)
        else:
            z = np.stack([keyed_noise(s, k, 1, i)[0] for s, k in keys_per_motion])
            new = ddim_eta_step_np(eps, t, lat, z, eta, sch)
        live = first <= i
        lat = np.where(live[:, None, None], new, lat).astype(f32)
        traj[i, live] = lat.reshape(B, 256)[live]
    return traj, lat.reshape(B, 256)
