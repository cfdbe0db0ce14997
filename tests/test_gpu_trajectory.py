"""Per-step latent trajectories (mldhip_sample_many_traj) on an MI355X: full 9-layer synthetic weights, 50 steps, F16X3.  Every step's row of every
loop family against the oracle's trace, the last row against latents_out to the bit, the call against the same call without a trajectory to the bit;
two cluster launches, graph replay with fresh buffers, mixed requests, the MLD surface.

Tolerance: the project's latent tolerance, 5e-3 absolute (tests/test_gpu_parity.py), applied to EVERY step.  The measured per-step maxima go to
profiles/traj_parity.json when MLDHIP_TRAJ_PARITY_OUT names a file (the committed copy was written that way)."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from mld_hip import _lib  # noqa: E402
from mld_hip import synthetic as syn  # noqa: E402
from oracle import mld_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
STEPS = 50
TOL = 5e-3
LENS9 = [24, 17, 3, 20, 1, 9, 24, 12, 5]
SEED, FIRST = 0xC0FFEE, 3
FAMILY = {"cluster": 0, "persistent": 3, "latency": 1}      # "loop_kernel": the default picks the cluster loop for a small F16X3 call

_measured = {}


def _load(eng):
    eng.load_state_dict(syn.make_denoiser_state_dict(), "denoiser.")
    eng.load_state_dict(syn.make_vae_state_dict(), "vae.")
    mean, std = syn.make_mean_std()
    eng.load_tensor("mean", mean)
    eng.load_tensor("std", std)
    eng.finalize()


def _cuda(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def oracle_trace(text_emb, init_latents, eta=0.0, indices=None):
    """[STEPS, B, 256]: prev_sample of every step -- O.diffusion_reverse's own trace at eta = 0; at eta > 0 the numpy loop of tests/test_gpu_ddim_eta.py
    (DDIMScheduler.step(eta) fed the Philox draws of the Noise contract), keeping each step"""
    ops = O.NumpyOps(f32)
    sd = O.to_backend(ops, syn.make_denoiser_state_dict())
    B = init_latents.shape[0]
    if eta == 0.0:
        tr = []
        O.diffusion_reverse(ops, sd, text_emb, init_latents, 7.5, STEPS, 4, trace=tr)
        return np.stack([np.asarray(t).reshape(B, 256) for t in tr])
    sch = O.DDIMSchedule()
    lat = init_latents.astype(f32)
    idx = np.asarray(indices, np.int64)
    rows = idx[:, None] * 256 + np.arange(256)[None, :]
    out = []
    for i, t in enumerate(sch.set_timesteps(STEPS)):
        e = np.asarray(O.denoiser_forward(ops, sd, np.concatenate([lat, lat], 0), t, text_emb, 4))
        u, c = e[:B], e[B:]
        eps = u + f32(7.5) * (c - u)
        z = O.philox_normal(int(idx.max() + 1) * 256, SEED, i)[rows].reshape(B, 1, 256)
        prev = int(t) - sch.num_train_timesteps // STEPS
        a_t = f32(sch.alphas_cumprod[int(t)])
        a_p = f32(sch.alphas_cumprod[prev]) if prev >= 0 else f32(sch.final_alpha_cumprod)
        var = f32(f32(f32(1) - a_p) / f32(f32(1) - a_t)) * f32(f32(1) - f32(a_t / a_p))
        sg = f32(f32(eta) * np.sqrt(var, dtype=f32))
        ce = np.sqrt(max(f32(f32(f32(1) - a_p) - f32(sg * sg)), f32(0)), dtype=f32)
        x0 = (lat - np.sqrt(f32(1) - a_t, dtype=f32) * eps) / np.sqrt(a_t, dtype=f32)
        lat = (np.sqrt(a_p, dtype=f32) * x0 + ce * eps + sg * z).astype(f32)
        out.append(lat.reshape(B, 256).copy())
    return np.stack(out)


def _req(b, dev, sl=slice(None), traj=True):
    B = len(b.lengths[sl])
    n = b.init_latents.shape[0]
    te = np.concatenate([b.text_emb[:n][sl], b.text_emb[n:][sl]], 0)
    T = max(b.lengths[sl])
    q = dict(text_emb=_cuda(te, dev), init_latents=_cuda(b.init_latents[sl], dev), lengths=b.lengths[sl],
             latents_out=_nan(dev, B, 1, 256), joints_out=_nan(dev, B, T, 22, 3))
    if traj:
        q["traj_out"] = _nan(dev, STEPS, B, 256)
    return q


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def eng():
    """the eta = 0 handle of this file: room for 128 + 8 motions (two cluster launches)"""
    e = _lib.Engine(device=0, max_batch=136, max_frames=24, precision=1)
    _load(e)
    yield e
    e.close()
    out = os.environ.get("MLDHIP_TRAJ_PARITY_OUT")
    if out and _measured:
        with open(out, "w") as f:
            json.dump({"what": "max |engine - oracle trace| over the B = 9 batch after each of the 50 scheduler steps, F16X3, MI355X; bound 5e-3 on every step",
                       "families": _measured}, f, indent=1)


@pytest.fixture(scope="module")
def batch9():
    return syn.make_batch(9, LENS9, seed=81)


@pytest.fixture(scope="module")
def ref9(batch9):
    return oracle_trace(batch9.text_emb, batch9.init_latents)


def _check_family(e, dev, b, ref, keys, name):
    q = _req(b, dev)
    e.sample_many_traj([q], keys)
    torch.cuda.synchronize()
    counts = e.launch_counts()
    q0 = _req(b, dev, traj=False)
    if keys is None:
        e.sample_many([q0])
    else:
        e.sample_many_seeded([q0], keys)
    torch.cuda.synchronize()
    assert e.launch_counts() == counts                       # no extra launch for the trajectory
    traj = q["traj_out"].cpu().numpy()
    err = np.abs(traj - ref).reshape(STEPS, -1).max(1)
    _measured[name] = {"per_step_max_abs_err": [float(x) for x in err], "max": float(err.max()), "step_of_max": int(err.argmax()), "last_step": float(err[-1])}
    print(f"{name}: per-step max error, worst {err.max():.3e} at step {int(err.argmax())}, last step {err[-1]:.3e}")
    assert np.isfinite(traj).all() and err.max() < TOL, (name, err.tolist())
    assert torch.equal(q["traj_out"][STEPS - 1], q["latents_out"][:, 0])
    assert torch.equal(q["latents_out"], q0["latents_out"]) and torch.equal(q["joints_out"], q0["joints_out"])
    ns = e.numeric_status()
    assert ns["nonfinite_values"] == 0 and ns["loop_split_ok"] == 1 and ns["cluster_loop"] in (1, 3), ns
    return counts, q["traj_out"]


def _forced_cluster_traj(eng, dev, b):
    """the trajectory of the batch on the cluster loop, forced ("loop_kernel" 4); leaves the option at 4"""
    eng.set_option("loop_kernel", 4)
    q = _req(b, dev)
    eng.sample_many_traj([q], None)
    torch.cuda.synchronize()
    assert eng.launch_counts()[0] == 2
    return q["traj_out"]


@pytest.mark.parametrize("family", list(FAMILY))
def test_every_step_of_every_family_matches_the_oracle_trace(eng, dev, batch9, ref9, family):
    """B = 9, ragged lengths up to 24 frames: cluster loop (default), persistent loop, latency kernels."""
    eng.set_option("loop_kernel", FAMILY[family])
    try:
        counts, traj = _check_family(eng, dev, batch9, ref9, None, family)
        # which loop ran: the latency family is a launch per GEMM; the two one-launch loops differ in summation order, i.e. in bits --
        # the default's result must be the forced cluster loop's ("loop_kernel" 4) to the bit, the persistent loop's must not be
        if family == "latency":
            assert counts[0] > 1000
        else:
            assert counts[0] == 2                            # condition rows + ONE launch for the 50 steps
        if family == "cluster":
            assert eng.numeric_status()["cluster_loop"] == 1  # available on this handle and device (not left, not another process's lane)
            assert torch.equal(_forced_cluster_traj(eng, dev, batch9), traj)
        if family == "persistent":
            assert not torch.equal(_forced_cluster_traj(eng, dev, batch9), traj)
    finally:
        eng.set_option("loop_kernel", 0)


def test_cluster_loop_eta_trajectory(dev, batch9):
    """eta = 0.5 on the cluster loop: every row against the numpy loop with the same Philox draws."""
    e = _lib.Engine(device=0, max_batch=16, max_frames=24, precision=1, eta=0.5)
    _load(e)
    ref = oracle_trace(batch9.text_emb, batch9.init_latents, 0.5, [FIRST + m for m in range(9)])
    counts, traj = _check_family(e, dev, batch9, ref, [(SEED, FIRST)], "cluster_eta0.5")
    assert counts[0] == 2 and e.numeric_status()["cluster_loop"] == 1
    e.set_option("loop_kernel", 4)                           # the default picked the cluster loop: forcing it gives the same bits
    forced = _req(batch9, dev)
    e.sample_many_traj([forced], [(SEED, FIRST)])
    torch.cuda.synchronize()
    assert torch.equal(forced["traj_out"], traj)
    e.close()


def test_two_cluster_launches(eng, dev):
    """B = 136 = 128 + 8: the second launch's motions land in their rows (the table is indexed by the motion of the CALL).  Motions of a call are
    independent: a spread subset against the oracle."""
    B = 136
    b = syn.make_batch(B, [1 + (7 * i) % 24 for i in range(B)], seed=82)
    q = _req(b, dev)
    eng.sample_many_traj([q], None)
    torch.cuda.synchronize()
    assert eng.launch_counts()[0] == 3                       # condition rows + two cluster launches
    sub = [0, 7, 127, 128, 135]
    te = np.concatenate([b.text_emb[:B][sub], b.text_emb[B:][sub]], 0)
    ref = oracle_trace(te, b.init_latents[sub])
    traj = q["traj_out"].cpu().numpy()
    err = np.abs(traj[:, sub] - ref).reshape(STEPS, -1).max(1)
    print(f"two launches: worst {err.max():.3e} at step {int(err.argmax())}")
    assert np.isfinite(traj).all() and err.max() < TOL, err.tolist()
    assert torch.equal(q["traj_out"][STEPS - 1], q["latents_out"][:, 0])
    assert eng.numeric_status()["nonfinite_values"] == 0


def test_graph_replay_with_fresh_buffers(eng, dev, batch9):
    """The same call twice with freshly allocated output and trajectory tensors, the first call's tensors overwritten with NaN in between: the captured
    graph holds no caller pointer.  Same launches as the call without a trajectory."""
    q1 = _req(batch9, dev)
    eng.sample_many_traj([q1], None)
    torch.cuda.synchronize()
    c1 = eng.launch_counts()
    keep = {k: q1[k].clone() for k in ("latents_out", "joints_out", "traj_out")}
    for k in keep:
        q1[k].fill_(float("nan"))
    q2 = _req(batch9, dev)
    assert q2["traj_out"].data_ptr() != q1["traj_out"].data_ptr()
    eng.sample_many_traj([q2], None)
    torch.cuda.synchronize()
    assert eng.launch_counts() == c1
    for k in keep:
        assert torch.equal(q2[k], keep[k]), k
        assert torch.isnan(q1[k]).all(), k                   # the replay wrote nothing to the first call's buffers
    q0 = _req(batch9, dev, traj=False)
    eng.sample_many([q0])
    torch.cuda.synchronize()
    assert eng.launch_counts() == c1


def test_mixed_requests_one_chain(eng, dev, batch9, ref9):
    """Two requests (B = 5 and B = 4) on one chain, a trajectory for the second only; NaN guard regions around the first request's outputs and around
    the trajectory buffer stay NaN."""
    pad = 1024
    qa, qb = _req(batch9, dev, slice(0, 5), traj=False), _req(batch9, dev, slice(5, 9), traj=False)
    flat_a, flat_j, flat_t = _nan(dev, 5 * 256 + 2 * pad), _nan(dev, qa["joints_out"].numel() + 2 * pad), _nan(dev, STEPS * 4 * 256 + 2 * pad)
    qa["latents_out"] = flat_a[pad:pad + 5 * 256].view(5, 1, 256)
    qa["joints_out"] = flat_j[pad:pad + qa["joints_out"].numel()].view(qa["joints_out"].shape)
    qb["traj_out"] = flat_t[pad:pad + STEPS * 4 * 256].view(STEPS, 4, 256)
    eng.sample_many_traj([qa, qb], None)
    torch.cuda.synchronize()
    for flat in (flat_a, flat_j, flat_t):
        assert torch.isnan(flat[:pad]).all() and torch.isnan(flat[-pad:]).all() and torch.isfinite(flat[pad:-pad]).all()
    one = _req(batch9, dev, slice(5, 9))
    eng.sample_many_traj([one], None)
    torch.cuda.synchronize()
    assert (qb["traj_out"] - one["traj_out"]).abs().max().item() < TOL
    assert np.abs(qb["traj_out"].cpu().numpy() - ref9[:, 5:9]).max() < TOL
    assert torch.equal(qb["traj_out"][STEPS - 1], qb["latents_out"][:, 0])
    pa, pb = _req(batch9, dev, slice(0, 5), traj=False), _req(batch9, dev, slice(5, 9), traj=False)
    eng.sample_many([pa, pb])
    torch.cuda.synchronize()
    assert torch.equal(pa["latents_out"], qa["latents_out"]) and torch.equal(pa["joints_out"], qa["joints_out"]) and torch.equal(pb["joints_out"], qb["joints_out"])


def test_mld_diffusion_reverse_tsne_on_gpu(dev):
    """MLD._diffusion_reverse_tsne through the reference-shaped surface: [50, B, 256] from the fused path, its last row == the latents MLD.sample returns
    (the same engine path, to the bit) and within the latent tolerance of _diffusion_reverse (the modular loop: other kernels, another summation order);
    with a part swapped out the method IS that modular loop and its last row equals _diffusion_reverse's result to the bit."""
    from mld_hip import config as C
    from mld_hip import engine as E
    from mld_hip.datamodule import HipDataModule
    from mld_hip.mld import MLD
    from mld_hip.text_encoder import SyntheticTextEncoder

    E.drop_engines()
    cfg = C.load_config()
    E.configure(max_batch=8, max_frames=196)
    model = MLD(cfg, HipDataModule(cfg), text_encoder=SyntheticTextEncoder()).to(dev).eval()
    assert model.fused
    texts = ["a man kicks with something or someone with his left leg.", "A person is skipping rope.", "a person walks backward slowly."]
    lengths = [50, 100, 100]
    lat0 = _cuda(syn.make_batch(3, lengths).init_latents, dev)
    emb = model.text_encoder([""] * 3 + texts)
    tr = model._diffusion_reverse_tsne(emb, lengths, init_latents=lat0)
    assert tuple(tr.shape) == (STEPS, 3, 256) and tr.is_cuda
    z = model._diffusion_reverse(emb, lengths, init_latents=lat0)
    assert (tr[-1] - z[0]).abs().max().item() < TOL
    joints, feats, lat, traj = model.sample(emb, lengths, lat0, return_trajectory=True)
    j0, _, l0 = model.sample(emb, lengths, lat0)
    assert torch.equal(traj, tr) and torch.equal(tr[-1], lat[:, 0]) and torch.equal(lat, l0) and torch.equal(joints, j0)
    ref = oracle_trace(emb.cpu().numpy(), lat0.cpu().numpy())
    assert np.abs(tr.cpu().numpy() - ref).max() < TOL

    class Modular(MLD):
        fused = property(lambda self: False)

    mod = Modular(cfg, HipDataModule(cfg), text_encoder=model.text_encoder).to(dev).eval()
    trm = mod._diffusion_reverse_tsne(emb, lengths, init_latents=lat0)
    assert tuple(trm.shape) == (STEPS, 3, 256)
    assert torch.equal(trm[-1], mod._diffusion_reverse(emb, lengths, init_latents=lat0)[0])
    assert (trm - tr).abs().max().item() < TOL
    E.drop_engines()
