"""Per-step latent trajectories (mldhip_sample_many_traj, MLD._diffusion_reverse_tsne) without a GPU: every reverse-loop family on the functional
simulator stores the latents after every scheduler step; each row against the oracle's trace (eta = 0) or a numpy loop fed the same Philox draws
(eta = 0.5), the last row against latents_out to the bit, everything else of the call against the same call without a trajectory to the bit."""
import numpy as np
import pytest
import torch

from mld_hip import _lib
from mld_hip import synthetic as syn
from oracle import mld_oracle as O

import simlib
from test_ddim_eta import ddim_eta_step_np, keyed_noise

f32 = np.float32
STEPS = 4          # (the scheduler needs num_train_timesteps = 1000 to be a multiple of the step count: the smallest such count above 2)
SEED, FIRST = 0x1234_5678_9ABC, 5
LENS9 = [8, 5, 3, 8, 1, 7, 2, 6, 4]
# the tolerances tests/test_ddim_eta.py holds the final latents of the simulator to, per family
TOL = {"latency": 2e-4, "strip": 5e-4, "persistent": 2e-4, "cluster4": 2e-4, "cluster8": 2e-4}
RUNS = {"latency": [("loop_kernel", 1)], "strip": [("loop_kernel", 2)], "persistent": [("loop_kernel", 3), ("fused_x3", 1)],
        "cluster4": [("loop_kernel", 4), ("cluster_groups", 4)], "cluster8": [("loop_kernel", 4), ("cluster_groups", 8)]}
FAMILIES = list(RUNS)

_cache = {}


def weights():
    if "w" not in _cache:
        _cache["w"] = simlib.text_weights(3)
    return _cache["w"]


def batch9():
    if "b9" not in _cache:
        _cache["b9"] = syn.make_batch(9, LENS9, seed=9)
    return _cache["b9"]


def trace_ref(eta, b=None, keys_per_motion=None):
    """[STEPS, B, 256]: prev_sample of every step -- the oracle's own trace at eta = 0; tests/test_ddim_eta.py's reverse_eta_np keeping each step otherwise.
    Computed once per (eta) for the shared B = 9 batch."""
    shared = b is None
    if shared and ("ref", eta) in _cache:
        return _cache["ref", eta]
    b = b or batch9()
    B = b.init_latents.shape[0]
    ops = O.NumpyOps(f32)
    sd = O.to_backend(ops, weights()[0])
    if eta == 0.0:
        tr = []
        O.diffusion_reverse(ops, sd, b.text_emb, b.init_latents, 7.5, STEPS, 4, trace=tr)
        out = np.stack([np.asarray(t).reshape(B, 256) for t in tr])
    else:
        keys_per_motion = keys_per_motion or [(SEED, FIRST + m) for m in range(B)]
        sch = O.DDIMSchedule()
        lat = b.init_latents.astype(f32)
        rows = []
        for i, t in enumerate(sch.set_timesteps(STEPS)):
            e = np.asarray(O.denoiser_forward(ops, sd, np.concatenate([lat, lat], 0), t, b.text_emb, 4))
            u, c = e[:B], e[B:]
            eps = u + f32(7.5) * (c - u)
            z = np.stack([keyed_noise(s, k, 1, i)[0] for s, k in keys_per_motion])
            lat = ddim_eta_step_np(eps, t, lat, z, eta, sch)
            rows.append(lat.reshape(B, 256).copy())
        out = np.stack(rows)
    if shared:
        _cache["ref", eta] = out
    return out


def text_engine(family, eta=0.0, max_batch=12, **cfg):
    prec = 0 if family in ("latency", "strip") else 1
    e = _lib.Engine(lib=simlib.sim_library(), use_graph=0, max_frames=8, num_inference_steps=STEPS, num_layers=3, max_batch=max_batch, precision=prec,
                    eta=eta, **cfg)
    sdd, sdv = weights()
    e.load_state_dict(sdd, "denoiser.")
    e.load_state_dict(sdv, "vae.")
    mean, std = syn.make_mean_std()
    e.load_tensor("mean", mean)
    e.load_tensor("std", std)
    e.finalize()
    for k, v in RUNS[family]:
        e.set_option(k, v)
    return e


def request(b, s=None, lat=None, joints=None, traj=None):
    """the request dict of motions `s` (a slice) of batch b"""
    B = b.init_latents.shape[0]
    s = s or slice(0, B)
    te = np.ascontiguousarray(np.concatenate([b.text_emb[:B][s], b.text_emb[B:][s]], 0))
    q = dict(text_emb=te, init_latents=np.ascontiguousarray(b.init_latents[s]), lengths=b.lengths[s])
    if lat is not None:
        q["latents_out"] = lat
    if joints is not None:
        q["joints_out"] = joints
    if traj is not None:
        q["traj_out"] = traj
    return q


# ------------------------------------------------------------------------------------------------ every family, eta = 0 and eta = 0.5
@pytest.mark.parametrize("eta", [0.0, 0.5])
@pytest.mark.parametrize("family", FAMILIES)
def test_every_loop_family_stores_its_trajectory(family, eta):
    """B = 9: the second workgroup / cluster holds one real motion and seven missing ones.  Every row against the reference trace within the family's
    tolerance; traj[-1] == latents_out, and latents / joints == the same call through sample_many_seeded, to the bit."""
    e = text_engine(family, eta)
    b = batch9()
    keys = [(SEED, FIRST)]
    T = max(LENS9)
    lat = np.full((9, 1, 256), np.nan, f32)
    joints = np.full((9, T, 22, 3), np.nan, f32)
    traj = np.full((STEPS, 9, 256), np.nan, f32)
    e.sample_many_traj([request(b, lat=lat, joints=joints, traj=traj)], keys)
    counts = e.launch_counts()
    lat0 = np.full((9, 1, 256), np.nan, f32)
    joints0 = np.full((9, T, 22, 3), np.nan, f32)
    e.sample_many_seeded([request(b, lat=lat0, joints=joints0)], keys)
    assert e.launch_counts() == counts                       # no extra launch for the trajectory
    ref = trace_ref(eta)
    err = [float(np.abs(traj[s] - ref[s]).max()) for s in range(STEPS)]
    print(f"{family} eta={eta}: per-step max error {err}")
    assert np.isfinite(traj).all() and max(err) < TOL[family], (family, eta, err)
    assert np.array_equal(traj[-1], lat.reshape(9, 256))
    assert np.array_equal(lat, lat0) and np.array_equal(joints, joints0)
    if family == "latency":
        # every entry NULL / no table at all: the call is mldhip_sample_many_seeded
        lat1 = np.full((9, 1, 256), np.nan, f32)
        e.sample_many_traj([request(b, lat=lat1)], keys)
        assert np.array_equal(lat1, lat0)
        if eta == 0.0:                                      # ... whose keys an eta = 0 handle does not need
            lat2 = np.full((9, 1, 256), np.nan, f32)
            tr2 = np.full((STEPS, 9, 256), np.nan, f32)
            e.sample_many_traj([request(b, lat=lat2, traj=tr2)], None)
            assert np.array_equal(lat2, lat0) and np.array_equal(tr2, traj)
    if family == "persistent":
        # the exact-fp32 instantiations of the persistent loop (den_loop_kernel<false, ...>), as tests/test_ddim_eta.py drives them
        e.set_option("fused_x3", 0)
        lat3 = np.full((9, 1, 256), np.nan, f32)
        tr3 = np.full((STEPS, 9, 256), np.nan, f32)
        e.sample_many_traj([request(b, lat=lat3, traj=tr3)], keys)
        err3 = [float(np.abs(tr3[s] - ref[s]).max()) for s in range(STEPS)]
        print(f"{family} fused_x3=0 eta={eta}: per-step max error {err3}")
        assert np.isfinite(tr3).all() and max(err3) < TOL[family], (family, eta, err3)
        assert np.array_equal(tr3[-1], lat3.reshape(9, 256)) and not np.array_equal(tr3, traj)      # (another kernel: other bits)
    e.close()


# ------------------------------------------------------------------------------------------------ two cluster launches
def test_two_cluster_launches_store_both_halves():
    """cluster_chunk 8, B = 9: motions 0-7 and motion 8 come from different launches; the table is indexed by the motion of the CALL."""
    e = text_engine("cluster8")
    e.set_option("cluster_chunk", 8)
    b = batch9()
    lat = np.full((9, 1, 256), np.nan, f32)
    traj = np.full((STEPS, 9, 256), np.nan, f32)
    e.sample_many_traj([request(b, lat=lat, traj=traj)], None)
    assert e.launch_counts()[0] == 3                        # condition rows + two cluster launches
    ref = trace_ref(0.0)
    assert np.isfinite(traj).all()
    assert np.abs(traj[:, :8] - ref[:, :8]).max() < TOL["cluster8"] and np.abs(traj[:, 8] - ref[:, 8]).max() < TOL["cluster8"]
    assert np.array_equal(traj[-1], lat.reshape(9, 256))
    e.close()


# ------------------------------------------------------------------------------------------------ mixed requests, guard regions
def _guarded(shape, pad=512):
    """a NaN-filled flat buffer with `pad` guard floats on both sides of a view of `shape`"""
    n = int(np.prod(shape))
    flat = np.full(n + 2 * pad, np.nan, f32)
    return flat, flat[pad:pad + n].reshape(shape)


@pytest.mark.parametrize("family", ["persistent", "latency"])
def test_mixed_requests_one_chain(family):
    """Two requests (B = 5 and B = 4) in one call, a trajectory for the second only: its rows match a single-request call's within the family's tolerance
    ; nothing is written around the first request's outputs or behind
    the trajectory buffer."""
    e = text_engine(family)
    b = batch9()
    flat_a, lat_a = _guarded((5, 1, 256))
    flat_b, lat_b = _guarded((4, 1, 256))
    flat_t, traj_b = _guarded((STEPS, 4, 256))
    e.sample_many_traj([request(b, slice(0, 5), lat=lat_a), request(b, slice(5, 9), lat=lat_b, traj=traj_b)], None)
    for flat, n in ((flat_a, 5 * 256), (flat_b, 4 * 256), (flat_t, STEPS * 4 * 256)):
        assert np.isnan(flat[:512]).all() and np.isnan(flat[512 + n:]).all() and np.isfinite(flat[512:512 + n]).all()
    one_lat = np.full((4, 1, 256), np.nan, f32)
    one = np.full((STEPS, 4, 256), np.nan, f32)
    e.sample_many_traj([request(b, slice(5, 9), lat=one_lat, traj=one)], None)
    assert np.abs(traj_b - one).max() < TOL[family]
    assert np.abs(traj_b - trace_ref(0.0)[:, 5:9]).max() < TOL[family]
    assert np.array_equal(traj_b[-1], lat_b.reshape(4, 256))
    # the first request's latents: what the call gives without any trajectory
    lat_a0, lat_b0 = np.full((5, 1, 256), np.nan, f32), np.full((4, 1, 256), np.nan, f32)
    e.sample_many([request(b, slice(0, 5), lat=lat_a0), request(b, slice(5, 9), lat=lat_b0)])
    assert np.array_equal(lat_a, lat_a0) and np.array_equal(lat_b, lat_b0)
    e.close()


# ------------------------------------------------------------------------------------------------ action engine
def test_action_engine_trajectory():
    """B = 3 on the action-conditioned engine (latency family): every row against the oracle's trace, the last row == latents_out."""
    e = simlib.sim_action_engine(max_batch=4, max_frames=8, num_inference_steps=STEPS)
    e.set_option("loop_kernel", 1)
    sdd, _ = simlib.action_weights()
    g = np.random.default_rng(4)
    lat0 = g.standard_normal((3, 1, 256)).astype(f32)
    acts, lens = [3, 0, 11], [8, 5, 2]
    lat = np.full((3, 1, 256), np.nan, f32)
    feats = np.full((3, 8, 150), np.nan, f32)
    traj = np.full((STEPS, 3, 256), np.nan, f32)
    e.sample_many_traj([dict(actions=acts, init_latents=lat0, lengths=lens, latents_out=lat, feats_out=feats, traj_out=traj)], None)
    lat1 = np.full((3, 1, 256), np.nan, f32)
    feats1 = np.full((3, 8, 150), np.nan, f32)
    e.sample_action(acts, lat0, lens, lat1, feats1)
    assert np.array_equal(lat, lat1) and np.array_equal(feats, feats1) and np.array_equal(traj[-1], lat.reshape(3, 256))
    # the oracle's action loop (O.sample_action) keeps no trace: the same loop, keeping every step
    ops = O.NumpyOps(f32)
    sd = O.to_backend(ops, sdd)
    sch = O.DDIMSchedule()
    x = lat0 * sch.init_noise_sigma
    cond = np.concatenate([np.zeros(3, np.int64), np.asarray(acts, np.int64)])
    tr = []
    for t in sch.set_timesteps(STEPS):
        eps = O.denoiser_forward_action(ops, sd, ops.cat([x, x], 0), t, cond, 4, 7.5)
        u, c = eps[:3], eps[3:]
        x = sch.step(u + 7.5 * (c - u), t, x)
        tr.append(ops.to_numpy(x).copy())
    ref = np.stack([np.asarray(t).reshape(3, 256) for t in tr])
    assert np.abs(traj - ref).max() < 2e-4
    e.close()


# ------------------------------------------------------------------------------------------------ cluster timeout
def test_cluster_timeout_poisons_the_last_row():
    """"cluster_inject": one member never raises its first flag, the launch runs into its (shortened) bound and gives up: the latents are NaN, and so is
    the last trajectory row of the same motions -- traj[-1] == latents also behind a failed launch."""
    e = text_engine("cluster4", max_batch=8)
    e.set_option("cluster_inject", 1 + 2)
    b = syn.make_batch(8, [8] * 8, seed=23)
    lat = np.zeros((8, 1, 256), f32)
    traj = np.zeros((STEPS, 8, 256), f32)
    e.sample_many_traj([request(b, lat=lat, traj=traj)], None)
    assert np.isnan(lat).all()
    assert np.array_equal(np.isnan(traj[-1]), np.isnan(lat.reshape(8, 256)))
    e.numeric_status()
    e.close()


# ------------------------------------------------------------------------------------------------ error paths
def test_trajectory_error_paths():
    b = syn.make_batch(2, [4, 4], seed=1)
    traj = np.zeros((STEPS, 2, 256), f32)
    lat = np.zeros((2, 1, 256), f32)
    # eta > 0: the keys are required, with a trajectory as without one
    e = text_engine("latency", eta=0.5, max_batch=4)
    with pytest.raises(_lib.MldHipError) as ei:
        e.sample_many_traj([request(b, lat=lat, traj=traj)], None)
    assert ei.value.code == -1 and "keys" in str(ei.value)
    with pytest.raises(_lib.MldHipError) as ei:
        e.sample_many_traj([request(b, lat=lat, traj=traj)], [(1, -1)])
    assert ei.value.code == -1
    # a trajectory buffer that is not 16-byte aligned is refused (the rows are stored four floats at a time)
    flat = np.zeros(STEPS * 2 * 256 + 8, f32)
    off = 1 + (-(flat.ctypes.data // 4) % 4)                  # first float whose address is 4 mod 16
    with pytest.raises(_lib.MldHipError) as ei:
        e.sample_many_traj([request(b, lat=lat, traj=flat[off:off + STEPS * 2 * 256].reshape(STEPS, 2, 256))], [(1, 0)])
    assert ei.value.code == -1 and "aligned" in str(ei.value)
    e.close()
    # the diffusion-only variant has no latent trajectory
    en = _lib.Engine(lib=simlib.sim_library(), use_graph=0, num_layers=3, max_batch=2, max_frames=8, **simlib.NOVAE_CFG)
    with pytest.raises(_lib.MldHipError) as ei:
        en.sample_many_traj([dict(text_emb=b.text_emb, init_latents=np.zeros((2, 4, 263), f32), lengths=[4, 4], traj_out=traj)], None)
    assert ei.value.code == -1 and "diffusion-only" in str(ei.value)
    en.close()


def test_symbol_is_added_at_abi_8():
    """One more exported symbol, no version bump: callers detect mldhip_sample_many_traj by its presence."""
    lib = simlib.sim_library()
    assert lib.mldhip_abi_version() == 8 and hasattr(lib, "mldhip_sample_many_traj")
    assert "mldhip_sample_many_traj" in _lib.exported_symbols()


# ------------------------------------------------------------------------------------------------ host mirror
@pytest.mark.parametrize("fused", [False, True])
def test_mld_diffusion_reverse_tsne(fused):
    """MLD._diffusion_reverse_tsne (mld.py:362-424) -> [n, B, 256]: the modular Python loop over the drop-in parts collecting prev_sample per step, and the
    fused path (one mldhip_sample_many_traj call), both against the oracle's trace; return_trajectory on MLD.sample."""
    from mld_hip import config as C
    from mld_hip import engine as E
    from mld_hip.datamodule import HipDataModule
    from mld_hip.mld import MLD
    from mld_hip.text_encoder import SyntheticTextEncoder

    eng = _lib.Engine(lib=simlib.sim_library(), use_graph=0, max_batch=4, max_frames=40, num_inference_steps=STEPS, num_layers=3)
    key = E.inject_engine(eng, "inject:trajectory")
    try:
        cfg = C.load_config(overrides={"model.scheduler.num_inference_timesteps": STEPS, "model.denoiser.params.num_layers": 3,
                                       "model.motion_vae.params.num_layers": 3})
        enc = SyntheticTextEncoder()

        class Modular(MLD):
            fused = property(lambda self: False)

        model = (MLD if fused else Modular)(cfg, HipDataModule(cfg, engine_key=key), text_encoder=enc, engine_key=key).eval()
        assert model.fused == fused
        texts, lengths = ["a man kicks with his left leg.", "a person walks backward slowly."], [24, 17]
        lat0 = torch.from_numpy(syn.make_batch(2, lengths).init_latents)
        emb = enc([""] * 2 + texts)
        tr = model._diffusion_reverse_tsne(emb, lengths, init_latents=lat0)
        assert tuple(tr.shape) == (STEPS, 2, 256)
        ops = O.NumpyOps(f32)
        ref = []
        O.diffusion_reverse(ops, O.to_backend(ops, simlib.text_weights()[0]), emb.numpy(), lat0.numpy(), 7.5, STEPS, 4, trace=ref)
        ref = np.stack([np.asarray(t).reshape(2, 256) for t in ref])
        assert np.abs(tr.numpy() - ref).max() < 2e-4
        z = model._diffusion_reverse(emb, lengths, init_latents=lat0)
        if fused:
            assert np.abs(tr[-1].numpy() - z[0].numpy()).max() < 2e-4
            joints, feats, lat, traj = model.sample(emb, lengths, lat0, return_trajectory=True)
            j0, f0, l0 = model.sample(emb, lengths, lat0)
            assert torch.equal(traj, tr) and torch.equal(traj[-1], lat[:, 0]) and torch.equal(joints, j0) and torch.equal(lat, l0)
            outs = model.sample_many([(emb, lengths)], init_latents=[lat0], return_trajectory=True)
            assert torch.equal(outs[0][3], tr) and torch.equal(outs[0][0], j0)
        else:
            assert torch.equal(tr[-1], z[0])                    # the same loop: the same bits
    finally:
        E._engines.pop(key, None)
        eng.close()
