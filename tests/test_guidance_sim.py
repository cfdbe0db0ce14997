"""Per-request classifier-free-guidance scale (mldhip_sample_many_guided, MLD.forward(guidance_scale=...)) without a GPU: every reverse-loop family on the
functional simulator against the numpy loop of tests/sample_from_ref.py fed one scale per motion, the bit identities (a motion does not see its
neighbours' scales; a call that names none IS mldhip_sample_many_from), the cluster loop's second launch, the action engine, the argument errors and
the module surface.  3 layers, 4 steps; B = 9 as nine one-motion requests: eight motions in the first workgroup / cluster, one alone in the second."""
import numpy as np
import pytest
import torch

from mld_hip import _lib
from mld_hip import synthetic as syn
from oracle import mld_oracle as O

import simlib
from sample_from_ref import NONE, SOURCE, reverse_from_np
from test_sample_from_sim import F9, FIRST, KIND9, SEED, batch9, per_motion_requests
from test_trajectory_sim import FAMILIES, LENS9, RUNS, STEPS, TOL, weights

f32 = np.float32
ONE_LAUNCH = ("persistent", "cluster4", "cluster8")
HANDLE_G = 7.5
# -1: the handle's own; 0: the unconditional prediction; 1: the conditional one; below, at and above nothing special; one motion alone in the second workgroup
G9 = [-1, 0.0, 1.0, 2.5, 7.5, 4.0, 0.5, 6.0, 3.0]
# the neighbour test: motions 0, 3, 5, 8 get another scale, the others keep theirs
G9_OTHER = [3.5, 0.0, 1.0, 5.5, 7.5, 0.25, 0.5, 6.0, 9.0]
CHANGED = (0, 3, 5, 8)
assert len(LENS9) == 9 and STEPS == 4

_cache = {}


def engine(family, eta=0.0):
    """one engine per (family, eta) for the module: a finalize on the simulator costs as much as a call"""
    if (family, eta) not in _cache:
        prec = 0 if family in ("latency", "strip") else 1
        e = _lib.Engine(lib=simlib.sim_library(), use_graph=0, max_frames=8, num_inference_steps=STEPS, num_layers=3, max_batch=12, precision=prec, eta=eta)
        simlib.load_synthetic_weights(e, num_layers=3)
        for k, v in RUNS[family]:
            e.set_option(k, v)
        _cache[family, eta] = e
    return _cache[family, eta]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for k, v in list(_cache.items()):
        if isinstance(v, _lib.Engine):
            v.close()
            del _cache[k]


def garray(gs):
    """[B, 1, 1] float32 for reverse_from_np: a negative entry is the handle's scale"""
    return np.asarray([HANDLE_G if g is None or g < 0 else g for g in gs], f32).reshape(-1, 1, 1)


def ref9(eta, gs, kinds=None, firsts=None):
    """the numpy loop for the shared batch, one scale per motion; computed once per case"""
    key = ("ref", eta, tuple(gs), kinds is None)
    if key not in _cache:
        b, src = batch9()
        kinds, firsts = kinds or [NONE] * 9, firsts or [0] * 9
        ops = O.NumpyOps(f32)
        _cache[key] = reverse_from_np(O.to_backend(ops, weights()[0]), b.text_emb, b.init_latents,
                                      [(k, f, src[m] if k != NONE else None) for m, (k, f) in enumerate(zip(kinds, firsts))], STEPS, eta,
                                      [(SEED, FIRST + m) for m in range(9)], guidance=garray(gs))
    return _cache[key]


def run9(e, gs, kinds=None, firsts=None, call=None):
    """nine one-motion requests with their scales (None: the key is absent) -> (latents [9, 256], trajectories [n, 9, 256])"""
    b, src = batch9()
    reqs, keys, lat, tr = per_motion_requests(b, kinds or [NONE] * 9, firsts or [0] * 9, src)
    for q, g in zip(reqs, gs):
        if g is not None:
            q["guidance"] = g
    (call or e.sample_many_guided)(reqs, keys)
    return lat.reshape(-1, 256), np.concatenate(tr, 1)


def check_against(ref, lat, traj, firsts, tol, what):
    rtraj, rlat = ref
    for m, f in enumerate(firsts):
        assert np.isnan(traj[:f, m]).all(), (what, m, "rows below the first step keep their NaN fill")
        err = [float(np.abs(traj[s, m] - rtraj[s, m]).max()) for s in range(f, STEPS)]
        assert np.isfinite(traj[f:, m]).all() and max(err) < tol, (what, m, f, err)
    assert np.array_equal(traj[-1], lat)                                        # row n - 1 == latents_out, to the bit
    assert np.abs(lat - rlat).max() < tol, what


# ------------------------------------------------------------------------------------------------ 1. every family, eta = 0 and eta = 0.5
@pytest.mark.parametrize("eta", [0.0, 0.5])
@pytest.mark.parametrize("family", FAMILIES)
def test_every_loop_family_takes_a_scale_per_motion(family, eta):
    e = engine(family, eta)
    lat, traj = run9(e, G9)
    _cache["A", family, eta] = (lat, traj)
    check_against(ref9(eta, G9), lat, traj, [0] * 9, TOL[family], (family, eta))
    if family in ONE_LAUNCH:
        assert e.launch_counts()[0] == 2                     # condition rows + ONE loop launch


# cases 2 and 3: the 12-workgroup cluster form shares the 8-workgroup form's body (and is in case 1): one cluster family here keeps the module quick
FAMILIES_ONE_CLUSTER = [f for f in FAMILIES if f != "cluster4"]


# ------------------------------------------------------------------------------------------------ 2. mixed with sources
@pytest.mark.parametrize("family", FAMILIES_ONE_CLUSTER)
def test_scales_and_sources_in_one_call(family):
    """the mixed first steps of tests/test_sample_from_sim.py (no source, source starts at every step) with the scales of case 1"""
    e = engine(family)
    lat, traj = run9(e, G9, KIND9, F9)
    check_against(ref9(0.0, G9, KIND9, F9), lat, traj, F9, TOL[family], (family, "sources"))
    if family in ONE_LAUNCH:
        assert e.launch_counts()[0] == 2


# ------------------------------------------------------------------------------------------------ 3. neighbours
@pytest.mark.parametrize("family", FAMILIES_ONE_CLUSTER)
def test_a_motion_does_not_see_its_neighbours_scales(family):
    e = engine(family)
    if ("A", family, 0.0) not in _cache:
        _cache["A", family, 0.0] = run9(e, G9)
    lat_a, traj_a = _cache["A", family, 0.0]
    lat, traj = run9(e, G9_OTHER)
    for m in range(9):
        if m in CHANGED:
            assert not np.array_equal(lat[m], lat_a[m]), (family, m)
        else:
            assert np.array_equal(lat[m], lat_a[m]) and np.array_equal(traj[:, m], traj_a[:, m]), (family, m)
    check_against(ref9(0.0, G9_OTHER), lat, traj, [0] * 9, TOL[family], (family, "other scales"))


# ------------------------------------------------------------------------------------------------ 4. no scale anywhere: the from-call
@pytest.mark.parametrize("family", ["persistent", "latency"])
def test_a_call_that_names_no_scale_is_the_from_call(family):
    """no `guidance` key anywhere, then -1 everywhere: latents, trajectories and launch counts of sample_many_from on the same requests -- without sources (there
    the from-call in turn is the trajectory call, on the plain forms) and with them (the from-forms, whose table then carries the handle's scale)"""
    e = engine(family)
    for kinds, firsts in ((None, None), (KIND9, F9)):
        lat_f, traj_f = run9(e, [None] * 9, kinds, firsts, call=e.sample_many_from)
        counts = e.launch_counts()
        for gs in ([None] * 9, [-1] * 9) if kinds is None else ([-1.0] * 9,):
            lat, traj = run9(e, gs, kinds, firsts)
            assert np.array_equal(lat, lat_f) and np.array_equal(traj, traj_f, equal_nan=True) and e.launch_counts() == counts, (family, gs[0])


# ------------------------------------------------------------------------------------------------ 5. the cluster loop's second launch
def test_two_cluster_launches_index_the_scales_by_the_motion_of_the_call():
    """cluster_chunk 8, B = 9: motions 0-7 and motion 8 come from different launches; motions 7 (6.0) and 8 (3.0) have distinct scales, so a second launch
    that indexed the table from 0 would give motion 8 the scale of motion 0"""
    assert G9[7] != G9[8] and G9[8] != HANDLE_G
    e = engine("cluster8")
    e.set_option("cluster_chunk", 8)
    try:
        lat, traj = run9(e, G9)
        assert e.launch_counts()[0] == 3                    # condition rows + two cluster launches
    finally:
        e.set_option("cluster_chunk", 128)
    check_against(ref9(0.0, G9), lat, traj, [0] * 9, TOL["cluster8"], "two launches")


# ------------------------------------------------------------------------------------------------ 6. action engine
def test_action_engine_takes_a_scale_per_request():
    e = simlib.sim_action_engine(max_batch=4, max_frames=8, num_inference_steps=STEPS)
    e.set_option("loop_kernel", 1)
    sdd, _ = simlib.action_weights()
    lat0 = np.random.default_rng(4).standard_normal((3, 1, 256)).astype(f32)
    acts, lens, gs = [3, 0, 11], [8, 5, 2], [2.5, -1, 0.0]
    lat = np.full((3, 1, 256), np.nan, f32)
    tr = [np.full((STEPS, 1, 256), np.nan, f32) for _ in range(3)]
    reqs = [dict(actions=[acts[m]], lengths=[lens[m]], init_latents=np.ascontiguousarray(lat0[m:m + 1]), latents_out=lat[m:m + 1], traj_out=tr[m], guidance=gs[m])
            for m in range(3)]
    e.sample_many_guided(reqs, None)
    ops = O.NumpyOps(f32)
    sd = O.to_backend(ops, sdd)
    cond = np.concatenate([np.zeros(3, np.int64), np.asarray(acts, np.int64)])
    ref = reverse_from_np(sd, None, lat0, [(NONE, 0, None)] * 3, STEPS, guidance=garray(gs),
                          denoise=lambda x2, t: O.denoiser_forward_action(ops, sd, x2, t, cond, 4, 7.5))
    check_against(ref, lat.reshape(3, 256), np.concatenate(tr, 1), [0] * 3, 2e-4, "action")
    e.close()


# ------------------------------------------------------------------------------------------------ 7. errors
def test_guided_error_paths():
    e = engine("latency")
    b = syn.make_batch(2, [4, 4], seed=1)
    te, lat = np.ascontiguousarray(b.text_emb), np.zeros((2, 1, 256), f32)
    base = dict(text_emb=te, init_latents=b.init_latents, lengths=b.lengths, latents_out=lat)

    def refused(eng, reqs):
        with pytest.raises(_lib.MldHipError) as ei:
            eng.sample_many_guided(reqs, None)
        assert ei.value.code == -1, str(ei.value)
        return str(ei.value)

    for bad in (float("nan"), float("inf"), -float("inf")):
        assert "finite" in refused(e, [{**base, "guidance": bad}])
        assert "finite" in refused(e, [{**base, "guidance": 2.0}, {**base, "guidance": bad}])
    # more motions than max_batch (12): a guided call is one chain
    assert "max_batch" in refused(e, [{**base, "guidance": 2.0}] * 7)
    # a handle that does no classifier-free guidance
    e1 = _lib.Engine(lib=simlib.sim_library(), use_graph=0, max_frames=8, num_inference_steps=STEPS, num_layers=3, max_batch=4, guidance_scale=1.0)
    simlib.load_synthetic_weights(e1, num_layers=3)
    assert "guidance_scale" in refused(e1, [{**base, "guidance": 2.0}])
    e1.sample_many_guided([{**base, "guidance": -1}], None)          # names none: the from-call, which serves such a handle
    e1.close()


def test_diffusion_only_variant_refuses_a_scale():
    en = _lib.Engine(lib=simlib.sim_library(), use_graph=0, num_layers=3, max_batch=2, max_frames=8, **simlib.NOVAE_CFG)
    b = syn.make_batch(2, [4, 4], seed=1)
    with pytest.raises(_lib.MldHipError) as ei:
        en.sample_many_guided([dict(text_emb=b.text_emb, init_latents=np.zeros((2, 4, 263), f32), lengths=[4, 4], guidance=2.0)], None)
    assert ei.value.code == -1 and "diffusion-only" in str(ei.value)
    en.close()


def test_symbol_is_added_without_a_version_bump():
    lib = simlib.sim_library()
    assert lib.mldhip_abi_version() == 8 and hasattr(lib, "mldhip_sample_many_guided")
    assert "mldhip_sample_many_guided" in _lib.exported_symbols()


# ------------------------------------------------------------------------------------------------ 8. module surface
def test_mld_forward_with_a_scale_per_prompt():
    """MLD.forward with a per-prompt sequence == MLD.sample_many with the same values per request, to the bit (and within 1e-3 of the numpy loop + the
    oracle's decode); batch["guidance_scale"] is honoured; a float is the whole batch's; None leaves forward what it was, to the bit."""
    from mld_hip import config as C
    from mld_hip import engine as E
    from mld_hip.datamodule import HipDataModule
    from mld_hip.mld import MLD
    from mld_hip.text_encoder import SyntheticTextEncoder

    eng = _lib.Engine(lib=simlib.sim_library(), use_graph=0, max_batch=4, max_frames=40, num_inference_steps=STEPS, num_layers=3)
    key = E.inject_engine(eng, "inject:guidance")
    try:
        cfg = C.load_config(overrides={"model.scheduler.num_inference_timesteps": STEPS, "model.denoiser.params.num_layers": 3,
                                       "model.motion_vae.params.num_layers": 3})
        enc = SyntheticTextEncoder()
        model = MLD(cfg, HipDataModule(cfg, engine_key=key), text_encoder=enc, engine_key=key).eval()
        texts = ["a man kicks with his left leg.", "a person walks backward slowly.", "a person jumps twice."]
        lengths, gs = [24, 17, 9], [2.5, 2.5, 6.0]
        lat0 = torch.from_numpy(syn.make_batch(3, lengths).init_latents)
        batch = {"text": texts, "length": lengths}
        out = model.forward(batch, lat0, guidance_scale=gs)
        assert [tuple(j.shape) for j in out] == [(24, 22, 3), (17, 22, 3), (9, 22, 3)]
        emb = enc([""] * 3 + texts)
        res = model.sample_many([(torch.cat([emb[m:m + 1], emb[3 + m:4 + m]]), [lengths[m]]) for m in range(3)], [lat0[m:m + 1] for m in range(3)], guidance=gs)
        for m, n in enumerate(lengths):
            assert torch.equal(out[m], res[m][0][0, :n].cpu()), m
        out_b = model.forward({**batch, "guidance_scale": gs}, lat0)
        assert all(torch.equal(a, b) for a, b in zip(out, out_b))
        # against the numpy loop and the oracle's decode
        ops = O.NumpyOps(f32)
        sdd, sdv = (O.to_backend(ops, w) for w in simlib.text_weights())
        mean, std = syn.make_mean_std()
        _, z = reverse_from_np(sdd, emb.numpy(), lat0.numpy(), [(NONE, 0, None)] * 3, STEPS, guidance=garray(gs))
        jr = np.asarray(O.feats2joints(ops, O.vae_decode(ops, sdv, z.reshape(3, 1, 256), lengths), mean, std))
        for m, n in enumerate(lengths):
            assert np.abs(out[m].numpy() - jr[m, :n]).max() < 1e-3
        # a float: every prompt at that scale == the sequence of equal values
        out_f, out_s = model.forward(batch, lat0, guidance_scale=2.5), model.forward(batch, lat0, guidance_scale=[2.5] * 3)
        assert all(torch.equal(a, b) for a, b in zip(out_f, out_s))
        assert not torch.equal(out_f[2], out[2]) and torch.equal(out_f[0], out[0])
        # None: today's call (mldhip_sample), to the bit
        j, _, _ = model.sample(emb, lengths, lat0)
        out_n = model.forward(batch, lat0)
        for m, n in enumerate(lengths):
            assert torch.equal(out_n[m], j[m, :n].cpu())
        assert eng.launch_counts()[0] > 0
    finally:
        E._engines.pop(key, None)
        eng.close()
