"""The action-conditioned models on every reverse-loop family and serving entry without a GPU: the code paths of tests/test_gpu_action_edges.py at
simulator sizes, so that their index arithmetic -- the label rows of action_rows_kernel, the label staging paths of engine/serve.hpp, the per-motion
tables of the one-launch loops, the ActorVae's PE rows and its partial last column tile -- is checked against the oracle on the CPU.

simlib.sim_action_engine (3 denoiser layers, 2 ActorVae layers, 12 classes), a batch of 9 motions: one full workgroup / cluster of 8 and one motion alone
in the second; "cluster_chunk" 8 puts that motion into a second cluster launch.  2 steps: the step count must divide 1000, and a cluster launch on the
simulator costs several seconds per step -- two steps carry the loop state from one step to the next, which is what the index arithmetic needs.  References
and tolerances: tests/action_edges_ref.py.  The file takes about two minutes, nearly all of it the 20 cluster launches."""
import numpy as np
import pytest

import action_edges_ref as AE
import config_envelope_ref as R
import simlib
from mld_hip import synthetic as syn
from oracle import mld_oracle as O
from sample_from_ref import NONE, RESUME, SOURCE
from test_trajectory_sim import RUNS

f32 = np.float32
STEPS, BMAX, T = 2, 9, 8
# family -> (precision, options)
# (the 4-group form of the cluster loop: half the workgroups of the 8-group form, half the simulator time; the coalesced case runs the 8-group form)
FAMS = {"latency": (0, RUNS["latency"]), "persistent": (1, RUNS["persistent"]), "cluster": (1, RUNS["cluster4"])}
ONE_LAUNCH = ("persistent", "cluster")
SEED, FIRST = 0x5EED_AC71, 2 ** 31 - 4

_cache = {}


def weights():
    if "w" not in _cache:
        _cache["w"] = simlib.action_weights()
    return _cache["w"]


def engine(family, eta=0.0):
    """one engine per (precision, eta) for the module, switched to the family"""
    prec, opts = FAMS[family]
    if (prec, eta) not in _cache:
        _cache[prec, eta] = simlib.sim_action_engine(precision=prec, max_batch=12, max_frames=40, num_inference_steps=STEPS, eta=eta, max_in_flight=2)
    e = _cache[prec, eta]
    for k, v in opts:
        e.set_option(k, v)
    e.set_option("cluster_chunk", 8 if family == "cluster" else 128)
    return e, prec


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for k, v in list(_cache.items()):
        if hasattr(v, "close"):
            v.close()
            del _cache[k]


@pytest.fixture(scope="module")
def rec():
    return R.Record("MLDHIP_ACTION_EDGES_SIM_JSON")


def outs(rot=0):
    return AE.loop_reference(weights(), STEPS, BMAX, rot, tag="sim")


def nan(*shape):
    return np.full(shape, np.nan, f32)


def launches(family, B):
    """condition rows + one persistent launch, or one cluster launch per 8 motions ("cluster_chunk" 8); the per-launch chain of 3 layers otherwise"""
    return {"latency": R.chain_launches(STEPS, 3), "persistent": 2, "cluster": 1 + (B + 7) // 8}[family]


# ------------------------------------------------------------------ 0. the references
def test_references_are_not_degenerate():
    for rot in (0, 1):
        e32 = AE.sanity(outs(rot))
        print("rot %d: e32 %.3e" % (rot, e32))
    acts, _ = AE.batch(BMAX)
    assert len(set(acts.tolist())) == BMAX and all(a != b for a, b in zip(acts, acts[1:]))
    assert not np.array_equal(outs(0)[0][-1], outs(1)[0][-1])


# ------------------------------------------------------------------ 1. coalesced requests
@pytest.mark.parametrize("family", list(FAMS))
def test_coalesced_requests_with_distinct_labels(rec, family):
    """requests of 2 + 1 + 3 motions, each with its own labels (the host-side gather into one [2 Btot] array); the second and third ask for features with
    ragged lengths: each request against the reference of its motions, padded frames exactly 0"""
    e, prec = engine(family)
    if family == "cluster":
        e.set_option("cluster_groups", 8)
    acts, lat0 = AE.batch(BMAX)
    lens = [8, 5, 3, 8, 1, 7]
    reqs, lo = [], 0
    for i, n in enumerate((2, 1, 3)):
        q = dict(actions=acts[lo:lo + n].tolist(), init_latents=np.ascontiguousarray(lat0[lo:lo + n]), lengths=lens[lo:lo + n], latents_out=nan(n, 1, 256))
        if i:
            q["feats_out"] = nan(n, max(q["lengths"]), 150)
        reqs.append(q)
        lo += n
    e.sample_many(reqs)
    assert e.launch_counts()[0] == launches(family, 6)
    fr, ef = AE.feats_reference(weights(), outs(), range(6), lens, "sim")
    lo = 0
    for i, q in enumerate(reqs):
        n = len(q["lengths"])
        r64, e32 = AE.prefix(outs(), n, lo=lo)
        rec.rule("sim coalesced, %s, request %d latents" % (family, i), q["latents_out"][:, 0], r64, e32, prec)
        if i:
            f, tm = q["feats_out"], max(q["lengths"])
            rec.rule("sim coalesced, %s, request %d feats" % (family, i), f, fr[lo:lo + n, :tm], ef, prec)
            for m, ln in enumerate(q["lengths"]):
                assert np.all(f[m, ln:] == 0), (family, i, m)
        lo += n
    assert e.numeric_status()["nonfinite_values"] == 0
    assert not rec.failures()


# ------------------------------------------------------------------ 2. labels select rows
@pytest.mark.parametrize("family", list(FAMS))
def test_labels_select_rows(rec, family):
    """9 motions through mldhip_sample_action (stage_actions on the caller's stream; the cluster loop in two launches), then the same start latents with every
    label rotated by one class: every motion moves by more than 100 x its e32, and the result is the reference's of the rotated labels -- a label read from
    the wrong half or at the wrong offset gives some motion its neighbour's row, or the null row"""
    e, prec = engine(family)
    got = {}
    for rot in (0, 1):
        acts, lat0 = AE.batch(BMAX, rot)
        lat = nan(BMAX, 1, 256)
        e.sample_action(acts.tolist(), lat0, [T] * BMAX, lat)
        assert e.launch_counts()[0] == launches(family, BMAX)
        r64, e32 = AE.prefix(outs(rot), BMAX)
        rec.rule("sim labels, %s, rotated by %d" % (family, rot), lat[:, 0], r64, e32, prec)
        got[rot] = lat[:, 0]
    for m in range(BMAX):
        _, e32 = AE.prefix(outs(0), 1, lo=m)
        assert np.abs(got[1][m] - got[0][m]).max() > 100 * e32, (family, m)
    assert not rec.failures()


# ------------------------------------------------------------------ 3. trajectories, sources, guidance on the one-launch loops
def _traj_call(family):
    """the plain 9-motion call with a trajectory, once per family: (latents [9, 256], trajectory [STEPS, 9, 256], reverse-loop launches)"""
    if ("traj", family) not in _cache:
        e, _ = engine(family)
        acts, lat0 = AE.batch(BMAX)
        lat, traj = nan(BMAX, 1, 256), nan(STEPS, BMAX, 256)
        e.sample_many_traj([dict(actions=acts.tolist(), init_latents=lat0, lengths=[T] * BMAX, latents_out=lat, traj_out=traj)], None)
        _cache["traj", family] = (lat[:, 0], traj, e.launch_counts()[0])
    return _cache["traj", family]


@pytest.mark.parametrize("family", ONE_LAUNCH)
def test_trajectory_of_a_one_launch_loop(rec, family):
    lat, traj, n = _traj_call(family)
    assert n == launches(family, BMAX)
    for s in range(STEPS):
        r64, e32 = AE.prefix(outs(), BMAX, step=s)
        rec.rule("sim trajectory, %s, step %d" % (family, s), traj[s], r64, e32, FAMS[family][0])
    assert np.array_equal(traj[-1], lat)
    assert not rec.failures()


@pytest.mark.parametrize("family", ONE_LAUNCH)
def test_sources_and_guidance_on_a_one_launch_loop(rec, family):
    """one mldhip_sample_many_guided call of four requests: a clean source at first_step 1 under g = 0 (motions 0-1), no source under g = 1 (2-3) and g = 3
    (4-5), and motions 6-8 resumed at step 1 from row 0 of the trajectory of the plain call, without init_latents, under -1 (the handle's 7.5) -- the
    resumed motions equal the uninterrupted run to the bit"""
    lat_a, traj_a, _ = _traj_call(family)
    e, prec = engine(family)
    acts, lat0 = AE.batch(BMAX)
    src = (syn._rng(142, "simsrc").standard_normal((2, 1, 256)) * 0.7).astype(f32)
    resume = np.ascontiguousarray(traj_a[0, 6:9]).reshape(3, 1, 256)
    sizes, gs = (2, 2, 2, 3), (0.0, 1.0, 3.0, -1.0)
    extras = (dict(src_latents=src, first_step=1), {}, {}, dict(src_latents=resume, first_step=1, noised=1))
    reqs, lo = [], 0
    for i, (n, g, extra) in enumerate(zip(sizes, gs, extras)):
        q = dict(actions=acts[lo:lo + n].tolist(), lengths=[T] * n, latents_out=nan(n, 1, 256), traj_out=nan(STEPS, n, 256), guidance=g, **extra)
        if i != 3:
            q["init_latents"] = np.ascontiguousarray(lat0[lo:lo + n])
        reqs.append(q)
        lo += n
    e.sample_many_guided(reqs, None)
    assert e.launch_counts()[0] == launches(family, BMAX)
    starts = [(SOURCE, 1, src[m]) for m in range(2)] + [(NONE, 0, None)] * 4 + [(RESUME, 1, resume[m]) for m in range(3)]
    per_motion = [g for n, g in zip(sizes, gs) for _ in range(n)]
    rtraj, rlat = AE.numpy_loop(weights(), acts, lat0, STEPS, starts, gs=per_motion)
    lat = np.concatenate([q["latents_out"][:, 0] for q in reqs])
    traj = np.concatenate([q["traj_out"] for q in reqs], 1)
    for m, (_, f, _) in enumerate(starts):
        assert np.isnan(traj[:f, m]).all() and np.isfinite(traj[f:, m]).all(), (family, m)
    rec.bound("sim sources and guidance, %s, latents" % family, lat, rlat, AE.ETA_TOL)
    rec.bound("sim sources and guidance, %s, written rows" % family, np.nan_to_num(traj), np.nan_to_num(rtraj), AE.ETA_TOL)
    assert np.array_equal(traj[-1], lat)
    assert np.array_equal(lat[6:9], lat_a[6:9]) and np.array_equal(traj[1:, 6:9], traj_a[1:, 6:9])
    # the bound can tell the scales apart: g = 1 and g = 3 end further from the handle's 7.5 than it allows
    assert np.abs(lat[2:4] - lat_a[2:4]).max() > AE.ETA_TOL and np.abs(lat[4:6] - lat_a[4:6]).max() > AE.ETA_TOL
    assert not rec.failures()


# ------------------------------------------------------------------ 4. stochastic DDIM
@pytest.mark.parametrize("family", list(FAMS))
def test_seeded_call(rec, family):
    """eta 0.5, two requests whose keys continue each other at first_index 2^31 - 4: the index crosses 2^31 inside the call"""
    e, _ = engine(family, 0.5)
    acts, lat0 = AE.batch(BMAX)
    reqs = [dict(actions=acts[s].tolist(), init_latents=np.ascontiguousarray(lat0[s]), lengths=[T] * (s.stop - s.start), latents_out=nan(s.stop - s.start, 1, 256))
            for s in (slice(0, 5), slice(5, 9))]
    e.sample_many_seeded(reqs, [(SEED, FIRST), (SEED, FIRST + 5)])
    assert e.launch_counts()[0] == launches(family, BMAX)
    _, rlat = AE.numpy_loop(weights(), acts, lat0, STEPS, eta=0.5, keys_per_motion=[(SEED, FIRST + m) for m in range(BMAX)], tag="sim eta")
    rec.bound("sim seeded, %s" % family, np.concatenate([q["latents_out"][:, 0] for q in reqs]), rlat, AE.ETA_TOL)
    assert not rec.failures()


# ------------------------------------------------------------------ 5. pipelined issue
def test_pipelined_requests_with_permuted_labels():
    """"many_pipeline" 1 (eager issue on the simulator: two contexts alternate, stage_actions per request): three requests of two motions with the same start
    latents and lengths and different labels, all asking for features, each bit-identical to its own sample_action call; then the call again with the labels
    permuted between the requests -- the third request reuses the first one's context: every request gives what its labels gave alone"""
    e, _ = engine("cluster")
    e.set_option("cluster_chunk", 128)
    acts, lat0 = AE.batch(BMAX)
    x0, lens = np.ascontiguousarray(lat0[:2]), [7, 4]
    labels = [acts[0:2].tolist(), acts[2:4].tolist(), acts[4:6].tolist()]
    try:
        solo = []
        for a in labels:
            lat, feats = nan(2, 1, 256), nan(2, 7, 150)
            e.sample_action(a, x0, lens, lat, feats)
            assert np.isfinite(lat).all() and np.all(feats[1, 4:] == 0)
            solo.append((lat, feats))
        assert not np.array_equal(solo[0][0], solo[1][0]) and not np.array_equal(solo[0][0], solo[2][0])
        e.set_option("many_pipeline", 1)
        for order in ((0, 1, 2), (2, 0, 1)):
            reqs = [dict(actions=labels[k], init_latents=x0, lengths=lens, latents_out=nan(2, 1, 256), feats_out=nan(2, 7, 150)) for k in order]
            e.sample_many(reqs)
            assert e.launch_counts()[0] == 2                    # the last request's own loop, not a 6-motion chain
            for q, k in zip(reqs, order):
                assert np.array_equal(q["latents_out"], solo[k][0]) and np.array_equal(q["feats_out"], solo[k][1]), (order, k)
        assert e.numeric_status()["nonfinite_values"] == 0
    finally:
        e.set_option("many_pipeline", 0)


# ------------------------------------------------------------------ 6. ActorVae
def _ragged(n):
    return max(1, n * 5 // 8)


@pytest.mark.parametrize("family", ["latency", "persistent"], ids=["f32", "f16x3"])
def test_actor_vae_frame_lengths(rec, family):
    """ActorVae decode at T = 1, 16, 17, 33 and encode at T = 14, 15, 30 (16, 17, 32 tokens), a full motion next to a ragged one, against fp64: the sinusoidal PE
    rows, the ping-pong of the plain stack, the N = 150 final GEMM with its padded rows, the encoder's K = 150 padded to 160"""
    e, prec = engine(family)
    w = weights()
    for n in (1, 16, 17, 33):
        lens = [n, _ragged(n)]
        z = syn._rng(143, "simdec%d" % n).standard_normal((2, 1, 256)).astype(f32)
        key = ("dec", n)
        if key not in _cache:
            _cache[key] = R.reference64(lambda ops, W: O.actor_decode(ops, W(w[1]), ops.asarray(z), lens))[0]
        feats = nan(2, n, 150)
        e.vae_decode(z, lens, feats)
        rec.bound("sim actor decode, %s, T %d" % (R.MODE[prec], n), feats, _cache[key], R.OP_TOL)
        assert np.all(feats[1, lens[1]:] == 0)
    for n in (14, 15, 30):
        lens = [n, _ragged(n)]
        g = syn._rng(144, "simenc%d" % n)
        fe = g.standard_normal((2, n, 150)).astype(f32)
        fe[1, lens[1]:] = 0
        eps = g.standard_normal((2, 1, 256)).astype(f32)
        key = ("enc", n)
        if key not in _cache:
            _cache[key] = R.reference64(lambda ops, W: O.actor_encode(ops, W(w[1]), ops.asarray(fe), lens)[1:])
        mr, lvr = _cache[key]
        lat, mu, lv = nan(2, 1, 256), nan(2, 1, 256), nan(2, 1, 256)
        e.vae_encode(fe, lens, n, eps, lat, mu, lv)
        rec.bound("sim actor encode, %s, T %d mu" % (R.MODE[prec], n), mu, mr, R.OP_TOL)
        rec.bound("sim actor encode, %s, T %d logvar" % (R.MODE[prec], n), lv, lvr, R.OP_TOL)
        rec.bound("sim actor encode, %s, T %d latent" % (R.MODE[prec], n), lat, mu.astype(np.float64) + np.sqrt(np.exp(lv.astype(np.float64))) * eps, R.OP_TOL)
    assert not rec.failures()
