"""Start the reverse loop from a source latent at a chosen step (mldhip_sample_many_from, MLD.edit) without a GPU: every reverse-loop family on the
functional simulator against a numpy loop with per-motion starts (tests/sample_from_ref.py), the bit identities that hold inside the from-forms, the
cluster loop's two-launch, injected-fault and stale-flag paths on a from-launch, the action engine, the argument errors and the module surface."""
import numpy as np
import pytest
import torch

from mld_hip import _lib
from mld_hip import synthetic as syn
from oracle import mld_oracle as O

import simlib
from sample_from_ref import NONE, RESUME, SOURCE, reverse_from_np
from test_trajectory_sim import FAMILIES, LENS9, RUNS, STEPS, TOL, weights

f32 = np.float32
SEED, FIRST = 0x0BAD_5EED_CAFE, 3
# first steps mixed inside the first workgroup / cluster (no source, every step 0 .. n - 1 as a source start), one motion alone in the second
KIND9 = [NONE, SOURCE, SOURCE, SOURCE, SOURCE, SOURCE, SOURCE, SOURCE, SOURCE]
F9 = [0, 3, 3, 1, 2, 0, 1, 3, 2]
assert STEPS == 4

_cache = {}


def batch9():
    if "b9" not in _cache:
        b = syn.make_batch(9, LENS9, seed=9)
        src = np.random.default_rng(31).standard_normal((9, 1, 256)).astype(f32) * f32(0.7)      # "clean" latents of other motions
        _cache["b9"] = (b, src)
    return _cache["b9"]


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


def ref9(eta, kinds=None, firsts=None, srcs=None):
    """the numpy loop for the shared batch; cached for the shared mixed-start case"""
    shared = kinds is None
    if shared and ("ref", eta) in _cache:
        return _cache["ref", eta]
    b, src = batch9()
    kinds, firsts = kinds or KIND9, firsts or F9
    srcs = srcs if srcs is not None else src
    ops = O.NumpyOps(f32)
    out = reverse_from_np(O.to_backend(ops, weights()[0]), b.text_emb, b.init_latents, [(k, f, srcs[m]) for m, (k, f) in enumerate(zip(kinds, firsts))], STEPS, eta,
                          [(SEED, FIRST + m) for m in range(9)])
    if shared:
        _cache["ref", eta] = out
    return out


def per_motion_requests(b, kinds, firsts, srcs, motions=range(9), traj=True, joints=False):
    """one request per motion (a start is a property of a request): -> (requests, keys, latents [len, 1, 256], trajectories [n, len, 256])"""
    motions = list(motions)
    lat = np.full((len(motions), 1, 256), np.nan, f32)
    tr = [np.full((STEPS, 1, 256), np.nan, f32) for _ in motions]
    reqs, keys = [], []
    for i, m in enumerate(motions):
        q = dict(text_emb=np.ascontiguousarray(np.stack([b.text_emb[m], b.text_emb[9 + m]])), lengths=[b.lengths[m]], latents_out=lat[i:i + 1])
        if kinds[m] != RESUME:
            q["init_latents"] = np.ascontiguousarray(b.init_latents[m:m + 1])
        if kinds[m] != NONE:
            q.update(src_latents=np.ascontiguousarray(srcs[m:m + 1]), first_step=firsts[m], noised=int(kinds[m] == RESUME))
        if traj:
            q["traj_out"] = tr[i]
        reqs.append(q)
        keys.append((SEED, FIRST + m))
    return reqs, keys, lat, tr


def run9(e, kinds=KIND9, firsts=F9, srcs=None, motions=range(9)):
    b, src = batch9()
    reqs, keys, lat, tr = per_motion_requests(b, kinds, firsts, src if srcs is None else srcs, motions)
    e.sample_many_from(reqs, keys)
    return lat.reshape(-1, 256), np.concatenate(tr, 1)


def check_against(ref, lat, traj, firsts, tol, what):
    rtraj, rlat = ref
    for m, f in enumerate(firsts):
        assert np.isnan(traj[:f, m]).all(), (what, m, "rows below the first step are left untouched")
        err = [float(np.abs(traj[s, m] - rtraj[s, m]).max()) for s in range(f, STEPS)]
        assert np.isfinite(traj[f:, m]).all() and max(err) < tol, (what, m, f, err)
    assert np.array_equal(traj[-1], lat)                                        # row n - 1 == latents_out, to the bit
    assert np.abs(lat - rlat).max() < tol, what


# ------------------------------------------------------------------------------------------------ every family, eta = 0 and eta = 0.5
@pytest.mark.parametrize("eta", [0.0, 0.5])
@pytest.mark.parametrize("family", FAMILIES)
def test_every_loop_family_starts_from_sources(family, eta):
    """B = 9 as nine one-motion requests: first steps [0 (no source), 3, 3, 1, 2, 0 (source), 1, 3 | 2] -- source starts at f = 0, 1 and n - 1 among them --
    against the numpy loop: final latents and every written trajectory row; untouched rows keep their NaN fill; row n - 1 == latents_out."""
    e = engine(family, eta)
    lat, traj = run9(e)
    _cache["A", family, eta] = (lat, traj)
    check_against(ref9(eta), lat, traj, F9, TOL[family], (family, eta))
    if family in ("persistent", "cluster4", "cluster8"):
        assert e.launch_counts()[0] == 2                     # condition rows + ONE loop launch


@pytest.mark.parametrize("eta", [0.0, 0.5])
@pytest.mark.parametrize("family", FAMILIES)
def test_resume_reproduces_the_call_it_was_cut_from(family, eta):
    """Resume starts, and the first bit identity: every motion that has a row f in the mixed call's trajectory resumes at f' = f + 1 from that row
    (noised = 1, no init_latents); the others start as before.  Rows f' .. n - 1 and the latents are those of the mixed call, to the bit -- and so
    within the family's tolerance of the numpy loop resumed from the same rows."""
    e = engine(family, eta)
    if ("A", family, eta) not in _cache:
        _cache["A", family, eta] = run9(e)
    lat_a, traj_a = _cache["A", family, eta]
    b, src = batch9()
    kinds = [RESUME if f + 1 < STEPS else k for k, f in zip(KIND9, F9)]
    firsts = [f + 1 if f + 1 < STEPS else f for f in F9]
    srcs = np.stack([traj_a[f, m][None] if f + 1 < STEPS else src[m] for m, f in enumerate(F9)]).astype(f32)
    lat, traj = run9(e, kinds, firsts, srcs)
    for m, f in enumerate(firsts):
        assert np.isnan(traj[:f, m]).all() and np.array_equal(traj[f:, m], traj_a[f:, m]), (family, eta, m, f)
    assert np.array_equal(lat, lat_a)
    check_against(ref9(eta, kinds, firsts, srcs), lat, traj, firsts, TOL[family], (family, eta, "resume"))


@pytest.mark.parametrize("family", FAMILIES)
def test_neighbours_do_not_matter_and_a_late_workgroup_skips(family):
    """The second bit identity, and a workgroup / cluster whose motions ALL start late (its step loop begins at step 2): motions 1, 2, 7 keep their start
    (a source at f = 3), the five others of the first workgroup move to f = 2 or 3 and the second workgroup's motion is dropped from the call.
    Motions 1, 2, 7: the bits of the mixed call; everything against the numpy loop."""
    e = engine(family)
    if ("A", family, 0.0) not in _cache:
        _cache["A", family, 0.0] = run9(e)
    lat_a, _ = _cache["A", family, 0.0]
    kinds = [SOURCE] * 9
    firsts = [2, 3, 3, 2, 2, 3, 2, 3, 2]
    lat, traj = run9(e, kinds, firsts, motions=range(8))
    for m in (1, 2, 7):
        assert np.array_equal(lat[m], lat_a[m]), (family, m)
    rtraj, rlat = ref9(0.0, kinds, firsts)
    check_against((rtraj[:, :8], rlat[:8]), lat, traj, firsts[:8], TOL[family], (family, "late"))


@pytest.mark.parametrize("family", ["persistent", "latency", "cluster8"])
def test_two_requests_straddle_a_workgroup(family):
    """A call of two requests, of 5 and 4 motions: the first from a source at f = 1, the second at f = 2 with a trajectory; motions 5-7 share the
    first workgroup with request 0, motion 8 sits in the second."""
    e = engine(family)
    b, src = batch9()
    te = lambda s: np.ascontiguousarray(np.concatenate([b.text_emb[:9][s], b.text_emb[9:][s]], 0))
    lat_a, lat_b = np.full((5, 1, 256), np.nan, f32), np.full((4, 1, 256), np.nan, f32)
    traj_b = np.full((STEPS, 4, 256), np.nan, f32)
    sa, sb = slice(0, 5), slice(5, 9)
    e.sample_many_from([dict(text_emb=te(sa), init_latents=np.ascontiguousarray(b.init_latents[sa]), lengths=b.lengths[sa], latents_out=lat_a,
                             src_latents=np.ascontiguousarray(src[sa]), first_step=1),
                        dict(text_emb=te(sb), init_latents=np.ascontiguousarray(b.init_latents[sb]), lengths=b.lengths[sb], latents_out=lat_b,
                             src_latents=np.ascontiguousarray(src[sb]), first_step=2, traj_out=traj_b)], [(SEED, FIRST), (SEED, FIRST + 5)])
    firsts = [1] * 5 + [2] * 4
    rtraj, rlat = ref9(0.0, [SOURCE] * 9, firsts)
    assert np.abs(lat_a.reshape(5, 256) - rlat[:5]).max() < TOL[family]
    check_against((rtraj[:, 5:], rlat[5:]), lat_b.reshape(4, 256), traj_b, firsts[5:], TOL[family], (family, "two requests"))


# ------------------------------------------------------------------------------------------------ no source: the trajectory call
def test_starts_without_a_source_are_the_trajectory_call():
    e = engine("persistent")
    b, _ = batch9()
    te = np.ascontiguousarray(b.text_emb)
    out = []
    for call in (e.sample_many_from, e.sample_many_traj):
        lat, traj = np.full((9, 1, 256), np.nan, f32), np.full((STEPS, 9, 256), np.nan, f32)
        call([dict(text_emb=te, init_latents=b.init_latents, lengths=b.lengths, latents_out=lat, traj_out=traj)], None)
        out.append((lat, traj))
    assert np.isfinite(out[0][1]).all() and np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


# ------------------------------------------------------------------------------------------------ cluster loop: two launches, bounded waits, entry check
def test_two_cluster_launches_from_sources():
    """cluster_chunk 8, B = 9: motions 0-7 and motion 8 come from different launches; the start table is indexed by the motion of the CALL."""
    e = engine("cluster8")
    e.set_option("cluster_chunk", 8)
    try:
        lat, traj = run9(e)
        assert e.launch_counts()[0] == 3                    # condition rows + two cluster launches
    finally:
        e.set_option("cluster_chunk", 128)
    check_against(ref9(0.0), lat, traj, F9, TOL["cluster8"], "two launches")


@pytest.mark.parametrize("groups", [4, 8])
def test_cluster_from_launch_keeps_its_bounded_waits_and_entry_check(groups):
    """A from-launch whose cluster starts at step 2 counts its flag epochs from there: the muted member ("cluster_inject") is missed at the FIRST
    executed step and the wait runs into its bound; a stale epoch in a polled word ("cluster_stale") fails the entry check.  Either way the call
    returns, the latents and trajectory row n - 1 are NaN, the non-finite counter sees them and the handle leaves the cluster loop."""
    b, src = batch9()
    for option, value in (("cluster_inject", 1 + (5 if groups == 8 else 2)), ("cluster_stale", 1)):
        prec = 1
        e = _lib.Engine(lib=simlib.sim_library(), use_graph=0, max_frames=8, num_inference_steps=STEPS, num_layers=3, max_batch=8, precision=prec)
        simlib.load_synthetic_weights(e, num_layers=3)
        e.set_option("loop_kernel", 4)
        e.set_option("cluster_groups", groups)
        e.set_option(option, value)
        reqs, keys, lat, tr = per_motion_requests(b, [SOURCE] * 9, [2, 3, 3, 2, 2, 3, 2, 3, 2], src, range(8))
        e.sample_many_from(reqs, None)
        traj = np.concatenate(tr, 1)
        assert e.launch_counts()[0] == 2 and np.isnan(lat).all() and np.isnan(traj[-1]).all(), option
        ns = e.numeric_status()
        assert ns["nonfinite_values"] == 8 * 256 and ns["cluster_loop"] == 2, (option, ns)
        e.close()


# ------------------------------------------------------------------------------------------------ action engine
def test_action_engine_from_sources():
    """B = 3 on the action-conditioned engine (latency family): a source at f = 2, no source, a resume at f = 1."""
    e = simlib.sim_action_engine(max_batch=4, max_frames=8, num_inference_steps=STEPS)
    e.set_option("loop_kernel", 1)
    sdd, _ = simlib.action_weights()
    g = np.random.default_rng(4)
    lat0 = g.standard_normal((3, 1, 256)).astype(f32)
    src = g.standard_normal((3, 1, 256)).astype(f32) * f32(0.7)
    acts, lens = [3, 0, 11], [8, 5, 2]
    starts = [(SOURCE, 2, src[0]), (NONE, 0, None), (RESUME, 1, src[2])]
    lat = np.full((3, 1, 256), np.nan, f32)
    tr = [np.full((STEPS, 1, 256), np.nan, f32) for _ in range(3)]
    reqs = []
    for m, (k, f, s) in enumerate(starts):
        q = dict(actions=[acts[m]], lengths=[lens[m]], latents_out=lat[m:m + 1], traj_out=tr[m])
        if k != RESUME:
            q["init_latents"] = np.ascontiguousarray(lat0[m:m + 1])
        if k != NONE:
            q.update(src_latents=np.ascontiguousarray(s[None]), first_step=f, noised=int(k == RESUME))
        reqs.append(q)
    e.sample_many_from(reqs, None)
    ops = O.NumpyOps(f32)
    sd = O.to_backend(ops, sdd)
    cond = np.concatenate([np.zeros(3, np.int64), np.asarray(acts, np.int64)])
    ref = reverse_from_np(sd, None, lat0, starts, STEPS, denoise=lambda x2, t: O.denoiser_forward_action(ops, sd, x2, t, cond, 4, 7.5))
    check_against(ref, lat.reshape(3, 256), np.concatenate(tr, 1), [2, 0, 1], 2e-4, "action")
    e.close()


# ------------------------------------------------------------------------------------------------ error paths
def test_from_error_paths():
    e = engine("latency")
    b = syn.make_batch(2, [4, 4], seed=1)
    te, lat, src = np.ascontiguousarray(b.text_emb), np.zeros((2, 1, 256), f32), np.zeros((2, 1, 256), f32)
    base = dict(text_emb=te, init_latents=b.init_latents, lengths=b.lengths, latents_out=lat)

    def refused(**kw):
        q = {**base, **kw}
        if q.get("init_latents") is None:
            q.pop("init_latents")
        with pytest.raises(_lib.MldHipError) as ei:
            e.sample_many_from([q], None)
        assert ei.value.code == -1, str(ei.value)
        return str(ei.value)

    assert "first_step" in refused(src_latents=src, first_step=STEPS)
    assert "first_step" in refused(src_latents=src, first_step=-1)
    assert "without a source" in refused(first_step=1)
    assert "noised" in refused(src_latents=src, first_step=1, noised=2)
    assert "null input" in refused(src_latents=src, first_step=1, init_latents=None)                 # a source start mixes with init_latents
    flat = np.zeros(2 * 256 + 8, f32)
    off = 1 + (-(flat.ctypes.data // 4) % 4)                  # first float whose address is 4 mod 16
    assert "aligned" in refused(src_latents=flat[off:off + 512].reshape(2, 1, 256), first_step=1)
    # ... and a resumed request needs none
    e.sample_many_from([{k: v for k, v in {**base, "src_latents": src, "first_step": 1, "noised": 1}.items() if k != "init_latents"}], None)
    ee = _lib.Engine(lib=simlib.sim_library(), use_graph=0, max_frames=8, num_inference_steps=STEPS, num_layers=3, max_batch=4, eta=0.5)
    simlib.load_synthetic_weights(ee, num_layers=3)
    with pytest.raises(_lib.MldHipError) as ei:                # eta > 0: the keys are required, as for the trajectory call
        ee.sample_many_from([{**base, "src_latents": src, "first_step": 1}], None)
    assert ei.value.code == -1 and "keys" in str(ei.value)
    ee.close()


def test_diffusion_only_variant_refuses_a_start():
    en = _lib.Engine(lib=simlib.sim_library(), use_graph=0, num_layers=3, max_batch=2, max_frames=8, **simlib.NOVAE_CFG)
    b = syn.make_batch(2, [4, 4], seed=1)
    with pytest.raises(_lib.MldHipError) as ei:
        en.sample_many_from([dict(text_emb=b.text_emb, init_latents=np.zeros((2, 4, 263), f32), lengths=[4, 4], src_latents=np.zeros((2, 1, 256), f32),
                                  first_step=1)], None)
    assert ei.value.code == -1 and "diffusion-only" in str(ei.value)
    en.close()


def test_symbol_is_added_without_a_version_bump():
    lib = simlib.sim_library()
    assert lib.mldhip_abi_version() == 8 and hasattr(lib, "mldhip_sample_many_from")
    assert "mldhip_sample_many_from" in _lib.exported_symbols()


# ------------------------------------------------------------------------------------------------ module surface
def test_mld_edit():
    """MLD.edit: encode (the distribution's mean) -> noised to step n - int(n * strength) -> denoised under the prompts -> joints, against
    O.vae_encode, the numpy loop and O.vae_decode + O.feats2joints; strength 0 is the reconstruction."""
    from mld_hip import config as C
    from mld_hip import engine as E
    from mld_hip.datamodule import HipDataModule
    from mld_hip.mld import MLD
    from mld_hip.text_encoder import SyntheticTextEncoder

    eng = _lib.Engine(lib=simlib.sim_library(), use_graph=0, max_batch=4, max_frames=40, num_inference_steps=STEPS, num_layers=3)
    key = E.inject_engine(eng, "inject:sample_from")
    try:
        cfg = C.load_config(overrides={"model.scheduler.num_inference_timesteps": STEPS, "model.denoiser.params.num_layers": 3,
                                       "model.motion_vae.params.num_layers": 3})
        enc = SyntheticTextEncoder()
        model = MLD(cfg, HipDataModule(cfg, engine_key=key), text_encoder=enc, engine_key=key).eval()
        texts, lengths = ["a man kicks with his left leg.", "a person walks backward slowly."], [24, 17]
        g = torch.Generator().manual_seed(5)
        motion = torch.randn(2, 24, 263, generator=g) * 0.3
        motion[1, 17:] = 0
        lat0 = torch.from_numpy(syn.make_batch(2, lengths).init_latents)
        out = model.edit({"motion": motion, "text": texts, "length": lengths}, 0.5, init_latents=lat0)
        assert [tuple(j.shape) for j in out] == [(24, 22, 3), (17, 22, 3)]
        ops = O.NumpyOps(f32)
        sdd, sdv = (O.to_backend(ops, w) for w in simlib.text_weights())
        _, mu, _ = O.vae_encode(ops, sdv, motion.numpy(), lengths, np.zeros((2, 1, 256), f32))
        mu = np.asarray(mu, f32).reshape(2, 1, 256)
        emb = enc([""] * 2 + texts).numpy()
        mean, std = syn.make_mean_std()
        f = STEPS - int(STEPS * 0.5)
        _, z = reverse_from_np(sdd, emb, lat0.numpy(), [(SOURCE, f, mu[m]) for m in range(2)], STEPS)
        jr = np.asarray(O.feats2joints(ops, O.vae_decode(ops, sdv, z.reshape(2, 1, 256), lengths), mean, std))
        for m, n in enumerate(lengths):
            assert np.abs(out[m].numpy() - jr[m, :n]).max() < 1e-3
        # strength 0: first_step == n, no loop -- the reconstruction
        rec = model.edit({"motion": motion, "text": texts, "length": lengths}, 0.0)
        j0 = np.asarray(O.feats2joints(ops, O.vae_decode(ops, sdv, mu, lengths), mean, std))
        for m, n in enumerate(lengths):
            assert np.abs(rec[m].numpy() - j0[m, :n]).max() < 1e-3
        # the keyword surface of MLD.sample: a resume from the source-start call's own trajectory gives its latents back, to the bit
        src = torch.from_numpy(mu)
        temb = torch.from_numpy(emb)
        _, _, lat, traj = model.sample(temb, lengths, lat0, return_trajectory=True, src_latents=src, first_step=1)
        _, _, lat2 = model.sample(temb, lengths, None, src_latents=traj[1].reshape(2, 1, 256), first_step=2, noised=True)
        assert torch.equal(lat, lat2)
    finally:
        E._engines.pop(key, None)
        eng.close()
