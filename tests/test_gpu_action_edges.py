"""The action-conditioned models (HumanAct12 / UESTC: MLDHIP_COND_ACTION, ActorVae, time embedding of width 256) on the MI355X against the float64 oracle:
every reverse-loop family at its batch-size edges, labels that really select their embedding rows, every serving entry (mldhip_sample_many, _seeded, _traj,
_from, _guided, "many_pipeline" 1) on every family, the host-array contract of include/mldhip.h, and the ActorVae over the frame lengths of
tests/test_gpu_shape_edges.py.

5 denoiser layers, 3 ActorVae layers, 12 classes, nfeats 150, guidance 7.5.  Latents-only calls run on max_frames 16 handles with every length 8, 4 steps up
to 257 motions and 2 above; the reference of a call is a prefix of one batch's (tests/action_edges_ref.py), a rotated-label call that of the same batch
under rotated labels.  Tolerances are the project's own: config_envelope_ref.Record.rule (4 x e32 on an F32 handle, 16 x e32 on an F16X3 one) for eta = 0
latents, trajectories and sampled features, OP_TOL for single decode / encode calls against fp64, batch_edges_ref.ETA_TOL for stochastic, source and
guided calls against the float32 numpy loop.  Output buffers start NaN-filled; every test ends after TIME_LIMIT_S at the latest.  With
MLDHIP_ACTION_EDGES_JSON set, every comparison is written there (profiles/action_edges.json was written that way).

Measured there (277 comparisons): the worst ratio to e32 is 2.03 on an F32 handle (bound 4; persistent loop, 4 steps, B = 1) and 1.26 on an F16X3 one (bound 16;
coalesced call on the persistent loop); the latency kernels stay below 1.04, the throughput kernels below 1.84, the cluster loop below 0.92, every trajectory
step below 1.85, the sampled features of the 288-frame call below 0.86.  Source calls end 1.0e-4, guided calls 8.3e-5 and stochastic calls 1.1e-4 from the numpy
loop (bound 5e-3); ActorVae decode 2.7e-6 and encode 2.9e-6 from fp64 at every frame length (bound 1e-4).  The whole file takes 14 s, 9 of them the references."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import action_edges_ref as AE  # noqa: E402
import config_envelope_ref as R  # noqa: E402
from mld_hip import _lib  # noqa: E402
from mld_hip import synthetic as syn  # noqa: E402
from oracle import mld_oracle as O  # noqa: E402
from sample_from_ref import NONE, RESUME, SOURCE  # noqa: E402
from test_gpu_shape_edges import ENC_TS, TS, _ragged  # noqa: E402

pytestmark = pytest.mark.gpu

TIME_LIMIT_S = 120
BMAX = {4: 257, 2: 2049}          # motions of the reference batch of a step count
PRECS = pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f16x3"])
CHAIN = R.chain_launches(4, AE.DEN_LAYERS)      # one action_rows launch stands where the text projection stood
SEED = 0xAC710_5EED
_cache = {}


@pytest.fixture(autouse=True)
def time_limit():
    """every test of this file ends after TIME_LIMIT_S at the latest, also when it is blocked inside a device synchronisation"""
    faulthandler.dump_traceback_later(TIME_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def rec():
    r = R.Record("MLDHIP_ACTION_EDGES_JSON")
    yield r
    r.dump(what="max |engine - reference| of every case of tests/test_gpu_action_edges.py on an MI355X.  eta = 0 latents, trajectories and sampled features: the "
                "float64 oracle, e32 = the float32 CPU oracle's own error on the same motions, ratio = err / e32, bound by the factor of the handle's precision; "
                "single decode / encode calls: the float64 oracle, absolute bound; stochastic, source and guided calls: the float32 numpy loop, absolute bound")


def _cuda(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _engine(prec, max_batch, steps, options=None, max_frames=AE.MAX_FRAMES, **cfg):
    e = _lib.Engine(device=0, precision=prec, max_batch=max_batch, max_frames=max_frames, num_inference_steps=steps, **{**AE.ENGINE_CFG, **cfg})
    try:
        w = AE.weights()
        e.load_state_dict(w[0], "denoiser.")
        e.load_state_dict(w[1], "vae.")
        e.finalize()
        for k, v in (options or {}).items():
            e.set_option(k, v)
    except Exception:
        e.close()
        raise
    return e


def _status_ok(e, prec):
    ns = e.numeric_status()
    assert ns["nonfinite_values"] == 0, ns
    if prec == 1:
        assert ns["loop_split_ok"] == 1, ns
    return ns


def _cluster_or_skip(e):
    if e.numeric_status()["cluster_loop"] == 3:
        e.close()
        pytest.skip("another process holds the device's cluster lane: this handle runs no cluster launches")


def _outs(steps, rot=0):
    """the reference traces of a step count; rotated labels: the first 17 motions of the 4-step batch alone"""
    return AE.loop_reference(AE.weights(), steps, BMAX[steps], rot, n=None if rot == 0 else 17)


def _call(e, dev, steps, B, rot=0):
    """the call of the first B motions of the step count's batch: (latents [B, 256] as numpy, reverse-loop launches)"""
    acts, lat0 = AE.batch(BMAX[steps], rot)
    lat = _nan(dev, B, 1, 256)
    e.sample_action(acts[:B].tolist(), _cuda(lat0[:B], dev), [AE.LENGTH] * B, lat)
    torch.cuda.synchronize()
    return lat.cpu().numpy()[:, 0], e.launch_counts()[0]


def _rule(rec, name, got, steps, B, prec, rot=0):
    r64, e32 = AE.prefix(_outs(steps, rot), B)
    return rec.rule(name, got, r64, e32, prec)


def _labels_select_rows(e, dev, rec, name, prec, want):
    """17 motions, then the same start latents with every label rotated by one class: every motion moves by more than 100 x its e32 and the result is the
    reference's of the rotated labels -- a label read from the wrong half or offset, which a symmetric batch would hide"""
    got = {}
    for rot in (0, 1):
        got[rot], launches = _call(e, dev, 4, 17, rot)
        assert launches == want, (name, rot, launches)
        _rule(rec, "%s, B 17, labels rotated by %d" % (name, rot), got[rot], 4, 17, prec, rot)
    for m in range(17):
        _, e32 = AE.prefix(_outs(4), 1, lo=m)
        moved = float(np.abs(got[1][m] - got[0][m]).max())
        assert moved > 100 * e32, (name, m, moved, e32)
    return got[0]


# ------------------------------------------------------------------ a. loop families at their edges, b. labels select rows
def test_references_are_not_degenerate():
    for steps in (4, 2):
        assert AE.sanity(_outs(steps)) > 0
    assert AE.sanity(_outs(4, 1)) > 0


@PRECS
def test_latency_kernels(dev, rec, prec):
    """gemm_tile32_kernel behind action_rows_kernel: B = 171, 86, 43, 42 (the 32 | 16-row switches of the out-projection, the skip linear and FFN2), 8, 3 (a
    32-row tile with an empty second half), 1"""
    e = _engine(prec, 171, 4, {"loop_kernel": 1})
    try:
        name = "latency, %s" % R.MODE[prec]
        for B in (171, 86, 43, 42, 8, 3, 1):
            lat, launches = _call(e, dev, 4, B)
            assert launches == CHAIN, (name, B, launches)
            _rule(rec, "%s, B %d" % (name, B), lat, 4, B, prec)
        _labels_select_rows(e, dev, rec, name, prec, CHAIN)
        _status_ok(e, prec)
    finally:
        e.close()
    assert not rec.failures()


def test_throughput_kernels(dev, rec):
    """gemm_strip_kernel + the 32 x 64 staged FFN2 on an F32 max_batch 257 handle: 257, 129, 128, 127 (tile edges of 6 B token rows), 5, 1; at 17 motions the
    result differs in some bit from the latency kernels' on the same handle (the launch counts are equal)"""
    e = _engine(0, 257, 4, {"loop_kernel": 2})
    try:
        for B in (257, 129, 128, 127, 5, 1):
            lat, launches = _call(e, dev, 4, B)
            assert launches == CHAIN, (B, launches)
            _rule(rec, "throughput, f32, B %d" % B, lat, 4, B, 0)
        lat = _labels_select_rows(e, dev, rec, "throughput, f32", 0, CHAIN)
        e.set_option("loop_kernel", 1)
        other, _ = _call(e, dev, 4, 17)
        assert np.isfinite(other).all() and not np.array_equal(lat, other)
        _status_ok(e, 0)
    finally:
        e.close()
    assert not rec.failures()


@PRECS
def test_persistent_loop(dev, rec, prec):
    """den_loop_kernel<false / true> on max_batch 2049 handles: 2049 motions (257 workgroups: a second round, one motion in the last) and 2041 at 2 steps; 17, 9,
    8, 7, 1 at 4 steps.  One launch behind the condition rows; at B = 17 "loop_lean" 0 equals 1 to the bit."""
    for steps, bs in ((2, (2049, 2041)), (4, (17, 9, 8, 7, 1))):
        e = _engine(prec, 2049, steps, {"loop_kernel": 3})
        try:
            name = "persistent, %s" % R.MODE[prec]
            for B in bs:
                lat, launches = _call(e, dev, steps, B)
                assert launches == 2, (name, B, launches)
                _rule(rec, "%s, %d steps, B %d" % (name, steps, B), lat, steps, B, prec)
                if B == 17:
                    e.set_option("loop_lean", 0)
                    full, _ = _call(e, dev, steps, B)
                    e.set_option("loop_lean", 1)
                    assert np.array_equal(full, lat), (name, float(np.abs(full - lat).max()))
            if steps == 4:
                _labels_select_rows(e, dev, rec, name, prec, 2)
            _status_ok(e, prec)
        finally:
            e.close()
    assert not rec.failures()


def test_cluster_loop(dev, rec):
    """den_cluster_kernel<*, 8> up to 64 motions and <*, 4> above on an F16X3 max_batch 256 handle: 256 and 129 (a second launch, full and of one motion), 128,
    65 | 64 (the switch of the form), 9, 1; the 4-group form forced at 9.  One launch per 128 motions behind the condition rows; no launch ran into its wait bound."""
    e = _engine(1, 256, 4, {"loop_kernel": 4})
    _cluster_or_skip(e)
    try:
        for cg, bs in ((0, (256, 129, 128, 65, 64, 9, 1)), (4, (9,))):
            e.set_option("cluster_groups", cg)
            for B in bs:
                lat, launches = _call(e, dev, 4, B)
                assert launches == 1 + (B + 127) // 128, (cg, B, launches)
                _rule(rec, "cluster, f16x3, cluster_groups %d, B %d" % (cg, B), lat, 4, B, 1)
        e.set_option("cluster_groups", 0)
        _labels_select_rows(e, dev, rec, "cluster, f16x3", 1, 2)
        ns = _status_ok(e, 1)
        assert ns["cluster_loop"] == 1, ns
    finally:
        e.close()
    assert not rec.failures()


# ------------------------------------------------------------------ c. serving entries
SIZES = (3, 1, 8, 5)                                          # the requests of a coalesced call: 17 motions
LENS17 = [16, 9, 3, 11, 8, 5, 1, 16, 12, 7, 2, 14, 16, 6, 13, 4, 10]
WANT_FEATS = (1, 3)                                           # the requests that ask for features
# (name, precision, "loop_kernel"): auto is the latency kernels on an F32 handle and the cluster loop on an F16X3 one at 17 motions
SERVE = [("f32 auto", 0, 0), ("f32 persistent", 0, 3), ("f16x3 auto", 1, 0), ("f16x3 persistent", 1, 3)]


def _split(sizes=SIZES):
    lo = 0
    for n in sizes:
        yield slice(lo, lo + n)
        lo += n


def _requests(dev, feats=WANT_FEATS, traj=False, steps=4, rots=None, lat_in=True):
    """the 3 + 1 + 8 + 5 requests over the first 17 motions of the 4-step batch, with fresh NaN-filled outputs"""
    acts, lat0 = AE.batch(BMAX[4])
    reqs = []
    for i, s in enumerate(_split()):
        n = s.stop - s.start
        a = (acts[s] + (rots[i] if rots else 0)) % AE.NCLASSES
        q = dict(actions=a.tolist(), lengths=LENS17[s], latents_out=_nan(dev, n, 1, 256))
        if lat_in:
            q["init_latents"] = _cuda(lat0[s], dev)
        if i in feats:
            q["feats_out"] = _nan(dev, n, max(LENS17[s]), 150)
        if traj:
            q["traj_out"] = _nan(dev, steps, n, 256)
        reqs.append(q)
    return reqs


def _lat(reqs):
    return torch.cat([q["latents_out"] for q in reqs])[:, 0].cpu().numpy()


def _check_coalesced(rec, name, prec, reqs):
    outs = _outs(4)
    fr, ef = AE.feats_reference(AE.weights(), outs, range(17), LENS17, "gpu17")
    for i, (q, s) in enumerate(zip(reqs, _split())):
        r64, e32 = AE.prefix(outs, s.stop - s.start, lo=s.start)
        rec.rule("%s, request %d latents" % (name, i), q["latents_out"][:, 0].cpu().numpy(), r64, e32, prec)
        if "feats_out" in q:
            f, tm = q["feats_out"].cpu().numpy(), max(q["lengths"])
            rec.rule("%s, request %d feats" % (name, i), f, fr[s, :tm], ef, prec)
            for m, n in enumerate(q["lengths"]):
                assert np.all(f[m, n:] == 0), (name, i, m)


@pytest.mark.parametrize("name,prec,lk", SERVE, ids=[s[0].replace(" ", "_") for s in SERVE])
def test_serving_entries(dev, rec, name, prec, lk):
    """mldhip_sample_many, _traj, _from and _guided on one handle: requests of 3 + 1 + 8 + 5 motions, each with its own labels, two of them asking for
    features of ragged lengths.  Coalesced: each request against the reference of its motions, padded frames exactly 0.  Trajectory: every row against the
    reference trace, the last row == latents_out to the bit.  Sources, in one call: a clean source at first_step 1, a request without one, and a request
    resumed at step 2 from row 1 of that trajectory without init_latents -- it equals the uninterrupted run to the bit.  Guidance 0, 1, 3 and -1 (the
    handle's 7.5) per request."""
    e = _engine(prec, 17, 4, {"loop_kernel": lk})
    if prec == 1 and lk == 0:
        _cluster_or_skip(e)
    want = CHAIN if (prec, lk) == (0, 0) else 2
    acts, lat0 = AE.batch(BMAX[4])
    try:
        # coalesced
        reqs = _requests(dev)
        e.sample_many(reqs)
        torch.cuda.synchronize()
        assert e.launch_counts()[0] == want, (name, e.launch_counts())
        _check_coalesced(rec, "sample_many, " + name, prec, reqs)
        # trajectory
        reqs = _requests(dev, traj=True)
        e.sample_many_traj(reqs, None)
        torch.cuda.synchronize()
        assert e.launch_counts()[0] == want, (name, e.launch_counts())
        _check_coalesced(rec, "sample_many_traj, " + name, prec, reqs)
        traj = torch.cat([q["traj_out"] for q in reqs], 1)
        assert torch.equal(traj[3], torch.cat([q["latents_out"] for q in reqs])[:, 0])
        t = traj.cpu().numpy()
        for s in range(4):
            r64, e32 = AE.prefix(_outs(4), 17, step=s)
            rec.rule("sample_many_traj, %s, step %d" % (name, s), t[s], r64, e32, prec)
        lat_a = _lat(reqs)
        # sources: motions 0-2 a clean source at step 1, 3-11 none, 12-16 resumed at step 2
        src = (syn._rng(145, "gpusrc").standard_normal((3, 1, 256)) * 0.7).astype(np.float32)
        resume = traj[1, 12:17].clone().reshape(5, 1, 256)
        froms = []
        for i, (s, extra) in enumerate(((slice(0, 3), dict(src_latents=_cuda(src, dev), first_step=1)), (slice(3, 12), {}),
                                        (slice(12, 17), dict(src_latents=resume, first_step=2, noised=1)))):
            n = s.stop - s.start
            q = dict(actions=acts[s].tolist(), lengths=[AE.LENGTH] * n, latents_out=_nan(dev, n, 1, 256), traj_out=_nan(dev, 4, n, 256), **extra)
            if i != 2:
                q["init_latents"] = _cuda(lat0[s], dev)
            froms.append(q)
        e.sample_many_from(froms, None)
        torch.cuda.synchronize()
        starts = [(SOURCE, 1, src[m]) for m in range(3)] + [(NONE, 0, None)] * 9 + [(RESUME, 2, t[1, 12 + m][None]) for m in range(5)]
        # (the resumed rows of the reference start from the engine's own row 1: what the call was given)
        rtraj, rlat = AE.numpy_loop(AE.weights(), acts[:17], lat0[:17], 4, starts)
        lat_f, traj_f = _lat(froms), torch.cat([q["traj_out"] for q in froms], 1).cpu().numpy()
        for m, (_, f, _) in enumerate(starts):
            assert np.isnan(traj_f[:f, m]).all() and np.isfinite(traj_f[f:, m]).all(), (name, m)
        rec.bound("sample_many_from, %s, latents" % name, lat_f, rlat, AE.ETA_TOL)
        rec.bound("sample_many_from, %s, written rows" % name, np.nan_to_num(traj_f), np.nan_to_num(rtraj), AE.ETA_TOL)
        assert np.array_equal(traj_f[3], lat_f)
        assert np.array_equal(lat_f[12:], lat_a[12:]) and np.array_equal(traj_f[2:, 12:], t[2:, 12:]), (name, float(np.abs(lat_f[12:] - lat_a[12:]).max()))
        # guidance per request
        gs = (0.0, 1.0, 3.0, -1.0)
        reqs = _requests(dev, feats=())
        for q, g in zip(reqs, gs):
            q["guidance"] = g
        e.sample_many_guided(reqs, None)
        torch.cuda.synchronize()
        per_motion = [g for n, g in zip(SIZES, gs) for _ in range(n)]
        _, rlat = AE.numpy_loop(AE.weights(), acts[:17], lat0[:17], 4, gs=per_motion, tag="gpu guided")
        lat_g = _lat(reqs)
        rec.bound("sample_many_guided, %s" % name, lat_g, rlat, AE.ETA_TOL)
        r64, e32 = AE.prefix(_outs(4), 5, lo=12)
        rec.rule("sample_many_guided, %s, the handle's own scale" % name, lat_g[12:], r64, e32, prec)
        ns = _status_ok(e, prec)
        if prec == 1 and lk == 0:
            assert ns["cluster_loop"] == 1, ns
    finally:
        e.close()
    assert not rec.failures()


# (precision, family, "loop_kernel"): den_final_step's eta form behind the latency kernels, den_loop_kernel<false / true, kLoopEta>, den_cluster_eta_kernel
ETA_CASES = [(0, "latency", 1), (0, "persistent", 3), (1, "latency", 1), (1, "persistent", 3), (1, "cluster", 4)]


@pytest.mark.parametrize("prec,fam,lk", ETA_CASES, ids=["%s_%s" % (R.MODE[p], f) for p, f, _ in ETA_CASES])
def test_seeded_calls_on_a_stochastic_handle(dev, rec, prec, fam, lk):
    """eta 0.5, 4 steps, both precisions: mldhip_sample_many_seeded with first_index 0 and 2^31 - 4 (the index crosses 2^31 inside the call) on the latency and
    persistent families and, on F16X3, the cluster loop, against the float32 numpy loop fed the same Philox draws; a request alone equals the same request
    inside the coalesced call to the bit (include/mldhip.h "Noise contract").  Only the cluster case needs the device's cluster lane."""
    e = _engine(prec, 17, 4, {"loop_kernel": lk}, eta=0.5)
    if lk == 4:
        _cluster_or_skip(e)
    acts, lat0 = AE.batch(BMAX[4])
    try:
        for first in (0, 2 ** 31 - 4):
            _, rlat = AE.numpy_loop(AE.weights(), acts[:17], lat0[:17], 4, eta=0.5, keys_per_motion=[(SEED, first + m) for m in range(17)], tag=("gpu eta", first))
            reqs = _requests(dev, feats=())
            e.sample_many_seeded(reqs, [(SEED, first + s.start) for s in _split()])
            torch.cuda.synchronize()
            assert e.launch_counts()[0] == (CHAIN if lk == 1 else 2), (fam, e.launch_counts())
            rec.bound("sample_many_seeded, %s, %s, first_index %d" % (R.MODE[prec], fam, first), _lat(reqs), rlat, AE.ETA_TOL)
            alone = _requests(dev, feats=())[2]
            e.sample_many_seeded([alone], [(SEED, first + 4)])
            torch.cuda.synchronize()
            assert torch.isfinite(alone["latents_out"]).all() and torch.equal(alone["latents_out"], reqs[2]["latents_out"]), (fam, first)
        ns = _status_ok(e, prec)
        if lk == 4:
            assert ns["cluster_loop"] == 1, ns
    finally:
        e.close()
    assert not rec.failures()


PIPE_SIZES = (8, 3, 8, 1)
LENS20 = LENS17 + [9, 15, 5]


def _pipe_requests(dev, rots, feats=True, swap=False):
    """the requests of 8, 3, 8, 1 motions, request i's labels rotated by rots[i]; swap: requests 0 and 2 (8 motions each) exchange their label lists"""
    acts, lat0 = AE.batch(BMAX[4])
    labels = [((acts[s] + rot) % AE.NCLASSES).tolist() for s, rot in zip(_split(PIPE_SIZES), rots)]
    if swap:
        labels[0], labels[2] = labels[2], labels[0]
    reqs = []
    for s, a in zip(_split(PIPE_SIZES), labels):
        n = s.stop - s.start
        q = dict(actions=a, init_latents=_cuda(lat0[s], dev), lengths=LENS20[s], latents_out=_nan(dev, n, 1, 256))
        if feats:
            q["feats_out"] = _nan(dev, n, max(q["lengths"]), 150)
        reqs.append(q)
    return reqs


def test_pipelined_requests_read_their_own_labels(dev, rec):
    """"many_pipeline" 1 on an F16X3, max_in_flight 2 handle (cluster loop): requests of 8, 3, 8, 1 motions with different labels, all asking for features,
    each bit-identical to its own mldhip_sample_action call on the same handle; then the call again with the label lists of the two 8-motion requests
    exchanged and the other two rotated by 5 and 7 classes -- graph replay and context reuse: the labels are read at replay time, and each request is
    staged on the prep stream beside the previous launch"""
    e = _engine(1, 20, 4, max_in_flight=2)
    _cluster_or_skip(e)
    try:
        for rots, swap in (((0, 0, 0, 0), False), ((0, 5, 0, 7), True)):
            e.set_option("many_pipeline", 1)
            reqs = _pipe_requests(dev, rots, swap=swap)
            e.sample_many(reqs)
            torch.cuda.synchronize()
            # the last request's own cluster launch, issued directly; its condition rows replay in a graph on the prep stream (a coalesced chain counts 2)
            assert e.launch_counts()[0] == 1, e.launch_counts()
            e.set_option("many_pipeline", 0)
            for i, q in enumerate(_pipe_requests(dev, rots, swap=swap)):
                e.sample_action(q["actions"], q["init_latents"], q["lengths"], q["latents_out"], q["feats_out"])
                torch.cuda.synchronize()
                assert torch.isfinite(q["latents_out"]).all() and torch.isfinite(q["feats_out"]).all(), (rots, i)
                assert torch.equal(q["latents_out"], reqs[i]["latents_out"]) and torch.equal(q["feats_out"], reqs[i]["feats_out"]), (rots, i)
                if not swap:
                    s = list(_split(PIPE_SIZES))[i]
                    r64, e32 = AE.prefix(_outs(4), s.stop - s.start, lo=s.start)
                    rec.rule("many_pipeline, f16x3, request %d latents" % i, reqs[i]["latents_out"][:, 0].cpu().numpy(), r64, e32, 1)
            _cache["pipe", swap] = [q["latents_out"].clone() for q in reqs]
        for a, b in zip(_cache["pipe", False], _cache["pipe", True]):      # every request's labels changed between the two calls, and so did its result
            assert not torch.equal(a, b)
        ns = _status_ok(e, 1)
        assert ns["cluster_loop"] == 1, ns
    finally:
        e.close()
    assert not rec.failures()


def _raw_seeded(e, reqs, keys, stream, disturb):
    """mldhip_sample_many_seeded through raw ctypes with test-owned label, length and key arrays; with `disturb`, the arrays are overwritten with other valid
    values when the call has returned, before anything is synchronised"""
    n = len(reqs)
    arr = (_lib.Request * n)()
    labs = [(C.c_int32 * len(q["actions"]))(*q["actions"]) for q in reqs]
    lens = [(C.c_int32 * len(q["lengths"]))(*q["lengths"]) for q in reqs]
    ks = (_lib.NoiseKey * n)(*[_lib.NoiseKey(s, f) for s, f in keys])
    for r, q, la, le in zip(arr, reqs, labs, lens):
        r.actions_host, r.lengths_host, r.B = la, le, len(q["lengths"])
        r.init_latents_dev, r.latents_out_dev, r.feats_out_dev = q["init_latents"].data_ptr(), q["latents_out"].data_ptr(), q["feats_out"].data_ptr()
    rc = e.lib.mldhip_sample_many_seeded(e._h, arr, ks, n, stream)
    if disturb:
        for la, le in zip(labs, lens):
            tmax = max(le)
            for k in range(len(la)):
                la[k] = (la[k] + 5) % AE.NCLASSES                       # another class
                le[k] = le[k] - 1 if le[k] > 1 else min(2, tmax)        # another length, inside the request's own frame count
        for k in range(n):
            ks[k].seed, ks[k].first_index = 12345, 99
    assert rc == 0, e.lib.mldhip_last_error(e._h)


@pytest.mark.parametrize("pipeline", [0, 1], ids=["coalesced", "pipelined"])
def test_pageable_host_arrays_are_consumed_when_the_call_returns(dev, pipeline):
    """include/mldhip.h, Conventions: label and length arrays in PAGEABLE memory (ctypes arrays here) and the key table may be overwritten as soon as the
    call returns.  One call on a side stream with earlier work queued, eta 0.5 so that the keys are read: the results equal the undisturbed call's to the
    bit.  The engine hands the arrays to hipMemcpyAsync as they are, so what this checks is the runtime's treatment of pageable sources under the engine's
    call sequence.  The premise is asserted on the third call, which replays the graphs the first two captured: the earlier work on the stream (60 matrix
    products) was still running when the call returned and the arrays were overwritten, so the copies had been staged, not run.  Page-locked arrays are
    outside the promise and not tried."""
    e = _engine(1, 20, 4, max_in_flight=2, eta=0.5)
    if pipeline:                                        # (the pipelined form serves cluster-loop requests only; the coalesced call runs on any family)
        _cluster_or_skip(e)
    try:
        e.set_option("many_pipeline", pipeline)
        keys = [(SEED, 7 + s.start) for s in _split(PIPE_SIZES)]
        side = torch.cuda.Stream()
        busy = torch.randn(2048, 2048, device=dev)
        got, running = [], []
        for disturb in (False, True, True):             # (the second disturbed call replays the graphs the first two captured)
            reqs = _pipe_requests(dev, (0, 3, 6, 9))
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                for _ in range(60):
                    busy = (busy @ busy).clamp_(-1, 1)
                queued = torch.cuda.Event()
                queued.record()
            _raw_seeded(e, reqs, keys, side.cuda_stream, disturb)
            done = queued.query()
            print("pipeline %d, disturb %s: earlier work %s when the call returned" % (pipeline, disturb, "done" if done else "still running"))
            torch.cuda.synchronize()
            running.append(not done)
            got.append(reqs)
        # the premise of the replayed call: it returned, and its arrays were overwritten, while the stream had not reached it -- the copies were staged, not run
        assert running[-1], running
        for other in got[1:]:
            for i, (a, b) in enumerate(zip(got[0], other)):
                assert torch.isfinite(a["latents_out"]).all() and torch.isfinite(a["feats_out"]).all(), i
                assert torch.equal(a["latents_out"], b["latents_out"]) and torch.equal(a["feats_out"], b["feats_out"]), (pipeline, i)
        _status_ok(e, 1)
    finally:
        e.close()


# ------------------------------------------------------------------ d. ActorVae frame-length sweep
def _vae_ref(key, fn):
    if key not in _cache:
        _cache[key] = R.reference64(fn)
    return _cache[key]


def _decode(e, dev, rec, name, z, lens, key):
    w = AE.weights()
    (fr,) = _vae_ref(key, lambda ops, W: O.actor_decode(ops, W(w[1]), ops.asarray(z), lens))
    feats = _nan(dev, len(lens), max(lens), 150)
    e.vae_decode(_cuda(z, dev), lens, feats)
    torch.cuda.synchronize()
    f = feats.cpu().numpy()
    rec.bound(name, f, fr, R.OP_TOL)
    for i, n in enumerate(lens):
        assert np.all(f[i, n:] == 0), (name, i)


@PRECS
def test_actor_vae_frame_length_sweep(dev, rec, prec):
    """ActorVae on a max_frames 288 handle.  Decode at every T of tests/test_gpu_shape_edges.py's TS, a full motion next to a ragged one; B = 5 all of length 64
    and B = 1 (layer 0's one-sample-per-length form with and without duplicates); on F16X3 once more at T = 129 with "flash_attn" 2.  Encode at every T of ENC_TS:
    mu and logvar against O.actor_encode, the latent against mu + exp(logvar)^0.5 eps.  Then one 2-step sample of lengths 288, 1, 257, 16: the sampled features
    against the reference.  The plain stack of 3 layers ends in Ha after visiting Hb; the final GEMM has N = 150 columns (a partial last column tile, padded
    rows zeroed, all-padding tiles skipped), the encoder pads K = 150 to 160; the sinusoidal PE table is read up to row 287 (decode) and 287 (encode: 286 + 2 tokens)."""
    w = AE.weights()
    mode = R.MODE[prec]
    e = _engine(prec, 5, 2, max_frames=288)
    try:
        for T in TS:
            z = syn._rng(146, "actdec%d" % T).standard_normal((2, 1, 256)).astype(np.float32)
            _decode(e, dev, rec, "actor decode, %s, T %d" % (mode, T), z, [T, _ragged(T)], ("dec", T))
        z = syn._rng(146, "actdec5").standard_normal((5, 1, 256)).astype(np.float32)
        _decode(e, dev, rec, "actor decode, %s, B 5 all of length 64" % mode, z, [64] * 5, ("dec", "b5"))
        _decode(e, dev, rec, "actor decode, %s, B 1, T 64" % mode, z[:1], [64], ("dec", "b1"))
        for T in ENC_TS:
            lens = [T, _ragged(T)]
            g = syn._rng(147, "actenc%d" % T)
            fe = g.standard_normal((2, T, 150)).astype(np.float32)
            fe[1, lens[1]:] = 0
            eps = g.standard_normal((2, 1, 256)).astype(np.float32)
            mr, lvr = _vae_ref(("enc", T), lambda ops, W: O.actor_encode(ops, W(w[1]), ops.asarray(fe), lens)[1:])
            lat, mu, lv = (_nan(dev, 2, 1, 256) for _ in range(3))
            e.vae_encode(_cuda(fe, dev), lens, T, _cuda(eps, dev), lat, mu, lv)
            torch.cuda.synchronize()
            m, v = mu.cpu().numpy().astype(np.float64), lv.cpu().numpy().astype(np.float64)
            rec.bound("actor encode, %s, T %d mu" % (mode, T), m, mr, R.OP_TOL)
            rec.bound("actor encode, %s, T %d logvar" % (mode, T), v, lvr, R.OP_TOL)
            rec.bound("actor encode, %s, T %d latent" % (mode, T), lat.cpu().numpy(), m + np.sqrt(np.exp(v)) * eps, R.OP_TOL)
        # one sample to capacity: the first four motions of the 2-step batch
        lens = [288, 1, 257, 16]
        acts, lat0 = AE.batch(BMAX[2])
        outs = AE.loop_reference(w, 2, BMAX[2], n=4)
        fr, ef = AE.feats_reference(w, outs, range(4), lens, "gpu288")
        lat, feats = _nan(dev, 4, 1, 256), _nan(dev, 4, 288, 150)
        e.sample_action(acts[:4].tolist(), _cuda(lat0[:4], dev), lens, lat, feats)
        torch.cuda.synchronize()
        r64, e32 = AE.prefix(outs, 4)
        rec.rule("sample_action, %s, lengths 288 1 257 16, latents" % mode, lat.cpu().numpy()[:, 0], r64, e32, prec)
        f = feats.cpu().numpy()
        rec.rule("sample_action, %s, lengths 288 1 257 16, feats" % mode, f, fr, ef, prec)
        for i, n in enumerate(lens):
            assert np.all(f[i, n:] == 0), i
        if prec == 1:
            e.set_option("flash_attn", 2)
            z = syn._rng(146, "actdec129").standard_normal((2, 1, 256)).astype(np.float32)
            _decode(e, dev, rec, "actor decode, f16x3, flash_attn 2, T 129", z, [129, _ragged(129)], ("dec", 129))
        _status_ok(e, prec)
    finally:
        e.close()
    assert not rec.failures()
