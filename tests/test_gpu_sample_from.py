"""Start the reverse loop from a source latent at a chosen step (mldhip_sample_many_from) on an MI355X: full 9-layer synthetic weights, 50 steps, F16X3,
B = 9.  Mixed first steps on every loop family against the numpy loop of tests/sample_from_ref.py, the two bit identities, graph replay with fresh
buffers and changed first steps, launch counts, the eta = 0.5 cluster case, MLD.edit, and the timing that shows skipped steps are not run.

Tolerance: the project's latent tolerance, 5e-3 absolute (tests/test_gpu_parity.py), on every written row; joints within 1e-3.  The measured per-step
maxima and the two timings go to profiles/sample_from.json when MLDHIP_SAMPLE_FROM_OUT names a file (the committed copy was written that way)."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from mld_hip import _lib  # noqa: E402
from mld_hip import synthetic as syn  # noqa: E402
from oracle import mld_oracle as O  # noqa: E402

from sample_from_ref import NONE, RESUME, SOURCE, reverse_from_np  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
STEPS = 50
TOL, TOL_JOINTS = 5e-3, 1e-3
LENS9 = [24, 17, 3, 20, 1, 9, 24, 12, 5]
SEED, FIRST = 0xC0FFEE, 3
FAMILY = {"cluster": 0, "persistent": 3, "latency": 1}      # "loop_kernel": the default picks the cluster loop for a small F16X3 call
# mixed inside the first workgroup / cluster, one motion alone in the second
KIND9 = [NONE, SOURCE, SOURCE, SOURCE, SOURCE, SOURCE, SOURCE, SOURCE, SOURCE]
F9 = [0, 49, 25, 10, 25, 0, 10, 49, 25]
LATE8 = [25, 49, 25, 10, 25, 49, 10, 49]                     # a workgroup whose motions all start late; motions 1, 2, 4, 6, 7 as in F9

_measured = {}
_cache = {}


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


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(device=0, max_batch=16, max_frames=24, precision=1)
    _load(e)
    yield e
    e.close()
    out = os.environ.get("MLDHIP_SAMPLE_FROM_OUT")
    if out and _measured:
        with open(out, "w") as f:
            json.dump({"what": "mldhip_sample_many_from on an MI355X, F16X3, 9 layers, 50 steps, B = 9: max |engine - numpy loop| over the motions that have "
                               "started, after each scheduler step (bound 5e-3 on every written row), and the call time in ms (HIP events, median of five) "
                               "with every motion at first_step 40 against first_step 0 (asserted: t(40) < 0.5 t(0))", **_measured}, f, indent=1)


@pytest.fixture(scope="module")
def batch9():
    b = syn.make_batch(9, LENS9, seed=81)
    src = np.random.default_rng(83).standard_normal((9, 1, 256)).astype(f32) * f32(0.7)
    return b, src


def _ref(batch9, kinds, firsts, eta=0.0):
    """(trajectory, latents, joints) of the numpy loop + the oracle's decode; once per case"""
    key = (tuple(kinds), tuple(firsts), eta)
    if key not in _cache:
        b, src = batch9
        ops = O.NumpyOps(f32)
        B = len(firsts)
        te = np.concatenate([b.text_emb[:9][:B], b.text_emb[9:][:B]], 0)
        traj, lat = reverse_from_np(O.to_backend(ops, syn.make_denoiser_state_dict()), te, b.init_latents[:B],
                                    [(k, f, src[m]) for m, (k, f) in enumerate(zip(kinds, firsts))], STEPS, eta, [(SEED, FIRST + m) for m in range(B)])
        mean, std = syn.make_mean_std()
        feats = O.vae_decode(ops, O.to_backend(ops, syn.make_vae_state_dict()), lat.reshape(B, 1, 256), b.lengths[:B])
        _cache[key] = (traj, lat, np.asarray(O.feats2joints(ops, feats, mean, std)))
    return _cache[key]


def _requests(batch9, dev, kinds, firsts, srcs=None, motions=range(9), joints=True):
    """one request per motion (a start is a property of a request) with fresh NaN-filled outputs"""
    b, src = batch9
    srcs = src if srcs is None else srcs
    reqs, keys = [], []
    for m in motions:
        q = dict(text_emb=_cuda(np.stack([b.text_emb[m], b.text_emb[9 + m]]), dev), lengths=[b.lengths[m]], latents_out=_nan(dev, 1, 1, 256),
                 traj_out=_nan(dev, STEPS, 1, 256))
        if joints:
            q["joints_out"] = _nan(dev, 1, b.lengths[m], 22, 3)
        if kinds[m] != RESUME:
            q["init_latents"] = _cuda(b.init_latents[m:m + 1], dev)
        if kinds[m] != NONE:
            s = srcs[m]
            q.update(src_latents=s.reshape(1, 1, 256).contiguous() if torch.is_tensor(s) else _cuda(s.reshape(1, 1, 256), dev), first_step=firsts[m],
                     noised=int(kinds[m] == RESUME))
        reqs.append(q)
        keys.append((SEED, FIRST + m))
    return reqs, keys


def _run(e, reqs, keys=None):
    e.sample_many_from(reqs, keys)
    torch.cuda.synchronize()
    return torch.cat([q["latents_out"] for q in reqs])[:, 0], torch.cat([q["traj_out"] for q in reqs], 1)


def _check(name, ref, lat, traj, reqs, firsts, lengths):
    rtraj, rlat, rj = ref
    t = traj.cpu().numpy()
    err = np.zeros(STEPS)
    for m, f in enumerate(firsts):
        assert np.isnan(t[:f, m]).all(), (name, m, "rows below the first step are left untouched")
        assert np.isfinite(t[f:, m]).all(), (name, m)
        err[f:] = np.maximum(err[f:], np.abs(t[f:, m] - rtraj[f:, m]).max(1))
    ej = max(float(np.abs(q["joints_out"][0].cpu().numpy() - rj[m, :lengths[m]]).max()) for m, q in enumerate(reqs))
    _measured.setdefault("families", {})[name] = {"first_steps": list(firsts), "per_step_max_abs_err": [float(x) for x in err], "max": float(err.max()),
                                                  "step_of_max": int(err.argmax()), "last_step": float(err[-1]), "joints_max_abs_err": ej}
    print(f"{name}: per-step max error, worst {err.max():.3e} at step {int(err.argmax())}, last step {err[-1]:.3e}; joints {ej:.3e}")
    assert err.max() < TOL and ej < TOL_JOINTS, (name, err.tolist(), ej)
    assert torch.equal(traj[STEPS - 1], lat)


@pytest.mark.parametrize("family", list(FAMILY))
def test_mixed_first_steps_and_the_bit_identities(eng, dev, batch9, family):
    """First steps {0, 10, 25, 49} mixed inside a workgroup against the numpy loop; then, with fresh buffers and CHANGED first steps (on the one-launch
    loops: the same captured graph), the resume identity (every motion resumed one step later from its own trajectory row: the same bits); then a call whose first workgroup starts
    late everywhere (neighbour identity, launch count of the launch family)."""
    b, src = batch9
    eng.set_option("loop_kernel", FAMILY[family])
    try:
        plain = dict(text_emb=_cuda(b.text_emb, dev), init_latents=_cuda(b.init_latents, dev), lengths=b.lengths, latents_out=_nan(dev, 9, 1, 256))
        eng.sample_many([plain])
        torch.cuda.synchronize()
        n_plain = eng.launch_counts()[0]
        reqs, _ = _requests(batch9, dev, KIND9, F9)
        lat_a, traj_a = _run(eng, reqs)
        counts = eng.launch_counts()
        _check(family, _ref(batch9, KIND9, F9), lat_a, traj_a, reqs, F9, b.lengths)
        if family == "latency":
            per_step = (n_plain - 2) // STEPS                 # a plain call: condition rows + init + 50 x the per-step launches
            assert per_step * STEPS == n_plain - 2 and counts[0] == n_plain
        else:
            assert counts[0] == 2                             # condition rows + ONE launch
        ns = eng.numeric_status()
        assert ns["nonfinite_values"] == 0 and ns["loop_split_ok"] == 1 and ns["cluster_loop"] in (1, 3), ns
        if family == "cluster":
            assert ns["cluster_loop"] == 1
        # graph replay: fresh buffers, changed first steps; the first call's buffers are not written again
        keep = [(q["latents_out"], q["traj_out"]) for q in reqs]
        kinds = [RESUME if f + 1 < STEPS else k for k, f in zip(KIND9, F9)]
        firsts = [f + 1 if f + 1 < STEPS else f for f in F9]
        srcs = [traj_a[f, m].clone() if f + 1 < STEPS else src[m] for m, f in enumerate(F9)]
        for la, tr in keep:
            la.fill_(float("nan"))
            tr.fill_(float("nan"))
        reqs2, _ = _requests(batch9, dev, kinds, firsts, srcs)
        lat_b, traj_b = _run(eng, reqs2)
        if family == "latency":                              # the smallest first step moved from 0 to 1: one step's launches fewer (and a graph of its own)
            assert eng.launch_counts()[0] == 2 + (STEPS - min(firsts)) * per_step and eng.launch_counts()[1:] == counts[1:]
        else:                                                # the one-launch loops read the first steps from the table: the same graph
            assert eng.launch_counts() == counts
        assert all(torch.isnan(la).all() and torch.isnan(tr).all() for la, tr in keep)
        assert torch.equal(lat_b, lat_a)
        for m, f in enumerate(firsts):
            assert torch.isnan(traj_b[:f, m]).all() and torch.equal(traj_b[f:, m], traj_a[f:, m]), (family, m, f)
        assert all(torch.equal(q["joints_out"], p["joints_out"]) for q, p in zip(reqs2, reqs))
        # a workgroup whose motions all start late: neighbours changed, motions 1, 2, 4, 6, 7 keep their start and their bits
        reqs3, _ = _requests(batch9, dev, [SOURCE] * 8, LATE8, motions=range(8), joints=False)
        lat_c, traj_c = _run(eng, reqs3)
        for m in (1, 2, 4, 6, 7):
            assert torch.equal(lat_c[m], lat_a[m]), (family, m)
        assert torch.isnan(traj_c[:10]).all() and torch.equal(traj_c[STEPS - 1], lat_c)
        if family == "latency":                              # the init launch + the steps from the smallest first step on
            assert eng.launch_counts()[0] == 2 + (STEPS - min(LATE8)) * per_step
        else:
            assert eng.launch_counts()[0] == 2
        assert eng.numeric_status()["nonfinite_values"] == 0
    finally:
        eng.set_option("loop_kernel", 0)


def test_no_source_is_the_trajectory_call(eng, dev, batch9):
    b, _ = batch9
    out = []
    for call in (eng.sample_many_from, eng.sample_many_traj):
        q = dict(text_emb=_cuda(b.text_emb, dev), init_latents=_cuda(b.init_latents, dev), lengths=b.lengths, latents_out=_nan(dev, 9, 1, 256),
                 joints_out=_nan(dev, 9, 24, 22, 3), traj_out=_nan(dev, STEPS, 9, 256))
        call([q], None)
        torch.cuda.synchronize()
        out.append((q, eng.launch_counts()))
    (qa, ca), (qb, cb) = out
    assert ca == cb and torch.isfinite(qa["traj_out"]).all()
    assert all(torch.equal(qa[k], qb[k]) for k in ("latents_out", "joints_out", "traj_out"))


def test_cluster_loop_eta_from_sources(dev, batch9):
    """eta = 0.5 on the cluster loop: step i draws with the absolute step index i, wherever the motion started."""
    b, _ = batch9
    e = _lib.Engine(device=0, max_batch=16, max_frames=24, precision=1, eta=0.5)
    _load(e)
    reqs, keys = _requests(batch9, dev, KIND9, F9)
    lat, traj = _run(e, reqs, keys)
    assert e.launch_counts()[0] == 2 and e.numeric_status()["cluster_loop"] == 1
    _check("cluster_eta0.5", _ref(batch9, KIND9, F9, 0.5), lat, traj, reqs, F9, b.lengths)
    assert e.numeric_status()["nonfinite_values"] == 0
    e.close()


@pytest.mark.parametrize("family", ["persistent", "cluster"])
def test_skipped_steps_are_not_run(eng, dev, batch9, family):
    """Every motion at first_step 40 against first_step 0, one request of 9 motions, latents only: 10 of 50 steps plus a fixed prologue.  HIP events, median of
    five; t(40) < 0.5 t(0) (expected 0.2 + the prologue; the margin covers it and the clock ramp)."""
    b, src = batch9
    eng.set_option("loop_kernel", 3 if family == "persistent" else 4)
    try:
        ms = {}
        for f in (0, 40):
            q = dict(text_emb=_cuda(b.text_emb, dev), init_latents=_cuda(b.init_latents, dev), lengths=b.lengths, latents_out=_nan(dev, 9, 1, 256),
                     src_latents=_cuda(src, dev), first_step=f)
            t = []
            for it in range(7):                               # two warm-up calls (capture, clocks), five timed
                a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                eng.sample_many_from([q], None, torch.cuda.current_stream().cuda_stream)
                z.record()
                z.synchronize()
                if it >= 2:
                    t.append(a.elapsed_time(z))
            assert eng.launch_counts()[0] == 2 and torch.isfinite(q["latents_out"]).all()
            ms[f] = float(np.median(t))
        _measured.setdefault("call_ms", {})[family] = {"first_step_0": ms[0], "first_step_40": ms[40], "ratio": ms[40] / ms[0]}
        print(f"{family}: first_step 0 {ms[0]:.3f} ms, first_step 40 {ms[40]:.3f} ms, ratio {ms[40] / ms[0]:.3f}")
        assert ms[40] < 0.5 * ms[0], ms
    finally:
        eng.set_option("loop_kernel", 0)


def test_mld_edit_on_gpu(dev):
    """MLD.edit on the module surface: encode -> noised to step n - int(n * strength) -> denoised under the prompts -> joints, against O.vae_encode, the numpy
    loop and the oracle's decode."""
    from mld_hip import config as C
    from mld_hip import engine as E
    from mld_hip.datamodule import HipDataModule
    from mld_hip.mld import MLD
    from mld_hip.text_encoder import SyntheticTextEncoder

    E.drop_engines()
    cfg = C.load_config()
    E.configure(max_batch=8, max_frames=24)
    model = MLD(cfg, HipDataModule(cfg), text_encoder=SyntheticTextEncoder()).to(dev).eval()
    assert model.fused
    texts, lengths = ["a man kicks with his left leg.", "a person walks backward slowly."], [24, 17]
    g = torch.Generator().manual_seed(5)
    motion = torch.randn(2, 24, 263, generator=g) * 0.3
    motion[1, 17:] = 0
    lat0 = syn.make_batch(2, lengths).init_latents
    out = model.edit({"motion": motion.to(dev), "text": texts, "length": lengths}, 0.3, init_latents=_cuda(lat0, dev))
    assert [tuple(j.shape) for j in out] == [(24, 22, 3), (17, 22, 3)]
    ops = O.NumpyOps(f32)
    sdd, sdv = O.to_backend(ops, syn.make_denoiser_state_dict()), O.to_backend(ops, syn.make_vae_state_dict())
    _, mu, _ = O.vae_encode(ops, sdv, motion.numpy(), lengths, np.zeros((2, 1, 256), f32))
    mu = np.asarray(mu, f32).reshape(2, 1, 256)
    emb = model.text_encoder([""] * 2 + texts).cpu().numpy()
    f = STEPS - int(STEPS * 0.3)
    assert f == 35
    _, z = reverse_from_np(sdd, emb, lat0, [(SOURCE, f, mu[m]) for m in range(2)], STEPS)
    mean, std = syn.make_mean_std()
    jr = np.asarray(O.feats2joints(ops, O.vae_decode(ops, sdv, z.reshape(2, 1, 256), lengths), mean, std))
    ej = max(float(np.abs(out[m].numpy() - jr[m, :n]).max()) for m, n in enumerate(lengths))
    print(f"MLD.edit strength 0.3: joints max error {ej:.3e}")
    assert ej < TOL_JOINTS
    E.drop_engines()
