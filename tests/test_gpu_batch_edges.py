"""The number of motions B of a call, on the MI355X against the float64 oracle: every edge at which the reverse loop of the latent models changes its
kernels, its tile height, its cluster form or its launch count (the lists and the formula behind each edge: tests/batch_edges_ref.py), the automatic
selection at its boundaries, noise keys with a global first_index up to 2^40, and the grid-stride elementwise kernels beyond one pass of their grid.

Default weights, guidance 7.5, max_frames 16, every length 8, latents only.  A handle has one step count: calls of up to 257 motions are compared at 4 steps,
larger ones at 2 -- a family whose list spans both gets a 2-step handle that runs the whole list, largest first (so small calls follow large ones on
workspace rows whose stride comes from max_batch), and a 4-step handle of the same max_batch for the calls of up to 257 motions.  The reference of a call
is a prefix of one batch's (batch_edges_ref.loop_reference); tolerances are tests/config_envelope_ref.py's relative rule (4 x e32 on an F32 handle, 16 x e32
on an F16X3 one) and tests/test_gpu_ddim_eta.py's 5e-3 for stochastic calls.  Output buffers start NaN-filled.  With MLDHIP_BATCH_EDGES_JSON set, every
comparison is written there (profiles/batch_edges.json was written that way; the worst ratios measured there are quoted at the end of this text).

Measured there: the worst ratio to e32 is 1.85 on an F32 handle (bound 4; persistent loop, 4 steps, B = 7 .. 17) and 1.37 on an F16X3 one (bound 16; persistent
loop, 2 steps, B = 16); the latency kernels stay below 1.07 at every B, the throughput kernels below 1.81, the cluster loop below 1.02.  Stochastic calls end
3.2e-5 .. 5.9e-5 from the numpy loop (bound 5e-3) at every first_index on every family; the Philox stream 4.8e-7 from the oracle's (2e-5), the DDPM step 1.4e-6 (2e-6)
and the stochastic DDIM step 9.5e-7 (1e-5) at 4 x 2^20 + 5 elements.  The whole file takes 19 s."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import batch_edges_ref as BE  # noqa: E402
import config_envelope_ref as R  # noqa: E402
from mld_hip import _lib  # noqa: E402
from mld_hip import synthetic as syn  # noqa: E402
from oracle import mld_oracle as O  # noqa: E402
from test_ddim_eta import ddim_eta_step_np  # noqa: E402
from test_gpu_ddim_eta import oracle_eta  # noqa: E402

pytestmark = pytest.mark.gpu

BMAX = {4: 257, 2: 2049}          # motions of the reference batch of a step count
PRECS = pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f16x3"])
_cache = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def rec():
    r = R.Record("MLDHIP_BATCH_EDGES_JSON")
    yield r
    r.dump(what="max |engine - reference| of every case of tests/test_gpu_batch_edges.py on an MI355X.  eta = 0 calls: the float64 oracle, e32 = the float32 "
                "CPU oracle's own error on the same motions, ratio = err / e32, bound by the factor of the handle's precision; stochastic calls and the "
                "elementwise kernels: a float32 numpy evaluation fed the same Philox draws, absolute bound")


def _cuda(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _engine(prec, max_batch, steps, options=None, **cfg):
    e = _lib.Engine(device=0, precision=prec, max_batch=max_batch, max_frames=BE.MAX_FRAMES, num_inference_steps=steps, **cfg)
    try:
        w = R.text_weights()
        e.load_state_dict(w[0], "denoiser.")
        e.load_state_dict(w[1], "vae.")
        mean, std = syn.make_mean_std()
        e.load_tensor("mean", mean)
        e.load_tensor("std", std)
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


def _call(e, dev, steps, B):
    """the call of the first B motions of the step count's batch: (latents [B, 1, 256] as numpy, reverse-loop launches)"""
    text, lat0, lens = BE.call_inputs(BMAX[steps], B)
    lat = _nan(dev, B, 1, 256)
    e.sample(_cuda(text, dev), _cuda(lat0, dev), lens, lat)
    torch.cuda.synchronize()
    return lat.cpu().numpy(), e.launch_counts()[0]


def _rule(rec, name, got, steps, B, prec):
    r64, e32 = BE.prefix(BE.loop_reference(R.text_weights(), steps, BMAX[steps]), B)
    return rec.rule(name, got, r64, e32, prec)


def _handles(bs):
    """[(steps, the B of the list that handle runs)]: see the module text"""
    out = []
    if any(B > 257 for B in bs):
        out.append((2, list(bs)))
    out.append((4, [B for B in bs if B <= 257]))
    return out


# ------------------------------------------------------------------ 1. latency kernels
@PRECS
def test_latency_kernels(dev, rec, prec):
    """gemm_tile32_kernel on a max_batch 192 handle, B = 171, 170, 86, 85, 43, 42 (the 32 | 16-row switch of the out-projection, the skip linear and FFN2), 8, 3 (a
    32-row tile with an empty second half), 6, 5, 2, 1 (partial tiles), then 191 on the rows the small calls left; and B = 43 on a max_batch 43 handle, where the
    slab stride 6 x max_batch x 256 equals the call's."""
    for max_batch, bs in ((192, BE.LATENCY_BS), (43, [43])):
        e = _engine(prec, max_batch, 4, {"loop_kernel": 1})
        try:
            for B in bs:
                lat, launches = _call(e, dev, 4, B)
                name = "latency, %s, max_batch %d, B %d" % (R.MODE[prec], max_batch, B)
                assert launches == R.chain_launches(4, 9), (name, launches)
                _rule(rec, name, lat, 4, B, prec)
                _cache["latency", prec, max_batch, B] = lat
            _status_ok(e, prec)
        finally:
            e.close()
    print("B 43: max_batch 43 and 192 %s" % ("agree to the bit" if np.array_equal(_cache["latency", prec, 43, 43], _cache["latency", prec, 192, 43]) else "differ"))
    assert not rec.failures()


# ------------------------------------------------------------------ 2. column-split throughput kernels
def test_throughput_kernels(dev, rec):
    """gemm_strip_kernel (32 x 128) + the 32 x 64 staged FFN2 with two K slices on an F32 max_batch 1279 handle: 1279 and 128 (the ends of the range auto gives
    them), 127, 129, 171, and the small calls 16, 11, 6, 5, 1.  Up to 191 motions the result differs in some bit from the latency kernels' on the same handle:
    "loop_kernel" 2 really ran other kernels (the launch counts are equal)."""
    for steps, bs in _handles(BE.THROUGHPUT_BS):
        e = _engine(0, 1279, steps)
        try:
            for B in bs:
                e.set_option("loop_kernel", 2)
                lat, launches = _call(e, dev, steps, B)
                name = "throughput, f32, %d steps, B %d" % (steps, B)
                assert launches == R.chain_launches(steps, 9), (name, launches)
                _rule(rec, name, lat, steps, B, 0)
                if B <= 191 and B != 8:
                    e.set_option("loop_kernel", 1)
                    other, _ = _call(e, dev, steps, B)
                    assert np.isfinite(other).all() and not np.array_equal(lat, other), name
            _status_ok(e, 0)
        finally:
            e.close()
    assert not rec.failures()


# ------------------------------------------------------------------ 3. persistent loop
@PRECS
def test_persistent_loop(dev, rec, prec):
    """den_loop_kernel<false / true> on a max_batch 2049 handle: 2049 motions = 257 workgroups, one more than the chip has CUs (a second round), with a single
    motion in the last one; 2048 and 2041 (a ragged last workgroup of the first round); 17, 16, 9, 8, 7, 1.  One launch behind the condition rows."""
    for steps, bs in _handles(BE.PERSISTENT_BS):
        e = _engine(prec, 2049, steps, {"loop_kernel": 3})
        try:
            for B in bs:
                lat, launches = _call(e, dev, steps, B)
                name = "persistent, %s, %d steps, B %d" % (R.MODE[prec], steps, B)
                assert launches == 2, (name, launches)
                _rule(rec, name, lat, steps, B, prec)
            _status_ok(e, prec)
        finally:
            e.close()
    assert not rec.failures()


# ------------------------------------------------------------------ 4. cluster loop
def _cluster_or_skip(e):
    if e.numeric_status()["cluster_loop"] == 3:
        e.close()
        pytest.skip("another process holds the device's cluster lane: this handle runs no cluster launches")


def test_cluster_loop(dev, rec):
    """den_cluster_kernel<*, 8> up to 64 motions and <*, 4> above on an F16X3 max_batch 256 handle: 57, 64 | 65 (the last full launch of the 8-group form, the
    first of the 4-group form), 72 | 73 (9 | 10 clusters: idle slots of the second row of 8), 127, 128 | 129 (a second launch of one motion), 255, 256; 9, 8, 1; then
    the 4-group form forced at 64, 9, 1.  One launch per 128 motions behind the condition rows; no launch ran into its wait bound."""
    e = _engine(1, 256, 4, {"loop_kernel": 4})
    _cluster_or_skip(e)
    try:
        for cg, bs in ((0, BE.CLUSTER_BS), (4, BE.CLUSTER_G4_BS)):
            e.set_option("cluster_groups", cg)
            for B in bs:
                lat, launches = _call(e, dev, 4, B)
                name = "cluster, f16x3, cluster_groups %d, B %d" % (cg, B)
                assert launches == BE.cluster_launches(B), (name, launches)
                _rule(rec, name, lat, 4, B, 1)
        ns = _status_ok(e, 1)
        assert ns["cluster_loop"] == 1, ns
    finally:
        e.close()
    assert not rec.failures()


# ------------------------------------------------------------------ 5. automatic selection
CHAIN = R.chain_launches(2, 9)
# handle: (precision, max_batch, options, [(B, the forced "loop_kernel" auto must equal to the bit, its launch count, also unequal to the latency result)])
AUTO = {
    "f16x3 default": (1, 257, {}, [(256, 4, 3, False), (257, 3, 2, False)]),
    "f16x3 cluster_max_batch 0": (1, 192, {"cluster_max_batch": 0}, [(191, 1, CHAIN, False), (192, 3, 2, False)]),
    "f32": (0, 1280, {}, [(127, 1, CHAIN, False), (128, 2, CHAIN, True), (1279, 2, CHAIN, True), (1280, 3, 2, False)]),
}


@pytest.mark.parametrize("handle", list(AUTO))
def test_automatic_selection(dev, rec, handle):
    """"loop_kernel" 0 at every boundary of use_cluster / use_fused / use_strip (engine/path_loop.hpp), 2 steps: the result is the forced family's to the bit,
    with its launch count.  F16X3: cluster loop up to "cluster_max_batch" 256 (two launches above 128), persistent loop from 257; without the cluster loop the latency
    kernels up to 191 and the persistent loop from 192.  F32: latency kernels up to 127, throughput kernels from 128 ("strip_min_rows" 768 token rows) to 1 279,
    persistent loop from 1 280."""
    prec, max_batch, options, cases = AUTO[handle]
    e = _engine(prec, max_batch, 2, options)
    if any(lk == 4 for _, lk, _, _ in cases):
        _cluster_or_skip(e)
    try:
        for B, lk, want, unlike_latency in cases:
            e.set_option("loop_kernel", 0)
            auto, launches = _call(e, dev, 2, B)
            name = "auto, %s, B %d" % (handle, B)
            assert launches == want, (name, launches)
            _rule(rec, name, auto, 2, B, prec)
            e.set_option("loop_kernel", lk)
            forced, launches = _call(e, dev, 2, B)
            assert launches == want, (name, lk, launches)
            assert np.array_equal(auto, forced), (name, lk, float(np.abs(auto - forced).max()))
            if unlike_latency:
                e.set_option("loop_kernel", 1)
                other, _ = _call(e, dev, 2, B)
                assert np.isfinite(other).all() and not np.array_equal(auto, other), name
        _status_ok(e, prec)
    finally:
        e.close()
    assert not rec.failures()


# ------------------------------------------------------------------ 6. noise keys
# (name, "loop_kernel", "cluster_groups") of every family of a precision
KEY_FAMILIES = {0: [("latency", 1, 0), ("throughput", 2, 0), ("persistent", 3, 0)],
                1: [("latency", 1, 0), ("throughput", 2, 0), ("persistent", 3, 0), ("cluster_g4", 4, 4), ("cluster_g8", 4, 8)]}


def _eta_reference(b, first, n=None):
    n = n or len(b.lengths)
    return _cache.setdefault(("eta", n, first), oracle_eta(b.text_emb, b.init_latents, b.lengths, 1.0, BE.KEY_SEED, [first + m for m in range(n)], steps=2)[0])


def _seeded(e, dev, b, keys, sizes):
    """one request per key over consecutive slices of the batch; the latents [B, 1, 256] as numpy"""
    n, lo, reqs = len(b.lengths), 0, []
    for size in sizes:
        s = slice(lo, lo + size)
        reqs.append(dict(text_emb=_cuda(np.concatenate([b.text_emb[:n][s], b.text_emb[n:][s]], 0), dev), init_latents=_cuda(b.init_latents[s], dev),
                         lengths=b.lengths[s], latents_out=_nan(dev, size, 1, 256)))
        lo += size
    e.sample_many_seeded(reqs, keys)
    torch.cuda.synchronize()
    return np.concatenate([q["latents_out"].cpu().numpy() for q in reqs], 0)


@PRECS
def test_noise_keys_with_large_first_index(dev, rec, prec):
    """eta 1.0, 2 steps, 11 motions, first_index 2^25 - 4, 2^26 - 4, 2^31 - 4 and 2^40 + 3 through mldhip_sample_many_seeded on every family of the precision:
    each family draws z in its own code from the Philox quad index x 64 + q (den_final_step_eta_kernel, den_loop_kernel<*, kLoopEta>, den_cluster_eta_kernel) --
    the quad crosses 2^31 and 2^32 and the index 2^31 inside the call.  A draw from a truncated counter moves an element by sigma x |dz|, orders above the bound.
    Two requests whose keys continue each other equal the one-request call to the bit."""
    b = BE.key_batch()
    e = _engine(prec, 129 if prec == 1 else BE.KEY_MOTIONS, 2, eta=1.0)
    cluster = prec == 1
    if cluster:
        _cluster_or_skip(e)
    try:
        for first in BE.KEY_INDICES:
            ref = _eta_reference(b, first)
            for fam, lk, cg in KEY_FAMILIES[prec]:
                e.set_option("loop_kernel", lk)
                e.set_option("cluster_groups", cg)
                lat = _seeded(e, dev, b, [(BE.KEY_SEED, first)], [BE.KEY_MOTIONS])
                assert e.launch_counts()[0] == (R.chain_launches(2, 9) if lk in (1, 2) else 2), (fam, e.launch_counts())
                rec.bound("noise keys, %s, %s, first_index %d" % (R.MODE[prec], fam, first), lat, ref, BE.ETA_TOL)
        e.set_option("loop_kernel", 3)
        first = 2 ** 31 - 4
        one = _seeded(e, dev, b, [(BE.KEY_SEED, first)], [11])
        two = _seeded(e, dev, b, [(BE.KEY_SEED, first), (BE.KEY_SEED, first + 5)], [5, 6])
        assert np.isfinite(one).all() and np.array_equal(one, two)
        if cluster:
            # 129 motions: two cluster launches; motion 100 is index 2^26 (quad 2^32), the second launch starts at s_base 128
            first = 2 ** 26 - 100
            bb = syn.make_batch(129, [BE.LENGTH] * 129, seed=133)
            e.set_option("loop_kernel", 4)
            e.set_option("cluster_groups", 0)
            lat = _seeded(e, dev, bb, [(BE.KEY_SEED, first)], [129])
            assert e.launch_counts()[0] == 3, e.launch_counts()
            rec.bound("noise keys, f16x3, cluster, 129 motions, first_index %d" % first, lat, _eta_reference(bb, first), BE.ETA_TOL)
        ns = _status_ok(e, prec)
        if cluster:
            assert ns["cluster_loop"] == 1, ns
    finally:
        e.close()
    assert not rec.failures()


# ------------------------------------------------------------------ 7. grid-stride elementwise kernels
# 4 x 2^20 + 5 elements = 2^20 + 2 quads: two quads beyond one pass of the 4096 x 256 grid (the stochastic DDIM step: 1024 x 256, a fifth pass), the last one partial;
# 1, 5 and 1023 elements: a partial quad alone, one full and one partial quad, no full block
ELEMENT_NS = [4 * 1048576 + 5, 1, 5, 1023]
STREAM = (0x1234567890ABCDEF, 7)


def _elementwise_inputs(n):
    if ("elem", n) not in _cache:
        g = syn._rng(134, "elem%d" % n)
        # uniform in [-2, 2): the bounds below were set on 1 001 normal draws (|x| < 4); 4 M normal draws would reach the next binade
        _cache["elem", n] = (g.uniform(-2, 2, n).astype(np.float32), g.uniform(-2, 2, n).astype(np.float32), O.philox_normal(n, *STREAM))
    return _cache["elem", n]


@pytest.mark.parametrize("n", ELEMENT_NS)
def test_philox_normal_and_ddpm_step_beyond_one_grid_pass(dev, rec, n):
    """philox_normal_kernel and cfg_ddpm_step_kernel with NULL noise (the diffusion-only handle): the stream against oracle.philox_normal (2e-5: the same Philox bits,
    other log / cos / sin), the step with in-kernel noise against the step fed that stream (1e-6) and that against DDPMSchedule.step (2e-6) -- the bounds of
    tests/test_sim_kernels.py; the element behind the n-th keeps its NaN."""
    eps, x, zr = _elementwise_inputs(n)
    e = _lib.Engine(device=0, max_batch=2, max_frames=16, num_layers=1, ff_size=512, num_inference_steps=4, latent_dim=512, vae_arch=_lib.VAE_NONE,
                    denoiser_arch=_lib.ARCH_TRANS_DEC, scheduler_type=_lib.SCHED_DDPM, steps_offset=0)
    try:
        sch = O.DDPMSchedule()
        sch.set_timesteps(4)
        z = _nan(dev, n + 1)
        e.philox_normal(z, n, *STREAM)
        torch.cuda.synchronize()
        assert torch.isnan(z[n]).item()
        rec.bound("philox_normal, n %d" % n, z[:n].cpu().numpy(), zr, 2e-5)
        ed, xd = _cuda(eps, dev), _cuda(x, dev)
        o1, o2 = _nan(dev, n + 1), _nan(dev, n + 1)
        e.ddpm_step(ed, 500, xd, None, o1, n, seed=STREAM[0], step_index=STREAM[1])
        e.ddpm_step(ed, 500, xd, z, o2, n)
        torch.cuda.synchronize()
        assert torch.isnan(o1[n]).item() and torch.isnan(o2[n]).item()
        rec.bound("ddpm_step, in-kernel noise against the injected stream, n %d" % n, o1[:n].cpu().numpy(), o2[:n].cpu().numpy().astype(np.float64), 1e-6)
        rec.bound("ddpm_step, n %d" % n, o2[:n].cpu().numpy(), sch.step(eps, 500, x, z[:n].cpu().numpy()), 2e-6)
    finally:
        e.close()
    assert not rec.failures()


@pytest.mark.parametrize("n", ELEMENT_NS)
def test_ddim_step_eta_beyond_one_grid_pass(dev, rec, n):
    """ddim_step_eta_kernel with NULL noise on an eta 0.5 handle, t = 981 and 1 (the last step: the final alpha), against the numpy step of tests/test_ddim_eta.py
    fed oracle.philox_normal, within that file's 1e-5; the element behind the n-th keeps its NaN."""
    eps, x, zr = _elementwise_inputs(n)
    e = _lib.Engine(device=0, max_batch=2, max_frames=16, eta=0.5)
    try:
        ref = O.DDIMSchedule()
        ref.set_timesteps(50)
        ed, xd = _cuda(eps, dev), _cuda(x, dev)
        for t in (981, 1):
            out = _nan(dev, n + 1)
            e.ddim_step_eta(ed, t, xd, None, out, n, seed=STREAM[0], step_index=STREAM[1])
            torch.cuda.synchronize()
            assert torch.isnan(out[n]).item()
            rec.bound("ddim_step_eta, t %d, n %d" % (t, n), out[:n].cpu().numpy(), ddim_eta_step_np(eps, t, x, zr, 0.5, ref), 1e-5)
    finally:
        e.close()
    assert not rec.failures()
