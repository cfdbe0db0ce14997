"""Option "loop_lean" of the persistent reverse loop (kernels/loop_fused.hpp `full`) on the functional simulator: behind the last denoiser layer only the latent
token's rows are read, so that layer works on row tile 0 alone (its K and V products excepted).  Every tile-0 value is per row -- accumulators, row statistics,
scores, GELU -- and untouched by what is skipped, so "loop_lean" 1 must give the latents of "loop_lean" 0 TO THE BIT: np.array_equal, both operand formats,
"loop_kernel" 3, 2 steps, on
  - B = 3 (one workgroup, rows beyond B repeat motion B - 1) and B = 9 (a second workgroup with one real motion) of the 9-layer model, B = 9 of a 5-layer one;
  - one call each through the eta > 0, the from (a start step > 0 among the requests), the per-request guidance and the trajectory entry points (5 layers,
    requests of 5 + 4 motions: the second request straddles the two workgroups).
One case checks "loop_lean" 1 against the fp64 reference of tests/batch_edges_ref.py under the rule of tests/test_batch_edges_sim.py: equality alone could be two
wrong answers agreeing.  The simulator runs the same source as the GPU build with the branches taken per fiber; the machine code is checked by
tests/test_isa_properties.py and on the MI355X by tests/test_gpu_loop_lean.py."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import batch_edges_ref as BE  # noqa: E402
import config_envelope_ref as R  # noqa: E402
import simlib  # noqa: E402
from mld_hip import _lib  # noqa: E402
from mld_hip import synthetic as syn  # noqa: E402

f32 = np.float32
STEPS, BMAX = 2, 9
PRECS = pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f16x3"])
SEED, FIRST = 0x5EED_0F_1EA4, 5

_cache = {}


def engine(prec, layers, eta=0.0):
    """one engine per (format, depth, eta) for the module: a finalize on the simulator costs as much as a call"""
    key = ("engine", prec, layers, eta)
    if key not in _cache:
        e = _lib.Engine(lib=simlib.sim_library(), use_graph=0, precision=prec, num_layers=layers, max_batch=BMAX, max_frames=BE.MAX_FRAMES,
                        num_inference_steps=STEPS, eta=eta)
        w = R.text_weights(num_layers=layers)
        e.load_state_dict(w[0], "denoiser.")
        e.load_state_dict(w[1], "vae.")
        mean, std = syn.make_mean_std()
        e.load_tensor("mean", mean)
        e.load_tensor("std", std)
        e.finalize()
        e.set_option("loop_kernel", 3)
        _cache[key] = e
    return _cache[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for k, v in list(_cache.items()):
        if isinstance(v, _lib.Engine):
            v.close()
        del _cache[k]


def both(e, prec, run, nan_ok=()):
    """run() -> list of arrays, with "loop_lean" 0 and then 1: equal to the bit, finite, the same launches, a clean numeric status; returns the lean results"""
    outs, counts = [], []
    for lean in (0, 1):
        e.set_option("loop_lean", lean)
        outs.append(run())
        counts.append(e.launch_counts())
    ns = e.numeric_status()
    assert ns["nonfinite_values"] == 0 and (prec == 0 or ns["loop_split_ok"] == 1), ns
    assert counts[0] == counts[1] and counts[0][0] == 2, counts          # condition rows + ONE loop launch
    for i, (a, b) in enumerate(zip(*outs)):
        assert i in nan_ok or np.isfinite(b).all(), i
        assert np.array_equal(a, b, equal_nan=True), (i, float(np.nanmax(np.abs(a - b))))
    return outs[1]


def plain(prec, layers, B):
    key = ("plain", prec, layers, B)
    if key not in _cache:
        e = engine(prec, layers)
        text, lat0, lens = BE.call_inputs(BMAX, B)

        def run():
            lat = np.full((B, 1, 256), np.nan, f32)
            e.sample(text, lat0, lens, lat)
            return [lat]
        _cache[key] = both(e, prec, run)[0]
    return _cache[key]


@PRECS
@pytest.mark.parametrize("layers,B", [(9, 3), (9, 9), (5, 9)], ids=["L9-B3", "L9-B9", "L5-B9"])
def test_lean_last_layer_gives_the_same_latents(prec, layers, B):
    plain(prec, layers, B)


@PRECS
def test_lean_latents_against_fp64(prec):
    """"loop_lean" 1 on the 5-layer model, B = 9, against the float64 loop: the relative rule of tests/config_envelope_ref.py (4 x e32 on an F32 handle, 16 x on F16X3)"""
    rec = R.Record("MLDHIP_LOOP_LEAN_SIM_JSON")
    r64, e32 = BE.prefix(BE.loop_reference(R.text_weights(num_layers=5), STEPS, BMAX, tag="lean5"), BMAX)
    rec.rule("sim loop_lean 1, %s, 5 layers, B 9" % R.MODE[prec], plain(prec, 5, BMAX), r64, e32, prec)
    rec.dump(what="max |simulator - reference| of tests/test_loop_lean_sim.py")
    assert not rec.failures()


def requests(traj=False, starts=False, scales=False):
    """the batch's 9 motions as requests of 5 and 4 -> (requests, keys, [latents, trajectories ...])"""
    b = BE.batch(BMAX)
    src = np.random.default_rng(77).standard_normal((BMAX, 1, 256)).astype(f32) * f32(0.7)
    reqs, keys, outs = [], [], []
    for i, (m0, m1) in enumerate(((0, 5), (5, 9))):
        n = m1 - m0
        lat = np.full((n, 1, 256), np.nan, f32)
        q = dict(text_emb=np.ascontiguousarray(np.concatenate([b.text_emb[m0:m1], b.text_emb[BMAX + m0:BMAX + m1]], 0)),
                 init_latents=np.ascontiguousarray(b.init_latents[m0:m1]), lengths=[BE.LENGTH] * n, latents_out=lat)
        outs.append(lat)
        if traj:
            q["traj_out"] = np.full((STEPS, n, 256), np.nan, f32)
            outs.append(q["traj_out"])
        if starts and i == 1:                      # the second request enters at step 1 from a clean source: the first workgroup then holds both kinds
            q.update(src_latents=np.ascontiguousarray(src[m0:m1]), first_step=1, noised=0)
        if scales and i == 0:
            q["guidance"] = 2.5                    # the other request keeps the handle's 7.5
        reqs.append(q)
        keys.append((SEED, FIRST + m0))
    return reqs, keys, outs


def entry(prec, eta, call, nan_ok=(), **kw):
    e = engine(prec, 5, eta)

    def run():
        reqs, keys, outs = requests(**kw)
        getattr(e, call)(reqs, keys)
        return outs
    return both(e, prec, run, nan_ok)


def test_lean_through_the_eta_entry_point():
    """den_loop_kernel<true, kLoopEta>: eta 0.5, seeded"""
    entry(1, 0.5, "sample_many_seeded")


def test_lean_through_the_from_entry_point():
    """den_loop_kernel<false, kLoopFrom>: a request that starts at step 1 beside one that starts at 0; the skipped step's trajectory rows keep their NaN fill"""
    outs = entry(0, 0.0, "sample_many_from", nan_ok=(3,), traj=True, starts=True)
    assert np.isnan(outs[3][0]).all() and np.array_equal(outs[3][1], outs[2][:, 0])


def test_lean_through_the_guided_entry_point():
    """den_loop_kernel<true, kLoopFrom> on the start table's scales: 2.5 for the first request, the handle's for the second"""
    entry(1, 0.0, "sample_many_guided", scales=True)


def test_lean_through_the_trajectory_entry_point():
    """den_loop_kernel<false, 0> with a trajectory table: every step's row, the last one the latents"""
    outs = entry(0, 0.0, "sample_many_traj", traj=True)
    assert np.array_equal(outs[1][-1], outs[0][:, 0]) and np.array_equal(outs[3][-1], outs[2][:, 0])
