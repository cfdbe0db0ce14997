"""The batch-size edges on the functional simulator (tests/hipemu): the twin of tests/test_gpu_batch_edges.py at the sizes the simulator can afford -- a 3-layer
model, 1 step (2 for the noise keys), max_frames 16, every length 8, latents only.  Latency kernels (gemm_tile32_kernel) and throughput kernels (gemm_strip_kernel +
the staged FFN2) at B = 1, 2, 3, 5, 6, 8 (partial tiles, the 32-row tile with an empty second half), 43 and 86 (the 32-row switch of FFN2 and of the skip linear; 171,
the out-projection's, is marked slow); the persistent loop at 1, 7, 8, 9, 17 (ragged last workgroups); the cluster loop with 4 and 8 column groups at 1 and 9 motions
(slow); noise keys with first_index 2^25 - 4 .. 2^40 + 3 on the latency kernels and the persistent loop (one on the cluster loop, slow); oracle.philox_normal's
`first`.  Same reference (a prefix of one batch's float64 result), same rule and bounds as the GPU file (tests/batch_edges_ref.py).  The simulator runs neither the
machine code nor the real grid: what it checks is the index arithmetic of every form.  With MLDHIP_BATCH_EDGES_SIM_JSON set, every comparison is written there.

Measured (one run): the file takes 4 min 34 s (2 min 5 s of it in the tests marked slow; the eight-call latency + throughput list 45 - 52 s per precision);
the worst ratio to e32 is 1.40 on an F32 handle (bound 4) and 1.85 on an F16X3 one (bound 16), both at B = 1, whose e32 comes from a single motion; stochastic
calls end 3.0e-5 .. 8.5e-5 from the numpy loop (bound 5e-3) at |latents| up to 12.8."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import batch_edges_ref as BE  # noqa: E402
import config_envelope_ref as R  # noqa: E402
import simlib  # noqa: E402
from mld_hip import _lib  # noqa: E402
from mld_hip import synthetic as syn  # noqa: E402
from oracle import mld_oracle as O  # noqa: E402
from test_ddim_eta import reverse_eta_np  # noqa: E402

SIM_BMAX = 171
SMALL_BS = [86, 43, 8, 6, 5, 3, 2, 1]          # largest first: the small calls run on workspace rows the large ones wrote
PRECS = pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f16x3"])


@pytest.fixture(scope="module")
def rec():
    r = R.Record("MLDHIP_BATCH_EDGES_SIM_JSON")
    yield r
    r.dump(what="max |simulator - reference| of every case of tests/test_batch_edges_sim.py")


def _weights():
    return R.text_weights(num_layers=simlib.SIM_LAYERS)


def _engine(prec, max_batch, steps=1, options=None, **cfg):
    e = _lib.Engine(lib=simlib.sim_library(), use_graph=0, precision=prec, num_layers=simlib.SIM_LAYERS, max_batch=max_batch, max_frames=BE.MAX_FRAMES,
                    num_inference_steps=steps, **cfg)
    try:
        w = _weights()
        e.load_state_dict(w[0], "denoiser.")
        e.load_state_dict(w[1], "vae.")
        mean, std = syn.make_mean_std()
        e.load_tensor("mean", mean)
        e.load_tensor("std", std)
        e.finalize()
        for k, v in (options or {}).items():          # (behind finalize: "loop_kernel" 4 in front of it adds the cluster loop to finalize's probe, 20 s on the simulator)
            e.set_option(k, v)
    except Exception:
        e.close()
        raise
    return e


def _status_ok(e, prec):
    ns = e.numeric_status()
    assert ns["nonfinite_values"] == 0 and (prec == 0 or ns["loop_split_ok"] == 1), ns
    return ns


def _call(e, B):
    text, lat0, lens = BE.call_inputs(SIM_BMAX, B)
    lat = np.full((B, 1, 256), np.nan, np.float32)
    e.sample(text, lat0, lens, lat)
    return lat, e.launch_counts()[0]


def _rule(rec, name, got, B, prec):
    r64, e32 = BE.prefix(BE.loop_reference(_weights(), 1, SIM_BMAX, tag="sim"), B)
    return rec.rule(name, got, r64, e32, prec)


def _run_list(rec, family, lk, prec, max_batch, bs, launches_of, options=None):
    e = _engine(prec, max_batch, options={"loop_kernel": lk, **(options or {})})
    outs = {}
    try:
        for B in bs:
            lat, launches = _call(e, B)
            name = "sim %s, %s, B %d" % (family, R.MODE[prec], B)
            assert launches == launches_of(B), (name, launches)
            _rule(rec, name, lat, B, prec)
            outs[B] = lat
        ns = _status_ok(e, prec)
    finally:
        e.close()
    return outs, ns


# ------------------------------------------------------------------ oracle.philox_normal(first=)
def test_philox_normal_from_an_element_offset():
    """element first + i of the stream: a prefix stream's tail to the bit; above 2^32 quads (no prefix can be generated) a restatement on Python integers"""
    s, k = BE.KEY_SEED, 3
    assert np.array_equal(O.philox_normal(512, s, k, first=1024).view(np.uint32), O.philox_normal(1536, s, k)[1024:].view(np.uint32))
    assert np.array_equal(O.philox_normal(7, s, k, first=0).view(np.uint32), O.philox_normal(7, s, k).view(np.uint32))
    for quad in (5, 2 ** 31, 2 ** 32 - 1, 2 ** 32, (2 ** 40 + 3) * 64 + 63):
        assert np.abs(O.philox_normal(4, s, k, first=4 * quad) - BE.philox_quad_scalar(s, k, quad)).max() < 2e-6, quad
    # two quads on either side of 2^32: the low word wraps, the high word takes the carry
    z = O.philox_normal(8, s, k, first=4 * (2 ** 32 - 1))
    assert np.abs(z[4:] - BE.philox_quad_scalar(s, k, 2 ** 32)).max() < 2e-6
    with pytest.raises(ValueError):
        O.philox_normal(4, s, k, first=2)


# ------------------------------------------------------------------ latency and throughput kernels
@PRECS
def test_latency_and_throughput_kernels_sim(rec, prec):
    """B = 86, 43, 8, 6, 5, 3, 2, 1 on one max_batch 86 handle per family; where both ran, the two families differ in some bit (except B = 8, which the engine
    does not promise)"""
    lat, _ = _run_list(rec, "latency", 1, prec, 86, SMALL_BS, lambda B: R.chain_launches(1, 3))
    thr, _ = _run_list(rec, "throughput", 2, prec, 86, SMALL_BS, lambda B: R.chain_launches(1, 3))
    same = [B for B in SMALL_BS if B != 8 and np.array_equal(lat[B], thr[B])]
    assert not same, same
    assert not rec.failures()


@pytest.mark.slow
@PRECS
def test_latency_kernels_171_motions_sim(rec, prec):
    """B = 171: 32-row tiles in the out-projection with its in-register 3-token attention (11 x 4 x 1 tiles of 16 rows would be 260 > 256)"""
    _run_list(rec, "latency", 1, prec, 171, [171], lambda B: R.chain_launches(1, 3))
    assert not rec.failures()


# ------------------------------------------------------------------ persistent loop
@PRECS
def test_persistent_loop_sim(rec, prec):
    """B = 17, 9, 8, 7, 1: three, two and one workgroup, the last one with 1, 1, 8, 7 and 1 motions"""
    _run_list(rec, "persistent", 3, prec, 17, [17, 9, 8, 7, 1], lambda B: 2)
    assert not rec.failures()


# ------------------------------------------------------------------ cluster loop
@pytest.mark.slow
@pytest.mark.parametrize("groups", [4, 8])
def test_cluster_loop_sim(rec, groups):
    """den_cluster_kernel<*, 4> and <*, 8> at 9 motions (a full cluster and one of a single motion) and 1"""
    _, ns = _run_list(rec, "cluster_g%d" % groups, 4, 1, 9, [9, 1], lambda B: 2, {"cluster_groups": groups})
    assert ns["cluster_loop"] == 1, ns
    assert not rec.failures()


# ------------------------------------------------------------------ noise keys
_eta_ref = {}


def _key_case(rec, family, options, prec, first):
    b = BE.key_batch()
    n = BE.KEY_MOTIONS
    if first not in _eta_ref:
        _eta_ref[first] = reverse_eta_np(_weights()[0], b.text_emb, b.init_latents, 2, 1.0, [(BE.KEY_SEED, first + m) for m in range(n)])
    e = _engine(prec, n, steps=2, options=options, eta=1.0)
    try:
        lat = np.full((n, 1, 256), np.nan, np.float32)
        e.sample_many_seeded([dict(text_emb=b.text_emb, init_latents=b.init_latents, lengths=b.lengths, latents_out=lat)], [(BE.KEY_SEED, first)])
        rec.bound("sim noise keys, %s, %s, first_index %d" % (R.MODE[prec], family, first), lat, _eta_ref[first], BE.ETA_TOL)
        ns = _status_ok(e, prec)
    finally:
        e.close()
    assert not rec.failures()
    return ns


@pytest.mark.parametrize("first", BE.KEY_INDICES)
@pytest.mark.parametrize("family,lk,prec", [("latency", 1, 0), ("latency", 1, 1), ("persistent", 3, 0), ("persistent", 3, 1)],
                         ids=["latency-f32", "latency-f16x3", "persistent-f32", "persistent-f16x3"])
def test_noise_keys_with_large_first_index_sim(rec, family, lk, prec, first):
    """eta 1.0, 2 steps, 11 motions: den_final_step_eta_kernel and den_loop_kernel<*, kLoopEta> draw z from quad index x 64 + q with first_index 2^25 - 4 (the quad
    crosses 2^31), 2^26 - 4 (2^32), 2^31 - 4 (the index crosses 2^31) and 2^40 + 3, against the numpy loop fed oracle.philox_normal(first=)"""
    _key_case(rec, family, {"loop_kernel": lk}, prec, first)


@pytest.mark.slow
def test_noise_keys_with_large_first_index_cluster_sim(rec):
    """den_cluster_eta_kernel at first_index 2^26 - 4"""
    ns = _key_case(rec, "cluster", {"loop_kernel": 4}, 1, 2 ** 26 - 4)
    assert ns["cluster_loop"] == 1, ns
