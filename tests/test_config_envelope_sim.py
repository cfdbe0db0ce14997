"""The configuration envelope on the functional simulator (tests/hipemu): the twin of tests/test_gpu_config_envelope.py at the sizes the simulator can
afford -- 3 layers (one 7-layer, one-step case), 5 motions of lengths 24, 17, 1, 16, 9, 2 - 4 steps.  Every field mldhip_create accepts beyond the
three YAML configurations is varied at least once: ff_size 256 / 512, guidance_scale <= 1 and 3.0, steps_offset / set_alpha_to_one / betas, text_dim,
nfeats, the action engine at guidance 1.0, and MLD.forward with model.guidance_scale 1.0 (the modular HipMldDenoiser + HipDDIMScheduler loop on [B] rows).
The reference is the float64 oracle, the tolerances are tests/config_envelope_ref.py's.  "gemm_small_m" is lowered where a kernel arm only opens above it,
so the arm runs on a few dozen rows.  With MLDHIP_CONFIG_ENVELOPE_SIM_JSON set, every comparison is written there."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import config_envelope_ref as R  # noqa: E402
import simlib  # noqa: E402
from mld_hip import _lib  # noqa: E402
from mld_hip import synthetic as syn  # noqa: E402
from oracle import mld_oracle as O  # noqa: E402

LENS5 = [24, 17, 1, 16, 9]
_cache = {}


@pytest.fixture(scope="module")
def rec():
    r = R.Record("MLDHIP_CONFIG_ENVELOPE_SIM_JSON")
    yield r
    r.dump(what="max |simulator - fp64 oracle| of every case of tests/test_config_envelope_sim.py")


def _nan(*shape):
    return np.full(shape, np.nan, np.float32)


def _cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _engine(prec, weights, nfeats=syn.NFEATS, options=None, **cfg):
    cfg.setdefault("num_layers", 3)
    e = _lib.Engine(lib=simlib.sim_library(), use_graph=0, precision=prec, nfeats=nfeats, **cfg)
    try:
        e.load_state_dict(weights[0], "denoiser.")
        e.load_state_dict(weights[1], "vae.")
        mean, std = syn.make_mean_std(nfeats)
        e.load_tensor("mean", mean)
        e.load_tensor("std", std)
        for k, v in (options or {}).items():
            e.set_option(k, v)
        e.finalize()
    except Exception:
        e.close()
        raise
    return e


def _status_ok(e, prec):
    ns = e.numeric_status()
    assert ns["nonfinite_values"] == 0 and (prec == 0 or ns["loop_split_ok"] == 1), ns


def _sample_reference(weights, b, guidance, steps, sch_kw=None, nfeats=syn.NFEATS):
    mean, std = syn.make_mean_std(nfeats)

    def fn(ops, W):
        lat = O.diffusion_reverse(ops, W(weights[0]), ops.asarray(b.text_emb), ops.asarray(b.init_latents), guidance, steps, 4,
                                  schedule=O.DDIMSchedule(**(sch_kw or {})))
        feats = O.vae_decode(ops, W(weights[1]), lat, b.lengths)
        return lat, feats, O.feats2joints(ops, feats, ops.asarray(mean), ops.asarray(std))
    return R.reference(fn)


def _sample(e, b, nfeats=syn.NFEATS):
    B, T = len(b.lengths), max(b.lengths)
    lat, feats, joints = _nan(B, 1, 256), _nan(B, T, nfeats), _nan(B, T, 22, 3)
    e.sample(b.text_emb, b.init_latents, b.lengths, lat, feats, joints)
    return lat, feats, joints


def _check_sample(rec, name, prec, lens, out, ref):
    """latents by the relative rule, features within the decode bound (short samples), joints within the contract, padded feature frames exactly zero"""
    (lr, fr, jr), (el, _, _) = ref
    lat, feats, joints = out
    rec.rule(name + " latents", lat, lr, el, prec)
    rec.bound(name + " feats", feats, fr, R.OP_TOL)
    assert np.isfinite(joints).all(), name
    for i, n in enumerate(lens):
        assert np.all(feats[i, n:] == 0), (name, i)
        assert np.abs(joints[i, :n] - jr[i, :n]).max() < R.JOINT_TOL, (name, i)


# (name, "loop_kernel") of a precision at default widths: 0 = auto, the cluster loop for a small F16X3 call
FAMILIES = {0: [("latency", 1), ("throughput", 2), ("persistent", 3)], 1: [("latency", 1), ("persistent", 3), ("cluster", 4)]}


# ------------------------------------------------------------------ ff_size 256 and 512
@pytest.mark.parametrize("ff,prec", [(256, 0), (256, 1), (512, 1)], ids=["256-f32", "256-f16x3", "512-f16x3"])
def test_narrow_ffn_sim(rec, ff, prec):
    """ff_size 256 / 512: the reverse loop on gemm_tile32_kernel (nz0 = ffn_slabs = 1 / 2) and on gemm_strip_kernel + the 32x64 staged FFN2 (nz = 1 / 2), the
    decoder and the encoder on ffn_block's two GEMMs; "loop_kernel" 3 and 4 refused.  The encode of 5 x 24 frames is at the handle's capacity: its padded
    features (288 columns) are larger than the feed-forward rows at ff 256 -- the FF buffer is sized for both (carve_latent), a sample before and after the
    encode is bit-identical."""
    w = R.text_weights(num_layers=3, ff_size=ff)
    b = syn.make_batch(5, LENS5, seed=61)
    ref = _cached(("ff", ff), lambda: _sample_reference(w, b, 7.5, 2))
    e = _engine(prec, w, ff_size=ff, max_batch=5, max_frames=24, num_inference_steps=2)
    try:
        for lk in (3, 4):
            with pytest.raises(_lib.MldHipError):
                e.set_option("loop_kernel", lk)
        outs = {}
        for fam, lk in (("latency", 1), ("throughput", 2)):
            e.set_option("loop_kernel", lk)
            outs[fam] = _sample(e, b)
            assert e.launch_counts()[0] == R.chain_launches(2, 3)
            _check_sample(rec, "sim ff %d, %s, %s" % (ff, R.MODE[prec], fam), prec, LENS5, outs[fam], ref)
        # decode
        z = syn._rng(62, "simff").standard_normal((5, 1, 256)).astype(np.float32)
        (fr,) = _cached(("ffdec", ff), lambda: R.reference64(lambda ops, W: O.vae_decode(ops, W(w[1]), ops.asarray(z), LENS5)))
        feats = _nan(5, 24, 263)
        e.vae_decode(z, LENS5, feats)
        rec.bound("sim ff %d, %s, decode" % (ff, R.MODE[prec]), feats, fr, R.OP_TOL)
        # the capacity encode
        g = syn._rng(63, "simffenc")
        fe = g.standard_normal((5, 24, 263)).astype(np.float32)
        for i, n in enumerate(LENS5):
            fe[i, n:] = 0
        _, mr, lvr = _cached(("ffenc", ff), lambda: R.reference64(lambda ops, W: O.vae_encode(ops, W(w[1]), ops.asarray(fe), LENS5)))
        mu, lv = _nan(5, 1, 256), _nan(5, 1, 256)
        e.vae_encode(fe, LENS5, 24, None, None, mu, lv)
        rec.bound("sim ff %d, %s, encode mu" % (ff, R.MODE[prec]), mu, mr, R.OP_TOL)
        rec.bound("sim ff %d, %s, encode logvar" % (ff, R.MODE[prec]), lv, lvr, R.OP_TOL)
        again = _sample(e, b)
        assert all(np.array_equal(a, o) for a, o in zip(again, outs["throughput"]))
        _status_ok(e, prec)
    finally:
        e.close()
    assert not rec.failures()


# ------------------------------------------------------------------ guidance and the schedule
SCHEDULE = dict(steps_offset=0, set_alpha_to_one=1, beta_start=1e-4, beta_end=2e-2)
LOOP_CASES = {
    "guidance 0.5": dict(guidance_scale=0.5, num_inference_steps=2),
    "guidance 1.0": dict(guidance_scale=1.0, num_inference_steps=2),
    "guidance 3.0": dict(guidance_scale=3.0, num_inference_steps=2),
    "offset 0, alpha to one, betas 1e-4 .. 2e-2": dict(num_inference_steps=2, **SCHEDULE),
    "7 layers, 1 step": dict(num_layers=7, num_inference_steps=1),
}


# the simulator's time budget: guidance 0.5 and 1.0 are the same kernel arguments (one per precision); the deep case on the precision with four loop forms
LOOP_RUNS = [("guidance 0.5", 0), ("guidance 1.0", 1), ("guidance 3.0", 0), ("guidance 3.0", 1), ("offset 0, alpha to one, betas 1e-4 .. 2e-2", 0),
             ("offset 0, alpha to one, betas 1e-4 .. 2e-2", 1), ("7 layers, 1 step", 1)]


@pytest.mark.parametrize("case,prec", LOOP_RUNS, ids=["%s-%s" % (c, R.MODE[p]) for c, p in LOOP_RUNS])
def test_loop_arguments_sim(rec, case, prec):
    """guidance_scale 0.5, 1.0 (the conditional batch alone: the kernels run guidance 1.0 on the [2B] batch the C ABI takes) and 3.0; a schedule with
    steps_offset 0, set_alpha_to_one 1 and betas 1e-4 .. 2e-2; 7 layers (three skips) for one step -- on every loop family of the precision: the schedule
    tables against the oracle's, the final latents against fp64, the launch count of the family."""
    cfg, sch_kw, g = R.split_cfg(LOOP_CASES[case])
    n, L = cfg["num_inference_steps"], cfg.get("num_layers", 3)
    w = R.text_weights(num_layers=L)
    b = syn.make_batch(5, LENS5, seed=64)

    def ref_fn(ops, W):
        return O.diffusion_reverse(ops, W(w[0]), ops.asarray(b.text_emb), ops.asarray(b.init_latents), g, n, 4, schedule=O.DDIMSchedule(**sch_kw))
    (lr,), (el,) = _cached(("loop", case), lambda: R.reference(ref_fn))
    e = _engine(prec, w, max_batch=5, max_frames=24, **cfg)
    try:
        sch = O.DDIMSchedule(**sch_kw)
        np.testing.assert_array_equal(e.timesteps(), sch.set_timesteps(n))
        np.testing.assert_allclose(e.alphas_cumprod(), sch.alphas_cumprod, rtol=2e-6)
        for fam, lk in FAMILIES[prec]:
            e.set_option("loop_kernel", lk)
            lat = _nan(5, 1, 256)
            e.sample(b.text_emb, b.init_latents, LENS5, lat)
            assert e.launch_counts()[0] == (R.chain_launches(n, L) if lk in (1, 2) else 2), (fam, e.launch_counts())
            rec.rule("sim %s, %s, %s" % (case, R.MODE[prec], fam), lat, lr, el, prec)
        _status_ok(e, prec)
    finally:
        e.close()
    assert not rec.failures()


# ------------------------------------------------------------------ text_dim
@pytest.mark.parametrize("td,prec", [(96, 0), (512, 0), (512, 1)], ids=["96-f32", "512-f32", "512-f16x3"])
def test_text_dim_sim(rec, td, prec):
    """text_dim 96 (no staged K: the 16x64 register-direct shape) and 512 with "gemm_small_m" 0 set before finalize: the time MLP's linear_1 (finalize's table
    and the single row of mldhip_denoiser_forward) and the text projection on the staged 64x128 tile with 16 K chunks; then a 2-step sample."""
    w = R.text_weights(num_layers=3, text_dim=td)
    e = _engine(prec, w, text_dim=td, max_batch=5, max_frames=24, num_inference_steps=2, options={"gemm_small_m": 0})
    try:
        g = syn._rng(65, "simtd")
        x = g.standard_normal((6, 1, 256)).astype(np.float32)
        te = (0.5 * g.standard_normal((6, 1, td))).astype(np.float32)
        (ref,) = _cached(("tdden", td), lambda: R.reference64(lambda ops, W: O.denoiser_forward(ops, W(w[0]), ops.asarray(x), 981, ops.asarray(te))))
        out = _nan(6, 1, 256)
        e.denoiser_forward(x, 981, te, 6, out)
        rec.bound("sim text_dim %d, %s, denoiser_forward" % (td, R.MODE[prec]), out, ref, R.OP_TOL)
        b = syn.make_batch(5, LENS5, seed=66, dims=syn.ModelDims(text_dim=td))
        (lr,), (el,) = _cached(("tdloop", td), lambda: R.reference(
            lambda ops, W: O.diffusion_reverse(ops, W(w[0]), ops.asarray(b.text_emb), ops.asarray(b.init_latents), 7.5, 2, 4)))
        lat = _nan(5, 1, 256)
        e.sample(b.text_emb, b.init_latents, LENS5, lat)
        rec.rule("sim text_dim %d, %s, sample" % (td, R.MODE[prec]), lat, lr, el, prec)
        _status_ok(e, prec)
    finally:
        e.close()
    assert not rec.failures()


# ------------------------------------------------------------------ nfeats
@pytest.mark.parametrize("nf", [67, 257, 264, 265, 380])
def test_nfeats_decode_and_encode_sim(rec, nf):
    """nfeats 67, 257, 264, 265, 380 on an F16X3 handle with "gemm_small_m" 16, so that 2 x 24 rows are "many": MldVae.decode ends in final_strip_x3_kernel
    at 257 (one valid row in the third weight block) and 264 (the parking image full) -- one launch less than layernorm_rows + the ragged-N GEMM of the
    other widths; MldVae.encode's skel_embedding at K = 96, 288, 288, 288 (the 16x64 register-direct shape) and 384 (the fp32-only staged tile)."""
    w = R.text_weights(num_layers=3, nfeats=nf)
    lens = [24, 15]
    e = _engine(1, w, nfeats=nf, max_batch=2, max_frames=24, num_inference_steps=2, options={"gemm_small_m": 16})
    try:
        z = syn._rng(67, "simnf").standard_normal((2, 1, 256)).astype(np.float32)
        (fr,) = R.reference64(lambda ops, W: O.vae_decode(ops, W(w[1]), ops.asarray(z), lens))
        feats = _nan(2, 24, nf)
        e.vae_decode(z, lens, feats)
        _cache["nfcount", nf] = e.launch_counts()[1]
        rec.bound("sim nfeats %d, decode" % nf, feats, fr, R.OP_TOL)
        assert np.all(feats[1, 15:] == 0)
        fe = syn._rng(68, "simnfenc").standard_normal((2, 22, nf)).astype(np.float32)
        le = [22, 13]
        fe[1, 13:] = 0
        _, mr, lvr = R.reference64(lambda ops, W: O.vae_encode(ops, W(w[1]), ops.asarray(fe), le))
        mu, lv = _nan(2, 1, 256), _nan(2, 1, 256)
        e.vae_encode(fe, le, 22, None, None, mu, lv)
        rec.bound("sim nfeats %d, encode mu" % nf, mu, mr, R.OP_TOL)
        rec.bound("sim nfeats %d, encode logvar" % nf, lv, lvr, R.OP_TOL)
        _status_ok(e, 1)
    finally:
        e.close()
    if all(("nfcount", k) in _cache for k in (67, 257, 264, 265, 380)):      # (the last case of the file order; each case alone checks its numbers)
        c = {k: _cache["nfcount", k] for k in (67, 257, 264, 265, 380)}
        assert c[67] == c[265] == c[380] and c[257] == c[264] == c[67] - 1, c
    assert not rec.failures()


# ------------------------------------------------------------------ the action engine at guidance 1.0
@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f16x3"])
def test_action_engine_guidance_one_sim(rec, prec):
    """guidance_scale 1.0 on the action engine: action_rows_kernel zeroes no row in mldhip_denoiser_forward_action (the reference's EmbedAction masks the
    first half only when guidance_scale > 1), and mldhip_sample_action's u + 1 x (c - u) is the conditional half."""
    w = R.action_weights(simlib.SIM_ACTION_LAYERS, simlib.SIM_ACTOR_VAE_LAYERS, 12)
    e = _lib.Engine(lib=simlib.sim_library(), use_graph=0, precision=prec, guidance_scale=1.0, max_batch=5, max_frames=24, num_inference_steps=2,
                    **simlib.SIM_ACTION_CFG)
    try:
        e.load_state_dict(w[0], "denoiser.")
        e.load_state_dict(w[1], "vae.")
        e.finalize()
        g = syn._rng(69, "simact")
        acts = g.integers(0, 12, size=5).astype(np.int32)
        lat0 = g.standard_normal((5, 1, 256)).astype(np.float32)
        x, cond = np.concatenate([lat0, lat0]), np.concatenate([np.zeros_like(acts), acts])
        (ref,) = _cached("actden", lambda: R.reference64(lambda ops, W: O.denoiser_forward_action(ops, W(w[0]), ops.asarray(x), 741, cond, 4, 1.0)))
        out = _nan(10, 1, 256)
        e.denoiser_forward_action(x, 741, cond.tolist(), out)
        rec.bound("sim action guidance 1.0, %s, denoiser_forward_action" % R.MODE[prec], out, ref, R.OP_TOL)
        (fr, lr), (ef, el) = _cached("actsample", lambda: R.reference(
            lambda ops, W: O.sample_action(ops, W(w[0]), W(w[1]), acts, ops.asarray(lat0), LENS5, 1.0, 2, 4, return_intermediates=True)))
        lat, feats = _nan(5, 1, 256), _nan(5, 24, 150)
        e.sample_action(acts.tolist(), lat0, LENS5, lat, feats)
        rec.rule("sim action guidance 1.0, %s, sample_action latents" % R.MODE[prec], lat, lr, el, prec)
        rec.bound("sim action guidance 1.0, %s, sample_action feats" % R.MODE[prec], feats, fr, R.OP_TOL)
        for i, n in enumerate(LENS5):
            assert np.all(feats[i, n:] == 0)
        _status_ok(e, prec)
    finally:
        e.close()
    assert not rec.failures()


# ------------------------------------------------------------------ MLD.forward without classifier-free guidance
def test_mld_forward_guidance_one_runs_the_modular_loop_sim(rec):
    """model.guidance_scale 1.0: MLD.fused is false, so MLD.forward runs the reference's Python loop over HipMldDenoiser + HipDDIMScheduler on [B] rows (no CFG
    duplicate, no empty prompts), then HipMldVae.decode and feats2joints.  Against the fp64 oracle fed the same embeddings on both halves (u = c)."""
    from mld_hip import config as C
    from mld_hip import engine as E
    from mld_hip.datamodule import HipDataModule
    from mld_hip.mld import MLD
    from mld_hip.text_encoder import SyntheticTextEncoder

    steps = 2
    eng = _lib.Engine(lib=simlib.sim_library(), use_graph=0, max_batch=4, max_frames=24, num_inference_steps=steps, num_layers=3, guidance_scale=1.0)
    key = E.inject_engine(eng, "inject:config_envelope")
    try:
        cfg = C.load_config(overrides={"model.scheduler.num_inference_timesteps": steps, "model.denoiser.params.num_layers": 3,
                                       "model.motion_vae.params.num_layers": 3, "model.guidance_scale": 1.0})
        enc = SyntheticTextEncoder()
        model = MLD(cfg, HipDataModule(cfg, engine_key=key), text_encoder=enc, engine_key=key).eval()
        assert not model.fused and not model.do_classifier_free_guidance
        texts, lengths = ["a man kicks with his left leg.", "a person walks backward slowly.", "a person jumps."], [24, 17, 1]
        lat0 = syn.make_batch(3, lengths, seed=70).init_latents
        joints = model({"text": texts, "length": lengths}, init_latents=torch.from_numpy(lat0))
        emb = enc(texts).numpy()
        assert emb.shape[0] == 3
        w = simlib.text_weights()
        mean, std = syn.make_mean_std()
        b = syn.SyntheticBatch(np.concatenate([emb, emb]), lat0, lengths)

        def fn(ops, W):
            lat = O.diffusion_reverse(ops, W(w[0]), ops.asarray(b.text_emb), ops.asarray(lat0), 1.0, steps, 4)
            return lat, O.feats2joints(ops, O.vae_decode(ops, W(w[1]), lat, lengths), ops.asarray(mean), ops.asarray(std))
        (lr, jr), (el, _) = R.reference(fn)
        z = model._diffusion_reverse(torch.from_numpy(emb), lengths, init_latents=torch.from_numpy(lat0))      # [1, B, 256]
        rec.rule("sim MLD.forward guidance 1.0, modular loop latents", z.permute(1, 0, 2).numpy(), lr, el, 0)
        for i, n in enumerate(lengths):
            assert tuple(joints[i].shape) == (n, 22, 3)
            assert np.abs(joints[i].numpy() - jr[i, :n]).max() < R.JOINT_TOL
    finally:
        E._engines.pop(key, None)
        eng.close()
    assert not rec.failures()
