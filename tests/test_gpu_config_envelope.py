"""Every model configuration mldhip_create accepts (config_error, csrc/engine/create.hpp), on the MI355X against the float64 oracle.

The three YAML configurations fix guidance 7.5, text_dim 768, nfeats 263 / 150, ff_size 1024 and 9 / 15 layers; the fields select kernels and
index arithmetic nothing else runs:
  A  guidance_scale, num_inference_steps, steps_offset / set_alpha_to_one / betas -> kernel arguments and finalize's tables of all four
     reverse-loop families (tile32 latency kernels, column-split strip kernels, den_loop_kernel, den_cluster_kernel<*, 4 / 8>)
  B  ff_size 256 / 512 -> no persistent loop, cluster loop or weight streams; ffn_slabs 1 / 2 in the loop; the staged GEMMs instead of
     ffn_strip / dec_tail / dec_l0_lean in the decoder and encoder; the encoder's padded features in the FF buffer (carve_latent)
  C  num_layers 3 .. 17 -> the skip stack S[8], the parking rows of the persistent and cluster loops to their declared depth
  D  nfeats 67 .. 380 -> final_strip_x3_kernel / final_joints_x3_kernel (256 < nfeats <= 264) or layernorm_rows + a ragged-N GEMM; the encoder's
     K = roundup(nfeats, 32) GEMM on the staged tile (256), the fp32 K = 384 tile or the 16x64 register-direct shape
  E  text_dim 96 .. 1024 -> the K = text_dim GEMMs of the time MLP and the text projection, small or staged
  F  action engines: nclasses, vae_num_layers, guidance <= 1 (no row gets the zero embedding)
  G  the diffusion-only variant: 1 and 24 layers, ff_size 512, guidance <= 1

The reference is always the float64 oracle; tolerances are tests/config_envelope_ref.py's.  Output buffers start NaN-filled, padded frames must
be exactly zero, every engine is closed.  With MLDHIP_CONFIG_ENVELOPE_JSON set, every comparison is written there (profiles/config_envelope.json
was written that way; measured there: the worst ratio to e32 is 2.5 on an F16X3 handle (bound 16), 2.4 on an F32 one (bound 4), 2.6 over the per-step
trajectories; the worst single-call or feature error 1.1e-5 against the 1e-4 bound).  For guidance_scale <= 1 the reference is the conditional batch alone -- the oracle at guidance 1.0; the C ABI still
takes the [2B] embeddings."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import config_envelope_ref as R  # noqa: E402
from mld_hip import _lib  # noqa: E402
from mld_hip import synthetic as syn  # noqa: E402
from oracle import mld_oracle as O  # noqa: E402
from test_gpu_ddim_eta import oracle_eta  # noqa: E402

pytestmark = pytest.mark.gpu

LENS11 = [24, 17, 1, 64, 9, 33, 48, 5, 40, 12, 3]          # one full workgroup / cluster of 8 motions and a ragged one of 3
# loop families of a precision: (name, "loop_kernel", "cluster_groups")
FAMILIES = {0: [("latency", 1, 0), ("throughput", 2, 0), ("persistent", 3, 0)],
            1: [("latency", 1, 0), ("persistent", 3, 0), ("cluster_g4", 4, 4), ("cluster_g8", 4, 8)]}
TRAJ_FAMILY = {0: "persistent", 1: "cluster_g8"}            # the family whose every step is compared (mldhip_sample_many_traj)

_cache = {}          # oracle results shared by the precisions and families


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def rec():
    r = R.Record("MLDHIP_CONFIG_ENVELOPE_JSON")
    yield r
    r.dump(what="max |engine - fp64 oracle| of every case of tests/test_gpu_config_envelope.py on an MI355X; e32 = the float32 CPU oracle's own error "
                "(the larger of NumpyOps(float32) and TorchOps('float32')); ratio = err / e32, bound by the factor of the handle's precision")


def _cuda(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _text_engine(prec, weights, nfeats=syn.NFEATS, options=None, **cfg):
    e = _lib.Engine(device=0, precision=prec, nfeats=nfeats, **cfg)
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
    assert ns["nonfinite_values"] == 0, ns
    if prec == 1:
        assert ns["loop_split_ok"] == 1, ns          # finalize's range probe passed: the split-f16 loops are what ran
    return ns


def _set_family(e, lk, cg):
    e.set_option("loop_kernel", lk)
    e.set_option("cluster_groups", cg)


def _loop_reference(weights, b, guidance, steps, sch_kw):
    """the reverse loop on the three backends, once: (fp64 final latents, their e32, fp64 latents after every step [n, B, 256], e32 of every step [n])"""
    trs = []
    for ops in R.backends():
        tr = []
        O.diffusion_reverse(ops, O.to_backend(ops, weights[0]), ops.asarray(b.text_emb), ops.asarray(b.init_latents), guidance, steps, 4,
                            schedule=O.DDIMSchedule(**sch_kw), trace=tr)
        trs.append(np.stack(tr)[:, :, 0].astype(np.float64))
    t64 = trs[0]
    e32 = np.maximum(*[np.abs(t - t64).reshape(steps, -1).max(1) for t in trs[1:]])
    return t64[-1][:, None, :], float(e32[-1]), t64, e32


def _sample_reference(weights, b, guidance, steps, nfeats=syn.NFEATS):
    """fp64 (latents, feats, joints) of a whole sample call on the default schedule, with e32"""
    mean, std = syn.make_mean_std(nfeats)

    def fn(ops, W):
        lat = O.diffusion_reverse(ops, W(weights[0]), ops.asarray(b.text_emb), ops.asarray(b.init_latents), guidance, steps, 4)
        feats = O.vae_decode(ops, W(weights[1]), lat, b.lengths)
        return lat, feats, O.feats2joints(ops, feats, ops.asarray(mean), ops.asarray(std))
    return R.reference(fn)


def _joint_err(j, jr, lens):
    return max(float(np.abs(j[i, :n] - jr[i, :n]).max()) for i, n in enumerate(lens))


def _check_sample(rec, name, prec, lens, lat, feats, joints, ref):
    """latents by the relative rule; the features of these short default-guidance samples within the bound tests/test_gpu_shape_edges.py has for them
    (test_sample_longest_and_shortest_motion: 4 steps, guidance 7.5); joints within the contract; padded feature frames exactly zero"""
    (lr, fr, jr), (el, _, _) = ref
    if lat is not None:
        rec.rule(name + " latents", lat.cpu().numpy(), lr, el, prec)
    if feats is not None:
        f = feats.cpu().numpy()
        rec.bound(name + " feats", f, fr, R.OP_TOL)
        for i, n in enumerate(lens):
            assert np.all(f[i, n:] == 0), (name, i)
    if joints is not None:
        j = joints.cpu().numpy()
        assert np.isfinite(j).all(), name
        err = _joint_err(j, jr, lens)
        rec.cases[name + " joints"] = {"err": err, "bound": R.JOINT_TOL}
        print("%s joints: err %.3e" % (name, err))
        assert err < R.JOINT_TOL, (name, err)


# ------------------------------------------------------------------ A. the four loop families under non-default arguments
A_CASES = {
    "guidance 0.5": dict(guidance_scale=0.5, num_inference_steps=10),
    "guidance 1.0": dict(guidance_scale=1.0, num_inference_steps=10),
    "guidance 1.5": dict(guidance_scale=1.5, num_inference_steps=10),
    "guidance 3.0": dict(guidance_scale=3.0, num_inference_steps=10),
    "guidance 12.0": dict(guidance_scale=12.0, num_inference_steps=10),
    "1 step": dict(num_inference_steps=1),
    "25 steps": dict(num_inference_steps=25),
    "100 steps": dict(num_inference_steps=100),
    "200 steps, guidance 1.5": dict(num_inference_steps=200, guidance_scale=1.5),
    "offset 0, alpha to one": dict(steps_offset=0, set_alpha_to_one=1, num_inference_steps=20),
    "betas 1e-4 .. 2e-2": dict(beta_start=1e-4, beta_end=2e-2, num_inference_steps=20),
}


@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f16x3"])
@pytest.mark.parametrize("case", list(A_CASES))
def test_loop_families_under_non_default_arguments(dev, rec, case, prec):
    """Default widths and depth, 11 motions (a full workgroup / cluster of 8 and a ragged one of 3): the final latents of gemm_tile32_kernel
    (latency), gemm_strip_kernel + the 32x64 staged FFN2 (throughput, F32), den_loop_kernel<false / true> (persistent) and
    den_cluster_kernel<*, 4> / <*, 8> (F16X3) against fp64; every step of one family per precision through mldhip_sample_many_traj; the schedule
    tables against the oracle's; the launch count of the family asked for.  guidance <= 1 runs the same kernels with guidance 1.0 on the [2B]
    batch the C ABI takes: the reference is the conditional batch alone."""
    cfg, sch_kw, g = R.split_cfg(A_CASES[case])
    n = cfg["num_inference_steps"]
    w = R.text_weights()
    b = syn.make_batch(11, LENS11, seed=91)
    lr, el, tr, e32_steps = _cached(("A", case), lambda: _loop_reference(w, b, g, n, sch_kw))
    e = _text_engine(prec, w, max_batch=11, max_frames=64, **cfg)
    try:
        sch = O.DDIMSchedule(**sch_kw)
        np.testing.assert_array_equal(e.timesteps(), sch.set_timesteps(n))
        np.testing.assert_allclose(e.alphas_cumprod(), sch.alphas_cumprod, rtol=2e-6)
        text, lat0 = _cuda(b.text_emb, dev), _cuda(b.init_latents, dev)
        outs = {}
        for fam, lk, cg in FAMILIES[prec]:
            _set_family(e, lk, cg)
            name = "A %s, %s, %s" % (case, R.MODE[prec], fam)
            q = dict(text_emb=text, init_latents=lat0, lengths=LENS11, latents_out=_nan(dev, 11, 1, 256))
            if fam == TRAJ_FAMILY[prec]:
                q["traj_out"] = _nan(dev, n, 11, 256)
            e.sample_many_traj([q], None)
            torch.cuda.synchronize()
            assert e.launch_counts()[0] == (R.chain_launches(n, 9) if lk in (1, 2) else 2), (name, e.launch_counts())
            outs[fam] = q["latents_out"].cpu().numpy()
            rec.rule(name, outs[fam], lr, el, prec)
            if "traj_out" in q:
                t = q["traj_out"].cpu().numpy().astype(np.float64)
                assert np.isfinite(t).all(), name
                assert torch.equal(q["traj_out"][n - 1], q["latents_out"][:, 0])
                err = np.abs(t - tr).reshape(n, -1).max(1)
                ratio = err / e32_steps
                s = int(ratio.argmax())
                rec.cases[name + " every step"] = {"worst_ratio": float(ratio[s]), "step": s, "err": float(err[s]), "e32": float(e32_steps[s]), "factor": R.FACTOR[prec]}
                print("%s every step: worst ratio %.2f at step %d (err %.3e, e32 %.3e)" % (name, ratio[s], s, err[s], e32_steps[s]))
                if not (err <= R.FACTOR[prec] * e32_steps).all():
                    rec.bad.append((name + " every step", s, float(err[s]), float(e32_steps[s])))
        _status_ok(e, prec)
        # the launch count cannot tell latency from throughput: they are different kernels (4 against 2 FFN2 slabs), another summation order, other bits
        if prec == 0:
            assert not np.array_equal(outs["latency"], outs["throughput"]), case
    finally:
        e.close()
    assert not rec.failures()


@pytest.mark.parametrize("family", ["cluster", "persistent"])
def test_stochastic_ddim_at_guidance_3(dev, rec, family):
    """eta = 0.5 at guidance 3.0, 10 steps, through mldhip_sample_many_seeded: den_cluster_eta_kernel and den_loop_kernel<true, kLoopEta> with a guidance
    other than 7.5, against the numpy loop of tests/test_gpu_ddim_eta.py fed the same Philox draws (a float32 reference: that file's bounds, latents
    5e-3 and joints 1e-3)."""
    b = syn.make_batch(11, LENS11, seed=92)
    seed, first = 0xBEEF, 5
    lr, jr = _cached("eta", lambda: oracle_eta(b.text_emb, b.init_latents, LENS11, 0.5, seed, [first + m for m in range(11)], steps=10, guidance=3.0))
    e = _text_engine(1, R.text_weights(), max_batch=11, max_frames=64, eta=0.5, guidance_scale=3.0, num_inference_steps=10)
    try:
        e.set_option("loop_kernel", 4 if family == "cluster" else 3)
        q = dict(text_emb=_cuda(b.text_emb, dev), init_latents=_cuda(b.init_latents, dev), lengths=LENS11, latents_out=_nan(dev, 11, 1, 256),
                 joints_out=_nan(dev, 11, 64, 22, 3))
        e.sample_many_seeded([q], [(seed, first)])
        torch.cuda.synchronize()
        assert e.launch_counts()[0] == 2
        rec.bound("A eta 0.5, guidance 3.0, %s latents" % family, q["latents_out"].cpu().numpy(), lr, 5e-3)
        err = _joint_err(q["joints_out"].cpu().numpy(), jr, LENS11)
        print("eta 0.5 %s joints: err %.3e" % (family, err))
        assert err < R.JOINT_TOL
        _status_ok(e, 1)
    finally:
        e.close()
    assert not rec.failures()


# ------------------------------------------------------------------ B. ff_size 256 and 512
@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f16x3"])
@pytest.mark.parametrize("ff", [256, 512])
def test_narrow_ffn_sample(dev, rec, ff, prec):
    """ff_size 256 / 512, 9 layers, 11 motions, 4 steps: gemm_tile32_kernel with nz0 = ffn_slabs = 1 / 2 (latency; split-f16 operands on an F16X3
    handle) and gemm_strip_kernel + the 32x64 staged FFN2 with Kz = 256 and nz = 1 / 2 (throughput), then the decoder on the two staged GEMMs of
    ffn_block (no ffn_strip_x3_kernel, no dec_tail, no weight streams) and layernorm_rows + the final GEMM.  The persistent loop and the cluster loop
    are not built for these widths: "loop_kernel" 3 and 4 are refused, and auto never picks them -- a 300-motion, 8-frame, 1-step call runs a launch per GEMM
    and matches the oracle."""
    w = R.text_weights(ff_size=ff)
    b = syn.make_batch(11, LENS11, seed=93)
    ref = _cached(("B", ff), lambda: _sample_reference(w, b, 7.5, 4))
    e = _text_engine(prec, w, ff_size=ff, max_batch=11, max_frames=64, num_inference_steps=4)
    try:
        for lk in (3, 4):
            with pytest.raises(_lib.MldHipError) as ei:
                e.set_option("loop_kernel", lk)
            assert ei.value.code == -1
        assert e.numeric_status()["cluster_loop"] == 0
        text, lat0 = _cuda(b.text_emb, dev), _cuda(b.init_latents, dev)
        outs = {}
        for fam, lk in (("latency", 1), ("throughput", 2), ("auto", 0)):
            e.set_option("loop_kernel", lk)
            lat, feats, joints = _nan(dev, 11, 1, 256), _nan(dev, 11, 64, 263), _nan(dev, 11, 64, 22, 3)
            e.sample(text, lat0, LENS11, lat, feats, joints)
            torch.cuda.synchronize()
            assert e.launch_counts()[0] == R.chain_launches(4, 9)
            outs[fam] = lat.cpu().numpy()
            _check_sample(rec, "B ff %d, %s, %s" % (ff, R.MODE[prec], fam), prec, LENS11, lat, feats, joints, ref)
        assert not np.array_equal(outs["latency"], outs["throughput"])
        assert np.array_equal(outs["auto"], outs["latency"])            # 66 token rows: below "strip_min_rows"
        _status_ok(e, prec)
    finally:
        e.close()
    lens = [1 + (5 * i) % 8 for i in range(300)]
    bb = syn.make_batch(300, lens, seed=94)
    lr, el, _, _ = _cached(("B300", ff), lambda: _loop_reference(w, bb, 7.5, 1, {}))
    e = _text_engine(prec, w, ff_size=ff, max_batch=300, max_frames=8, num_inference_steps=1)
    try:
        lat = _nan(dev, 300, 1, 256)
        e.sample(_cuda(bb.text_emb, dev), _cuda(bb.init_latents, dev), lens, lat)
        torch.cuda.synchronize()
        assert e.launch_counts()[0] == R.chain_launches(1, 9)          # 300 motions: where ff 1024 takes the persistent loop (F16X3) -- here a launch per GEMM
        rec.rule("B ff %d, %s, auto at 300 motions" % (ff, R.MODE[prec]), lat.cpu().numpy(), lr, el, prec)
        _status_ok(e, prec)
    finally:
        e.close()
    assert not rec.failures()


B_TS = [16, 64, 160, 288]


@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f16x3"])
@pytest.mark.parametrize("ff", [256, 512])
def test_narrow_ffn_decode_and_encode_to_capacity(dev, rec, ff, prec):
    """ff_size 256 / 512 on a max_batch 2, max_frames 288 handle: MldVae.decode at T = 16, 64, 160, 288 and MldVae.encode at T = 16, 64, 160, 286 (the
    encoder's cap), lengths [T, 5T/8].  2 x 160 rows are above "gemm_small_m": the staged 64x128 tile and gemm_ln (K = 256 / 512) in the handle's
    precision; below it the 16x64 register-direct shape.  The encoder pads the features to 288 columns into the FF buffer: at ff 256, T = 286 this
    is the capacity encode that needs carve_latent's max(F, KP) -- a sample on the same handle before and after it is bit-identical.  "ffn_strip",
    "dec_tail", "dec_lean" and "dec_l0_once" set to their defaults change nothing: those kernels are not built for these widths."""
    w = R.text_weights(ff_size=ff)
    e = _text_engine(prec, w, ff_size=ff, max_batch=2, max_frames=288, num_inference_steps=4)
    try:
        b = syn.make_batch(2, [288, 1], seed=95)
        text, lat0 = _cuda(b.text_emb, dev), _cuda(b.init_latents, dev)

        def sample():
            lat, joints = _nan(dev, 2, 1, 256), _nan(dev, 2, 288, 22, 3)
            e.sample(text, lat0, b.lengths, lat, None, joints)
            torch.cuda.synchronize()
            return lat, joints
        before = sample()
        for T in B_TS:
            lens = [T, max(1, T * 5 // 8)]
            z = syn._rng(41, f"envB{T}").standard_normal((2, 1, 256)).astype(np.float32)
            (fr,) = _cached(("Bdec", ff, T), lambda: R.reference64(lambda ops, W: O.vae_decode(ops, W(w[1]), ops.asarray(z), lens)))
            feats = _nan(dev, 2, T, 263)
            n0 = e.launch_counts()[1]          # (mldhip_vae_decode adds to the decode count; only a sample call resets it)
            e.vae_decode(_cuda(z, dev), lens, feats)
            torch.cuda.synchronize()
            n1 = e.launch_counts()[1]
            f = feats.cpu().numpy()
            rec.bound("B ff %d, %s, decode T %d" % (ff, R.MODE[prec], T), f, fr, R.OP_TOL)
            assert np.all(f[1, lens[1]:] == 0)
            for opt, val in (("ffn_strip", 1), ("dec_tail", 1), ("dec_lean", 1), ("dec_l0_once", 1)):
                e.set_option(opt, val)
            again = _nan(dev, 2, T, 263)
            e.vae_decode(_cuda(z, dev), lens, again)
            torch.cuda.synchronize()
            assert torch.equal(again, feats) and e.launch_counts()[1] - n1 == n1 - n0
            Te = min(T, 286)
            lens = [Te, max(1, Te * 5 // 8)]
            g = syn._rng(42, f"envB{Te}")
            fe = g.standard_normal((2, Te, 263)).astype(np.float32)
            fe[1, lens[1]:] = 0
            eps = g.standard_normal((2, 1, 256)).astype(np.float32)
            _, mr, lvr = _cached(("Benc", ff, Te), lambda: R.reference64(lambda ops, W: O.vae_encode(ops, W(w[1]), ops.asarray(fe), lens, ops.asarray(eps))))
            lat, mu, lv = (_nan(dev, 2, 1, 256) for _ in range(3))
            e.vae_encode(_cuda(fe, dev), lens, Te, _cuda(eps, dev), lat, mu, lv)
            torch.cuda.synchronize()
            assert torch.isfinite(lat).all()
            rec.bound("B ff %d, %s, encode T %d mu" % (ff, R.MODE[prec], Te), mu.cpu().numpy(), mr, R.OP_TOL)
            rec.bound("B ff %d, %s, encode T %d logvar" % (ff, R.MODE[prec], Te), lv.cpu().numpy(), lvr, R.OP_TOL)
        after = sample()
        assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
        _status_ok(e, prec)
    finally:
        e.close()
    assert not rec.failures()


# ------------------------------------------------------------------ C. depth
@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f16x3"])
@pytest.mark.parametrize("layers", [3, 5, 11, 17])
def test_depth(dev, rec, layers, prec):
    """num_layers 3, 5, 11, 17 at default widths, 11 motions, 4 steps, every family of the precision, with decode and joints.  17 layers fill the skip
    stack S[8] of the per-launch families and of the decoder, the FS parking rows of den_loop_kernel and cl_park of den_cluster_kernel<*, 4 / 8> to
    their declared depth of 8; 3 layers are the shallowest the SkipTransformer builds (one skip)."""
    w = R.text_weights(num_layers=layers)
    b = syn.make_batch(11, LENS11, seed=96)
    ref = _cached(("C", layers), lambda: _sample_reference(w, b, 7.5, 4))
    e = _text_engine(prec, w, num_layers=layers, max_batch=11, max_frames=64, num_inference_steps=4)
    try:
        text, lat0 = _cuda(b.text_emb, dev), _cuda(b.init_latents, dev)
        for fam, lk, cg in FAMILIES[prec]:
            _set_family(e, lk, cg)
            lat, feats, joints = _nan(dev, 11, 1, 256), _nan(dev, 11, 64, 263), _nan(dev, 11, 64, 22, 3)
            e.sample(text, lat0, LENS11, lat, feats, joints)
            torch.cuda.synchronize()
            assert e.launch_counts()[0] == (R.chain_launches(4, layers) if lk in (1, 2) else 2), (fam, e.launch_counts())
            _check_sample(rec, "C %d layers, %s, %s" % (layers, R.MODE[prec], fam), prec, LENS11, lat, feats, joints, ref)
        _status_ok(e, prec)
    finally:
        e.close()
    assert not rec.failures()


# ------------------------------------------------------------------ D. nfeats
NFEATS = [67, 256, 257, 264, 265, 380]
D_LENS = [160, 100, 1]                                       # 480 frame rows: above "gemm_small_m" (256)
D_SMALL = [40, 25]                                           # 80 rows: below it


def _nfeats_case(dev, rec, nf, prec):
    """every entry point of one (nfeats, precision) handle; returns the decode launch counts {call: count} (cached: the launch-count test reads all of them)"""
    if ("Dout", nf, prec) in _cache:
        return _cache["Dout", nf, prec]
    w = R.text_weights(nfeats=nf)
    mean, std = syn.make_mean_std(nf)
    tag = "D nfeats %d, %s" % (nf, R.MODE[prec])
    counts = {}
    e = _text_engine(prec, w, nfeats=nf, max_batch=3, max_frames=160, num_inference_steps=2)
    try:
        # MldVae.decode above and below "gemm_small_m"
        for lens in (D_LENS, D_SMALL):
            B, T = len(lens), max(lens)
            z = syn._rng(43, f"envD{B}").standard_normal((B, 1, 256)).astype(np.float32)
            (fr,) = _cached(("Ddec", nf, B), lambda: R.reference64(lambda ops, W: O.vae_decode(ops, W(w[1]), ops.asarray(z), lens)))
            feats = _nan(dev, B, T, nf)
            n0 = e.launch_counts()[1]          # (mldhip_vae_decode adds to the decode count; only a sample call resets it)
            e.vae_decode(_cuda(z, dev), lens, feats)
            torch.cuda.synchronize()
            counts["decode %d rows" % (B * T)] = e.launch_counts()[1] - n0
            f = feats.cpu().numpy()
            rec.bound("%s, decode %d rows" % (tag, B * T), f, fr, R.OP_TOL)
            for i, n in enumerate(lens):
                assert np.all(f[i, n:] == 0)
        # sample: joints only, features only, both
        b = syn.make_batch(3, D_LENS, seed=97)
        ref = _cached(("Dsample", nf), lambda: _sample_reference(w, b, 7.5, 2, nfeats=nf))
        text, lat0 = _cuda(b.text_emb, dev), _cuda(b.init_latents, dev)
        for what in ("joints", "feats", "both"):
            lat = _nan(dev, 3, 1, 256)
            feats = _nan(dev, 3, 160, nf) if what != "joints" else None
            joints = _nan(dev, 3, 160, 22, 3) if what != "feats" else None
            e.sample(text, lat0, D_LENS, lat, feats, joints)
            torch.cuda.synchronize()
            counts["sample " + what] = e.launch_counts()[1]
            _check_sample(rec, "%s, sample %s" % (tag, what), prec, D_LENS, lat, feats, joints, ref)
        # MldVae.encode: 2 x 158 frame rows above "gemm_small_m", 2 x 30 below
        for Te in (158, 30):
            lens = [Te, max(1, Te * 5 // 8)]
            g = syn._rng(44, f"envD{Te}")
            fe = g.standard_normal((2, Te, nf)).astype(np.float32)
            fe[1, lens[1]:] = 0
            _, mr, lvr = _cached(("Denc", nf, Te), lambda: R.reference64(lambda ops, W: O.vae_encode(ops, W(w[1]), ops.asarray(fe), lens)))
            mu, lv = _nan(dev, 2, 1, 256), _nan(dev, 2, 1, 256)
            e.vae_encode(_cuda(fe, dev), lens, Te, None, None, mu, lv)
            torch.cuda.synchronize()
            rec.bound("%s, encode T %d mu" % (tag, Te), mu.cpu().numpy(), mr, R.OP_TOL)
            rec.bound("%s, encode T %d logvar" % (tag, Te), lv.cpu().numpy(), lvr, R.OP_TOL)
        # feats2joints
        f = syn._rng(45, "envDf2j").standard_normal((2, 160, nf)).astype(np.float32)
        (jr,) = _cached(("Df2j", nf), lambda: R.reference64(lambda ops, W: O.feats2joints(ops, ops.asarray(f), ops.asarray(mean), ops.asarray(std))))
        joints = _nan(dev, 2, 160, 22, 3)
        e.feats2joints(_cuda(f, dev), 2, 160, joints)
        torch.cuda.synchronize()
        rec.bound("%s, feats2joints" % tag, joints.cpu().numpy(), jr, R.OP_TOL)
        _status_ok(e, prec)
    finally:
        e.close()
    _cache["Dout", nf, prec] = counts
    return counts


@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f16x3"])
@pytest.mark.parametrize("nf", NFEATS)
def test_nfeats(dev, rec, nf, prec):
    """nfeats 67, 256, 257, 264, 265, 380 with the MLD VAE and make_mean_std(nfeats).  Final stage of the decoder: final_strip_x3_kernel (F16X3, more than
    "gemm_small_m" rows, nfeats 257 -- a single valid row in the third weight block -- and 264 -- the parking image exactly full), final_joints_x3_kernel for
    the joints-only sample at the same two widths, layernorm_rows + a ragged-N GEMM everywhere else (67: joint_feat_cols == nfeats; 256 and 265: one column
    outside the strip's range on either side; 380; every F32 handle; 80 rows).  Encoder's skel_embedding at K = roundup(nfeats, 32): 96 and 288 (257, 264,
    265) on the 16x64 register-direct shape, 256 on the staged tile in the handle's precision and 384 on the fp32-only K = 384 tile once there are more than
    "gemm_small_m" rows (2 x 158), the register-direct shape below (2 x 30).  feats2joints_kernel<256> reads columns 0 .. 66 at row pitch nfeats."""
    _nfeats_case(dev, rec, nf, prec)
    assert not rec.failures()


def test_nfeats_final_stage_by_launch_count(dev, rec):
    """The row-strip final stage is one launch where layernorm_rows + GEMM are two: on an F16X3 handle the decode of 480 rows and all three sample forms
    take one launch less at nfeats 257 and 264 than at 67, 256, 265 and 380; at 80 rows, and on an F32 handle at any size, all widths launch alike."""
    c = {(nf, prec): _nfeats_case(dev, rec, nf, prec) for nf in NFEATS for prec in (0, 1)}
    rec.failures()                                           # (the parametrised test reports them)
    strip = (257, 264)
    for call in c[67, 0]:
        assert len({c[nf, 0][call] for nf in NFEATS}) == 1, (call, "f32", {nf: c[nf, 0][call] for nf in NFEATS})
        plain = {c[nf, 1][call] for nf in NFEATS if nf not in strip}
        assert len(plain) == 1, (call, {nf: c[nf, 1][call] for nf in NFEATS})
        want = plain.pop() - (0 if call == "decode 80 rows" else 1)
        assert all(c[nf, 1][call] == want for nf in strip), (call, {nf: c[nf, 1][call] for nf in NFEATS})


# ------------------------------------------------------------------ E. text_dim
# (text_dim, "gemm_small_m"): 0 only where it changes the arm -- 96 and 800 are no K the staged tile is built for
E_CASES = [(96, 256), (512, 256), (512, 0), (800, 256), (1024, 256), (1024, 0)]


@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f16x3"])
@pytest.mark.parametrize("td,small_m", E_CASES)
def test_text_dim(dev, rec, td, small_m, prec):
    """text_dim 96, 512, 800, 1024: the time MLP's linear_1 and the text projection are K = text_dim GEMMs (engine/dispatch.hpp gemm).  96 and 800 are no
    staged K: the 16x64 register-direct shape at any row count.  512 and 1024 take the staged 64x128 tile (K / 32 = 16 / 32 chunks) for the 300 text rows of
    mldhip_denoiser_forward at R = 300, and with "gemm_small_m" 0 (set before finalize) at R = 6, for the single time row and for finalize's table of
    all steps too.  Then a 4-step sample on every loop family: the families read the text rows and the time table these GEMMs wrote."""
    w = R.text_weights(text_dim=td)
    dims = syn.ModelDims(text_dim=td)
    tag = "E text_dim %d, %s, small_m %d" % (td, R.MODE[prec], small_m)
    e = _text_engine(prec, w, text_dim=td, max_batch=150, max_frames=64, num_inference_steps=4, options={"gemm_small_m": small_m})
    try:
        for Rr, t in ((6, 981), (300, 1)):
            g = syn._rng(46, f"envE{Rr}")
            x = g.standard_normal((Rr, 1, 256)).astype(np.float32)
            te = (0.5 * g.standard_normal((Rr, 1, td))).astype(np.float32)
            (ref,) = _cached(("Eden", td, Rr), lambda: R.reference64(lambda ops, W: O.denoiser_forward(ops, W(w[0]), ops.asarray(x), t, ops.asarray(te))))
            out = _nan(dev, Rr, 1, 256)
            e.denoiser_forward(_cuda(x, dev), t, _cuda(te, dev), Rr, out)
            torch.cuda.synchronize()
            rec.bound("%s, denoiser_forward R %d" % (tag, Rr), out.cpu().numpy(), ref, R.OP_TOL)
        b = syn.make_batch(11, LENS11, seed=98, dims=dims)
        lr, el, _, _ = _cached(("Eloop", td), lambda: _loop_reference(w, b, 7.5, 4, {}))
        text, lat0 = _cuda(b.text_emb, dev), _cuda(b.init_latents, dev)
        for fam, lk, cg in FAMILIES[prec]:
            _set_family(e, lk, cg)
            lat = _nan(dev, 11, 1, 256)
            e.sample(text, lat0, LENS11, lat)
            torch.cuda.synchronize()
            assert e.launch_counts()[0] == (R.chain_launches(4, 9) if lk in (1, 2) else 2), (fam, e.launch_counts())
            rec.rule("%s, %s" % (tag, fam), lat.cpu().numpy(), lr, el, prec)
        _status_ok(e, prec)
    finally:
        e.close()
    assert not rec.failures()


# ------------------------------------------------------------------ F. action engines
@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f16x3"])
@pytest.mark.parametrize("guidance", [1.0, 3.0])
@pytest.mark.parametrize("vae_layers", [0, 2])
@pytest.mark.parametrize("nclasses", [1, 40])
def test_action_engines(dev, rec, nclasses, vae_layers, guidance, prec):
    """Action condition, ActorVae, 5 denoiser layers, nfeats 150: nclasses 1 (every label 0) and 40; vae_num_layers 0 (= num_layers: 5 decoder and encoder
    layers) and 2; guidance 3.0 and 1.0 -- at 1.0 action_rows_kernel zeroes no row in mldhip_denoiser_forward_action (engine/serve.hpp), and the sample's
    u + 1 x (c - u) is the conditional half.  mldhip_denoiser_forward_action, mldhip_sample_action (4 steps, 11 motions), actor decode and encode against
    O.denoiser_forward_action, O.sample_action, O.actor_decode, O.actor_encode."""
    Lv = vae_layers or 5
    w = R.action_weights(5, Lv, nclasses)
    tag = "F nclasses %d, vae_num_layers %d, guidance %g, %s" % (nclasses, vae_layers, guidance, R.MODE[prec])
    e = _lib.Engine(device=0, precision=prec, condition=_lib.COND_ACTION, nclasses=nclasses, vae_arch=_lib.VAE_ACTOR, vae_num_layers=vae_layers, num_layers=5,
                    nfeats=150, guidance_scale=guidance, max_batch=11, max_frames=64, num_inference_steps=4)
    try:
        e.load_state_dict(w[0], "denoiser.")
        e.load_state_dict(w[1], "vae.")
        e.finalize()
        g = syn._rng(47, f"envF{nclasses}")
        acts = g.integers(0, nclasses, size=11).astype(np.int32)
        lat0 = g.standard_normal((11, 1, 256)).astype(np.float32)
        # one denoiser call on the CFG batch of 22 rows
        x = np.concatenate([lat0, lat0])
        cond = np.concatenate([np.zeros_like(acts), acts])
        (ref,) = _cached(("Fden", nclasses, guidance), lambda: R.reference64(lambda ops, W: O.denoiser_forward_action(ops, W(w[0]), ops.asarray(x), 741, cond, 4, guidance)))
        out = _nan(dev, 22, 1, 256)
        e.denoiser_forward_action(_cuda(x, dev), 741, cond.tolist(), out)
        torch.cuda.synchronize()
        rec.bound(tag + ", denoiser_forward_action", out.cpu().numpy(), ref, R.OP_TOL)
        # the sample
        (fr, lr), (ef, el) = _cached(("Fsample", nclasses, Lv, guidance), lambda: R.reference(
            lambda ops, W: O.sample_action(ops, W(w[0]), W(w[1]), acts, ops.asarray(lat0), LENS11, guidance, 4, 4, return_intermediates=True)))
        lat, feats = _nan(dev, 11, 1, 256), _nan(dev, 11, 64, 150)
        e.sample_action(acts.tolist(), _cuda(lat0, dev), LENS11, lat, feats)
        torch.cuda.synchronize()
        # auto: the latency kernels on an F32 handle, one den_cluster_kernel<*, 8> launch on an F16X3 one (the loops are built for the action condition too)
        assert e.launch_counts()[0] == (R.chain_launches(4, 5) if prec == 0 else 2), e.launch_counts()
        rec.rule(tag + ", sample_action latents", lat.cpu().numpy(), lr, el, prec)
        f = feats.cpu().numpy()
        rec.rule(tag + ", sample_action feats", f, fr, ef, prec)
        for i, n in enumerate(LENS11):
            assert np.all(f[i, n:] == 0)
        # actor decode and encode
        lens = [64, 40, 1]
        g = syn._rng(47, "envF vae")                 # (the references of the VAE calls are shared by the label counts)
        z = g.standard_normal((3, 1, 256)).astype(np.float32)
        (dr,) = _cached(("Fdec", Lv), lambda: R.reference64(lambda ops, W: O.actor_decode(ops, W(w[1]), ops.asarray(z), lens)))
        feats = _nan(dev, 3, 64, 150)
        e.vae_decode(_cuda(z, dev), lens, feats)
        torch.cuda.synchronize()
        f = feats.cpu().numpy()
        rec.bound(tag + ", actor decode", f, dr, R.OP_TOL)
        for i, n in enumerate(lens):
            assert np.all(f[i, n:] == 0)
        fe = g.standard_normal((3, 62, 150)).astype(np.float32)
        lens = [62, 40, 1]
        for i, n in enumerate(lens):
            fe[i, n:] = 0
        mr, lvr = _cached(("Fenc", Lv), lambda: R.reference64(lambda ops, W: O.actor_encode(ops, W(w[1]), ops.asarray(fe), lens)[1:]))
        mu, lv = _nan(dev, 3, 256), _nan(dev, 3, 256)
        e.vae_encode(_cuda(fe, dev), lens, 62, None, None, mu, lv)
        torch.cuda.synchronize()
        rec.bound(tag + ", actor encode mu", mu.cpu().numpy(), mr[:, 0], R.OP_TOL)
        rec.bound(tag + ", actor encode logvar", lv.cpu().numpy(), lvr[:, 0], R.OP_TOL)
        _status_ok(e, prec)
    finally:
        e.close()
    assert not rec.failures()


# ------------------------------------------------------------------ G. the diffusion-only variant
NOVAE_CFG = dict(latent_dim=512, vae_arch=_lib.VAE_NONE, denoiser_arch=_lib.ARCH_TRANS_DEC, scheduler_type=_lib.SCHED_DDPM, steps_offset=0)


@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f16x3"])
@pytest.mark.parametrize("guidance", [1.0, 3.0])
@pytest.mark.parametrize("layers", [1, 24])
def test_diffusion_only_variant(dev, rec, layers, guidance, prec):
    """vae none / trans_dec / DDPM with 1 and 24 decoder layers and ff_size 512, guidance 3.0 and 1.0 (cfg_ddpm_step_kernel with guidance 1.0 on the [2B]
    batch), B = 2, T = 40 (lengths 40 and 25), 4 DDPM steps with injected noise, "cross_fold" 1 (layer 0 on the de-duplicated CFG half, cross2_fold_ln_kernel)
    and 0.  The K = 512 feed-forward GEMMs run on the staged 64x128 tile with 16 chunks where ff 1024 has 32."""
    w = R.novae_weights(layers, 512)
    lens = [40, 25]
    g = syn._rng(48, "envG")
    lat0 = g.standard_normal((2, 40, 263)).astype(np.float32)
    te = (0.5 * g.standard_normal((4, 1, 768))).astype(np.float32)
    noise = g.standard_normal((4, 2, 40, 263)).astype(np.float32)
    ge = guidance if guidance > 1.0 else 1.0
    (fr,), (ef,) = _cached(("G", layers, guidance), lambda: R.reference(
        lambda ops, W: O.sample_novae(ops, W(w), ops.asarray(te), ops.asarray(lat0), lens, ops.asarray(noise), guidance_scale=ge, steps=4)))
    e = _lib.Engine(device=0, precision=prec, num_layers=layers, ff_size=512, guidance_scale=guidance, max_batch=2, max_frames=40, num_inference_steps=4, **NOVAE_CFG)
    try:
        e.load_state_dict(w, "denoiser.")
        mean, std = syn.make_mean_std()
        e.load_tensor("mean", mean)
        e.load_tensor("std", std)
        e.finalize()
        for fold in (1, 0):
            e.set_option("cross_fold", fold)
            feats = _nan(dev, 2, 40, 263)
            e.sample_novae(_cuda(te, dev), _cuda(lat0, dev), lens, _cuda(noise, dev), 0, feats, None)
            torch.cuda.synchronize()
            f = feats.cpu().numpy()
            # (all 40 rows of both motions: the result IS the latent, whose padded rows keep their noise -- only the predicted noise is zero there)
            rec.rule("G %d layers, guidance %g, %s, cross_fold %d" % (layers, guidance, R.MODE[prec], fold), f, fr, ef, prec)
        assert e.numeric_status()["nonfinite_values"] == 0
    finally:
        e.close()
    assert not rec.failures()
