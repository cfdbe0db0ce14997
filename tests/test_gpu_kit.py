"""KIT-ML (21 joints, 251 features) on the MI355X against the float64 oracle: every entry point of a 21 / 251 handle in both precisions, the two-block
one-launch final stage of MldVae.decode (final_strip2_x3_kernel) by launch count against its neighbours 256 and 257, the joints-only form, graph replay,
mldhip_sample_many, the diffusion-only variant at that width and the Python surface with configs/config_mld_kit.yaml.  Tolerances are
tests/config_envelope_ref.py's; output buffers start NaN-filled, padded frames must be exactly zero, every engine is closed.  With MLDHIP_KIT_ENVELOPE_JSON
set, every comparison is written there (profiles/kit_envelope.json was written that way)."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import config_envelope_ref as R  # noqa: E402
from mld_hip import _lib  # noqa: E402
from mld_hip import synthetic as syn  # noqa: E402
from oracle import mld_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

KIT_NF, KIT_NJ = 251, 21
LENS = [160, 37, 1]                                          # 480 frame rows: above "gemm_small_m" (256)
DEC_LENS, DEC_SMALL = [160, 100, 1], [40, 25]               # 480 rows and 80 rows
_cache = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def rec():
    r = R.Record("MLDHIP_KIT_ENVELOPE_JSON")
    yield r
    r.dump(what="max |engine - fp64 oracle| of every case of tests/test_gpu_kit.py on an MI355X; e32 = the float32 CPU oracle's own error; ratio = err / e32, "
                "bound by the factor of the handle's precision")


def _cuda(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _engine(prec, weights, nfeats=KIT_NF, njoints=KIT_NJ, **cfg):
    e = _lib.Engine(device=0, precision=prec, nfeats=nfeats, njoints=njoints, **cfg)
    try:
        e.load_state_dict(weights[0], "denoiser.")
        e.load_state_dict(weights[1], "vae.")
        mean, std = syn.make_mean_std(nfeats)
        e.load_tensor("mean", mean)
        e.load_tensor("std", std)
        e.finalize()
    except Exception:
        e.close()
        raise
    return e


def _status_ok(e, prec):
    ns = e.numeric_status()
    assert ns["nonfinite_values"] == 0, ns
    if prec == 1:
        assert ns["loop_split_ok"] == 1 and ns["decode_split_ok"] == 1, ns


def _sample_reference(w, b, lens, steps):
    mean, std = syn.make_mean_std(KIT_NF)

    def fn(ops, W):
        lat = O.diffusion_reverse(ops, W(w[0]), ops.asarray(b.text_emb), ops.asarray(b.init_latents), 7.5, steps, 4)
        feats = O.vae_decode(ops, W(w[1]), lat, lens)
        return lat, feats, O.feats2joints(ops, feats, ops.asarray(mean), ops.asarray(std), njoints=KIT_NJ)
    return R.reference(fn)


def _check_sample(rec, name, prec, lens, lat, feats, joints, ref):
    (lr, fr, jr), (el, _, _) = ref
    rec.rule(name + " latents", lat.cpu().numpy(), lr, el, prec)
    if feats is not None:
        f = feats.cpu().numpy()
        rec.bound(name + " feats", f, fr, R.OP_TOL)
        for i, n in enumerate(lens):
            assert np.all(f[i, n:] == 0), (name, i)
    if joints is not None:
        j = joints.cpu().numpy()
        assert np.isfinite(j).all(), name
        err = max(float(np.abs(j[i, :n] - jr[i, :n]).max()) for i, n in enumerate(lens))
        rec.cases[name + " joints"] = {"err": err, "bound": R.JOINT_TOL}
        print("%s joints: err %.3e" % (name, err))
        assert err < R.JOINT_TOL, (name, err)


def _decode_counts(dev, rec, nf, nj, prec):
    """decode of 480 and of 80 rows at (nf, nj): fp64 within OP_TOL, padded frames zero; returns {rows: launches} (cached)"""
    if ("dec", nf, prec) in _cache:
        return _cache["dec", nf, prec]
    w = R.text_weights(nfeats=nf)
    counts = {}
    e = _engine(prec, w, nf, nj, max_batch=3, max_frames=160, num_inference_steps=2)
    try:
        for lens in (DEC_LENS, DEC_SMALL):
            B, T = len(lens), max(lens)
            z = syn._rng(91, f"kitD{B}").standard_normal((B, 1, 256)).astype(np.float32)
            (fr,) = _cached(("decref", nf, B), lambda: R.reference64(lambda ops, W: O.vae_decode(ops, W(w[1]), ops.asarray(z), lens)))
            feats = _nan(dev, B, T, nf)
            n0 = e.launch_counts()[1]
            e.vae_decode(_cuda(z, dev), lens, feats)
            torch.cuda.synchronize()
            counts[B * T] = e.launch_counts()[1] - n0
            f = feats.cpu().numpy()
            rec.bound("nfeats %d, %s, decode %d rows" % (nf, R.MODE[prec], B * T), f, fr, R.OP_TOL)
            for i, n in enumerate(lens):
                assert np.all(f[i, n:] == 0)
        _status_ok(e, prec)
    finally:
        e.close()
    _cache["dec", nf, prec] = counts
    return counts


@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f16x3"])
def test_kit_decode(dev, rec, prec):
    """MldVae.decode of 3 x 160 frames (480 rows: above "gemm_small_m", final_strip2_x3_kernel on an F16X3 handle) and of 80 rows (staged) at 21 / 251"""
    _decode_counts(dev, rec, KIT_NF, KIT_NJ, prec)
    assert not rec.failures()


def test_kit_final_stage_by_launch_count(dev, rec):
    """On an F16X3 handle the decode of 480 rows at nfeats 251 takes one launch less than at 256 (layernorm_rows + the staged GEMM) and as many as at 257
    (final_strip_x3_kernel); at 80 rows, and on an F32 handle at either size, the three widths launch alike."""
    c = {(nf, prec): _decode_counts(dev, rec, nf, nj, prec) for nf, nj in ((KIT_NF, KIT_NJ), (256, 22), (257, 22)) for prec in (0, 1)}
    assert not rec.failures()
    assert c[KIT_NF, 1][480] == c[256, 1][480] - 1 == c[257, 1][480], c
    assert c[KIT_NF, 1][80] == c[256, 1][80] == c[257, 1][80], c
    for rows in (480, 80):
        assert c[KIT_NF, 0][rows] == c[256, 0][rows] == c[257, 0][rows], c


@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f16x3"])
def test_kit_sample_encode_joints(dev, rec, prec):
    """mldhip_sample at 21 / 251 (2 steps, lengths 160, 37, 1) asking for joints, features, both: latents by the relative rule, features within OP_TOL, joints
    within JOINT_TOL; the joints-only call (final_joints_x3_kernel, 64 columns at pitch 64, on an F16X3 handle) gives the bits of the call that also asks for
    features, and a second identical call replays the captured graph to the same bits.  mldhip_sample_many with a joints-only request and a longer one that
    asks for features (the whole call then runs the full form): each request equals its single call within the same bounds.  MldVae.encode at T = 158 and 30
    (K padded to 256), mldhip_feats2joints at T = 160 with 21 joints."""
    w = R.text_weights(nfeats=KIT_NF)
    mean, std = syn.make_mean_std(KIT_NF)
    tag = "kit %s" % R.MODE[prec]
    b = syn.make_batch(3, LENS, seed=92)
    ref = _cached("sample", lambda: _sample_reference(w, b, LENS, 2))
    lens2 = [64, 20]
    b2 = syn.make_batch(2, lens2, seed=93)
    ref2 = _cached("sample2", lambda: _sample_reference(w, b2, lens2, 2))
    e = _engine(prec, w, max_batch=5, max_frames=160, num_inference_steps=2)
    try:
        text, lat0 = _cuda(b.text_emb, dev), _cuda(b.init_latents, dev)
        out, counts = {}, {}
        for what in ("joints", "feats", "both"):
            for rep in range(2):                                 # the second call replays the graph of the first
                lat = _nan(dev, 3, 1, 256)
                feats = _nan(dev, 3, 160, KIT_NF) if what != "joints" else None
                joints = _nan(dev, 3, 160, KIT_NJ, 3) if what != "feats" else None
                e.sample(text, lat0, LENS, lat, feats, joints)
                torch.cuda.synchronize()
                if rep == 0:
                    counts[what] = e.launch_counts()[1]
                    out[what] = (lat, feats, joints)
                    _check_sample(rec, "%s, sample %s" % (tag, what), prec, LENS, lat, feats, joints, ref)
                else:
                    for a, o in zip((lat, feats, joints), out[what]):
                        assert a is None or torch.equal(a, o), (what, "replay")
        assert torch.equal(out["joints"][2], out["both"][2])
        assert torch.equal(out["feats"][1], out["both"][1]) and torch.equal(out["joints"][0], out["both"][0])
        assert counts["joints"] == counts["both"] == counts["feats"], counts
        _cache["samplecounts", prec] = counts
        # two requests, different Tmax: joints only / features too
        text2, lat02 = _cuda(b2.text_emb, dev), _cuda(b2.init_latents, dev)
        la, ja = _nan(dev, 3, 1, 256), _nan(dev, 3, 160, KIT_NJ, 3)
        lb, fb, jb = _nan(dev, 2, 1, 256), _nan(dev, 2, 64, KIT_NF), _nan(dev, 2, 64, KIT_NJ, 3)
        e.sample_many([dict(text_emb=text, init_latents=lat0, lengths=LENS, latents_out=la, joints_out=ja),
                       dict(text_emb=text2, init_latents=lat02, lengths=lens2, latents_out=lb, feats_out=fb, joints_out=jb)])
        torch.cuda.synchronize()
        _check_sample(rec, "%s, sample_many request 0" % tag, prec, LENS, la, None, ja, ref)
        _check_sample(rec, "%s, sample_many request 1" % tag, prec, lens2, lb, fb, jb, ref2)
        # encode
        for Te in (158, 30):
            lens = [Te, max(1, Te * 5 // 8)]
            g = syn._rng(94, f"kitE{Te}")
            fe = g.standard_normal((2, Te, KIT_NF)).astype(np.float32)
            fe[1, lens[1]:] = 0
            _, mr, lvr = _cached(("enc", Te), lambda: R.reference64(lambda ops, W: O.vae_encode(ops, W(w[1]), ops.asarray(fe), lens)))
            mu, lv = _nan(dev, 2, 1, 256), _nan(dev, 2, 1, 256)
            e.vae_encode(_cuda(fe, dev), lens, Te, None, None, mu, lv)
            torch.cuda.synchronize()
            rec.bound("%s, encode T %d mu" % (tag, Te), mu.cpu().numpy(), mr, R.OP_TOL)
            rec.bound("%s, encode T %d logvar" % (tag, Te), lv.cpu().numpy(), lvr, R.OP_TOL)
        # feats2joints
        f = syn._rng(95, "kitf2j").standard_normal((2, 160, KIT_NF)).astype(np.float32)
        (jr,) = _cached("f2j", lambda: R.reference64(lambda ops, W: O.feats2joints(ops, ops.asarray(f), ops.asarray(mean), ops.asarray(std), njoints=KIT_NJ)))
        joints = _nan(dev, 2, 160, KIT_NJ, 3)
        e.feats2joints(_cuda(f, dev), 2, 160, joints)
        torch.cuda.synchronize()
        rec.bound("%s, feats2joints" % tag, joints.cpu().numpy(), jr, R.OP_TOL)
        _status_ok(e, prec)
    finally:
        e.close()
    assert not rec.failures()


def _sample_counts(dev, nf, nj):
    """decode launches of the three sample forms on an F16X3 handle at (nf, nj)"""
    w = R.text_weights(nfeats=nf)
    b = syn.make_batch(3, LENS, seed=92)
    counts = {}
    e = _engine(1, w, nf, nj, max_batch=3, max_frames=160, num_inference_steps=2)
    try:
        text, lat0 = _cuda(b.text_emb, dev), _cuda(b.init_latents, dev)
        for what in ("joints", "feats", "both"):
            lat = _nan(dev, 3, 1, 256)
            feats = _nan(dev, 3, 160, nf) if what != "joints" else None
            joints = _nan(dev, 3, 160, nj, 3) if what != "feats" else None
            e.sample(text, lat0, LENS, lat, feats, joints)
            torch.cuda.synchronize()
            counts[what] = e.launch_counts()[1]
    finally:
        e.close()
    return counts


def test_kit_sample_final_stage_by_launch_count(dev):
    """every sample form at 251 on an F16X3 handle decodes with one launch less than the same form at nfeats 256 (no one-launch final stage there)
    and with as many as at 257 (the three-block kernel and the same joints-only kernel)"""
    kit = _cache.get(("samplecounts", 1)) or _sample_counts(dev, KIT_NF, KIT_NJ)
    c256, c257 = _sample_counts(dev, 256, 22), _sample_counts(dev, 257, 22)
    for what in ("joints", "feats", "both"):
        assert kit[what] == c256[what] - 1 == c257[what], (what, kit, c256, c257)


NOVAE_CFG = dict(latent_dim=512, vae_arch=_lib.VAE_NONE, denoiser_arch=_lib.ARCH_TRANS_DEC, scheduler_type=_lib.SCHED_DDPM, steps_offset=0)


@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f16x3"])
def test_kit_diffusion_only(dev, rec, prec):
    """vae none / trans_dec / DDPM at 251 / 21, one layer, B = 2, T = 64 (256 rows of the CFG batch), 4 DDPM steps with injected noise:
    pose_embd on K = 256 in the handle's precision (not the fp32-only K = 384 tile of 263), pose_proj with a ragged N = 251.  Features by the relative rule
    tests/test_gpu_config_envelope.py::test_diffusion_only_variant has for the same call; joints of the valid frames within JOINT_TOL."""
    sd = syn.make_novae_denoiser_state_dict(dims=syn.ModelDims(latent_dim=512, num_layers=1, nfeats=KIT_NF))
    lens = [64, 41]
    g = syn._rng(96, "kitG")
    lat0 = g.standard_normal((2, 64, KIT_NF)).astype(np.float32)
    te = (0.5 * g.standard_normal((4, 1, 768))).astype(np.float32)
    noise = g.standard_normal((4, 2, 64, KIT_NF)).astype(np.float32)
    mean, std = syn.make_mean_std(KIT_NF)

    def fn(ops, W):
        f = O.sample_novae(ops, W(sd), ops.asarray(te), ops.asarray(lat0), lens, ops.asarray(noise), steps=4)
        return f, O.feats2joints(ops, f, ops.asarray(mean), ops.asarray(std), njoints=KIT_NJ)
    (fr, jr), (ef, _) = _cached("novae", lambda: R.reference(fn))
    e = _lib.Engine(device=0, precision=prec, num_layers=1, nfeats=KIT_NF, njoints=KIT_NJ, max_batch=2, max_frames=64, num_inference_steps=4, **NOVAE_CFG)
    try:
        e.load_state_dict(sd, "denoiser.")
        e.load_tensor("mean", mean)
        e.load_tensor("std", std)
        e.finalize()
        feats, joints = _nan(dev, 2, 64, KIT_NF), _nan(dev, 2, 64, KIT_NJ, 3)
        e.sample_novae(_cuda(te, dev), _cuda(lat0, dev), lens, _cuda(noise, dev), 0, feats, joints)
        torch.cuda.synchronize()
        rec.rule("kit diffusion-only, %s, feats" % R.MODE[prec], feats.cpu().numpy(), fr, ef, prec)
        j = joints.cpu().numpy()
        err = max(float(np.abs(j[i, :n] - jr[i, :n]).max()) for i, n in enumerate(lens))
        rec.cases["kit diffusion-only, %s, joints" % R.MODE[prec]] = {"err": err, "bound": R.JOINT_TOL}
        print("kit diffusion-only %s joints: err %.3e" % (R.MODE[prec], err))
        assert err < R.JOINT_TOL
        assert e.numeric_status()["nonfinite_values"] == 0
    finally:
        e.close()
    assert not rec.failures()


def test_kit_mld_forward(dev, rec):
    """MLD(cfg_kit, HipDataModule(cfg_kit))(batch) with configs/config_mld_kit.yaml (4 steps): the registry creates a 21-joint, 251-feature handle from the
    datamodule's and the VAE's fields; [len_i, 21, 3] within JOINT_TOL of the oracle."""
    from mld_hip import config as C
    from mld_hip import engine as E
    from mld_hip.datamodule import HipDataModule
    from mld_hip.mld import MLD
    from mld_hip.text_encoder import SyntheticTextEncoder

    steps = 4
    before = {k: E._defaults["text"][k] for k in ("max_batch", "max_frames")}
    E.configure("text", max_batch=8, max_frames=64)
    try:
        cfg = C.load_config(os.path.join(C.CONFIG_DIR, "config_mld_kit.yaml"), overrides={"model.scheduler.num_inference_timesteps": steps})
        enc = SyntheticTextEncoder()
        model = MLD(cfg, HipDataModule(cfg), text_encoder=enc).to(dev).eval()
        texts, lengths = ["a person walks forward.", "a person waves the right hand.", "a person jumps."], [64, 37, 1]
        lat0 = syn.make_batch(3, lengths, seed=97).init_latents
        joints = model({"text": texts, "length": lengths}, init_latents=_cuda(lat0, dev))
        eng = model._engine()
        assert eng.cfg.njoints == KIT_NJ and eng.cfg.nfeats == KIT_NF
        emb = enc([""] * 3 + texts).cpu().numpy()
        sdd = {k: v.detach().cpu().numpy() for k, v in model.denoiser.state_dict().items()}
        sdv = {k: v.detach().cpu().numpy() for k, v in model.vae.state_dict().items()}
        dm = model.datamodule

        def fn(ops, W):
            lat = O.diffusion_reverse(ops, W(sdd), ops.asarray(emb), ops.asarray(lat0), 7.5, steps, 4)
            return O.feats2joints(ops, O.vae_decode(ops, W(sdv), lat, lengths), ops.asarray(dm.mean), ops.asarray(dm.std), njoints=KIT_NJ)
        (jr,) = R.reference64(fn)
        for i, n in enumerate(lengths):
            assert tuple(joints[i].shape) == (n, KIT_NJ, 3)
            err = float(np.abs(joints[i].numpy() - jr[i, :n]).max())
            rec.cases["kit MLD.forward motion %d joints" % i] = {"err": err, "bound": R.JOINT_TOL}
            print("kit MLD.forward motion %d: err %.3e" % (i, err))
            assert err < R.JOINT_TOL
        assert eng.numeric_status()["nonfinite_values"] == 0
    finally:
        E.drop_engines()
        E.configure("text", **before)
