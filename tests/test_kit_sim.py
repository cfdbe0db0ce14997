"""KIT-ML (21 joints, 251 = 12 x 21 - 1 features) on the functional simulator: which skeletons mldhip_create accepts, the two-block one-launch final
stage of MldVae.decode (final_strip2_x3_kernel, 128 < nfeats < 256) with its joints-only form, every entry point of a 21 / 251 handle, the diffusion-only
variant at that width and the Python surface with configs/config_mld_kit.yaml.  The reference is the float64 oracle (oracle/mld_oracle.py takes njoints),
the tolerances are tests/config_envelope_ref.py's.  "gemm_small_m" 0 makes a few dozen rows "many", so the row-strip kernels run on them.  With
MLDHIP_KIT_SIM_JSON set, every comparison is written there."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import config_envelope_ref as R  # noqa: E402
import simlib  # noqa: E402
from mld_hip import _lib  # noqa: E402
from mld_hip import synthetic as syn  # noqa: E402
from oracle import mld_oracle as O  # noqa: E402

KIT_NF, KIT_NJ = 251, 21
_counts = {}


@pytest.fixture(scope="module")
def rec():
    r = R.Record("MLDHIP_KIT_SIM_JSON")
    yield r
    r.dump(what="max |simulator - fp64 oracle| of every case of tests/test_kit_sim.py")


def _nan(*shape):
    return np.full(shape, np.nan, np.float32)


def _engine(prec, weights, nfeats, njoints=22, options=None, **cfg):
    cfg.setdefault("num_layers", 3)
    e = _lib.Engine(lib=simlib.sim_library(), use_graph=0, precision=prec, nfeats=nfeats, njoints=njoints, **cfg)
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
    assert ns["nonfinite_values"] == 0 and (prec == 0 or (ns["loop_split_ok"] == 1 and ns["decode_split_ok"] == 1)), ns


# ------------------------------------------------------------------ accepted and refused skeletons
@pytest.mark.parametrize("nj,nf", [(21, 251), (22, 263), (22, 67), (1, 67), (43, 263)])
def test_skeletons_accepted(nj, nf):
    """1 <= njoints <= 64 with nfeats >= 4 + 3 (njoints - 1) on an MldVae handle (43 joints need 130 of 263 columns) and on a diffusion-only one"""
    e = _lib.Engine(lib=simlib.sim_library(), use_graph=0, num_layers=3, njoints=nj, nfeats=nf, max_batch=2, max_frames=24)
    assert e.cfg.njoints == nj and e.cfg.nfeats == nf
    e.close()
    e = _lib.Engine(lib=simlib.sim_library(), use_graph=0, num_layers=1, njoints=nj, nfeats=nf, max_batch=2, max_frames=24, **simlib.NOVAE_CFG)
    e.close()


@pytest.mark.parametrize("nj,nf", [(0, 263), (65, 263), (23, 67)])
def test_skeletons_refused(nj, nf):
    """no joints, more than 64, and 23 joints on 67 columns (they need 70): MLDHIP_EINVAL, the rule in mldhip_last_error"""
    for extra in ({"num_layers": 3}, {"num_layers": 1, **simlib.NOVAE_CFG}):
        with pytest.raises(_lib.MldHipError) as ei:
            _lib.Engine(lib=simlib.sim_library(), use_graph=0, njoints=nj, nfeats=nf, max_batch=2, max_frames=24, **extra)
        assert ei.value.code == -1, ei.value                    # MLDHIP_EINVAL
        msg = str(ei.value)
        assert "1 <= njoints <= 64" in msg and "4 + 3 (njoints - 1)" in msg, msg


def test_actor_handle_keeps_its_rule():
    """ActorVae joints need SMPL: njoints is not read, 25 (HumanAct12) is taken as before"""
    e = _lib.Engine(lib=simlib.sim_library(), use_graph=0, max_batch=2, max_frames=24, njoints=25, **simlib.SIM_ACTION_CFG)
    assert e.cfg.njoints == 25
    e.close()


# ------------------------------------------------------------------ the two-block final stage
def _decode_count(nf, lens=(24, 13, 7)):
    """decode launches of an F16X3 handle at nfeats nf, "gemm_small_m" 0 (cached)"""
    if nf not in _counts:
        w = R.text_weights(num_layers=3, nfeats=nf)
        e = _engine(1, w, nf, max_batch=3, max_frames=24, num_inference_steps=2, options={"gemm_small_m": 0})
        try:
            z = syn._rng(81, "kitcount").standard_normal((3, 1, 256)).astype(np.float32)
            feats = _nan(3, 24, nf)
            n0 = e.launch_counts()[1]
            e.vae_decode(z, list(lens), feats)
            _counts[nf] = e.launch_counts()[1] - n0
            assert np.isfinite(feats).all()
        finally:
            e.close()
    return _counts[nf]


@pytest.mark.parametrize("nf", [129, 251, 255])
def test_two_block_final_stage_decode_sim(rec, nf):
    """MldVae.decode on an F16X3 handle at nfeats 129 (one valid row in block 1), 251 (KIT-ML) and 255 (the upper edge): lengths [24, 13, 7] and
    [21, 5, 11] -- 72 and 63 rows: a full 48-row strip and a partial one of 24 / 15 rows (15 x 251 floats end off a 16-byte boundary) -- against fp64
    within OP_TOL, padded frames exactly zero in a NaN-filled buffer; a caller buffer 4 bytes off a 16-byte boundary gives the same bits as an aligned
    one (the kernel's 4-byte store path).  One launch less than at nfeats 256, the same count as at 257."""
    w = R.text_weights(num_layers=3, nfeats=nf)
    e = _engine(1, w, nf, max_batch=3, max_frames=24, num_inference_steps=2, options={"gemm_small_m": 0})
    try:
        for lens in ([24, 13, 7], [21, 5, 11]):
            T = max(lens)
            z = syn._rng(82, "kitdec%d" % T).standard_normal((3, 1, 256)).astype(np.float32)
            (fr,) = R.reference64(lambda ops, W: O.vae_decode(ops, W(w[1]), ops.asarray(z), lens))
            n = 3 * T * nf
            raw = _nan(n + 8)
            off = (-raw.ctypes.data // 4) % 4                    # floats to the next 16-byte boundary
            aligned = raw[off:off + n].reshape(3, T, nf)
            shifted_raw = _nan(n + 8)
            off2 = (-shifted_raw.ctypes.data // 4) % 4 + 1
            shifted = shifted_raw[off2:off2 + n].reshape(3, T, nf)
            assert aligned.ctypes.data % 16 == 0 and shifted.ctypes.data % 16 == 4
            n0 = e.launch_counts()[1]
            e.vae_decode(z, lens, aligned)
            count = e.launch_counts()[1] - n0
            e.vae_decode(z, lens, shifted)
            rec.bound("sim nfeats %d, decode %d rows" % (nf, 3 * T), aligned, fr, R.OP_TOL)
            assert np.array_equal(aligned, shifted), (nf, lens)
            for i, ln in enumerate(lens):
                assert np.all(aligned[i, ln:] == 0), (nf, lens, i)
            assert np.isnan(raw[:off]).all() and np.isnan(raw[off + n:]).all()                      # nothing outside the block
            assert np.isnan(shifted_raw[:off2]).all() and np.isnan(shifted_raw[off2 + n:]).all()
            if T == 24:
                assert count == _decode_count(256) - 1 == _decode_count(257), (count, _counts)
        _status_ok(e, 1)
    finally:
        e.close()
    assert not rec.failures()


def test_widths_128_and_256_stay_staged_sim():
    """the range is open at both ends: 128 and 256 launch what the two-launch widths (67, 265) launch"""
    assert _decode_count(128) == _decode_count(256) == _decode_count(265) == _decode_count(67) == _decode_count(257) + 1, _counts


# ------------------------------------------------------------------ a 21 / 251 handle
@pytest.fixture(scope="module")
def kit_weights():
    return R.text_weights(num_layers=3, nfeats=KIT_NF)


def test_kit_sample_forms_sim(rec, kit_weights):
    """mldhip_sample at 21 / 251, two steps, lengths [24, 17, 1], asking for joints only, features only, both: joints within JOINT_TOL of the fp64 oracle
    with njoints = 21; the joints-only call ends in final_joints_x3_kernel (NV = 64 columns at pitch 64) -- the same launch count as the full form, one less than
    the staged pair would give -- and its joints are the bits of the call that also asks for features."""
    w = kit_weights
    lens = [24, 17, 1]
    b = syn.make_batch(3, lens, seed=83)
    mean, std = syn.make_mean_std(KIT_NF)

    def fn(ops, W):
        lat = O.diffusion_reverse(ops, W(w[0]), ops.asarray(b.text_emb), ops.asarray(b.init_latents), 7.5, 2, 4)
        feats = O.vae_decode(ops, W(w[1]), lat, lens)
        return lat, feats, O.feats2joints(ops, feats, ops.asarray(mean), ops.asarray(std), njoints=KIT_NJ)
    (lr, fr, jr), (el, _, _) = R.reference(fn)
    assert jr.shape == (3, 24, KIT_NJ, 3)
    e = _engine(1, w, KIT_NF, KIT_NJ, max_batch=3, max_frames=24, num_inference_steps=2, options={"gemm_small_m": 0})
    out, counts = {}, {}
    try:
        for what in ("joints", "feats", "both"):
            lat = _nan(3, 1, 256)
            feats = _nan(3, 24, KIT_NF) if what != "joints" else None
            joints = _nan(3, 24, KIT_NJ, 3) if what != "feats" else None
            e.sample(b.text_emb, b.init_latents, lens, lat, feats, joints)
            counts[what] = e.launch_counts()
            out[what] = (lat, feats, joints)
            rec.rule("sim kit sample %s latents" % what, lat, lr, el, 1)
            if feats is not None:
                rec.bound("sim kit sample %s feats" % what, feats, fr, R.OP_TOL)
                for i, n in enumerate(lens):
                    assert np.all(feats[i, n:] == 0)
            if joints is not None:
                assert np.isfinite(joints).all()
                for i, n in enumerate(lens):
                    err = float(np.abs(joints[i, :n] - jr[i, :n]).max())
                    print("sim kit sample %s joints motion %d: err %.3e" % (what, i, err))
                    assert err < R.JOINT_TOL, (what, i, err)
        assert np.array_equal(out["joints"][2], out["both"][2])
        assert np.array_equal(out["feats"][1], out["both"][1])
        # decode launches: every form ends in ONE final-stage launch (the staged pair would add one to each)
        assert counts["joints"][1] == counts["both"][1] == counts["feats"][1], counts
        e.set_option("dec_lean", 0)                               # the full form for the joints-only call as well: the same count, hence the narrow kernel above was one launch too
        lat, joints = _nan(3, 1, 256), _nan(3, 24, KIT_NJ, 3)
        e.sample(b.text_emb, b.init_latents, lens, lat, None, joints)
        assert np.array_equal(joints, out["both"][2])
        _status_ok(e, 1)
    finally:
        e.close()
    # against a handle one column wider than the range's neighbour on the staged path: nfeats 256 launches one more in every form
    w256 = R.text_weights(num_layers=3, nfeats=256)
    e = _engine(1, w256, 256, 22, max_batch=3, max_frames=24, num_inference_steps=2, options={"gemm_small_m": 0})
    try:
        for what in ("joints", "both"):
            lat, joints = _nan(3, 1, 256), _nan(3, 24, 22, 3)
            feats = _nan(3, 24, 256) if what == "both" else None
            e.sample(b.text_emb, b.init_latents, lens, lat, feats, joints)
            assert e.launch_counts()[1] == counts[what][1] + 1, (what, e.launch_counts(), counts)
    finally:
        e.close()
    assert not rec.failures()


@pytest.mark.parametrize("prec", [1, 0], ids=["f16x3", "f32"])
def test_kit_encode_and_feats2joints_sim(rec, kit_weights, prec):
    """MldVae.encode at 251 features (skel_embedding's K padded to 256: the staged K = 256 tile with "gemm_small_m" 0) and mldhip_feats2joints on random
    features, T = 24, 21 joints; on an F32 handle both run the staged path, and so does its decode."""
    w = kit_weights
    mean, std = syn.make_mean_std(KIT_NF)
    e = _engine(prec, w, KIT_NF, KIT_NJ, max_batch=2, max_frames=24, num_inference_steps=2, options={"gemm_small_m": 0})
    try:
        g = syn._rng(84, "kitenc")
        fe = g.standard_normal((2, 22, KIT_NF)).astype(np.float32)
        le = [22, 13]
        fe[1, 13:] = 0
        _, mr, lvr = R.reference64(lambda ops, W: O.vae_encode(ops, W(w[1]), ops.asarray(fe), le))
        mu, lv = _nan(2, 1, 256), _nan(2, 1, 256)
        e.vae_encode(fe, le, 22, None, None, mu, lv)
        rec.bound("sim kit %s, encode mu" % R.MODE[prec], mu, mr, R.OP_TOL)
        rec.bound("sim kit %s, encode logvar" % R.MODE[prec], lv, lvr, R.OP_TOL)
        f = g.standard_normal((2, 24, KIT_NF)).astype(np.float32)
        (jr,) = R.reference64(lambda ops, W: O.feats2joints(ops, ops.asarray(f), ops.asarray(mean), ops.asarray(std), njoints=KIT_NJ))
        joints = _nan(2, 24, KIT_NJ, 3)
        e.feats2joints(f, 2, 24, joints)
        rec.bound("sim kit %s, feats2joints" % R.MODE[prec], joints, jr, R.OP_TOL)
        if prec == 0:
            lens = [24, 15]
            z = g.standard_normal((2, 1, 256)).astype(np.float32)
            (fr,) = R.reference64(lambda ops, W: O.vae_decode(ops, W(w[1]), ops.asarray(z), lens))
            feats = _nan(2, 24, KIT_NF)
            e.vae_decode(z, lens, feats)
            rec.bound("sim kit f32, decode", feats, fr, R.OP_TOL)
            assert np.all(feats[1, 15:] == 0)
        _status_ok(e, prec)
    finally:
        e.close()
    assert not rec.failures()


# ------------------------------------------------------------------ the diffusion-only variant
@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f16x3"])
def test_kit_diffusion_only_sim(prec):
    """vae none at 251 / 21, one layer, B = 2, T = 24, two DDPM steps with injected noise: pose_embd on K = novae_kp = 256 (the staged K = 256 tile in the
    handle's precision with "gemm_small_m" 0, not the fp32-only K = 384 tile of 263), the output linear with a ragged N = 251.  Features and joints within the
    bound tests/test_sim_kernels.py::test_novae_full_sample_sim has for the same call."""
    sd = syn.make_novae_denoiser_state_dict(dims=syn.ModelDims(latent_dim=512, num_layers=1, nfeats=KIT_NF))
    ops = O.TorchOps("float64")
    B, T, lens = 2, 24, [24, 13]
    b = syn.make_batch(B, lens, seed=85)
    g = syn._rng(85, "kitnovae")
    lat0 = g.standard_normal((B, T, KIT_NF)).astype(np.float32)
    noise = g.standard_normal((2, B, T, KIT_NF)).astype(np.float32)
    mean, std = syn.make_mean_std(KIT_NF)
    fr = O.sample_novae(ops, O.to_backend(ops, sd), ops.asarray(b.text_emb), ops.asarray(lat0), lens, ops.asarray(noise), steps=2)
    jr = O.feats2joints(ops, fr, ops.asarray(mean), ops.asarray(std), njoints=KIT_NJ)
    jr, fr = ops.to_numpy(jr), ops.to_numpy(fr)
    for small_m in (None, 0):
        e = _lib.Engine(lib=simlib.sim_library(), use_graph=0, precision=prec, num_layers=1, nfeats=KIT_NF, njoints=KIT_NJ, max_batch=B, max_frames=T,
                        num_inference_steps=2, **simlib.NOVAE_CFG)
        try:
            e.load_state_dict(sd, "denoiser.")
            e.load_tensor("mean", mean)
            e.load_tensor("std", std)
            if small_m is not None:
                e.set_option("gemm_small_m", small_m)
            e.finalize()
            feats, joints = _nan(B, T, KIT_NF), _nan(B, T, KIT_NJ, 3)
            e.sample_novae(b.text_emb, lat0, lens, noise, 0, feats, joints)
            ef, ej = float(np.abs(feats - fr).max()), float(np.abs(joints - jr).max())
            print("sim kit diffusion-only %s, gemm_small_m %s: feats err %.3e, joints err %.3e" % (R.MODE[prec], small_m, ef, ej))
            assert ef < 2e-4 and ej < 2e-4, (ef, ej)
            assert e.numeric_status()["nonfinite_values"] == 0
        finally:
            e.close()


# ------------------------------------------------------------------ the Python surface
def test_kit_yaml_and_datamodule():
    from mld_hip import config as C
    from mld_hip.datamodule import HipDataModule

    cfg = C.load_config(os.path.join(C.CONFIG_DIR, "config_mld_kit.yaml"))
    assert cfg.DATASET.NFEATS == KIT_NF and cfg.DATASET.NJOINTS == KIT_NJ and cfg.TEST.DATASETS == ["kit"]
    assert cfg.DATASET.KIT.FRAME_RATE == 12.5 and cfg.DATASET.KIT.UNIT_LEN == 4
    assert cfg.model.motion_vae.params.nfeats == KIT_NF and cfg.model.denoiser.params.nfeats == KIT_NF
    ml = C.load_config()
    for k in ("latent_dim", "ff_size", "num_layers", "num_head", "guidance_scale", "condition", "target"):
        assert cfg.model[k] == ml.model[k], k
    assert cfg.model.motion_vae.target == ml.model.motion_vae.target and cfg.model.denoiser.target == ml.model.denoiser.target
    dm = HipDataModule(cfg)
    assert (dm.name, dm.nfeats, dm.njoints, dm.stats) == ("kit", KIT_NF, KIT_NJ, "synthetic") and dm.mean.shape == (KIT_NF,)
    assert dm._arch == {"nfeats": KIT_NF, "njoints": KIT_NJ}
    dm = HipDataModule(name="kit")
    assert (dm.nfeats, dm.njoints) == (KIT_NF, KIT_NJ)
    # what the existing calls construct is what they constructed before
    dm = HipDataModule(ml)
    assert (dm.name, dm.nfeats, dm.njoints, dm.mean.shape) == ("humanml3d", 263, 22, (263,))
    dm = HipDataModule()
    assert (dm.name, dm.nfeats, dm.njoints) == ("humanml3d", 263, 22)
    dm = HipDataModule(C.load_config(os.path.join(C.CONFIG_DIR, "config_novae_humanml3d.yaml")))
    assert (dm.name, dm.nfeats, dm.njoints) == ("humanml3d", 263, 22)
    dm = HipDataModule(ml, nfeats=150, njoints=25, name="humanact12")
    assert (dm.name, dm.nfeats, dm.njoints, dm._arch) == ("humanact12", 150, 25, {})
    with pytest.raises(NotImplementedError):
        dm.feats2joints(torch.zeros(1, 4, 150))


def test_kit_dataset_statistics_from_root(tmp_path):
    """Mean.npy / Std.npy from cfg.DATASET.KIT.ROOT when present"""
    from mld_hip import config as C
    from mld_hip.datamodule import HipDataModule

    mean, std = np.arange(KIT_NF, dtype=np.float32), np.full(KIT_NF, 2.0, np.float32)
    np.save(tmp_path / "Mean.npy", mean)
    np.save(tmp_path / "Std.npy", std)
    cfg = C.load_config(os.path.join(C.CONFIG_DIR, "config_mld_kit.yaml"), overrides={"DATASET.KIT.ROOT": str(tmp_path)})
    dm = HipDataModule(cfg)
    assert dm.stats == "dataset" and np.array_equal(dm.mean, mean) and np.array_equal(dm.std, std)


def test_kit_mld_forward_sim(rec):
    """MLD(cfg_kit, HipDataModule(cfg_kit)) on an injected simulator engine: forward returns [len_i, 21, 3] within JOINT_TOL of the oracle; gen_from_latent and
    recon_from_motion give 21-joint motions too."""
    from mld_hip import config as C
    from mld_hip import engine as E
    from mld_hip.datamodule import HipDataModule
    from mld_hip.mld import MLD
    from mld_hip.text_encoder import SyntheticTextEncoder

    steps = 2
    eng = _lib.Engine(lib=simlib.sim_library(), use_graph=0, max_batch=4, max_frames=24, num_inference_steps=steps, num_layers=3, nfeats=KIT_NF, njoints=KIT_NJ)
    key = E.inject_engine(eng, "inject:kit")
    try:
        cfg = C.load_config(os.path.join(C.CONFIG_DIR, "config_mld_kit.yaml"),
                            overrides={"model.scheduler.num_inference_timesteps": steps, "model.denoiser.params.num_layers": 3,
                                       "model.motion_vae.params.num_layers": 3})
        enc = SyntheticTextEncoder()
        model = MLD(cfg, HipDataModule(cfg, engine_key=key), text_encoder=enc, engine_key=key).eval()
        assert model.fused and model.njoints == KIT_NJ and model.nfeats == KIT_NF
        texts, lengths = ["a person walks forward.", "a person waves the right hand.", "a person jumps."], [24, 17, 1]
        lat0 = syn.make_batch(3, lengths, seed=86).init_latents
        joints = model({"text": texts, "length": lengths}, init_latents=torch.from_numpy(lat0))
        emb = enc([""] * 3 + texts).numpy()
        sdd = {k: v.detach().numpy() for k, v in model.denoiser.state_dict().items()}
        sdv = {k: v.detach().numpy() for k, v in model.vae.state_dict().items()}
        dm = model.datamodule

        def fn(ops, W):
            lat = O.diffusion_reverse(ops, W(sdd), ops.asarray(emb), ops.asarray(lat0), 7.5, steps, 4)
            return O.feats2joints(ops, O.vae_decode(ops, W(sdv), lat, lengths), ops.asarray(dm.mean), ops.asarray(dm.std), njoints=KIT_NJ)
        (jr,) = R.reference64(fn)
        for i, n in enumerate(lengths):
            assert tuple(joints[i].shape) == (n, KIT_NJ, 3)
            err = float(np.abs(joints[i].numpy() - jr[i, :n]).max())
            print("sim kit MLD.forward motion %d: err %.3e" % (i, err))
            assert err < R.JOINT_TOL
        z = torch.from_numpy(syn._rng(87, "kitz").standard_normal((1, 3, 256)).astype(np.float32))
        out = model.gen_from_latent({"latent": z, "length": lengths})
        assert [tuple(o.shape) for o in out] == [(n, KIT_NJ, 3) for n in lengths]
        motion = torch.from_numpy(syn._rng(88, "kitm").standard_normal((2, 22, KIT_NF)).astype(np.float32))
        rst, ref = model.recon_from_motion({"motion": motion, "length": [22, 9]})
        assert [tuple(o.shape) for o in rst] == [tuple(o.shape) for o in ref] == [(22, KIT_NJ, 3), (9, KIT_NJ, 3)]
    finally:
        E._engines.pop(key, None)
        eng.close()
