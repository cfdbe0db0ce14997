"""The SMPL body model through the Python surface (``mld_hip.smpl.HipSmpl``, the opt-in ``model.smpl`` node, ``MLD.a2m_eval``) on a simulator-backed
action model, modelled on tests/test_host_mirror.py::test_action_mld_fused_and_modular_agree_with_oracle; the expected values are the float64
restatement of tests/smpl_ref.py (no reference fixture: ``smplx`` is not installed)."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import simlib  # noqa: E402
import smpl_ref as R  # noqa: E402
from mld_hip import config as C  # noqa: E402
from mld_hip import engine as E  # noqa: E402
from mld_hip import synthetic as syn  # noqa: E402
from mld_hip.datamodule import HipDataModule  # noqa: E402
from mld_hip.mld import MLD  # noqa: E402
from mld_hip.smpl import HipSmpl, read_smpl_file  # noqa: E402

A2M_CFG = os.path.join(C.CONFIG_DIR, "config_mld_humanact12.yaml")
V = 19
OPT_IN = {"model.smpl.target": "mld_hip.smpl.HipSmpl", "model.smpl.params.V": V}


def test_the_node_is_off_by_default_and_resolves():
    cfg = C.load_config(A2M_CFG)
    assert cfg.model.smpl.target is None and cfg.model.smpl.params.smpl_path == cfg.DATASET.SMPL_PATH
    cfg = C.load_config(A2M_CFG, overrides=OPT_IN)
    sm = C.instantiate_from_config(cfg.model.smpl)
    assert isinstance(sm, HipSmpl) and sm.source == "synthetic" and sm.V == V and sm._arch == {"smpl_verts": V}
    assert {k: tuple(v.shape) for k, v in sm.state_dict().items()} == {
        "v_template": (V, 3), "posedirs": (207, 3 * V), "J_regressor": (24, V), "lbs_weights": (V, 24), "parents": (24,)}


@pytest.fixture(scope="module")
def model():
    eng = simlib.sim_action_engine(max_batch=4, max_frames=24, num_inference_steps=2, smpl_verts=V)
    key = E.inject_engine(eng, "inject:smpl_host")
    cfg = C.load_config(A2M_CFG, overrides={"model.scheduler.num_inference_timesteps": 2, **simlib.ACTION_OVERRIDES, **OPT_IN})
    dm = HipDataModule(cfg, nfeats=150, njoints=25, name="humanact12", engine_key=key)
    m = MLD(cfg, dm, engine_key=key).eval()
    sdd, sdv = simlib.action_weights()
    m.denoiser.load_state_dict({k: torch.from_numpy(v) for k, v in sdd.items()}, strict=True)
    m.vae.load_state_dict({k: torch.from_numpy(v) for k, v in sdv.items()}, strict=True)
    yield m
    E._engines.pop(key, None)
    eng.close()


def within(out, ref, what):
    r64, e32 = ref
    err = float(np.abs(out.astype(np.float64) - r64).max())
    print(f"{what}: err {err:.3e}  e32 {e32:.3e}  ratio {err / e32:.2f}")
    assert e32 > 0 and err <= R.F32_FACTOR * e32, (what, err, e32)


def test_a2m_eval_returns_the_joints_entries_of_the_reference(model):
    assert model.fused and isinstance(model.smpl, HipSmpl) and model.smpl.V == V
    acts, lat0, _ = syn.make_action_batch(3, 16)
    lengths = [16, 9, 16]
    batch = {"action": torch.from_numpy(acts.astype(np.int64))[:, None], "length": lengths}
    rs = model.a2m_eval(batch, init_latents=torch.from_numpy(lat0))
    assert set(rs) == {"m_action", "m_rst", "m_lens", "joints_rst", "joints_eval_rst"}
    assert rs["joints_rst"].shape == (3, V, 3, 16) and rs["joints_eval_rst"].shape == (3, 24, 3, 16)
    feats = rs["m_rst"].numpy()
    bd = {k: v.detach().numpy() for k, v in model.smpl.state_dict().items()}
    (rj, _), (rv, _) = R.reference(bd, feats, lengths, 0)                       # vertices: no translation
    (rjt, ej), (_, _) = R.reference(bd, feats, lengths, R.TRANS_JOINTS, want_verts=False)
    ev = R.reference(bd, feats, lengths, 0)[1][1]
    within(rs["joints_rst"].permute(0, 3, 1, 2).numpy(), (rv, ev), "a2m_eval joints_rst (vertices)")
    within(rs["joints_eval_rst"].permute(0, 3, 1, 2).numpy(), (rjt, ej), "a2m_eval joints_eval_rst")
    assert not rs["joints_rst"][1, :, :, 9:].any()                              # padded frames of the vertices: zeros
    # with the ground-truth motion in the batch: the reference's full rs_set
    motion = torch.from_numpy(R.make_feats(lengths, 16, seed=3))
    mask = torch.arange(16)[None, :] < torch.tensor(lengths)[:, None]
    rs = model.a2m_eval({**batch, "motion": motion, "mask": mask}, init_latents=torch.from_numpy(lat0))
    assert set(rs) == {"m_action", "m_ref", "m_rst", "m_lens", "joints_rst", "joints_ref", "joints_eval_rst", "joints_eval_ref"}
    assert rs["joints_ref"].shape == (3, V, 3, 16) and rs["joints_eval_ref"].shape == (3, 24, 3, 16) and torch.equal(rs["m_ref"], motion)
    (rjt, ej), (rv, ev) = R.reference(bd, motion.numpy(), lengths, R.TRANS_JOINTS)
    within(rs["joints_ref"].permute(0, 3, 1, 2).numpy(), (rv, ev), "a2m_eval joints_ref (vertices)")
    within(rs["joints_eval_ref"].permute(0, 3, 1, 2).numpy(), (rjt, ej), "a2m_eval joints_eval_ref")
    # the two lambdas have the reference's call shape
    assert torch.equal(model.feats2joints(motion, mask), rs["joints_ref"]) and torch.equal(model.feats2joints_eval(motion, mask), rs["joints_eval_ref"])


def test_rot2xyz_refuses_what_is_out_of_scope(model):
    x = torch.from_numpy(R.make_feats([4, 2], 4)).view(2, 4, 6, 25).permute(0, 3, 2, 1)
    mask = torch.tensor([[True] * 4, [True, True, False, False]])
    ok = dict(mask=mask, pose_rep="rot6d", translation=True, glob=True, jointstype="smpl", vertstrans=True)
    assert model.smpl.rot2xyz(x, **ok).shape == (2, 24, 3, 4)
    assert model.smpl.rot2xyz(x, **{**ok, "mask": None, "jointstype": "vertices"}).shape == (2, V, 3, 4)
    for change, word in (({"jointstype": "a2m"}, "a2m"), ({"jointstype": "a2mpl"}, "a2mpl"), ({"jointstype": "vibe"}, "vibe"), ({"pose_rep": "rotvec"}, "pose_rep"),
                         ({"glob": False, "glob_rot": [3.14, 0, 0]}, "glob"), ({"betas": torch.zeros(2, 10)}, "betas"), ({"beta": 1}, "beta"),
                         ({"jointstype": "nope"}, "jointstype")):
        with pytest.raises(NotImplementedError) as ei:
            model.smpl.rot2xyz(x, **{**ok, **change})
        assert word in str(ei.value), (change, str(ei.value))
    for bad in (torch.tensor([[True, False, True, True], [True] * 4]), torch.tensor([[False, True, True, True], [True] * 4]),
                torch.tensor([[True] * 4, [False] * 4])):
        with pytest.raises(ValueError):
            model.smpl.rot2xyz(x, **{**ok, "mask": bad})                        # not a prefix mask / an empty motion


def test_npz_round_trip_through_from_files(tmp_path, model):
    """A file in SMPL_NEUTRAL's layout (posedirs [V, 3, 207], kintree_table [2, 24] with 2^32 - 1 at the root, weights, a shapedirs nobody reads) -> the
    engine's tensors.  (The official .pkl cannot be read here: chumpy and a real model file are both out of reach; the error path is checked.)"""
    bd = R.body(V)
    kin = np.stack([np.asarray(syn.SMPL_PARENTS, np.int64) % 2 ** 32, np.arange(24)]).astype(np.uint32)
    np.savez(tmp_path / "SMPL_NEUTRAL.npz", v_template=bd["v_template"].astype(np.float64), weights=bd["lbs_weights"], J_regressor=bd["J_regressor"],
             posedirs=np.ascontiguousarray(bd["posedirs"].T).reshape(V, 3, 207), kintree_table=kin, shapedirs=np.zeros((V, 3, 10)))
    sm = HipSmpl.from_files(str(tmp_path))
    assert sm.source.endswith("SMPL_NEUTRAL.npz") and sm.V == V
    for k, v in bd.items():
        assert np.array_equal(sm.state_dict()[k].numpy(), v), k
    assert np.array_equal(read_smpl_file(str(tmp_path / "SMPL_NEUTRAL.npz"))["parents"], bd["parents"])
    sm.use_engine(model.smpl._engine_key)
    f = R.make_feats([5, 3], 5, seed=2)
    (rj, ej), (rv, ev) = R.reference(bd, f, [5, 3], 3)
    within(sm.joints(torch.from_numpy(f), [5, 3]).numpy(), (rj, ej), "from_files joints")
    within(sm.vertices(torch.from_numpy(f), [5, 3], vertstrans=True).numpy(), (rv, ev), "from_files vertices")
    with pytest.raises(FileNotFoundError):
        HipSmpl.from_files(str(tmp_path / "nowhere"))
    import pickle

    class _NeedsChumpy:
        def __reduce__(self):
            return (__import__, ("chumpy_is_not_installed_here",))
    with open(tmp_path / "SMPL_NEUTRAL.pkl", "wb") as fh:
        pickle.dump({"v_template": _NeedsChumpy()}, fh)
    with pytest.raises(RuntimeError) as ei:
        read_smpl_file(str(tmp_path / "SMPL_NEUTRAL.pkl"))
    assert "chumpy_is_not_installed_here" in str(ei.value)


def test_a_smpl_path_without_a_model_file_warns(tmp_path, recwarn):
    """The opt-in node passes DATASET.SMPL_PATH; when no SMPL_NEUTRAL file is there the stand-in body says so (no path: the stand-in asked for, no warning)"""
    with pytest.warns(RuntimeWarning, match="synthetic stand-in"):
        sm = HipSmpl(smpl_path=str(tmp_path / "nowhere"), V=V)
    assert sm.source == "synthetic"
    recwarn.clear()
    assert HipSmpl(V=V).source == "synthetic" and not [w for w in recwarn if issubclass(w.category, RuntimeWarning)]
