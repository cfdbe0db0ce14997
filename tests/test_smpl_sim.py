"""The SMPL body model of the engine (mldhip_smpl_forward) on the functional simulator, both arithmetic modes, against the project's float64
restatement (tests/smpl_ref.py has the restatement, the inputs and the tolerance rule; there is no reference fixture: ``smplx`` is not installed).
V = 83 (a partial 16-vertex block) at B = 3, T = 8, lengths 8 / 5 / 1; V = 16 at B = 5, T = 13 (65 frames: past the 16-frame tiles, and one frame
into the simulator build's second 64-frame chunk); the dense weights; the flags; the padded-frame rule; batch independence; the guards and the
ABI checks that need no device."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import simlib  # noqa: E402
import smpl_ref as R  # noqa: E402
from mld_hip import _lib  # noqa: E402

EINVAL, ESTATE = -1, -3
LENS, T, V = [8, 5, 1], 8, 83


def sim_engine(prec, V_=V, dense=False, finalize=True, **kw):
    eng = _lib.Engine(lib=simlib.sim_library(), use_graph=0, precision=prec, **R.engine_kwargs(V_, **kw))
    assert R.load_body(eng, R.body(V_, dense), finalize=finalize) == []
    return eng


def run(eng, feats, lens, flags=0, joints=True, verts=True, V_=V, T_=None):
    B, Tt = len(lens), feats.shape[1] if T_ is None else T_
    j = np.full((B, Tt, 24, 3), np.nan, np.float32) if joints else None
    v = np.full((B, Tt, V_, 3), np.nan, np.float32) if verts else None
    eng.smpl_forward(np.ascontiguousarray(feats), lens, Tt, j, v, flags)
    return j, v


def check(out, ref, what, prec):
    r64, e32 = ref
    err = float(np.abs(out.astype(np.float64) - r64).max())
    print(f"{what}: mode {prec}  err {err:.3e}  e32 {e32:.3e}  ratio {err / e32:.2f}  max|ref| {np.abs(r64).max():.3f}")
    assert e32 > 0 and np.isfinite(out).all()
    assert err <= R.F32_FACTOR * e32, (what, prec, err, e32)


@pytest.fixture(scope="module")
def engines():
    out = {prec: sim_engine(prec) for prec in (0, 1)}
    yield out
    for eng in out.values():
        eng.close()


@pytest.fixture(scope="module")
def feats():
    return R.make_feats(LENS, T)


@pytest.fixture(scope="module")
def outs(engines, feats):
    return {(prec, fl): run(eng, feats, LENS, fl) for prec, eng in engines.items() for fl in (0, 3)}


def test_parity_with_fp64_both_modes_flags_on_and_off(outs, feats):
    for fl in (0, 3):
        rj, rv = R.reference(R.body(V), feats, LENS, fl)
        for prec in (0, 1):
            check(outs[prec, fl][0], rj, f"joints V = 83 flags {fl} (simulator)", prec)
            check(outs[prec, fl][1], rv, f"vertices V = 83 flags {fl} (simulator)", prec)


def test_each_flag_moves_its_own_output_only(engines, feats, outs):
    eng = engines[0]
    j1, v1 = run(eng, feats, LENS, R.TRANS_JOINTS)
    j2, v2 = run(eng, feats, LENS, R.TRANS_VERTS)
    assert np.array_equal(j1, outs[0, 3][0]) and np.array_equal(v1, outs[0, 0][1])
    assert np.array_equal(j2, outs[0, 0][0]) and np.array_equal(v2, outs[0, 3][1])
    assert not np.array_equal(outs[0, 0][0], outs[0, 3][0]) and not np.array_equal(outs[0, 0][1], outs[0, 3][1])


def test_f16x3_handle_gives_the_bits_of_the_f32_handle(outs):
    for fl in (0, 3):
        assert np.array_equal(outs[0, fl][0], outs[1, fl][0]) and np.array_equal(outs[0, fl][1], outs[1, fl][1])


def test_joints_only_and_vertices_only_calls_are_bit_identical_to_the_full_call(engines, feats, outs):
    for prec, eng in engines.items():
        j, v = run(eng, feats, LENS, 3, verts=False)
        assert v is None and np.array_equal(j, outs[prec, 3][0])
        j, v = run(eng, feats, LENS, 3, joints=False)
        assert j is None and np.array_equal(v, outs[prec, 3][1])


def test_65_frames_cross_tiles_and_a_chunk_and_dense_weights():
    lens, T_ = [13, 7, 1, 13, 2], 13
    f = R.make_feats(lens, T_, seed=1)
    for dense in (False, True):
        bd = R.body(16, dense)
        rj, rv = R.reference(bd, f, lens, 3)
        res = {}
        for prec in (0, 1):
            eng = sim_engine(prec, 16, dense)
            res[prec] = run(eng, f, lens, 3, V_=16)
            check(res[prec][0], rj, f"joints V = 16, 65 frames, dense {dense} (simulator)", prec)
            check(res[prec][1], rv, f"vertices V = 16, 65 frames, dense {dense} (simulator)", prec)
            if prec == 0:      # the motion that straddles the chunk boundary (frames 52 .. 64), alone: the same bits
                j, v = run(eng, f[4:5], lens[4:5], 3, V_=16)
                assert np.array_equal(j[0], res[0][0][4]) and np.array_equal(v[0], res[0][1][4])
            eng.close()
        assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


def test_dense_weights_at_the_partial_block(feats):
    bd = R.body(V, True)
    rj, rv = R.reference(bd, feats, LENS, 0)
    eng = sim_engine(0, V, True)
    j, v = run(eng, feats, LENS, 0)
    eng.close()
    check(j, rj, "joints V = 83 dense (simulator)", 0)
    check(v, rv, "vertices V = 83 dense (simulator)", 0)


def test_padded_frame_rule(engines, feats, outs):
    """Padded frames hold zeros; with the translation flags every frame -- padded ones included -- gets trans[t] - trans[0], read from the frame as it is: zero
    padding gives -trans[0], garbage in a padded frame's slot 24 shows up in the translated outputs of that frame and nowhere else; garbage in its other
    slots shows up nowhere."""
    eng = engines[0]
    j0, v0 = outs[0, 0]
    j3, v3 = outs[0, 3]
    t0 = feats.reshape(3, T, 6, 25)[:, 0, :3, 24]
    for b, n in enumerate(LENS):
        assert not j0[b, n:].any() and not v0[b, n:].any()
        if n < T:
            assert np.array_equal(j3[b, n:], np.broadcast_to(0.0 - t0[b], j3[b, n:].shape))
            assert np.array_equal(v3[b, n:], np.broadcast_to(0.0 - t0[b], v3[b, n:].shape))
    g = feats.copy().reshape(3, T, 6, 25)
    g[1, 6, :, :24] = 7.5                                                      # padded frame 6 of motion 1: rotation slots
    g[1, 6, 3:, 24] = -3.0                                                     # ... the unused half of slot 24
    g = g.reshape(3, T, 150)
    jg, vg = run(eng, g, LENS, 3)
    assert np.array_equal(jg, j3) and np.array_equal(vg, v3)
    jg, vg = run(eng, g, LENS, 0)
    assert np.array_equal(jg, j0) and np.array_equal(vg, v0)
    g = g.reshape(3, T, 6, 25)
    g[1, 6, :3, 24] = [2.0, -4.0, 8.0]                                         # ... and its translation
    g = g.reshape(3, T, 150)
    jg, vg = run(eng, g, LENS, 0)
    assert np.array_equal(jg, j0) and np.array_equal(vg, v0)
    jg, vg = run(eng, g, LENS, 3)
    want = np.array([2.0, -4.0, 8.0], np.float32) - t0[1]
    assert np.array_equal(jg[1, 6], np.broadcast_to(want, (24, 3))) and np.array_equal(vg[1, 6], np.broadcast_to(want, (V, 3)))
    jg[1, 6], vg[1, 6] = j3[1, 6], v3[1, 6]
    assert np.array_equal(jg, j3) and np.array_equal(vg, v3)
    rj, rv = R.reference(R.body(V), g, LENS, 3)                                # the restatement follows the same rule
    check(run(eng, g, LENS, 3)[0], rj, "joints, garbage translation in a padded frame", 0)
    check(run(eng, g, LENS, 3)[1], rv, "vertices, garbage translation in a padded frame", 0)


def test_a_motion_is_bit_identical_alone_and_inside_a_batch(engines, feats, outs):
    for prec, eng in engines.items():
        for b in range(3):
            j, v = run(eng, feats[b:b + 1], LENS[b:b + 1], 3)
            assert np.array_equal(j[0], outs[prec, 3][0][b]) and np.array_equal(v[0], outs[prec, 3][1][b])
        j, v = run(eng, feats[::-1], LENS[::-1], 3)
        assert np.array_equal(j[::-1], outs[prec, 3][0]) and np.array_equal(v[::-1], outs[prec, 3][1])


def test_nothing_is_read_or_written_beyond_the_call(engines, feats, outs):
    eng = engines[0]
    big = np.full(feats.size + 4096, np.nan, np.float32)
    big[:feats.size] = feats.ravel()
    j = np.full(3 * T * 24 * 3 + 64, np.nan, np.float32)
    v = np.full(3 * T * V * 3 + 64, np.nan, np.float32)
    eng.smpl_forward(big, LENS, T, j, v, 3)
    assert np.array_equal(j[:-64].reshape(3, T, 24, 3), outs[0, 3][0]) and np.isnan(j[-64:]).all()
    assert np.array_equal(v[:-64].reshape(3, T, V, 3), outs[0, 3][1]) and np.isnan(v[-64:]).all()


def code(fn):
    with pytest.raises(_lib.MldHipError) as ei:
        fn()
    return ei.value.code


def test_guards(engines, feats):
    eng = engines[0]
    j, v = np.zeros((6, 16, 24, 3), np.float32), np.zeros((6, 16, V, 3), np.float32)
    assert code(lambda: eng.smpl_forward(feats, [8] * 6, T, j, v)) == EINVAL                      # B > max_batch
    assert code(lambda: eng.smpl_forward(feats, [], T, j, v)) == EINVAL                           # B = 0
    assert code(lambda: eng.smpl_forward(feats, LENS, 17, j, v)) == EINVAL                        # T > max_frames
    assert code(lambda: eng.smpl_forward(feats, [8, 5, 0], T, j, v)) == EINVAL                    # a length outside 1 .. T
    assert code(lambda: eng.smpl_forward(feats, [9, 5, 1], T, j, v)) == EINVAL
    assert code(lambda: eng.smpl_forward(feats, LENS, T, None, None)) == EINVAL                   # both outputs NULL
    assert code(lambda: eng.smpl_forward(feats, LENS, T, j, v, 4)) == EINVAL                      # unknown flag bits
    assert code(lambda: eng.smpl_forward(feats, LENS, T, j, v, -1)) == EINVAL
    assert code(lambda: eng.smpl_forward(None, LENS, T, j, v)) == EINVAL                          # a null input
    assert eng.lib.mldhip_smpl_forward(eng._h, feats.ctypes.data, None, 3, T, 0, j.ctypes.data, v.ctypes.data, None) == EINVAL


def test_states(feats):
    j, v = np.zeros((3, T, 24, 3), np.float32), np.zeros((3, T, V, 3), np.float32)
    plain = _lib.Engine(lib=simlib.sim_library(), use_graph=0, num_layers=3, max_batch=3, max_frames=16)      # no body model on the handle
    assert code(lambda: plain.smpl_forward(feats, LENS, T, j, v)) == ESTATE
    plain.close()
    eng = sim_engine(0, finalize=False)
    assert code(lambda: eng.smpl_forward(feats, LENS, T, j, v)) == ESTATE                         # not finalized
    eng.finalize()
    eng.smpl_forward(feats, LENS, T, j, v)
    eng.close()
    eng = _lib.Engine(lib=simlib.sim_library(), use_graph=0, **R.engine_kwargs(V))                # the group is not loaded (another one is)
    eng.load_tensor("mean", np.zeros(150, np.float32))
    eng.load_tensor("std", np.ones(150, np.float32))
    eng.finalize()
    assert code(lambda: eng.smpl_forward(feats, LENS, T, j, v)) == ESTATE
    eng.close()
    with pytest.raises(_lib.MldHipError) as ei:                                                   # smpl_verts > 0 needs the 150 rot6d features
        _lib.Engine(lib=simlib.sim_library(), use_graph=0, num_layers=3, max_batch=2, max_frames=16, smpl_verts=V)
    assert ei.value.code == EINVAL
    for bad in (-1, 16385):
        with pytest.raises(_lib.MldHipError) as ei:
            _lib.Engine(lib=simlib.sim_library(), use_graph=0, **R.engine_kwargs(bad))
        assert ei.value.code == EINVAL


def test_half_loaded_group_wrong_shapes_and_bad_parents():
    bd = R.body(V)
    eng = _lib.Engine(lib=simlib.sim_library(), use_graph=0, **R.engine_kwargs(V))
    with pytest.raises(_lib.MldHipError) as ei:
        eng.load_tensor("smpl.posedirs", np.zeros((V, 3, 207), np.float32))                      # the file's layout, not smplx's buffer
    assert ei.value.code == EINVAL
    assert R.load_body(eng, bd, finalize=False, skip=("lbs_weights", "parents")) == []
    missing = eng.missing_keys()
    assert "smpl.lbs_weights" in missing and "smpl.parents" in missing and "smpl.posedirs" not in missing
    with pytest.raises(_lib.MldHipError):
        eng.finalize()                                                         # a half-loaded group
    eng.load_tensor("smpl.lbs_weights", bd["lbs_weights"])
    for i, val in ((5, 5.0), (5, 7.0), (1, -1.0), (9, 2.5), (3, np.nan)):     # itself, a later joint, no parent, not an integer, NaN
        par = bd["parents"].copy()
        par[i] = val
        eng.load_tensor("smpl.parents", par)
        with pytest.raises(_lib.MldHipError) as ei:
            eng.finalize()
        assert ei.value.code == EINVAL and "parents" in str(ei.value)
    eng.load_tensor("smpl.parents", bd["parents"])
    eng.finalize()
    eng.close()


def test_smpl_verts_0_ignores_the_keys_and_an_older_struct_has_no_model():
    lib = simlib.sim_library()
    assert lib.mldhip_abi_version() == 8 == _lib.ABI_VERSION
    assert "mldhip_smpl_forward" in _lib.exported_symbols() and hasattr(lib, "mldhip_smpl_forward")
    cfg = _lib.Config()
    lib.mldhip_default_config(C.byref(cfg))
    assert cfg.struct_size == C.sizeof(_lib.Config) and cfg.smpl_verts == 0
    off = _lib.Engine(lib=lib, use_graph=0, num_layers=3, max_batch=2, max_frames=16)
    assert off.load_tensor("smpl.posedirs", np.zeros((3, 3), np.float32)) is False                # smpl_verts = 0: ignored, mis-shaped or not
    assert off.load_tensor("smpl.parents", np.zeros(24, np.float32)) is False
    assert not any(k.startswith("smpl.") for k in off.missing_keys())
    off.close()
    # a caller built before the field passes the struct that ends behind t2m_max_words: accepted, no body model whatever the bytes behind it say
    cfg.struct_size = _lib.Config.smpl_verts.offset
    cfg.num_layers, cfg.max_batch, cfg.max_frames, cfg.smpl_verts = 3, 2, 16, 83
    h = C.c_void_p()
    assert lib.mldhip_create(C.byref(cfg), 0, C.byref(h)) == 0
    assert lib.mldhip_load_tensor(h, b"smpl.parents", np.zeros(4, np.float32).ctypes.data, (C.c_int64 * 1)(4), 1, 0, 0) == 1      # ignored
    f = np.zeros((1, 4, 150), np.float32)
    j = np.zeros((1, 4, 24, 3), np.float32)
    assert lib.mldhip_smpl_forward(h, f.ctypes.data, (C.c_int32 * 1)(4), 1, 4, 0, j.ctypes.data, None, None) == ESTATE
    lib.mldhip_destroy(h)


def test_nan_feature_is_counted(engines, feats):
    eng = engines[1]
    assert eng.numeric_status()["nonfinite_values"] == 0
    run(eng, feats, LENS, 3)
    assert eng.numeric_status()["nonfinite_values"] == 0
    g = feats.copy()
    g[0, 2, 3] = np.nan                                                        # component 0 of joint 3 (spine1) in a valid frame
    j, v = run(eng, g, LENS, 0)
    n = eng.numeric_status()["nonfinite_values"]
    assert n == int((~np.isfinite(j)).sum() + (~np.isfinite(v)).sum()) and n > 0
    assert np.isfinite(j[0, :2]).all() and np.isfinite(j[0, 3:]).all() and np.isfinite(j[1:]).all()      # the frame's own rows only
    assert np.isfinite(v[0, :2]).all() and np.isfinite(v[0, 3:]).all() and np.isfinite(v[1:]).all()
    run(eng, g, LENS, 0, verts=False)
    assert eng.numeric_status()["nonfinite_values"] == int((~np.isfinite(j)).sum())
    g = feats.copy()
    g[1, 7, 24] = np.inf                                                       # the translation of a padded frame: seen only through the flags
    run(eng, g, LENS, 0)
    assert eng.numeric_status()["nonfinite_values"] == 0
    run(eng, g, LENS, 3)
    assert eng.numeric_status()["nonfinite_values"] == 24 + V


def test_waves_walk_several_vertex_blocks():
    """V = 300 (18 whole 16-vertex blocks + one of 12).  The simulator build gives the vertex kernel a budget of 2 workgroups where the GPU build gives 512,
    so its waves walk several blocks each, as on the GPU at a HumanAct12 batch (64 x 60 frames: 5 lanes of workgroups per frame group, about 22 blocks per
    wave): B = 3, T = 8 is one frame group on 2 lanes (blocks w, w + 8, w + 16 per wave); B = 5, T = 13 is two frame groups on 1 lane in the first 64-frame
    chunk (blocks w, w + 4, ..., w + 16) and one group on 2 lanes in the second."""
    V_ = 300
    for lens, T_, seed in (([8, 5, 1], 8, 4), ([13, 7, 1, 13, 2], 13, 5)):
        f = R.make_feats(lens, T_, seed=seed)
        rj, rv = R.reference(R.body(V_), f, lens, 3)
        res = {}
        for prec in (0, 1):
            eng = sim_engine(prec, V_)
            res[prec] = run(eng, f, lens, 3, V_=V_)
            if prec == 0:      # the last motion alone: the same bits
                j, v = run(eng, f[-1:], lens[-1:], 3, V_=V_)
                assert np.array_equal(j[0], res[0][0][-1]) and np.array_equal(v[0], res[0][1][-1])
            eng.close()
            check(res[prec][0], rj, f"joints V = 300, B {len(lens)}, T {T_} (simulator, multi-block walk)", prec)
            check(res[prec][1], rv, f"vertices V = 300, B {len(lens)}, T {T_} (simulator, multi-block walk)", prec)
        assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
