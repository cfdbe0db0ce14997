"""The HumanAct12 recognition GRU of the engine (mldhip_a2m_recognize) on the functional simulator, both arithmetic modes, against the project's float64
restatement (tests/a2m_rec_ref.py: the restatement, the inputs and both rules).  B = 3 at T = 13 (one partial motion tile) and B = 20 at T = 13 (a
full tile plus a partial one), both weight families, h0 = NULL as zeros, NaN in padded frames, batch independence, the non-finite counter, the guards
and the ABI checks that need no device."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import a2m_rec_ref as R  # noqa: E402
import simlib  # noqa: E402
from mld_hip import _lib  # noqa: E402

EINVAL, ESTATE = -1, -3
T = 13


def sim_engine(prec, family="default", finalize=True, **kw):
    eng = _lib.Engine(lib=simlib.sim_library(), use_graph=0, precision=prec, **R.engine_kwargs(**kw))
    assert R.load(eng, R.weights(family), finalize=finalize) == []
    return eng


def run(eng, joints, lens, h0, logits=True, act=True):
    B, Tt = len(lens), joints.shape[1]
    lo = np.full((B, 12), np.nan, np.float32) if logits else None
    ac = np.full((B, 30), np.nan, np.float32) if act else None
    eng.a2m_recognize(np.ascontiguousarray(joints, np.float32), lens, Tt, None if h0 is None else np.ascontiguousarray(h0, np.float32), lo, ac)
    return lo, ac


def check(out, ref, what, prec):
    r64, e32 = ref
    err = float(np.abs(out.astype(np.float64) - r64).max())
    print(f"{what}: mode {prec}  err {err:.3e}  e32 {e32:.3e}  ratio {err / e32:.2f}")
    assert e32 > 0 and np.isfinite(out).all()
    assert err <= R.F32_FACTOR * e32, (what, prec, err, e32)


CASES = {"B 3, T 13": (3, 13), "B 20, T 13": (20, 13)}


@pytest.fixture(scope="module")
def engines():
    out = {(fam, prec): sim_engine(prec, fam, max_batch=5) for fam in R.FAMILIES for prec in (0, 1)}
    yield out
    for eng in out.values():
        eng.close()


@pytest.fixture(scope="module")
def cases():
    """inputs and the float64 restatement of each (case, family), computed once and shared"""
    out = {}
    for name, (B, T_) in CASES.items():
        j, lens, h0 = R.make_case(B, T_)
        for fam in R.FAMILIES:
            out[name, fam] = (j, lens, h0, R.reference(R.weights(fam), j, lens, h0))
    return out


@pytest.fixture(scope="module")
def outs(engines, cases):
    return {(name, fam, prec): run(engines[fam, prec], j, lens, h0) for (name, fam), (j, lens, h0, _) in cases.items() for prec in (0, 1)}


@pytest.mark.parametrize("fam", list(R.FAMILIES))
@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_fp64_both_modes(cases, outs, name, fam):
    _, _, _, (rl, ra) = cases[name, fam]
    R.check_gaps(rl[0])
    for prec in (0, 1):
        lo, ac = outs[name, fam, prec]
        check(lo, rl, f"logits, {name}, {fam} (simulator)", prec)
        check(ac, ra, f"activations, {name}, {fam} (simulator)", prec)
        R.check_classes(lo, rl[0])
    assert np.array_equal(outs[name, fam, 0][0], outs[name, fam, 1][0]) and np.array_equal(outs[name, fam, 0][1], outs[name, fam, 1][1])


def test_h0_null_is_zeros(engines):
    j, lens, h0 = R.make_case(3, T, seed=5)
    z = np.zeros_like(h0)
    rl, ra = R.reference(R.weights(), j, lens, z)
    eng = engines["default", 0]
    lo, ac = run(eng, j, lens, None)
    check(lo, rl, "logits, h0 = NULL (simulator)", 0)
    check(ac, ra, "activations, h0 = NULL (simulator)", 0)
    lz, az = run(eng, j, lens, z)
    assert np.array_equal(lo, lz) and np.array_equal(ac, az)


def test_padded_frames_are_never_read_and_batch_independence(engines, cases, outs):
    j, lens, h0, _ = cases["B 20, T 13", "default"]
    eng = engines["default", 0]
    full = outs["B 20, T 13", "default", 0]
    g = j.copy()
    for b, n in enumerate(lens):
        g[b, n:] = np.nan
    lo, ac = run(eng, g, lens, h0)
    assert np.array_equal(lo, full[0]) and np.array_equal(ac, full[1])
    for b in (0, 7, 16, 19):      # alone: the first motion (T frames), one of each tile, the last (1 frame)
        lo, ac = run(eng, j[b:b + 1], lens[b:b + 1], h0[:, b:b + 1])
        assert np.array_equal(lo[0], full[0][b]) and np.array_equal(ac[0], full[1][b])
        n = lens[b]                 # ... and cut to its own length: T = len
        lo, ac = run(eng, j[b:b + 1, :n], lens[b:b + 1], h0[:, b:b + 1])
        assert np.array_equal(lo[0], full[0][b]) and np.array_equal(ac[0], full[1][b])
    lo, ac = run(eng, j[::-1], lens[::-1], h0[:, ::-1])
    assert np.array_equal(lo[::-1], full[0]) and np.array_equal(ac[::-1], full[1])


def test_single_outputs_are_bit_identical(engines, cases, outs):
    j, lens, h0, _ = cases["B 3, T 13", "default"]
    eng = engines["default", 1]
    lo, ac = run(eng, j, lens, h0, act=False)
    assert ac is None and np.array_equal(lo, outs["B 3, T 13", "default", 1][0])
    lo, ac = run(eng, j, lens, h0, logits=False)
    assert lo is None and np.array_equal(ac, outs["B 3, T 13", "default", 1][1])


def test_nan_is_counted(engines, cases):
    j, lens, h0, _ = cases["B 3, T 13", "default"]
    eng = engines["default", 1]
    assert eng.numeric_status()["nonfinite_values"] == 0
    g = j.copy()
    g[1, 0, 5] = np.nan                      # a valid frame of motion 1
    lo, ac = run(eng, g, lens, h0)
    n = eng.numeric_status()["nonfinite_values"]
    assert n == 42 and not np.isfinite(lo[1]).any() and not np.isfinite(ac[1]).any()
    assert np.isfinite(lo[[0, 2]]).all() and np.isfinite(ac[[0, 2]]).all()
    run(eng, g, lens, h0, act=False)
    assert eng.numeric_status()["nonfinite_values"] == 12


def code(fn):
    with pytest.raises(_lib.MldHipError) as ei:
        fn()
    return ei.value.code


def test_guards_and_capacity(engines):
    eng = engines["default", 0]                               # max_batch 5: a2m_max_motions = 20
    assert eng.cfg.a2m_max_motions == 0
    j, lens, h0 = R.make_case(21, T, seed=3)
    lo, ac = np.zeros((21, 12), np.float32), np.zeros((21, 30), np.float32)
    run(eng, j[:20], lens[:20], h0[:, :20])                  # B = a2m_max_motions
    assert code(lambda: eng.a2m_recognize(j, lens, T, h0, lo, ac)) == EINVAL                  # one more
    assert code(lambda: eng.a2m_recognize(j, [], T, h0, lo, ac)) == EINVAL                    # B = 0
    assert code(lambda: eng.a2m_recognize(j, lens[:3], 17, h0, lo, ac)) == EINVAL             # T > max_frames
    assert code(lambda: eng.a2m_recognize(j, lens[:3], 0, h0, lo, ac)) == EINVAL              # T = 0
    assert code(lambda: eng.a2m_recognize(j, [13, 0, 1], T, h0, lo, ac)) == EINVAL            # a length outside 1 .. T
    assert code(lambda: eng.a2m_recognize(j, [13, 14, 1], T, h0, lo, ac)) == EINVAL
    assert code(lambda: eng.a2m_recognize(j, lens[:3], T, h0, None, None)) == EINVAL          # both outputs NULL
    assert code(lambda: eng.a2m_recognize(None, lens[:3], T, h0, lo, ac)) == EINVAL           # a null input
    assert eng.lib.mldhip_a2m_recognize(eng._h, j.ctypes.data, None, None, 3, T, lo.ctypes.data, None, None) == EINVAL
    big = _lib.Engine(lib=simlib.sim_library(), use_graph=0, **R.engine_kwargs(max_batch=2, a2m_max_motions=3))
    R.load(big, R.weights())
    run(big, j[:3], lens[:3], h0[:, :3])
    assert code(lambda: big.a2m_recognize(j[:4], lens[:4], T, h0[:, :4], lo, ac)) == EINVAL
    big.close()


def test_states_and_weight_group():
    j, lens, h0 = R.make_case(3, T, seed=4)
    lo = np.zeros((3, 12), np.float32)
    plain = _lib.Engine(lib=simlib.sim_library(), use_graph=0, num_layers=3, max_batch=3, max_frames=16)      # no recognizer on the handle
    assert code(lambda: plain.a2m_recognize(j, lens, T, h0, lo)) == ESTATE
    assert plain.load_tensor("a2m_rec.linear1.weight", np.zeros((3, 3), np.float32)) is False               # ignored, mis-shaped or not
    assert not any(k.startswith("a2m_rec.") for k in plain.missing_keys())
    plain.close()
    eng = sim_engine(0, finalize=False)
    assert code(lambda: eng.a2m_recognize(j, lens, T, h0, lo)) == ESTATE                     # not finalized
    eng.finalize()
    eng.a2m_recognize(j, lens, T, h0, lo)
    eng.close()
    eng = _lib.Engine(lib=simlib.sim_library(), use_graph=0, **R.engine_kwargs())             # the group is not loaded (another one is)
    eng.load_tensor("mean", np.zeros(263, np.float32))
    eng.load_tensor("std", np.ones(263, np.float32))
    eng.finalize()
    assert code(lambda: eng.a2m_recognize(j, lens, T, h0, lo)) == ESTATE
    with pytest.raises(_lib.MldHipError) as ei:
        eng.load_tensor("a2m_rec.recurrent.weight_ih_l0", np.zeros((384, 128), np.float32))   # a wrong shape
    assert ei.value.code == EINVAL
    assert R.load(eng, R.weights(), finalize=False, skip=("linear2.bias", "recurrent.bias_hh_l1")) == []
    missing = eng.missing_keys()
    assert "a2m_rec.linear2.bias" in missing and "a2m_rec.recurrent.bias_hh_l1" in missing and "a2m_rec.linear1.bias" not in missing
    with pytest.raises(_lib.MldHipError):
        eng.finalize()                                                                         # a half-loaded group
    eng.close()
    for bad in (dict(a2m_rec=2), dict(a2m_max_motions=-1), dict(a2m_max_motions=(1 << 20) + 1)):
        with pytest.raises(_lib.MldHipError) as ei:
            _lib.Engine(lib=simlib.sim_library(), use_graph=0, **{**R.engine_kwargs(), **bad})
        assert ei.value.code == EINVAL


def test_an_older_struct_has_no_recognizer():
    lib = simlib.sim_library()
    assert lib.mldhip_abi_version() == 8 == _lib.ABI_VERSION
    assert "mldhip_a2m_recognize" in _lib.exported_symbols() and hasattr(lib, "mldhip_a2m_recognize")
    cfg = _lib.Config()
    lib.mldhip_default_config(C.byref(cfg))
    assert cfg.struct_size == C.sizeof(_lib.Config) and cfg.a2m_rec == 0 and cfg.a2m_max_motions == 0
    # a caller built before the fields passes the struct that ends behind smpl_verts: accepted, no recognizer whatever the bytes behind it say
    cfg.struct_size = _lib.Config.a2m_rec.offset
    cfg.num_layers, cfg.max_batch, cfg.max_frames, cfg.a2m_rec = 3, 2, 16, 1
    h = C.c_void_p()
    assert lib.mldhip_create(C.byref(cfg), 0, C.byref(h)) == 0
    assert lib.mldhip_load_tensor(h, b"a2m_rec.linear2.bias", np.zeros(12, np.float32).ctypes.data, (C.c_int64 * 1)(12), 1, 0, 0) == 1      # ignored
    x = np.zeros((1, 4, 72), np.float32)
    lo = np.zeros((1, 12), np.float32)
    assert lib.mldhip_a2m_recognize(h, x.ctypes.data, (C.c_int32 * 1)(4), None, 1, 4, lo.ctypes.data, None, None) == ESTATE
    lib.mldhip_destroy(h)
