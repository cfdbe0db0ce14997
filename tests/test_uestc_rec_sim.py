"""The UESTC recognition ST-GCN of the engine (mldhip_uestc_recognize) on the functional simulator, both arithmetic modes, against the project's float64
restatement (tests/uestc_rec_ref.py: the restatement, the inputs and both rules).  T = 13 (13 -> 7 -> 4: odd lengths at both strides), T = 5 (shorter
than the 9 taps) and T = 1, at B = 1 and B = 3 (partial 64-row tiles at every width: 24 B T rows); both stride conventions with identical bits, a
non-contiguous view against its copy, batch independence, NaN containment and the counter, the probe's fallback, the guards and the ABI checks."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import simlib  # noqa: E402
import uestc_rec_ref as R  # noqa: E402
from mld_hip import _lib  # noqa: E402

EINVAL, ESTATE = -1, -3


def sim_engine(prec, family="default", finalize=True, **kw):
    eng = _lib.Engine(lib=simlib.sim_library(), use_graph=0, precision=prec, **R.engine_kwargs(**kw))
    assert R.load(eng, R.weights(family), finalize=finalize) == []
    return eng


def run(eng, m, logits=True, feat=True, strides=None):
    """m: numpy [B, 24, 6, T] (any strides) or a (buffer, strides, B, T) tuple"""
    if isinstance(m, tuple):
        buf, strides, B, T = m
    else:
        B, T = m.shape[0], m.shape[3]
        buf, strides = m, [s // 4 for s in m.strides]
    lo = np.full((B, R.NC), np.nan, np.float32) if logits else None
    fe = np.full((B, 256), np.nan, np.float32) if feat else None
    eng.uestc_recognize(buf, strides, B, T, lo, fe)
    return lo, fe


CASES = {"B 3, T 13": (3, 13), "B 1, T 13": (1, 13), "B 3, T 5": (3, 5), "B 1, T 1": (1, 1)}
FAMILY_OF = {"B 3, T 13": ("default", "bn_x2"), "B 1, T 13": ("default",), "B 3, T 5": ("default", "bn_x2"), "B 1, T 1": ("default", "bn_x2")}
PAIRS = [(n, f) for n in CASES for f in FAMILY_OF[n]]


@pytest.fixture(scope="module")
def engines():
    out = {(fam, prec): sim_engine(prec, fam) for fam in R.FAMILIES for prec in (0, 1)}
    yield out
    for eng in out.values():
        eng.close()


@pytest.fixture(scope="module")
def cases():
    """inputs and the float64 restatement of each (case, family), computed once and shared"""
    out = {}
    for name, fam in PAIRS:
        m = R.make_case(*CASES[name])
        out[name, fam] = (m, R.reference(R.weights(fam), m))
    return out


@pytest.fixture(scope="module")
def outs(engines, cases):
    return {(name, fam, prec): run(engines[fam, prec], m) for (name, fam), (m, _) in cases.items() for prec in (0, 1)}


@pytest.mark.parametrize("name,fam", PAIRS)
def test_parity_with_fp64_both_modes(cases, outs, name, fam):
    _, (rl, rf) = cases[name, fam]
    R.check_gaps(rl[0])
    for prec in (0, 1):
        lo, fe = outs[name, fam, prec]
        R.check(lo, rl, f"logits, {name}, {fam} (simulator)", prec)
        R.check(fe, rf, f"features, {name}, {fam} (simulator)", prec)
        R.check_classes(lo, rl[0])


def test_both_stride_conventions_and_a_view_give_the_same_bits(engines, cases, outs):
    m, _ = cases["B 3, T 5", "default"]
    for prec in (0, 1):
        eng, full = engines["default", prec], outs["B 3, T 5", "default", prec]
        rows, view = R.feature_rows(m)                                       # MLD's view of [B, T, 150] rows: strides (150 T, 1, 25, 150)
        lo, fe = run(eng, (rows.numpy(), list(view.stride()), 3, 5))
        assert np.array_equal(lo, full[0]) and np.array_equal(fe, full[1])
        wide = np.zeros((3, 24, 6, 11), np.float32)                          # a non-contiguous slice of a longer tensor against its contiguous copy
        wide[..., 3:8] = m
        lo, fe = run(eng, wide[..., 3:8])
        assert not wide[..., 3:8].flags["C_CONTIGUOUS"] and np.array_equal(lo, full[0]) and np.array_equal(fe, full[1])


def test_batch_independence_and_single_outputs(engines, cases, outs):
    m, _ = cases["B 3, T 13", "default"]
    for prec in (0, 1):
        eng, full = engines["default", prec], outs["B 3, T 13", "default", prec]
        lo, fe = run(eng, m[1:2])
        assert np.array_equal(lo[0], full[0][1]) and np.array_equal(fe[0], full[1][1])
        lo, fe = run(eng, np.ascontiguousarray(m[::-1]))
        assert np.array_equal(lo[::-1], full[0]) and np.array_equal(fe[::-1], full[1])
    eng, full = engines["default", 1], outs["B 3, T 5", "default", 1]
    m5, _ = cases["B 3, T 5", "default"]
    lo, fe = run(eng, m5, feat=False)
    assert fe is None and np.array_equal(lo, full[0])
    lo, fe = run(eng, m5, logits=False)
    assert lo is None and np.array_equal(fe, full[1])


def test_nan_stays_in_its_motion_and_is_counted(engines, cases, outs):
    m, _ = cases["B 3, T 5", "default"]
    for prec in (0, 1):
        eng, full = engines["default", prec], outs["B 3, T 5", "default", prec]
        assert eng.numeric_status()["nonfinite_values"] == 0
        g = m.copy()
        g[1, 23, 5, 4] = np.nan                      # the last joint, component and frame of motion 1
        lo, fe = run(eng, g)
        assert eng.numeric_status()["nonfinite_values"] == R.NC + 256
        assert not np.isfinite(lo[1]).any() and not np.isfinite(fe[1]).any()
        assert np.array_equal(lo[[0, 2]], full[0][[0, 2]]) and np.array_equal(fe[[0, 2]], full[1][[0, 2]])
        run(eng, g, feat=False)
        assert eng.numeric_status()["nonfinite_values"] == R.NC


def test_probe_keeps_the_split_net_and_falls_back_on_overflow(cases, outs):
    """finalize's sixth probe stage on the simulator: the default family stays split; inputs scaled far beyond the half range (data_bn x 1e6) read a huge
    error, uestc_split_ok = 0, and the F16X3 handle then gives the F32 handle's bits"""
    m, _ = cases["B 1, T 1", "default"]
    eng = sim_engine(1, finalize=False)
    eng.set_option("range_probe", 1)
    eng.finalize()
    st = eng.numeric_status()
    print("probe, default family:", st["probe_err_uestc"])
    assert st["uestc_split_ok"] == 1 and 0 <= st["probe_err_uestc"] <= _lib.PROBE_TOL
    assert np.array_equal(run(eng, m)[0], outs["B 1, T 1", "default", 1][0])
    eng.close()
    eng = sim_engine(1, "overflow", finalize=False)
    eng.set_option("range_probe", 1)
    eng.finalize()
    st = eng.numeric_status()
    print("probe, overflow family:", st["probe_err_uestc"])
    assert st["uestc_split_ok"] == 0 and not st["probe_err_uestc"] <= _lib.PROBE_TOL
    f32 = sim_engine(0, "overflow")
    a, b = run(eng, m), run(f32, m)
    assert np.isfinite(b[0]).all() and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert f32.numeric_status()["uestc_split_ok"] == 0
    eng.close()
    f32.close()


def code(fn):
    with pytest.raises(_lib.MldHipError) as ei:
        fn()
    return ei.value.code


def test_guards_and_capacity(engines):
    eng = engines["default", 0]                               # max_batch 3: uestc_max_motions = 6
    assert eng.cfg.uestc_max_motions == 0 and eng.cfg.uestc_classes == 0
    m = R.make_case(7, 1, seed=3)
    st = [s // 4 for s in m.strides]
    lo, fe = np.zeros((7, R.NC), np.float32), np.zeros((7, 256), np.float32)
    eng.uestc_recognize(m, st, 6, 1, lo, fe)                                                    # B = uestc_max_motions
    assert code(lambda: eng.uestc_recognize(m, st, 7, 1, lo, fe)) == EINVAL                     # one more
    assert code(lambda: eng.uestc_recognize(m, st, 0, 1, lo, fe)) == EINVAL                     # B = 0
    assert code(lambda: eng.uestc_recognize(m, st, 1, 17, lo, fe)) == EINVAL                    # T > max_frames
    assert code(lambda: eng.uestc_recognize(m, st, 1, 0, lo, fe)) == EINVAL                     # T = 0
    assert code(lambda: eng.uestc_recognize(m, st, 1, 1, None, None)) == EINVAL                 # both outputs NULL
    assert code(lambda: eng.uestc_recognize(None, st, 1, 1, lo, fe)) == EINVAL                  # a null input
    assert code(lambda: eng.uestc_recognize(m, None, 1, 1, lo, fe)) == EINVAL                   # null strides
    for bad in ([0, 6, 1, 1], [144, -6, 1, 1], [144, 6, 0, 1], [144, 6, 1, -1]):
        assert code(lambda: eng.uestc_recognize(m, bad, 1, 1, lo, fe)) == EINVAL                # a non-positive stride
    small = _lib.Engine(lib=simlib.sim_library(), use_graph=0, **R.engine_kwargs(max_batch=2, uestc_max_motions=3, uestc_classes=7))
    sd = {**R.weights(), **{k: v[:7].copy() for k, v in R.weights().items() if k.startswith("fcn.")}}
    assert R.load(small, sd) == []
    lo7 = np.zeros((3, 7), np.float32)
    small.uestc_recognize(m, st, 3, 1, lo7, None)
    assert np.array_equal(lo7, run(eng, m[:3])[0][:, :7])                                       # fcn rows are independent: the first 7 classes of the 40
    assert code(lambda: small.uestc_recognize(m, st, 4, 1, lo, fe)) == EINVAL
    small.close()


def test_states_weight_group_and_config_checks():
    m = R.make_case(1, 1, seed=4)
    st = [s // 4 for s in m.strides]
    lo = np.zeros((1, R.NC), np.float32)
    plain = _lib.Engine(lib=simlib.sim_library(), use_graph=0, num_layers=3, max_batch=3, max_frames=16)      # no net on the handle
    assert code(lambda: plain.uestc_recognize(m, st, 1, 1, lo)) == ESTATE
    assert plain.load_tensor("uestc_rec.fcn.weight", np.zeros((3, 3), np.float32)) is False                  # ignored, mis-shaped or not
    assert plain.load_tensor("uestc_rec.A", R.weights()["A"]) is False
    assert not any(k.startswith("uestc_rec.") for k in plain.missing_keys())
    plain.close()
    eng = sim_engine(0, finalize=False)
    assert code(lambda: eng.uestc_recognize(m, st, 1, 1, lo)) == ESTATE                      # not finalized
    eng.close()
    eng = _lib.Engine(lib=simlib.sim_library(), use_graph=0, **R.engine_kwargs())             # the group is not loaded (another one is)
    eng.load_tensor("mean", np.zeros(263, np.float32))
    eng.load_tensor("std", np.ones(263, np.float32))
    eng.finalize()
    assert code(lambda: eng.uestc_recognize(m, st, 1, 1, lo)) == ESTATE
    with pytest.raises(_lib.MldHipError) as ei:
        eng.load_tensor("uestc_rec.st_gcn_networks.4.residual.0.weight", np.zeros((128, 128, 1, 1), np.float32))   # a wrong shape
    assert ei.value.code == EINVAL
    assert R.load(eng, R.weights(), finalize=False, skip=("fcn.bias", "edge_importance.7")) == []
    missing = eng.missing_keys()
    assert "uestc_rec.fcn.bias" in missing and "uestc_rec.edge_importance.7" in missing and "uestc_rec.fcn.weight" not in missing
    assert sum(k.startswith("uestc_rec.") for k in missing) == 2
    with pytest.raises(_lib.MldHipError):
        eng.finalize()                                                                         # a half-loaded group
    eng.close()
    for bad in (dict(uestc_rec=2), dict(uestc_max_motions=-1), dict(uestc_max_motions=(1 << 20) + 1), dict(uestc_classes=257), dict(uestc_classes=-1),
                dict(precision=2)):
        with pytest.raises(_lib.MldHipError) as ei:
            _lib.Engine(lib=simlib.sim_library(), use_graph=0, **{**R.engine_kwargs(), **bad})
        assert ei.value.code == EINVAL


def test_an_older_struct_has_no_net():
    lib = simlib.sim_library()
    assert lib.mldhip_abi_version() == 8 == _lib.ABI_VERSION
    assert "mldhip_uestc_recognize" in _lib.exported_symbols() and hasattr(lib, "mldhip_uestc_recognize")
    cfg = _lib.Config()
    lib.mldhip_default_config(C.byref(cfg))
    assert cfg.struct_size == C.sizeof(_lib.Config) and cfg.uestc_rec == 0 and cfg.uestc_max_motions == 0 and cfg.uestc_classes == 0
    # a caller built before the fields passes the struct that ends behind a2m_max_motions: accepted, no net whatever the bytes behind it say
    cfg.struct_size = _lib.Config.uestc_rec.offset
    cfg.num_layers, cfg.max_batch, cfg.max_frames, cfg.uestc_rec = 3, 2, 16, 1
    h = C.c_void_p()
    assert lib.mldhip_create(C.byref(cfg), 0, C.byref(h)) == 0
    assert lib.mldhip_load_tensor(h, b"uestc_rec.fcn.bias", np.zeros(40, np.float32).ctypes.data, (C.c_int64 * 1)(40), 1, 0, 0) == 1      # ignored
    x = np.zeros((1, 24, 6, 1), np.float32)
    lo = np.zeros((1, 40), np.float32)
    assert lib.mldhip_uestc_recognize(h, x.ctypes.data, (C.c_int64 * 4)(144, 6, 1, 1), 1, 1, lo.ctypes.data, None, None) == ESTATE
    # ... and a caller's numeric-info struct that ends behind probe_err_eval is accepted too
    info = _lib.NumericInfo()
    info.struct_size = _lib.NumericInfo.uestc_split_ok.offset
    info.uestc_split_ok = 77
    assert lib.mldhip_numeric_status(h, C.byref(info)) == 0 and info.uestc_split_ok == 77
    lib.mldhip_destroy(h)
