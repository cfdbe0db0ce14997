"""The text-to-motion metric kernels of the engine (mldhip_t2m_match / mldhip_act_stats / mldhip_pair_dist) on the functional simulator against the project's
float64 restatement (tests/t2m_metrics_ref.py: the inputs, the restatement, the value and rank rules) at the smallest shapes: match at (N, D, R) =
(32, 512, 32), (23, 6, 5) and (62, 30, 31) with tail rows, ties on both sides of the diagonal, a NaN row and either output NULL; statistics at (2, 1),
(3, 5), (257, 33) and one row below, at and above the chunk size, exact symmetry, call-to-call and mode-to-mode bit equality; pair distances at P = 1 and
40, D = 1, 3 and 512 with a == b; every guard, and the ABI checks that need no device."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import simlib  # noqa: E402
import t2m_metrics_ref as R  # noqa: E402
from mld_hip import _lib  # noqa: E402

EINVAL, ESTATE = -1, -3
MATCH = {"N 32, D 512, R 32": (32, 512, 32), "N 23, D 6, R 5": (23, 6, 5), "N 62, D 30, R 31": (62, 30, 31)}
c = R.CHUNK
STATS = {"N 2, D 1": (2, 1), "N 3, D 5": (3, 5), "N 257, D 33": (257, 33), f"N {c - 1}, D 7": (c - 1, 7), f"N {c}, D 7": (c, 7), f"N {c + 1}, D 7": (c + 1, 7)}


def code(fn):
    with pytest.raises(_lib.MldHipError) as ei:
        fn()
    return ei.value.code


@pytest.fixture(scope="module")
def engines():
    out = {prec: _lib.Engine(lib=simlib.sim_library(), use_graph=0, precision=prec, **R.engine_kwargs()) for prec in (0, 1)}
    yield out
    for eng in out.values():
        eng.close()


@pytest.fixture(scope="module")
def match_refs():
    out = {}
    for name, (N, D, Rr) in MATCH.items():
        t, m = R.match_inputs(N, D)
        out[name] = (t, m, R.match_reference(t, m, Rr))
    return out


def test_chunk_size_is_the_headers():
    assert R.CHUNK == R.header_chunk()


@pytest.mark.parametrize("name", list(MATCH))
def test_match_against_fp64(engines, match_refs, name):
    N, D, Rr = MATCH[name]
    t, m, ref = match_refs[name]
    n = N // Rr * Rr
    assert 0.05 < float((ref["rank64"] == 0).mean()) < 0.95
    rank, diag = R.run_match(engines[0], t, m, Rr)
    assert (rank[n:] == -7).all() and np.isnan(diag[n:]).all()                 # tail rows: untouched
    R.check_value(diag[:n], (ref["diag64"], ref["e32_diag"]), f"diag, {name} (simulator)")
    R.check_ranks(rank[:n], ref, name)
    rank1, diag1 = R.run_match(engines[1], t, m, Rr)                            # the F16X3 handle: the same bits
    assert np.array_equal(rank, rank1) and np.array_equal(diag, diag1, equal_nan=True)
    r_only, _ = R.run_match(engines[0], t, m, Rr, diag=False)                   # either output may be NULL
    _, d_only = R.run_match(engines[0], t, m, Rr, rank=False)
    assert np.array_equal(r_only, rank) and np.array_equal(d_only, diag, equal_nan=True)


def test_match_ties_and_nan(engines, match_refs):
    t, m, _ = match_refs["N 62, D 30, R 31"]
    rank, diag = R.run_match(engines[0], *R.tie_case(t, m), 31)
    R.check_ties(rank)
    rank, diag = R.run_match(engines[0], *R.nan_case(t, m), 31)
    R.check_nan_row(rank, diag)


def test_match_fewer_rows_than_a_group(engines):
    t, m = R.match_inputs(23, 6)
    rank, diag = R.run_match(engines[0], t[:4], m[:4], 5)
    assert (rank == -7).all() and np.isnan(diag).all()


@pytest.mark.parametrize("name", list(STATS))
def test_stats_against_fp64(engines, name):
    N, D = STATS[name]
    x = R.stats_inputs(N, D)
    rm, rc = R.stats_reference(x)
    mean, cov = R.run_stats(engines[0], x)
    R.check_value(mean, rm, f"mean, {name} (simulator)")
    R.check_value(cov, rc, f"cov, {name} (simulator)")
    assert np.array_equal(cov, cov.T)                                          # exactly symmetric
    for prec in (0, 1):                                                         # a second call, and the F16X3 handle: the same bits
        mean1, cov1 = R.run_stats(engines[prec], x)
        assert np.array_equal(mean, mean1) and np.array_equal(cov, cov1)


def test_stats_offset_is_centred_first(engines):
    """x + 100: a one-pass E[xx] - E[x]E[x] form loses the covariance in the rounding of 1e4-sized squares"""
    x = R.stats_inputs(300, 9, offset=100.0)
    rm, rc = R.stats_reference(x)
    mean, cov = R.run_stats(engines[0], x)
    R.check_value(mean, rm, "mean, N 300, D 9, x + 100 (simulator)")
    R.check_value(cov, rc, "cov, N 300, D 9, x + 100 (simulator)")


@pytest.mark.parametrize("D", [1, 3, 512])
@pytest.mark.parametrize("P", [1, 40])
def test_pairs_against_fp64(engines, P, D):
    x, a, b = R.pair_inputs(50, D, P)
    out = R.run_pairs(engines[0], x, a, b)
    R.check_value(out, R.pair_reference(x, a, b), f"dist, P {P}, D {D} (simulator)")
    if P > 1:
        assert out[0] == 0.0 and a[0] == b[0]                                   # a == b: exactly 0
    assert R.run_pairs(engines[0], x, a[:1], a[:1])[0] == 0.0
    assert np.array_equal(out, R.run_pairs(engines[1], x, a, b))


def test_results_do_not_depend_on_the_capacity(engines):
    small = _lib.Engine(lib=simlib.sim_library(), use_graph=0, **R.engine_kwargs(metrics_max_rows=300))
    x = R.stats_inputs(257, 33)
    for a_, b_ in zip(R.run_stats(small, x), R.run_stats(engines[0], x)):
        assert np.array_equal(a_, b_)
    assert code(lambda: R.run_stats(small, R.stats_inputs(301, 3))) == EINVAL
    small.close()


def test_guards(engines):
    eng = engines[0]
    assert eng.cfg.metrics_max_rows == 0                                        # the default: 8192
    x = R.stats_inputs(40, 6)
    big = np.zeros((8193, 2), np.float32)
    rank, diag = np.zeros(40, np.int32), np.zeros(40, np.float32)
    mean, cov = np.zeros(6, np.float32), np.zeros((6, 6), np.float32)
    a, b, out = [0, 1, 2], [3, 4, 5], np.zeros(3, np.float32)
    # mldhip_t2m_match
    assert code(lambda: eng.t2m_match(None, x, 40, 6, 5, rank, diag)) == EINVAL
    assert code(lambda: eng.t2m_match(x, None, 40, 6, 5, rank, diag)) == EINVAL
    assert code(lambda: eng.t2m_match(x, x, 40, 6, 5, None, None)) == EINVAL                  # both outputs NULL
    for R_ in (0, 33):
        assert code(lambda: eng.t2m_match(x, x, 40, 6, R_, rank, diag)) == EINVAL
    for D_ in (0, 1025):
        assert code(lambda: eng.t2m_match(x, x, 40, D_, 5, rank, diag)) == EINVAL
        assert code(lambda: eng.act_stats(x, 40, D_, mean, cov)) == EINVAL
        assert code(lambda: eng.pair_dist(x, 40, D_, a, b, out)) == EINVAL
    assert code(lambda: eng.t2m_match(x, x, 0, 6, 5, rank, diag)) == EINVAL
    assert code(lambda: eng.t2m_match(big, big, 8193, 2, 5, rank, diag)) == EINVAL            # N > metrics_max_rows
    # mldhip_act_stats
    assert code(lambda: eng.act_stats(None, 40, 6, mean, cov)) == EINVAL
    assert code(lambda: eng.act_stats(x, 40, 6, None, cov)) == EINVAL
    assert code(lambda: eng.act_stats(x, 40, 6, mean, None)) == EINVAL
    assert code(lambda: eng.act_stats(x, 1, 6, mean, cov)) == EINVAL                          # N >= 2
    assert code(lambda: eng.act_stats(big, 8193, 2, mean, cov)) == EINVAL
    # mldhip_pair_dist
    assert code(lambda: eng.pair_dist(None, 40, 6, a, b, out)) == EINVAL
    assert code(lambda: eng.pair_dist(x, 40, 6, a, b, None)) == EINVAL
    assert code(lambda: eng.pair_dist(x, 40, 6, [], [], out)) == EINVAL                       # P < 1
    assert code(lambda: eng.pair_dist(big, 8193, 2, a, b, out)) == EINVAL
    assert code(lambda: eng.pair_dist(x, 40, 6, [0] * 8193, [1] * 8193, np.zeros(8193, np.float32))) == EINVAL      # P > metrics_max_rows
    for bad in (-1, 40):                                                                        # an index outside 0 .. N - 1, in either table
        assert code(lambda: eng.pair_dist(x, 40, 6, [0, bad, 2], b, out)) == EINVAL
        assert code(lambda: eng.pair_dist(x, 40, 6, a, [3, 4, bad], out)) == EINVAL
    i32 = (C.c_int32 * 3)(0, 1, 2)
    assert eng.lib.mldhip_pair_dist(eng._h, x.ctypes.data, 40, 6, None, i32, 3, out.ctypes.data, None) == EINVAL
    assert eng.lib.mldhip_pair_dist(eng._h, x.ctypes.data, 40, 6, i32, None, 3, out.ctypes.data, None) == EINVAL
    assert eng.lib.mldhip_act_stats(None, x.ctypes.data, 40, 6, mean.ctypes.data, cov.ctypes.data, None) == EINVAL
    # the calls need no weights and no finalize (this handle has neither), and nothing above left a mark
    eng.pair_dist(x, 40, 6, a, b, out)
    assert np.isfinite(out).all()


def test_states_and_config():
    x = R.stats_inputs(40, 6)
    rank, diag = np.zeros(40, np.int32), np.zeros(40, np.float32)
    mean, cov = np.zeros(6, np.float32), np.zeros((6, 6), np.float32)
    plain = _lib.Engine(lib=simlib.sim_library(), use_graph=0, num_layers=3, max_batch=1, max_frames=16)      # t2m_metrics = 0
    assert code(lambda: plain.t2m_match(x, x, 40, 6, 5, rank, diag)) == ESTATE
    assert code(lambda: plain.act_stats(x, 40, 6, mean, cov)) == ESTATE
    assert code(lambda: plain.pair_dist(x, 40, 6, [0], [1], diag)) == ESTATE
    plain.close()
    for bad in (dict(t2m_metrics=2), dict(t2m_metrics=-1), dict(metrics_max_rows=1), dict(metrics_max_rows=-5), dict(metrics_max_rows=(1 << 20) + 1)):
        with pytest.raises(_lib.MldHipError) as ei:
            _lib.Engine(lib=simlib.sim_library(), use_graph=0, **{**R.engine_kwargs(), **bad})
        assert ei.value.code == EINVAL
    for ok in (2, 1 << 20):
        _lib.Engine(lib=simlib.sim_library(), use_graph=0, **R.engine_kwargs(metrics_max_rows=ok)).close()
    # independent of the other fields: an action engine in bf16 carries them as well
    act = _lib.Engine(lib=simlib.sim_library(), use_graph=0, precision=2, condition=_lib.COND_ACTION, nclasses=12, vae_arch=_lib.VAE_ACTOR, vae_num_layers=2,
                      nfeats=150, **R.engine_kwargs())
    ref = _lib.Engine(lib=simlib.sim_library(), use_graph=0, **R.engine_kwargs())
    for a_, b_ in zip(R.run_stats(act, x), R.run_stats(ref, x)):
        assert np.array_equal(a_, b_)
    act.close()
    ref.close()


def test_an_older_struct_has_no_metrics():
    lib = simlib.sim_library()
    assert lib.mldhip_abi_version() == 8 == _lib.ABI_VERSION
    for name in ("mldhip_t2m_match", "mldhip_act_stats", "mldhip_pair_dist"):
        assert name in _lib.exported_symbols() and hasattr(lib, name)
    cfg = _lib.Config()
    lib.mldhip_default_config(C.byref(cfg))
    assert cfg.struct_size == C.sizeof(_lib.Config) and cfg.t2m_metrics == 0 and cfg.metrics_max_rows == 0
    # a caller built before the fields passes the struct that ends behind uestc_classes: accepted, no metrics whatever the bytes behind it say
    cfg.struct_size = _lib.Config.t2m_metrics.offset
    cfg.num_layers, cfg.max_batch, cfg.max_frames, cfg.t2m_metrics = 3, 1, 16, 1
    h = C.c_void_p()
    assert lib.mldhip_create(C.byref(cfg), 0, C.byref(h)) == 0
    x = np.zeros((4, 3), np.float32)
    mean, cov = np.zeros(3, np.float32), np.zeros((3, 3), np.float32)
    assert lib.mldhip_act_stats(h, x.ctypes.data, 4, 3, mean.ctypes.data, cov.ctypes.data, None) == ESTATE
    lib.mldhip_destroy(h)
