"""The UESTC recognition ST-GCN of the engine (mldhip_uestc_recognize) on the MI355X, both arithmetic modes, against the project's float64 restatement
(tests/uestc_rec_ref.py: the restatement, the inputs and both rules -- F32 handles within 4 x, F16X3 handles within 16 x the float32-CPU error of the same
restatement on the same inputs, and the float64 argmax on every row whose top-two gap is >= 1e-4).  The simulator's cases (T = 13, 5, 1 at B = 1 and 3),
one UESTC-shaped call (B = 16, T = 60: 60 -> 30 -> 15), both weight families; both stride conventions and a non-contiguous view with identical bits;
batch independence; a call of more motions than the workspace holds (chunks); NaN containment and the counter; finalize's probe (kept split on both
families, fallback with F32 bits on the overflow family); the guards.  The measured ratios go to the file MLDHIP_UESTC_REC_JSON names
(profiles/uestc_rec.json is written from such a run)."""
import faulthandler
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import uestc_rec_ref as R  # noqa: E402
from mld_hip import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

TIME_LIMIT_S = 120
DEV = "cuda:0"
_cases = {}

CASES = {"B 3, T 13": (3, 13), "B 1, T 13": (1, 13), "B 3, T 5": (3, 5), "B 1, T 1": (1, 1), "B 16, T 60": (16, 60)}


@pytest.fixture(autouse=True)
def time_limit():
    """every test of this file ends after TIME_LIMIT_S at the latest, also when it is blocked inside a device synchronisation"""
    faulthandler.dump_traceback_later(TIME_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def make_engine(prec, fam, **kw):
    eng = _lib.Engine(device=0, precision=prec, **R.engine_kwargs(**{**dict(max_batch=8, max_frames=60, uestc_max_motions=80), **kw}))
    assert R.load(eng, R.weights(fam)) == []
    return eng


@pytest.fixture(scope="module")
def engines():
    out = {(fam, prec): make_engine(prec, fam) for fam in R.FAMILIES for prec in (0, 1)}
    probe = {fam: out[fam, 1].numeric_status() for fam in R.FAMILIES}
    yield out
    for eng in out.values():
        eng.close()
    dump = os.environ.get("MLDHIP_UESTC_REC_JSON")
    if dump:
        json.dump({"rule": "err = max|engine - fp64 restatement|, e32 = max|torch fp32 CPU restatement - fp64 restatement|; F32 handles within 4 x e32, "
                           "F16X3 handles within 16 x e32", "probe_err_uestc": {f: p["probe_err_uestc"] for f, p in probe.items()}, "cases": _cases},
                  open(dump, "w"), indent=1)


def run(eng, m, logits=True, feat=True):
    """m: a torch tensor [B, 24, 6, T] on the device (any positive strides) or a numpy array (uploaded as it is laid out)"""
    if isinstance(m, np.ndarray):
        m = torch.from_numpy(np.ascontiguousarray(m)).to(DEV)
    B, T = m.shape[0], m.shape[3]
    lo = torch.full((B, R.NC), float("nan"), device=DEV) if logits else None
    fe = torch.full((B, 256), float("nan"), device=DEV) if feat else None
    eng.uestc_recognize(m, m.stride(), B, T, lo, fe, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (lo.cpu().numpy() if logits else None), (fe.cpu().numpy() if feat else None)


def check(out, ref, what, prec):
    err, e32 = R.check(out, ref, what, prec)
    _cases[f"{what} / {'F16X3' if prec else 'F32'}"] = {"err": err, "e32": e32, "ratio": err / e32, "bound": R.X3_FACTOR if prec else R.F32_FACTOR}


@pytest.fixture(scope="module")
def refs():
    """inputs and the float64 restatement of every (case, family), computed once, shared, left unchanged"""
    out = {}
    for name, (B, T) in CASES.items():
        m = R.make_case(B, T)
        for fam in R.FAMILIES:
            out[name, fam] = (m, R.reference(R.weights(fam), m))
    return out


@pytest.fixture(scope="module")
def outs(engines, refs):
    return {(name, fam, prec): run(engines[fam, prec], m) for (name, fam), (m, _) in refs.items() for prec in (0, 1)}


def test_probe_kept_the_split_net(engines):
    for fam in R.FAMILIES:
        st = engines[fam, 1].numeric_status()
        print(f"{fam}: probe_err_uestc {st['probe_err_uestc']:.3e}")
        assert st["probed"] == 1 and st["uestc_split_ok"] == 1 and 0 <= st["probe_err_uestc"] <= _lib.PROBE_TOL
        assert engines[fam, 0].numeric_status()["uestc_split_ok"] == 0


@pytest.mark.parametrize("fam", list(R.FAMILIES))
@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_fp64_and_classes(refs, outs, name, fam):
    _, (rl, rf) = refs[name, fam]
    R.check_gaps(rl[0])
    for prec in (0, 1):
        lo, fe = outs[name, fam, prec]
        check(lo, rl, f"logits, {name}, {fam}", prec)
        check(fe, rf, f"features, {name}, {fam}", prec)
        R.check_classes(lo, rl[0])


def test_both_stride_conventions_and_a_view_give_the_same_bits(engines, refs, outs):
    for name in ("B 3, T 5", "B 16, T 60"):
        m, _ = refs[name, "default"]
        B, T = CASES[name]
        for prec in (0, 1):
            eng, full = engines["default", prec], outs[name, "default", prec]
            rows, _ = R.feature_rows(m)
            view = rows.to(DEV).view(B, T, 6, 25).permute(0, 3, 2, 1)[:, :-1]           # MLD's view of its feature rows: no copy
            assert view.stride() == (150 * T, 1, 25, 150) and not view.is_contiguous()
            lo, fe = run(eng, view)
            assert np.array_equal(lo, full[0]) and np.array_equal(fe, full[1])
            wide = torch.zeros(B, 24, 6, T + 6, device=DEV)
            wide[..., 3:3 + T] = torch.from_numpy(m).to(DEV)
            lo, fe = run(eng, wide[..., 3:3 + T])                                        # a non-contiguous slice against its contiguous copy
            assert np.array_equal(lo, full[0]) and np.array_equal(fe, full[1])


def test_batch_independence_and_single_outputs(engines, refs, outs):
    m, _ = refs["B 16, T 60", "bn_x2"]
    for prec in (0, 1):
        eng, full = engines["bn_x2", prec], outs["B 16, T 60", "bn_x2", prec]
        for b in (0, 7, 15):
            lo, fe = run(eng, m[b:b + 1])
            assert np.array_equal(lo[0], full[0][b]) and np.array_equal(fe[0], full[1][b])
        lo, fe = run(eng, m[::-1])
        assert np.array_equal(lo[::-1], full[0]) and np.array_equal(fe[::-1], full[1])
        lo, fe = run(eng, m, feat=False)
        assert fe is None and np.array_equal(lo, full[0])
        lo, fe = run(eng, m, logits=False)
        assert lo is None and np.array_equal(fe, full[1])


def test_a_call_larger_than_the_workspace_runs_in_chunks(engines, refs, outs):
    """max_frames = 60 and the workspace of 64 motions at that length: 80 motions of 60 frames go through in chunks of 64 and 16, every row with the
    bits it has in the 16-motion call (whose parity with float64 is checked above); the capacity edge is uestc_max_motions = 80"""
    m, _ = refs["B 16, T 60", "default"]
    big = np.concatenate([m, m[::-1], m[:8], m[8:], m, m[::-1]])
    assert len(big) == 80
    for prec in (0, 1):
        full = outs["B 16, T 60", "default", prec]
        lo, fe = run(engines["default", prec], big)
        assert np.array_equal(lo, np.concatenate([full[0], full[0][::-1], full[0], full[0], full[0][::-1]]))
        assert np.array_equal(fe, np.concatenate([full[1], full[1][::-1], full[1], full[1], full[1][::-1]]))
    with pytest.raises(_lib.MldHipError) as ei:
        run(engines["default", 0], np.concatenate([big, m[:1]]))
    assert ei.value.code == -1


def test_nan_stays_in_its_motion_and_is_counted(engines, refs, outs):
    m, _ = refs["B 16, T 60", "default"]
    for prec in (0, 1):
        eng, full = engines["default", prec], outs["B 16, T 60", "default", prec]
        eng.numeric_status()
        g = m.copy()
        g[9, 23, 5, 59] = np.nan
        lo, fe = run(eng, g)
        assert eng.numeric_status()["nonfinite_values"] == R.NC + 256
        assert not np.isfinite(lo[9]).any() and not np.isfinite(fe[9]).any()
        keep = [b for b in range(16) if b != 9]
        assert np.array_equal(lo[keep], full[0][keep]) and np.array_equal(fe[keep], full[1][keep])


def test_overflow_family_falls_back_to_f32_bits(refs):
    m, _ = refs["B 3, T 13", "default"]
    x3, f32 = make_engine(1, "overflow"), make_engine(0, "overflow")
    st = x3.numeric_status()
    print("overflow family: probe_err_uestc", st["probe_err_uestc"])
    assert st["probed"] == 1 and st["uestc_split_ok"] == 0 and not st["probe_err_uestc"] <= _lib.PROBE_TOL
    a, b = run(x3, m), run(f32, m)
    assert np.isfinite(b[0]).all() and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    x3.close()
    f32.close()


def test_guards(engines, refs):
    eng = engines["default", 0]
    m = torch.from_numpy(refs["B 3, T 5", "default"][0]).to(DEV)
    lo, fe = torch.zeros(3, R.NC, device=DEV), torch.zeros(3, 256, device=DEV)

    def code(fn):
        with pytest.raises(_lib.MldHipError) as ei:
            fn()
        return ei.value.code

    assert code(lambda: eng.uestc_recognize(m, m.stride(), 3, 61, lo, fe)) == -1
    assert code(lambda: eng.uestc_recognize(m, m.stride(), 0, 5, lo, fe)) == -1
    assert code(lambda: eng.uestc_recognize(m, m.stride(), 3, 5, None, None)) == -1
    assert code(lambda: eng.uestc_recognize(None, m.stride(), 3, 5, lo, fe)) == -1
    assert code(lambda: eng.uestc_recognize(m, (720, 30, 5, 0), 3, 5, lo, fe)) == -1
    plain = _lib.Engine(device=0, num_layers=3, max_batch=2, max_frames=16)
    assert code(lambda: plain.uestc_recognize(m, m.stride(), 3, 5, lo, fe)) == -3
    plain.close()
