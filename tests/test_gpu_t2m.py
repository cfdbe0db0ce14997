"""The T2M evaluator towers of the engine (mldhip_t2m_motion_embed / mldhip_t2m_text_embed) on the MI355X, both arithmetic modes, against the project's
float64 restatement (tests/t2m_ref.py: the reference and the tolerance rule, 4 x / 16 x the float32-CPU error of the same model on the same inputs) at the
smallest shapes that reach each edge of the recurrence step kernel (64 motions per workgroup, 16 per wave): one motion, 63 and 65 motions, t2m_max_motions
exactly, lengths mixing one GRU step, T / 4 steps and len % 4 = 3 with T = len, an odd T, the full 49 steps once, the 251-feature layout, captions of one word
and of t2m_max_words, and a call on a side stream beside foreign work.  The measured ratios go to the file MLDHIP_T2M_EVAL_JSON names (profiles/t2m_eval.json
is written from such a run)."""
import faulthandler
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import t2m_ref as R  # noqa: E402
from mld_hip import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_MOTIONS, MAX_WORDS = 65, 8
TIME_LIMIT_S = 120
_ratios = {}


@pytest.fixture(autouse=True)
def time_limit():
    """every test of this file ends after TIME_LIMIT_S at the latest, also when it is blocked inside a device synchronisation"""
    faulthandler.dump_traceback_later(TIME_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def engines():
    out = {}
    for prec in (0, 1):
        eng = _lib.Engine(device=0, precision=prec, **R.engine_kwargs(MAX_MOTIONS, max_frames=196, max_words=MAX_WORDS))
        assert R.load_evaluators(eng) == []
        out[prec] = eng
    yield out
    for eng in out.values():
        eng.close()
    dump = os.environ.get("MLDHIP_T2M_EVAL_JSON")
    if dump:
        json.dump({"rule": "err = max|engine - fp64|, e32 = max|torch fp32 CPU - fp64|; F32 within 4 x e32, F16X3 within 16 x e32", "cases": _ratios}, open(dump, "w"), indent=1)


def motion(eng, feats, lens, renorm=True, stream=None):
    f = torch.from_numpy(np.ascontiguousarray(feats)).to("cuda:0")
    out = torch.full((len(lens), 512), float("nan"), device="cuda:0")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())                        # the inputs were written on the current stream
    eng.t2m_motion_embed(f, lens, feats.shape[1], out, renorm=renorm, stream=(stream or torch.cuda.current_stream()).cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def text(eng, w, p, lens):
    wd, pd = torch.from_numpy(np.ascontiguousarray(w)).to("cuda:0"), torch.from_numpy(np.ascontiguousarray(p)).to("cuda:0")
    out = torch.full((len(lens), 512), float("nan"), device="cuda:0")
    eng.t2m_text_embed(wd, pd, lens, w.shape[1], out, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check(out, r64, e32, prec, what):
    err = float(np.abs(out.astype(np.float64) - r64).max())
    print(f"{what}: mode {prec}  err {err:.3e}  e32 {e32:.3e}  ratio {err / e32:.2f}  max|ref| {np.abs(r64).max():.3f}")
    _ratios[f"{what} / {'F16X3' if prec else 'F32'}"] = {"err": err, "e32": e32, "ratio": err / e32, "bound": (R.F32_FACTOR if prec == 0 else R.X3_FACTOR)}
    assert e32 > 0 and np.isfinite(out).all()
    assert err <= (R.F32_FACTOR if prec == 0 else R.X3_FACTOR) * e32, (what, prec, err, e32)


# 65 motions at T = 16: t2m_max_motions exactly, one motion past a workgroup's 64; lengths mix 4 steps (T / 4), one step, len % 4 = 1 and len % 4 = 3
EDGE_T = 16
EDGE_LENS = [[16, 4, 9, 7, 12, 15][i % 6] for i in range(MAX_MOTIONS)]


@pytest.fixture(scope="module")
def edge_case():
    feats = R.make_motions(EDGE_LENS, EDGE_T, seed=3)
    return feats, R.reference_motion(feats, EDGE_LENS)


@pytest.mark.parametrize("prec", [0, 1])
def test_motion_tower_at_the_step_kernels_row_edges(engines, edge_case, prec):
    feats, (r64, e32) = edge_case
    eng = engines[prec]
    full = motion(eng, feats, EDGE_LENS)
    check(full, r64, e32, prec, "65 motions x 16 frames")
    for n in (63, 1):                                                          # one short of the workgroup's rows; a single motion: the same rows to the bit
        assert np.array_equal(motion(eng, feats[:n], EDGE_LENS[:n]), full[:n])
    assert np.array_equal(motion(eng, feats[64:], EDGE_LENS[64:])[0], full[64])
    ns = eng.numeric_status()
    assert ns["nonfinite_values"] == 0
    if prec == 1:                                                              # the split kernels were what ran: finalize's probe kept the stage split
        print("probe_err_eval (MI355X, plain weights):", ns["probe_err_eval"])
        _ratios["probe_err_eval"] = ns["probe_err_eval"]
        assert ns["probed"] == 1 and ns["eval_split_ok"] == 1 and 0 <= ns["probe_err_eval"] <= _lib.PROBE_TOL


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("T,lens", [(37, [37, 35, 5, 20]), (39, [39, 4, 22])])
def test_odd_T_and_T_equal_to_a_length_with_remainder_3(engines, prec, T, lens):
    feats = R.make_motions(lens, T, seed=T)
    r64, e32 = R.reference_motion(feats, lens)
    check(motion(engines[prec], feats, lens), r64, e32, prec, f"T = {T}, lengths {lens}")


@pytest.mark.parametrize("prec", [0, 1])
def test_full_length_49_steps(engines, prec):
    lens = [196, 196, 180, 123, 64, 40, 7, 4]
    feats = R.make_motions(lens, 196, seed=9)
    r64, e32 = R.reference_motion(feats, lens)
    check(motion(engines[prec], feats, lens), r64, e32, prec, "8 motions x 196 frames")


@pytest.mark.parametrize("prec", [0, 1])
def test_kit_feature_layout(prec):
    eng = _lib.Engine(device=0, precision=prec, nfeats=251, njoints=21, **R.engine_kwargs(2, max_frames=24))
    assert R.load_evaluators(eng, nfeats=251, groups=("motion",)) == []
    lens = [24, 10]
    feats = R.make_motions(lens, 24, nfeats=251, seed=5)
    r64, e32 = R.reference_motion(feats, lens, nfeats=251)
    check(motion(eng, feats, lens), r64, e32, prec, "KIT-ML layout (251 features)")
    eng.close()


@pytest.mark.parametrize("prec", [0, 1])
def test_captions_of_one_word_and_of_max_words(engines, prec):
    eng = engines[prec]
    w, p = R.make_captions([1, 1], 1, seed=1)
    r64, e32 = R.reference_text(w, p, [1, 1])
    check(text(eng, w, p, [1, 1]), r64, e32, prec, "captions of one word")
    lens = [[MAX_WORDS, 1, 3, 5][i % 4] for i in range(MAX_MOTIONS)]
    w, p = R.make_captions(lens, MAX_WORDS, seed=2)
    r64, e32 = R.reference_text(w, p, lens)
    full = text(eng, w, p, lens)
    check(full, r64, e32, prec, f"65 captions x {MAX_WORDS} words")
    assert np.array_equal(text(eng, w[:1], p[:1], lens[:1])[0], full[0])


@pytest.mark.parametrize("prec", [0, 1])
def test_side_stream_beside_foreign_work_is_bit_identical(engines, edge_case, prec):
    feats, _ = edge_case
    eng = engines[prec]
    quiet = motion(eng, feats[:9], EDGE_LENS[:9])
    side, other = torch.cuda.Stream(), torch.cuda.Stream()
    a = torch.randn(2048, 2048, device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(other):
        for _ in range(20):
            a = (a @ a).clamp_(-1, 1)                                          # foreign work on another stream while the towers run
    busy = motion(eng, feats[:9], EDGE_LENS[:9], stream=side)
    assert np.array_equal(busy, quiet)
