"""The HumanAct12 recognition GRU of the engine (mldhip_a2m_recognize) on the MI355X, both arithmetic modes, against the project's float64 restatement
(tests/a2m_rec_ref.py: the restatement, the inputs and both rules -- within 4 x the float32-CPU error of the same restatement on the same inputs, and
the float64 argmax on every row whose top-two gap is >= 1e-4).  B = 1, 15, 16 and 17 (one below, at and one above the 16-motion tile) at T = 13 and
T = 60 with lengths 1, T and ragged, and B = 128 (one metric update's 4 x 32 motions) at T = 60; two weight families (PyTorch's default init, and the
recurrent weights x 3: saturated gates); the capacity edge; NaN in padded frames; a motion alone and in a batch; the non-finite counter; both modes
bit-equal; and one action-engine run: sample_action -> smpl_forward(MLDHIP_SMPL_TRANS_JOINTS) -> a2m_recognize on the same handle.  The measured ratios
go to the file MLDHIP_A2M_REC_JSON names (profiles/a2m_rec.json is written from such a run)."""
import faulthandler
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import a2m_rec_ref as R  # noqa: E402
import smpl_ref as S  # noqa: E402
from mld_hip import _lib  # noqa: E402
from mld_hip import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu

TIME_LIMIT_S = 120
MAX_BATCH = 32                    # a2m_max_motions = 4 x 32 = 128
_cases = {}

CASES = {f"B {B}, T {T}": (B, T, None) for T in (13, 60) for B in (1, 15, 16, 17)}
CASES["B 1, T 60, len 60"] = (1, 60, [60])
CASES["B 128, T 60"] = (128, 60, None)


@pytest.fixture(autouse=True)
def time_limit():
    """every test of this file ends after TIME_LIMIT_S at the latest, also when it is blocked inside a device synchronisation"""
    faulthandler.dump_traceback_later(TIME_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def engines():
    out = {}
    for fam in R.FAMILIES:
        for prec in (0, 1):
            eng = _lib.Engine(device=0, precision=prec, **R.engine_kwargs(max_batch=MAX_BATCH, max_frames=60))
            assert R.load(eng, R.weights(fam)) == []
            out[fam, prec] = eng
    yield out
    for eng in out.values():
        eng.close()
    dump = os.environ.get("MLDHIP_A2M_REC_JSON")
    if dump:
        json.dump({"rule": "err = max|engine - fp64 restatement|, e32 = max|torch fp32 CPU restatement - fp64 restatement|; both modes within 4 x e32 "
                           "(exact fp32 in both) and bit-equal", "cases": _cases}, open(dump, "w"), indent=1)


def run(eng, joints, lens, h0, logits=True, act=True):
    dev = "cuda:0"
    j = torch.from_numpy(np.ascontiguousarray(joints)).to(dev)
    h = None if h0 is None else torch.from_numpy(np.ascontiguousarray(h0)).to(dev)
    B = len(lens)
    lo = torch.full((B, 12), float("nan"), device=dev) if logits else None
    ac = torch.full((B, 30), float("nan"), device=dev) if act else None
    eng.a2m_recognize(j, lens, j.shape[1], h, lo, ac, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (lo.cpu().numpy() if logits else None), (ac.cpu().numpy() if act else None)


def check(out, ref, what, prec):
    r64, e32 = ref
    err = float(np.abs(out.astype(np.float64) - r64).max())
    print(f"{what}: mode {prec}  err {err:.3e}  e32 {e32:.3e}  ratio {err / e32:.2f}")
    _cases[f"{what} / {'F16X3' if prec else 'F32'}"] = {"err": err, "e32": e32, "ratio": err / e32, "bound": R.F32_FACTOR}
    assert e32 > 0 and np.isfinite(out).all()
    assert err <= R.F32_FACTOR * e32, (what, prec, err, e32)


@pytest.fixture(scope="module")
def refs():
    """inputs and the float64 restatement of every (case, family), computed once, shared, left unchanged"""
    out = {}
    for name, (B, T, lens) in CASES.items():
        j, ln, h0 = R.make_case(B, T, lens=lens)
        for fam in R.FAMILIES:
            out[name, fam] = (j, ln, h0, R.reference(R.weights(fam), j, ln, h0))
    return out


@pytest.fixture(scope="module")
def outs(engines, refs):
    return {(name, fam, prec): run(engines[fam, prec], j, ln, h0) for (name, fam), (j, ln, h0, _) in refs.items() for prec in (0, 1)}


@pytest.mark.parametrize("fam", list(R.FAMILIES))
@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_fp64_and_classes(refs, outs, name, fam):
    _, _, _, (rl, ra) = refs[name, fam]
    R.check_gaps(rl[0])
    for prec in (0, 1):
        lo, ac = outs[name, fam, prec]
        check(lo, rl, f"logits, {name}, {fam}", prec)
        check(ac, ra, f"activations, {name}, {fam}", prec)
        R.check_classes(lo, rl[0])


@pytest.mark.parametrize("fam", list(R.FAMILIES))
def test_both_modes_bit_equal(outs, fam):
    for name in CASES:
        assert np.array_equal(outs[name, fam, 0][0], outs[name, fam, 1][0]) and np.array_equal(outs[name, fam, 0][1], outs[name, fam, 1][1])


def test_capacity_edge(engines, refs, outs):
    eng = engines["default", 0]
    j, ln, h0, _ = refs["B 128, T 60", "default"]
    j2 = np.concatenate([j, j[:1]])
    h2 = np.concatenate([h0, h0[:, :1]], axis=1)
    with pytest.raises(_lib.MldHipError) as ei:
        run(eng, j2, ln + ln[:1], h2)
    assert ei.value.code == -1
    lo, ac = run(eng, j, ln, h0)                                                # B = a2m_max_motions still passes, with the same bits
    assert np.array_equal(lo, outs["B 128, T 60", "default", 0][0]) and np.array_equal(ac, outs["B 128, T 60", "default", 0][1])


@pytest.mark.parametrize("fam", list(R.FAMILIES))
def test_padded_frames_are_never_read(engines, refs, outs, fam):
    for name in ("B 17, T 60", "B 128, T 60"):
        j, ln, h0, _ = refs[name, fam]
        g = j.copy()
        for b, n in enumerate(ln):
            g[b, n:] = np.nan
        lo, ac = run(engines[fam, 0], g, ln, h0)
        assert np.array_equal(lo, outs[name, fam, 0][0]) and np.array_equal(ac, outs[name, fam, 0][1])


def test_a_motion_alone_and_in_a_batch(engines, refs, outs):
    eng = engines["rec_x3", 1]
    j, ln, h0, _ = refs["B 128, T 60", "rec_x3"]
    full = outs["B 128, T 60", "rec_x3", 1]
    for b in (0, 15, 16, 77, 127):
        n = ln[b]
        for T_ in (60, n):                                                      # ... also cut to its own length
            lo, ac = run(eng, j[b:b + 1, :T_], ln[b:b + 1], h0[:, b:b + 1])
            assert np.array_equal(lo[0], full[0][b]) and np.array_equal(ac[0], full[1][b])
    lo, ac = run(eng, j[::-1], ln[::-1], h0[:, ::-1])
    assert np.array_equal(lo[::-1], full[0]) and np.array_equal(ac[::-1], full[1])


def test_h0_null_is_zeros(engines, refs):
    j, ln, h0, _ = refs["B 17, T 13", "default"]
    z = np.zeros_like(h0)
    rl, ra = R.reference(R.weights(), j, ln, z)
    lo, ac = run(engines["default", 0], j, ln, None)
    check(lo, rl, "logits, B 17, T 13, h0 = NULL", 0)
    check(ac, ra, "activations, B 17, T 13, h0 = NULL", 0)


def test_counter(engines, refs):
    eng = engines["default", 1]
    j, ln, h0, _ = refs["B 17, T 13", "default"]
    run(eng, j, ln, h0)
    assert eng.numeric_status()["nonfinite_values"] == 0
    g = j.copy()
    g[16, 0, 3] = np.nan                                                       # the only frame of the last motion (the second tile)
    lo, ac = run(eng, g, ln, h0)
    assert eng.numeric_status()["nonfinite_values"] == int((~np.isfinite(lo)).sum() + (~np.isfinite(ac)).sum()) == 42
    assert np.isfinite(lo[:16]).all() and np.isfinite(ac[:16]).all()


def test_action_engine_sample_smpl_recognize():
    """config_mld_humanact12's engine (15-layer denoiser, 6-layer ActorVae; 10 steps) with the body model and the recognizer on the same handle:
    mldhip_sample_action, mldhip_smpl_forward(MLDHIP_SMPL_TRANS_JOINTS) on its features, mldhip_a2m_recognize on those joints, against the restatement
    applied to the engine's own joints."""
    cfg = dict(condition=_lib.COND_ACTION, nclasses=12, vae_arch=_lib.VAE_ACTOR, vae_num_layers=6, num_layers=15, nfeats=150)
    eng = _lib.Engine(device=0, precision=1, max_batch=4, max_frames=24, num_inference_steps=10, smpl_verts=6890, a2m_rec=1, **cfg)
    dims = syn.ModelDims(num_layers=15, nfeats=150)
    eng.load_state_dict(syn.make_denoiser_state_dict(seed=3, dims=dims, condition="action", nclasses=12), "denoiser.")
    eng.load_state_dict(syn.make_actor_vae_state_dict(num_layers=6), "vae.")
    assert S.load_body(eng, S.body(6890), finalize=False) == []
    assert R.load(eng, R.weights()) == []
    acts, lat0, _ = syn.make_action_batch(3, 24)
    lens = [24, 11, 17]
    dev = "cuda:0"
    stream = torch.cuda.current_stream().cuda_stream
    lat, feats = torch.empty(3, 1, 256, device=dev), torch.empty(3, 24, 150, device=dev)
    eng.sample_action([int(a) for a in acts], torch.from_numpy(lat0).to(dev), lens, lat, feats, stream)
    joints = torch.full((3, 24, 24, 3), float("nan"), device=dev)
    eng.smpl_forward(feats, lens, 24, joints, None, _lib.SMPL_TRANS_JOINTS, stream)
    h0 = torch.randn(2, 3, 128, generator=torch.Generator().manual_seed(9))
    lo, ac = torch.full((3, 12), float("nan"), device=dev), torch.full((3, 30), float("nan"), device=dev)
    eng.a2m_recognize(joints, lens, 24, h0.to(dev), lo, ac, stream)
    torch.cuda.synchronize()
    jn = joints.cpu().numpy().reshape(3, 24, 72)
    assert np.isfinite(jn).all() and eng.numeric_status()["nonfinite_values"] == 0
    rl, ra = R.reference(R.weights(), jn, lens, h0.numpy())
    check(lo.cpu().numpy(), rl, "logits of sample_action -> smpl_forward joints", 1)
    check(ac.cpu().numpy(), ra, "activations of sample_action -> smpl_forward joints", 1)
    R.check_classes(lo.cpu().numpy(), rl[0])
    eng.close()
