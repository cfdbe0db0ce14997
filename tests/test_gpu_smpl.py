"""The SMPL body model of the engine (mldhip_smpl_forward) on the MI355X at the real V = 6890 (430 whole 16-vertex blocks + one of 10: the partial
block is inherent), both arithmetic modes, against the project's float64 restatement (tests/smpl_ref.py: the restatement, the inputs and the tolerance
rule -- within 4 x the float32-CPU error of the same restatement on the same inputs; there is no reference fixture, ``smplx`` is not installed).
B = 3, T = 8, lengths 8 / 5 / 1 and B = 5, T = 13 (65 frames: past the 16-frame tiles and the 32 frames of a workgroup), one HumanAct12 batch of 64 x 60
frames (where each wave of the vertex kernel walks many vertex blocks), both modes bit-equal, batch independence, the non-finite counter, and one
action-engine run: sample_action, then the body model on its features.  The measured errors go to the
file MLDHIP_SMPL_JSON names (profiles/smpl.json is written from such a run)."""
import faulthandler
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import smpl_ref as R  # noqa: E402
from mld_hip import _lib  # noqa: E402
from mld_hip import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu

V = 6890
TIME_LIMIT_S = 120
_cases = {}


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
        eng = _lib.Engine(device=0, precision=prec, **R.engine_kwargs(V, max_batch=5, max_frames=16))
        assert R.load_body(eng, R.body(V)) == []
        out[prec] = eng
    yield out
    for eng in out.values():
        eng.close()
    dump = os.environ.get("MLDHIP_SMPL_JSON")
    if dump:
        json.dump({"rule": "err = max|engine - fp64 restatement|, e32 = max|torch fp32 CPU restatement - fp64 restatement|; both modes within 4 x e32 (exact fp32 in both)",
                   "V": V, "cases": _cases}, open(dump, "w"), indent=1)


def run(eng, feats, lens, flags=0, joints=True, verts=True, V_=V):
    f = torch.from_numpy(np.ascontiguousarray(feats)).to("cuda:0")
    B, T = f.shape[:2]
    j = torch.full((B, T, 24, 3), float("nan"), device="cuda:0") if joints else None
    v = torch.full((B, T, V_, 3), float("nan"), device="cuda:0") if verts else None
    eng.smpl_forward(f, lens, T, j, v, flags, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (j.cpu().numpy() if joints else None), (v.cpu().numpy() if verts else None)


def check(out, ref, what, prec):
    r64, e32 = ref
    err = float(np.abs(out.astype(np.float64) - r64).max())
    print(f"{what}: mode {prec}  err {err:.3e}  e32 {e32:.3e}  ratio {err / e32:.2f}  max|ref| {np.abs(r64).max():.3f}")
    _cases[f"{what} / {'F16X3' if prec else 'F32'}"] = {"err": err, "e32": e32, "ratio": err / e32, "bound": R.F32_FACTOR}
    assert e32 > 0 and np.isfinite(out).all()
    assert err <= R.F32_FACTOR * e32, (what, prec, err, e32)


CASES = {"B 3, T 8": ([8, 5, 1], 8, 0), "B 5, T 13": ([13, 7, 1, 13, 2], 13, 1)}


@pytest.fixture(scope="module")
def refs():
    """inputs and the float64 restatement of both shapes with both flags on (computed once, shared, left unchanged)"""
    out = {}
    for name, (lens, T, seed) in CASES.items():
        f = R.make_feats(lens, T, seed=seed)
        out[name] = (f, lens, R.reference(R.body(V), f, lens, 3))
    return out


@pytest.fixture(scope="module")
def outs(engines, refs):
    return {(name, prec): run(eng, f, lens, 3) for name, (f, lens, _) in refs.items() for prec, eng in engines.items()}


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_fp64(refs, outs, name, prec):
    _, _, (rj, rv) = refs[name]
    j, v = outs[name, prec]
    check(j, rj, f"joints, {name}", prec)
    check(v, rv, f"vertices, {name}", prec)


def test_flags_off_parity_and_padded_frames(engines, refs):
    f, lens, _ = refs["B 3, T 8"]
    rj, rv = R.reference(R.body(V), f, lens, 0)
    j, v = run(engines[0], f, lens, 0)
    check(j, rj, "joints, B 3, T 8, no translation", 0)
    check(v, rv, "vertices, B 3, T 8, no translation", 0)
    for b, n in enumerate(lens):
        assert not j[b, n:].any() and not v[b, n:].any()


@pytest.mark.parametrize("name", list(CASES))
def test_both_modes_bit_equal(outs, name):
    assert np.array_equal(outs[name, 0][0], outs[name, 1][0]) and np.array_equal(outs[name, 0][1], outs[name, 1][1])


def test_batch_independence_and_single_outputs(engines, refs, outs):
    f, lens, _ = refs["B 5, T 13"]
    eng = engines[0]
    full_j, full_v = outs["B 5, T 13", 0]
    for b in (0, 2, 4):
        j, v = run(eng, f[b:b + 1], lens[b:b + 1], 3)
        assert np.array_equal(j[0], full_j[b]) and np.array_equal(v[0], full_v[b])
    j, v = run(eng, f[::-1], lens[::-1], 3)
    assert np.array_equal(j[::-1], full_j) and np.array_equal(v[::-1], full_v)
    j, _ = run(eng, f, lens, 3, verts=False)                                   # the chain kernel alone
    assert np.array_equal(j, full_j)
    _, v = run(eng, f, lens, 3, joints=False)
    assert np.array_equal(v, full_v)


def test_counter(engines, refs):
    f, lens, _ = refs["B 3, T 8"]
    eng = engines[1]
    run(eng, f, lens, 3)
    assert eng.numeric_status()["nonfinite_values"] == 0
    g = f.copy()
    g[0, 2, 3] = np.nan                                                        # component 0 of joint 3 in a valid frame
    j, v = run(eng, g, lens, 0)
    n = eng.numeric_status()["nonfinite_values"]
    assert n == int((~np.isfinite(j)).sum() + (~np.isfinite(v)).sum()) and n >= 3 * V
    assert np.isfinite(v[0, :2]).all() and np.isfinite(v[0, 3:]).all() and np.isfinite(v[1:]).all()      # the frame's own rows only
    g = f.copy()
    g[1, 7, 24] = np.inf                                                       # the translation of a padded frame: seen only through the flags
    run(eng, g, lens, 0)
    assert eng.numeric_status()["nonfinite_values"] == 0
    run(eng, g, lens, 3)
    assert eng.numeric_status()["nonfinite_values"] == 24 + V


def test_humanact12_batch_waves_walk_several_vertex_blocks():
    """One HumanAct12 batch, B = 64 x T = 60 at V = 6890, with tools/ab_smpl.py's inputs.  Its 3 840 frames are 240 tiles in 120 frame groups, so the vertex
    kernel runs 5 lanes of workgroups per group and each wave walks about 22 of the 431 vertex blocks (the shapes above give each wave one block at
    most).  The F32 handle against the float64 restatement, computed one motion at a time on the CPU; the F16X3 handle bit-equal to it."""
    f, lens = R.humanact12_batch()
    rj, rv = R.reference_per_motion(R.body(V), f, lens, 3)
    res = {}
    for prec in (0, 1):
        eng = _lib.Engine(device=0, precision=prec, **R.engine_kwargs(V, max_batch=64, max_frames=60))
        assert R.load_body(eng, R.body(V)) == []
        res[prec] = run(eng, f, lens, 3)
        assert eng.numeric_status()["nonfinite_values"] == 0
        eng.close()
    check(res[0][0], rj, "joints, B 64, T 60", 0)
    check(res[0][1], rv, "vertices, B 64, T 60", 0)
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


def test_action_engine_sample_then_body_model():
    """config_mld_humanact12's engine (15-layer denoiser, 6-layer ActorVae; 10 steps) with the body model on the same handle: mldhip_sample_action, then
    mldhip_smpl_forward on the features it left on the device, against the restatement on those features."""
    cfg = dict(condition=_lib.COND_ACTION, nclasses=12, vae_arch=_lib.VAE_ACTOR, vae_num_layers=6, num_layers=15, nfeats=150)
    eng = _lib.Engine(device=0, precision=1, max_batch=4, max_frames=24, num_inference_steps=10, smpl_verts=V, **cfg)
    dims = syn.ModelDims(num_layers=15, nfeats=150)
    eng.load_state_dict(syn.make_denoiser_state_dict(seed=3, dims=dims, condition="action", nclasses=12), "denoiser.")
    eng.load_state_dict(syn.make_actor_vae_state_dict(num_layers=6), "vae.")
    assert R.load_body(eng, R.body(V)) == []
    acts, lat0, _ = syn.make_action_batch(3, 24)
    lens = [24, 11, 17]
    dev = "cuda:0"
    lat, feats = torch.empty(3, 1, 256, device=dev), torch.empty(3, 24, 150, device=dev)
    eng.sample_action([int(a) for a in acts], torch.from_numpy(lat0).to(dev), lens, lat, feats, torch.cuda.current_stream().cuda_stream)
    j = torch.full((3, 24, 24, 3), float("nan"), device=dev)
    v = torch.full((3, 24, V, 3), float("nan"), device=dev)
    eng.smpl_forward(feats, lens, 24, j, v, _lib.SMPL_TRANS_JOINTS, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    f = feats.cpu().numpy()
    assert np.isfinite(f).all() and eng.numeric_status()["nonfinite_values"] == 0
    rj, rv = R.reference(R.body(V), f, lens, R.TRANS_JOINTS)
    check(j.cpu().numpy(), rj, "joints of sample_action's features", 1)
    check(v.cpu().numpy(), rv, "vertices of sample_action's features", 1)
    eng.close()
