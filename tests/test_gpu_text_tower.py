"""The CLIP text tower of the engine (mldhip_text_encode, ABI 7) on the MI355X: parity with transformers' own
CLIPTextModelWithProjection in float64 in both arithmetic modes (two layers at the real widths; tests/clip_tower_ref.py has the
reference and the tolerance rule: 4 x / 16 x the float32-CPU error of the same model on the same ids), the causality and duplicate
rules to the bit, the guards, and MLD.forward with HipMldTextEncoder against the same model with MldTextEncoder."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytest.importorskip("transformers")

import clip_tower_ref as R  # noqa: E402
from mld_hip import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

LAYERS = 2
EOS_POS = [1, 15, 16, 17, 33, 76]          # the "" prompt, both sides of a key-tile edge, the full context
EINVAL, ESTATE = -1, -3
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ids():
    return R.make_ids(EOS_POS, seed=11)


@pytest.fixture(scope="module")
def reference(ids):
    return R.reference_embeddings(LAYERS, ids)


@pytest.fixture(scope="module")
def engines():
    out = {}
    for prec in (0, 1):
        eng = _lib.Engine(device=0, precision=prec, **R.engine_kwargs(LAYERS, 12))
        assert R.load_tower(eng, LAYERS) == []
        out[prec] = eng
    yield out
    for eng in out.values():
        eng.close()


def encode(eng, ids, eos):
    out = torch.full((len(eos), 1, R.WIDTH), float("nan"), device="cuda:0")
    eng.text_encode(ids, eos, out, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out[:, 0].cpu().numpy()


@pytest.fixture(scope="module")
def outputs(engines, ids):
    return {prec: encode(eng, ids, EOS_POS) for prec, eng in engines.items()}


def test_parity_with_transformers_fp64_both_modes(outputs, reference):
    r64, e32 = reference
    err = {prec: float(np.abs(out.astype(np.float64) - r64).max()) for prec, out in outputs.items()}
    print(f"text tower (MI355X, {LAYERS} layers, EOS at {EOS_POS}): e32 {e32:.3e}  F32 {err[0]:.3e}  F16X3 {err[1]:.3e}  max|ref| {np.abs(r64).max():.3f}")
    dump = os.environ.get("MLDHIP_TEXT_TOWER_PARITY_JSON")       # the record under profiles/ is written from a run with this set
    if dump:
        json.dump({"layers": LAYERS, "eos_positions": EOS_POS, "e32": e32, "err_f32": err[0], "err_f16x3": err[1], "bound_f32": R.F32_FACTOR * e32,
                   "bound_f16x3": R.X3_FACTOR * e32, "max_abs_reference": float(np.abs(r64).max())}, open(dump, "w"), indent=1)
    assert e32 > 0 and np.isfinite(outputs[0]).all() and np.isfinite(outputs[1]).all()
    assert err[0] <= R.F32_FACTOR * e32, (err[0], e32)
    assert err[1] <= R.X3_FACTOR * e32, (err[1], e32)


@pytest.mark.parametrize("prec", [0, 1])
def test_ids_behind_eos_never_reach_the_output(engines, ids, outputs, prec):
    rng = np.random.default_rng(3)
    noisy = ids.copy()
    for p, e in enumerate(EOS_POS):
        noisy[p, e + 1:] = rng.integers(0, R.BOS, size=R.CTX - e - 1)       # random non-EOS ids behind EOS, eos_pos unchanged
    assert (noisy != ids).any()
    assert np.array_equal(encode(engines[prec], noisy, EOS_POS), outputs[prec])


@pytest.mark.parametrize("prec", [0, 1])
def test_duplicates_and_batch_independence(engines, ids, outputs, prec):
    eng = engines[prec]
    many = np.concatenate([np.repeat(ids[:1], 3, axis=0), ids[1:]])
    out = encode(eng, many, [1, 1, 1] + EOS_POS[1:])
    alone = encode(eng, ids[:1], EOS_POS[:1])
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2]) and np.array_equal(out[0], alone[0])
    assert np.array_equal(out[3:], outputs[prec][1:])                       # a prompt's row does not depend on what else is in the call
    for p in (2, 5):
        assert np.array_equal(encode(eng, ids[p:p + 1], EOS_POS[p:p + 1])[0], outputs[prec][p])
    rev = encode(eng, ids[::-1].copy(), EOS_POS[::-1])
    assert np.array_equal(rev[::-1], outputs[prec])
    assert eng.numeric_status()["nonfinite_values"] == 0


def test_guards(engines, ids):
    eng = engines[0]
    out = torch.zeros(16, 1, R.WIDTH, device="cuda:0")

    def code(fn):
        with pytest.raises(_lib.MldHipError) as ei:
            fn()
        return ei.value.code
    assert code(lambda: eng.text_encode(np.repeat(ids[:1], 13, axis=0), [1] * 13, out)) == EINVAL           # P > clip_max_prompts = 12
    bad = ids.copy()
    bad[1, 3] = R.VOCAB
    assert code(lambda: eng.text_encode(bad, EOS_POS, out)) == EINVAL
    assert code(lambda: eng.text_encode(ids, EOS_POS[:-1] + [R.CTX], out)) == EINVAL
    tensors = R.tower_tensors(LAYERS)
    plain = _lib.Engine(device=0, num_layers=3, max_batch=2, max_frames=16)                                  # clip_layers = 0
    towered = _lib.Engine(device=0, **R.engine_kwargs(LAYERS, 12))
    try:
        missing = plain.missing_keys()
        assert all(plain.load_tensor(k, v) is False for k, v in tensors.items())                            # ignored (returns 1), as before
        assert plain.missing_keys() == missing
        assert code(lambda: plain.text_encode(ids, EOS_POS, out)) == ESTATE
        assert code(lambda: towered.text_encode(ids, EOS_POS, out)) == ESTATE                               # before the group is loaded
    finally:
        plain.close()
        towered.close()


def test_mld_forward_with_the_hip_text_encoder(tmp_path):
    """MLD.forward end to end: HipMldTextEncoder (tower in the engine) against MldTextEncoder (tower on PyTorch-ROCm), same CLIP directory,
    same injected start latents: joints within the project's 1e-3 contract."""
    from mld_hip import config as C
    from mld_hip import engine as E
    from mld_hip import synthetic as syn
    from mld_hip.datamodule import HipDataModule
    from mld_hip.mld import MLD
    from mld_hip.text_encoder import HipMldTextEncoder, MldTextEncoder

    d, _ = R.make_clip_dir(tmp_path, 2)
    E.drop_engines()
    saved = dict(E._defaults["text"])
    E.configure("text", max_batch=4, max_frames=64)
    over = {"model.scheduler.num_inference_timesteps": 4, "model.denoiser.params.num_layers": 3, "model.motion_vae.params.num_layers": 3}
    texts, lengths = ["a man walks.", "a person runs."], [12, 9]
    lat0 = torch.from_numpy(syn.make_batch(2, lengths).init_latents).cuda()
    joints = {}
    try:
        for cls in (MldTextEncoder, HipMldTextEncoder):
            conf = C.load_config(overrides=over)
            enc = cls(d).cuda()
            model = MLD(conf, HipDataModule(conf), text_encoder=enc).eval().cuda()
            joints[cls] = model({"text": texts, "length": lengths}, init_latents=lat0)
            if cls is HipMldTextEncoder:
                assert enc.hip_tower
                emb_hip = enc([""] * 2 + texts)
                emb_ref = MldTextEncoder.forward(enc, [""] * 2 + texts)
                print(f"embeddings: max|hip - torch| {float((emb_hip - emb_ref).abs().max()):.3e}")
                assert torch.equal(emb_hip[0], emb_hip[1])
            E.drop_engines()
    finally:
        E.drop_engines()
        E._defaults["text"] = saved
    diff = max(float((a - b).abs().max()) for a, b in zip(joints[MldTextEncoder], joints[HipMldTextEncoder]))
    print(f"MLD.forward joints: max|HipMldTextEncoder - MldTextEncoder| {diff:.3e}")
    assert [tuple(j.shape) for j in joints[HipMldTextEncoder]] == [(12, 22, 3), (9, 22, 3)]
    assert diff < 1e-3
