""""dec_lean" on the MI355X: the decoder that skips what the joints never read (joints-only final stage, layer 0 from the positional
table and one attention output per distinct length, non-finite joints counted where they are stored) against "dec_lean" 0, to the bit.

Shape and lengths of tests/test_dec_lean_sim.py: B = 5, T = 52 (48-row strips straddle sample boundaries, T no multiple of 16),
lengths [52, 37, 52, 37, 20] (samples 2 and 3 are not their own representatives, 3's is not sample 0, 4 is alone), with the options that
take 260 .. 416 frame rows through the fused layer tail, the key-blocked attention and the final strip; modes F32 (none of those kernels
exists there: the option must change nothing) and F16X3."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from mld_hip import _lib  # noqa: E402
from mld_hip import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu

T, LENS_A, LENS_B = 52, [52, 37, 52, 37, 20], [52, 20, 37]


@pytest.fixture(scope="module", params=[0, 1], ids=["f32", "f16x3"])
def eng(request):
    assert torch.cuda.is_available()
    e = _lib.Engine(device=0, precision=request.param, max_batch=8, max_frames=T, num_inference_steps=2, max_in_flight=2)
    e.load_state_dict(syn.make_denoiser_state_dict(), "denoiser.")
    e.load_state_dict(syn.make_vae_state_dict(), "vae.")
    mean, std = syn.make_mean_std()
    e.load_tensor("mean", mean)
    e.load_tensor("std", std)
    e.finalize()
    e.set_option("gemm_small_m", 0)
    e.set_option("ffn_strip", 3)
    e.set_option("flash_attn", 2)
    yield request.param, e
    e.close()


def _inputs(lens, seed):
    b = syn.make_batch(len(lens), lens, seed=seed)
    dev = torch.device("cuda:0")
    return torch.from_numpy(np.ascontiguousarray(b.text_emb)).to(dev), torch.from_numpy(np.ascontiguousarray(b.init_latents)).to(dev)


def _request(lens, seed, feats):
    dev = torch.device("cuda:0")
    text, lat0 = _inputs(lens, seed)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    q = {"lengths": lens, "text_emb": text, "init_latents": lat0, "latents_out": nan(len(lens), 1, 256), "joints_out": nan(len(lens), max(lens), 22, 3)}
    if feats:
        q["feats_out"] = nan(len(lens), max(lens), 263)
    return q


def _many(e, lean, feats=(False, False)):
    e.set_option("dec_lean", lean)
    rq = [_request(LENS_A, 11, feats[0]), _request(LENS_B, 12, feats[1])]
    e.sample_many(rq)
    torch.cuda.synchronize()
    return rq


def _same(a, b):
    for qa, qb in zip(a, b):
        for k in ("latents_out", "joints_out", "feats_out"):
            if k in qa:
                assert torch.isfinite(qa[k]).all() and torch.equal(qa[k], qb[k]), k


def test_sample_many_joints_only(eng):
    _, e = eng
    off, on = _many(e, 0), _many(e, 1)
    _same(on, off)
    assert e.numeric_status()["nonfinite_values"] == 0


def test_sample_many_one_request_wants_features(eng):
    _, e = eng
    off, on = _many(e, 0, (True, False)), _many(e, 1, (True, False))
    _same(on, off)
    f = on[0]["feats_out"]
    for i, n in enumerate(LENS_A):
        assert bool((f[i, n:] == 0).all()) and bool((f[i, :n].abs().amax(dim=0) > 0).all())      # all 263 columns filled, padded frames zero
    _same([on[1]], [_many(e, 1)[1]])                                   # the joints-only request: the same bits from the joints-only call


def test_many_pipeline_equals_serial(eng):
    prec, e = eng
    e.set_option("many_pipeline", 1)
    try:
        off, on = _many(e, 0), _many(e, 1)
        _same(on, off)
        if prec == 1:                                                   # the pipelined form exists in the split mode (cluster loop): every request = its own call
            e.set_option("dec_lean", 0)
            for q, (lens, seed) in zip(on, ((LENS_A, 11), (LENS_B, 12))):
                s = _request(lens, seed, False)
                e.sample(s["text_emb"], s["init_latents"], lens, s["latents_out"], None, s["joints_out"])
                torch.cuda.synchronize()
                _same([q], [s])
    finally:
        e.set_option("many_pipeline", 0)


@pytest.mark.parametrize("lens", [[52] * 5, [52, 45, 37, 29, 20]], ids=["one_length", "all_distinct"])
def test_representative_edges(eng, lens):
    """one representative for the whole batch / no sample shares its length"""
    _, e = eng
    out = {}
    for lean in (0, 1):
        e.set_option("dec_lean", lean)
        q = _request(lens, 13, False)
        e.sample(q["text_emb"], q["init_latents"], lens, q["latents_out"], None, q["joints_out"])
        torch.cuda.synchronize()
        out[lean] = q
    _same([out[1]], [out[0]])
