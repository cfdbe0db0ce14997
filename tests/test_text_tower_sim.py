"""The CLIP text tower of the engine (mldhip_text_encode, ABI 7) on the functional simulator: one layer, P = 3 prompts with EOS at
1, 17 and 20 (about 40 token rows), against transformers' own CLIPTextModelWithProjection in float64 (tests/clip_tower_ref.py has the
reference and the tolerance rule), plus the causality / duplicate rules and the ABI checks that need no device.  The second half looks at
token rows instead of EOS rows (clip_tower_ref.reference_rows: the prefixes of one id row return every row of the tower), at a second weight
regime and at the tower's stage of the range contract."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytest.importorskip("transformers")

import clip_tower_ref as R  # noqa: E402
import simlib  # noqa: E402
from mld_hip import _lib  # noqa: E402

LAYERS, EOS_POS = 1, [1, 17, 20]
EINVAL, ESTATE = -1, -3


@pytest.fixture(scope="module")
def ids():
    return R.make_ids(EOS_POS, seed=7)


@pytest.fixture(scope="module")
def reference(ids):
    return R.reference_embeddings(LAYERS, ids)


@pytest.fixture(scope="module")
def engines():
    out = {}
    for prec in (0, 1):
        eng = _lib.Engine(lib=simlib.sim_library(), use_graph=0, precision=prec, **R.engine_kwargs(LAYERS, 6))
        assert R.load_tower(eng, LAYERS) == []
        out[prec] = eng
    yield out
    for eng in out.values():
        eng.close()


def encode(eng, ids, eos):
    out = np.full((len(eos), 1, R.WIDTH), np.nan, dtype=np.float32)
    eng.text_encode(ids, eos, out)
    return out[:, 0]


@pytest.fixture(scope="module")
def outputs(engines, ids):
    return {prec: encode(eng, ids, EOS_POS) for prec, eng in engines.items()}


def test_parity_with_transformers_fp64_both_modes(outputs, reference):
    r64, e32 = reference
    err = {prec: float(np.abs(out.astype(np.float64) - r64).max()) for prec, out in outputs.items()}
    print(f"text tower (simulator, {LAYERS} layer): e32 {e32:.3e}  F32 {err[0]:.3e}  F16X3 {err[1]:.3e}  max|ref| {np.abs(r64).max():.3f}")
    assert e32 > 0 and np.isfinite(outputs[0]).all() and np.isfinite(outputs[1]).all()
    assert err[0] <= R.F32_FACTOR * e32, (err[0], e32)
    assert err[1] <= R.X3_FACTOR * e32, (err[1], e32)


def test_ids_behind_eos_never_reach_the_output(engines, ids, outputs):
    rng = np.random.default_rng(3)
    noisy = ids.copy()
    for p, e in enumerate(EOS_POS):
        noisy[p, e + 1:] = rng.integers(0, R.BOS, size=R.CTX - e - 1)       # random non-EOS ids behind EOS, eos_pos unchanged
    assert (noisy != ids).any()
    assert np.array_equal(encode(engines[1], noisy, EOS_POS), outputs[1])


def test_duplicates_and_batch_independence(engines, ids, outputs):
    eng = engines[1]
    many = np.concatenate([np.repeat(ids[:1], 3, axis=0), ids[1:]])
    out = encode(eng, many, [1, 1, 1] + EOS_POS[1:])
    alone = encode(eng, ids[:1], EOS_POS[:1])
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2]) and np.array_equal(out[0], alone[0])
    assert np.array_equal(out[3:], outputs[1][1:])                          # a prompt's row does not depend on what else is in the call
    assert np.array_equal(encode(eng, ids[2:], EOS_POS[2:])[0], outputs[1][2])
    assert eng.numeric_status()["nonfinite_values"] == 0


def test_abi_7_config_and_guards(engines, ids):
    lib = simlib.sim_library()
    assert lib.mldhip_abi_version() == 8 == _lib.ABI_VERSION      # (8 appended the tower's fields to mldhip_numeric_info; the config is ABI 7's)
    cfg = _lib.Config()
    lib.mldhip_default_config(C.byref(cfg))
    assert cfg.struct_size == C.sizeof(_lib.Config)
    assert (cfg.clip_layers, cfg.clip_heads, cfg.clip_ff, cfg.clip_vocab, cfg.clip_ctx) == (0, 12, 3072, 49408, 77)
    eng = engines[0]
    out = np.zeros((8, 1, R.WIDTH), dtype=np.float32)

    def code(fn):
        with pytest.raises(_lib.MldHipError) as ei:
            fn()
        return ei.value.code
    assert code(lambda: eng.text_encode(np.repeat(ids[:1], 7, axis=0), [1] * 7, out)) == EINVAL            # P > clip_max_prompts = 6
    bad = ids.copy()
    bad[1, 40] = R.VOCAB                                                                                  # behind EOS, still validated
    assert code(lambda: eng.text_encode(bad, EOS_POS, out)) == EINVAL
    assert code(lambda: eng.text_encode(ids, [1, 17, R.CTX], out)) == EINVAL
    assert code(lambda: eng.text_encode(ids, [1, -1, 20], out)) == EINVAL
    # refused configurations
    for kw in (dict(clip_heads=8), dict(clip_ctx=81), dict(clip_vocab=0), dict(precision=2)):
        with pytest.raises(_lib.MldHipError) as ei:
            _lib.Engine(lib=lib, use_graph=0, **{**R.engine_kwargs(LAYERS, 6), **kw})
        assert ei.value.code == EINVAL, kw


def test_handles_without_the_tower_are_unchanged(ids):
    lib = simlib.sim_library()
    tensors = R.tower_tensors(LAYERS)
    plain = _lib.Engine(lib=lib, use_graph=0, num_layers=3, max_batch=2, max_frames=16)                   # clip_layers = 0
    towered = _lib.Engine(lib=lib, use_graph=0, **R.engine_kwargs(LAYERS, 6))
    try:
        missing = plain.missing_keys()
        assert not any(k.startswith("text_encoder.") for k in missing)
        assert all(plain.load_tensor(k, v) is False for k, v in tensors.items())                          # accepted and ignored (returns 1)
        assert plain.missing_keys() == missing
        out = np.zeros((3, 1, R.WIDTH), dtype=np.float32)
        with pytest.raises(_lib.MldHipError) as ei:
            plain.text_encode(ids, EOS_POS, out)
        assert ei.value.code == ESTATE
        # the tower's keys are required on a clip_layers > 0 handle, the other text_encoder.* keys stay ignored there
        assert sorted(set(towered.missing_keys()) - set(missing)) == sorted(tensors)
        assert towered.load_tensor("text_encoder.text_model.logit_scale", np.zeros(1, np.float32)) is False
        assert towered.load_tensor("text_encoder.text_model.vision_model.post_layernorm.weight", np.zeros(32, np.float32)) is False
        with pytest.raises(_lib.MldHipError) as ei:
            towered.text_encode(ids, EOS_POS, out)                                                        # group not loaded / not finalized
        assert ei.value.code == ESTATE
    finally:
        plain.close()
        towered.close()


def test_hip_text_encoder_class_on_the_simulator(tmp_path):
    """HipMldTextEncoder (tokenizer on the CPU, EOS rule, weight sync into the model's one engine, mldhip_text_encode) against its parent's
    PyTorch path on the same random-init CLIP directory, and through MLD.forward."""
    from mld_hip import config as Cf
    from mld_hip import engine as E
    from mld_hip import synthetic as syn
    from mld_hip.datamodule import HipDataModule
    from mld_hip.mld import MLD
    from mld_hip.text_encoder import HipMldTextEncoder, MldTextEncoder

    d, vocab = R.make_clip_dir(tmp_path, LAYERS)
    enc = HipMldTextEncoder(d)
    assert enc.hip_tower and enc._arch == dict(text_dim=768, clip_layers=LAYERS, clip_heads=12, clip_ff=3072, clip_vocab=len(vocab), clip_ctx=77)
    eng = _lib.Engine(lib=simlib.sim_library(), use_graph=0, max_batch=2, max_frames=16, num_inference_steps=2, num_layers=simlib.SIM_LAYERS,
                      **enc._arch)
    key = E.inject_engine(eng, "inject:hip_clip")
    try:
        cfg = Cf.load_config(overrides={"model.scheduler.num_inference_timesteps": 2, "model.denoiser.params.num_layers": simlib.SIM_LAYERS,
                                        "model.motion_vae.params.num_layers": simlib.SIM_LAYERS})
        model = MLD(cfg, HipDataModule(cfg, engine_key=key), text_encoder=enc, engine_key=key).eval()
        texts, lengths = ["a man walks.", "run!"], [12, 9]
        emb = enc([""] * 2 + texts)
        want = MldTextEncoder.forward(enc, [""] * 2 + texts)
        ids = enc.tokenizer([""] + texts, padding="max_length", truncation=True, max_length=77, return_tensors="pt").input_ids
        assert enc.eos_positions(ids).tolist() == [1, 11, 5]      # BOS + one token per character (no merges) + EOS
        err = float((emb - want).abs().max())
        print(f"HipMldTextEncoder vs MldTextEncoder (torch fp32): {err:.3e}  max|emb| {float(want.abs().max()):.3f}")
        assert tuple(emb.shape) == (4, 1, 768) and torch.equal(emb[0], emb[1]) and err < 1e-4
        lat0 = torch.from_numpy(syn.make_batch(2, lengths).init_latents)
        joints = model({"text": texts, "length": lengths}, init_latents=lat0)
        model.text_encoder = MldTextEncoder(d)
        ref = model({"text": texts, "length": lengths}, init_latents=lat0)
        diff = max(float((a - b).abs().max()) for a, b in zip(joints, ref))
        print(f"MLD.forward joints, HipMldTextEncoder vs MldTextEncoder: {diff:.3e}")
        assert [tuple(j.shape) for j in joints] == [(12, 22, 3), (9, 22, 3)] and diff < 1e-3
    finally:
        E._engines.pop(key, None)
        eng.close()


# ---- every token row, not only EOS rows: prefixes of one id row (tests/test_gpu_text_tower_rows.py is the MI355X counterpart, all 77 rows)
PREFIXES = [1, 2, 16, 17, 32, 33]          # one row (eos_pos = 0), both sides of a 16-key tile edge and of the x3 form's 32-key P V block edge
REGIME_ROWS = [1, 17, 33]


@pytest.fixture(scope="module")
def ids_row():
    return R.make_ids([R.CTX - 1], seed=21)[0]


def rows_of(eng, ids_row, lengths):
    return encode(eng, *R.prefix_call(ids_row, lengths))


def check_rows(out, r64, r32, lengths, factor, what):
    err, e32 = R.row_ratios(out, r64, r32, lengths)
    print(f"{what}: e32 {e32:.3e}  per-row error / e32 {np.round(err / e32, 2).tolist()} at n = {lengths}")
    assert e32 > 0 and np.isfinite(out).all()
    assert (err <= factor * e32).all(), (what, (err / e32).tolist(), factor)


def test_prefix_rows_parity_both_modes(engines, ids_row):
    r64, r32 = R.reference_rows(LAYERS, ids_row)
    out = {prec: rows_of(engines[prec], ids_row, PREFIXES) for prec in (0, 1)}      # six prompts that differ in length alone: not merged by the dedupe
    check_rows(out[0], r64, r32, PREFIXES, R.F32_FACTOR, "prefix rows F32")
    check_rows(out[1], r64, r32, PREFIXES, R.X3_FACTOR, "prefix rows F16X3")
    again = rows_of(engines[1], ids_row, [33, 1, 17])                                 # other order, other company: the same bits
    assert np.array_equal(again, out[1][[PREFIXES.index(n) for n in (33, 1, 17)]])


def test_sharp_softmax_rows_both_modes(ids_row):
    """q_proj / k_proj x 4 (logits x 16): rows whose softmax is nearly one-hot, where the max subtraction and the log2-domain exp have work to do"""
    r64, r32 = R.reference_rows(LAYERS, ids_row, variant="sharp")
    assert np.isfinite(r32).all() and R.attention_shape(LAYERS, ids_row, variant="sharp")[0] > 0.5
    for prec, factor in ((0, R.F32_FACTOR), (1, R.X3_FACTOR)):
        eng = _lib.Engine(lib=simlib.sim_library(), use_graph=0, precision=prec, **R.engine_kwargs(LAYERS, 6))
        try:
            assert R.load_tower(eng, LAYERS, variant="sharp") == []
            check_rows(rows_of(eng, ids_row, REGIME_ROWS), r64, r32, REGIME_ROWS, factor, f"sharp, precision {prec}")
        finally:
            eng.close()


def test_small_weights_fall_back_to_fp32(ids_row):
    """fc1 x 64, fc2 x 1/64 (the small-operand limit of the split-f16 format, clip_tower_ref docstring): left on the split kernels the tower ends
    63 x e32 from fp64 with finite outputs and a silent counter; finalize's probe reads it above MLDHIP_PROBE_TOL, the handle reports the
    fallback and returns the F32 handle's numbers"""
    r64, r32 = R.reference_rows(LAYERS, ids_row, variant="small_w")
    out = {}
    for prec in (0, 1):
        eng = _lib.Engine(lib=simlib.sim_library(), use_graph=0, precision=prec, **R.engine_kwargs(LAYERS, 6))
        try:
            eng.set_option("range_probe", 1)               # (off by default on the simulator)
            assert R.load_tower(eng, LAYERS, variant="small_w") == []
            ns = eng.numeric_status()
            if prec == 1:
                print(f"small_w: probe_err_text {ns['probe_err_text']:.3e}")
                assert ns["probed"] == 1 and ns["text_split_ok"] == 0 and ns["probe_err_text"] > _lib.PROBE_TOL, ns
            else:
                assert ns["probed"] == 0 and ns["text_split_ok"] == 0 and ns["probe_err_text"] == -1.0, ns
            out[prec] = rows_of(eng, ids_row, REGIME_ROWS)
            assert eng.numeric_status()["nonfinite_values"] == 0
        finally:
            eng.close()
    assert np.array_equal(out[1], out[0])
    check_rows(out[1], r64, r32, REGIME_ROWS, R.F32_FACTOR, "small_w, F16X3 handle after the fallback")


def test_numeric_info_accepts_the_abi_7_struct(engines):
    """the two tower fields were appended: a caller that passes the shorter struct gets the fields it knows, any other size is refused"""
    lib = simlib.sim_library()
    info = _lib.NumericInfo()
    short = _lib.NumericInfo.text_split_ok.offset
    C.memset(C.byref(info), 0x55, C.sizeof(info))
    info.struct_size = short
    assert lib.mldhip_numeric_status(engines[1]._h, C.byref(info)) == 0
    assert info.text_split_ok == 0x55555555 and info.loop_split_ok in (0, 1)      # the tail was not written
    info.struct_size = short - 4
    assert lib.mldhip_numeric_status(engines[1]._h, C.byref(info)) == EINVAL
