"""The T2M evaluator towers of the engine (mldhip_t2m_motion_embed / mldhip_t2m_text_embed) on the functional simulator, both arithmetic modes, at the
real widths and few steps (B = 3, T = 16, lengths 16 / 9 / 4; captions B = 3, L = 4, lengths 4 / 2 / 1), against the project's float64 restatement
(tests/t2m_ref.py has the reference and the tolerance rule), plus the padded-frame rule, batch independence, the guards and the ABI checks that need no
device, and the towers' stage of the range contract."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import simlib  # noqa: E402
import t2m_ref as R  # noqa: E402
from mld_hip import _lib  # noqa: E402

EINVAL, ESTATE = -1, -3
LENS, T = [16, 9, 4], 16
TEXT_LENS, L = [4, 2, 1], 4
MAX_FRAMES = 24


def sim_engine(prec, groups=("motion", "text"), finalize=True, **extra):
    eng = _lib.Engine(lib=simlib.sim_library(), use_graph=0, precision=prec, **R.engine_kwargs(4, max_frames=MAX_FRAMES, max_words=6, **extra))
    assert R.load_evaluators(eng, groups=groups, finalize=finalize) == []
    return eng


@pytest.fixture(scope="module")
def engines():
    out = {prec: sim_engine(prec) for prec in (0, 1)}
    yield out
    for eng in out.values():
        eng.close()


def motion(eng, feats, lens, renorm=True, T_=None):
    out = np.full((len(lens), 512), np.nan, dtype=np.float32)
    eng.t2m_motion_embed(np.ascontiguousarray(feats), lens, feats.shape[1] if T_ is None else T_, out, renorm=renorm)
    return out


def text(eng, w, p, lens):
    out = np.full((len(lens), 512), np.nan, dtype=np.float32)
    eng.t2m_text_embed(np.ascontiguousarray(w), np.ascontiguousarray(p), lens, w.shape[1], out)
    return out


@pytest.fixture(scope="module")
def feats():
    return R.make_motions(LENS, T)


@pytest.fixture(scope="module")
def captions():
    return R.make_captions(TEXT_LENS, L)


@pytest.fixture(scope="module")
def motion_out(engines, feats):
    return {prec: motion(eng, feats, LENS) for prec, eng in engines.items()}


def check(out, r64, e32, prec, what):
    err = float(np.abs(out.astype(np.float64) - r64).max())
    print(f"{what}: mode {prec}  err {err:.3e}  e32 {e32:.3e}  ratio {err / e32:.2f}  max|ref| {np.abs(r64).max():.3f}")
    assert e32 > 0 and np.isfinite(out).all()
    assert err <= (R.F32_FACTOR if prec == 0 else R.X3_FACTOR) * e32, (what, prec, err, e32)


def test_motion_tower_parity_with_fp64_both_modes(motion_out, feats):
    r64, e32 = R.reference_motion(feats, LENS)
    for prec, out in motion_out.items():
        check(out, r64, e32, prec, "motion tower (simulator)")


def test_text_tower_parity_with_fp64_both_modes(engines, captions):
    r64, e32 = R.reference_text(*captions, TEXT_LENS)
    for prec, eng in engines.items():
        check(text(eng, *captions, TEXT_LENS), r64, e32, prec, "text tower (simulator)")
    assert engines[1].numeric_status()["nonfinite_values"] == 0


def test_a_motion_is_bit_identical_alone_and_in_any_order(engines, feats, motion_out, captions):
    for prec, eng in engines.items():
        for b in range(3):
            assert np.array_equal(motion(eng, feats[b:b + 1], LENS[b:b + 1])[0], motion_out[prec][b])
        rev = motion(eng, feats[::-1], LENS[::-1])
        assert np.array_equal(rev[::-1], motion_out[prec])                     # any order of lengths, rows in the caller's order
        full = text(eng, *captions, TEXT_LENS)
        assert np.array_equal(text(eng, captions[0][1:2], captions[1][1:2], TEXT_LENS[1:2])[0], full[1])


def test_embedding_depends_on_T_as_in_the_reference(engines, feats):
    """The padded-frame rule: frames at t >= len hold a non-zero constant behind the renorm and the convolutions of the last valid steps read them, so the
    embedding of a motion depends on T up to len + 6 and not beyond.  len = 9 (m_len 2; output step 1 of the second convolution reads first-convolution steps
    1 .. 4, i.e. frames 1 .. 10): T = 9 differs from T = 16; T = 16, 20 and 24 (all >= len + 7) agree."""
    eng = engines[0]
    one = feats[1:2]                                                           # length 9
    outs, refs = {}, {}
    for t in (9, 16, 20, 24):
        f = np.zeros((1, t, feats.shape[2]), np.float32)
        f[:, :min(t, T)] = one[:, :t]
        outs[t] = motion(eng, f, [9])
        refs[t], e32 = R.reference_motion(f, [9])
        check(outs[t], refs[t], e32, 0, f"T = {t}")
    assert np.array_equal(outs[16], outs[20]) and np.array_equal(outs[16], outs[24])
    assert np.abs(refs[16] - refs[24]).max() < 1e-12
    gap = float(np.abs(refs[9] - refs[16]).max())
    assert gap > 1e-3, gap                                                     # the reference's own dependence on T ...
    assert abs(float(np.abs(outs[9].astype(np.float64) - outs[16]).max()) - gap) < 1e-4      # ... and the engine follows it


def test_nothing_is_read_beyond_T_or_beyond_the_call(engines, feats, motion_out):
    """Rows behind the call's last frame are never read (the convolution pads with true zeros there): the same call from a buffer with NaN behind it."""
    big = np.full(feats.size + 4096, np.nan, dtype=np.float32)
    big[:feats.size] = feats.ravel()
    for prec, eng in engines.items():
        out = np.full((3, 512), np.nan, dtype=np.float32)
        eng.t2m_motion_embed(big, LENS, T, out)
        assert np.array_equal(out, motion_out[prec])


def test_renorm_switch(engines, feats, motion_out):
    """renorm = 0 on rows that already are in the evaluators' normalisation against renorm = 1 on the model's rows"""
    mean, std, mean_eval, std_eval = R.stats()
    pre = ((feats * std + mean - mean_eval) / std_eval).astype(np.float32)
    r64, e32 = R.reference_motion(feats, LENS)
    for prec, eng in engines.items():
        out = motion(eng, pre, LENS, renorm=False)
        check(out, r64, e32, prec, "renorm = 0")
        assert float(np.abs(out - motion_out[prec]).max()) <= 2 * R.X3_FACTOR * e32
        assert not np.array_equal(motion(eng, feats, LENS, renorm=False), motion_out[prec])


def test_guards(engines, feats, captions):
    eng = engines[0]
    out = np.zeros((4, 512), np.float32)
    w, p = captions

    def code(fn):
        with pytest.raises(_lib.MldHipError) as ei:
            fn()
        return ei.value.code

    assert code(lambda: eng.t2m_motion_embed(feats, [16, 9, 4, 4, 4], T, out)) == EINVAL          # B > t2m_max_motions
    assert code(lambda: eng.t2m_motion_embed(feats, [], T, out)) == EINVAL                        # B = 0
    assert code(lambda: eng.t2m_motion_embed(feats, LENS, MAX_FRAMES + 1, out)) == EINVAL         # T > max_frames
    assert code(lambda: eng.t2m_motion_embed(feats, [16, 9, 3], T, out)) == EINVAL                # len < 4: m_len 0
    assert code(lambda: eng.t2m_motion_embed(feats, [17, 9, 4], T, out)) == EINVAL                # len > T
    assert code(lambda: eng.t2m_motion_embed(None, LENS, T, out)) == EINVAL
    assert code(lambda: eng.t2m_motion_embed(feats, LENS, T, None)) == EINVAL
    assert code(lambda: eng.t2m_text_embed(w, p, [4, 2, 0], L, out)) == EINVAL                    # text length outside 1 .. L
    assert code(lambda: eng.t2m_text_embed(w, p, [5, 2, 1], L, out)) == EINVAL
    assert code(lambda: eng.t2m_text_embed(w, p, TEXT_LENS, 7, out)) == EINVAL                    # L > t2m_max_words
    assert code(lambda: eng.t2m_text_embed(w, p, [1] * 5, L, out)) == EINVAL
    assert code(lambda: eng.t2m_text_embed(None, p, TEXT_LENS, L, out)) == EINVAL
    assert code(lambda: eng.t2m_text_embed(w, None, TEXT_LENS, L, out)) == EINVAL


def test_states(feats, captions):
    out = np.zeros((3, 512), np.float32)

    def code(fn):
        with pytest.raises(_lib.MldHipError) as ei:
            fn()
        return ei.value.code

    plain = _lib.Engine(lib=simlib.sim_library(), use_graph=0, num_layers=3, max_batch=2, max_frames=16)      # no evaluators on the handle
    assert code(lambda: plain.t2m_motion_embed(feats, LENS, T, out)) == ESTATE
    assert code(lambda: plain.t2m_text_embed(*captions, TEXT_LENS, L, out)) == ESTATE
    plain.close()
    eng = sim_engine(0, groups=("motion",), finalize=False)
    assert code(lambda: eng.t2m_motion_embed(feats, LENS, T, out)) == ESTATE   # not finalized
    eng.finalize()
    assert code(lambda: eng.t2m_text_embed(*captions, TEXT_LENS, L, out)) == ESTATE   # the text group is absent
    eng.t2m_motion_embed(feats, LENS, T, out)
    eng.close()
    with pytest.raises(_lib.MldHipError) as ei:
        _lib.Engine(lib=simlib.sim_library(), precision=2, **R.engine_kwargs(4))
    assert ei.value.code == EINVAL                                             # MLDHIP_PREC_BF16 with t2m_eval = 1 is refused at create


def test_half_loaded_group_and_wrong_shapes():
    eng = _lib.Engine(lib=simlib.sim_library(), use_graph=0, **R.engine_kwargs(4))
    w = R.weights()
    with pytest.raises(_lib.MldHipError) as ei:
        eng.load_tensor("t2m_moveencoder.main.0.weight", np.zeros((3, 3), np.float32))
    assert ei.value.code == EINVAL
    assert eng.load_tensor("t2m_textencoder.hidden", w["t2m_textencoder.hidden"])
    missing = eng.missing_keys()
    assert "t2m_textencoder.gru.weight_hh_l0_reverse" in missing and "mean_eval" in missing
    with pytest.raises(_lib.MldHipError):
        eng.finalize()                                                         # a half-loaded group
    eng.close()
    off = _lib.Engine(lib=simlib.sim_library(), use_graph=0, num_layers=3, max_batch=2, max_frames=16)
    assert off.load_tensor("t2m_moveencoder.main.0.weight", np.zeros((3, 3), np.float32)) is False      # t2m_eval = 0: ignored, mis-shaped or not
    assert not any(k.startswith("t2m_") or k.endswith("_eval") for k in off.missing_keys())
    off.close()


def test_abi_and_config_defaults():
    lib = simlib.sim_library()
    assert lib.mldhip_abi_version() == 8 == _lib.ABI_VERSION
    assert {"mldhip_t2m_motion_embed", "mldhip_t2m_text_embed"} <= set(_lib.exported_symbols())
    assert hasattr(lib, "mldhip_t2m_motion_embed") and hasattr(lib, "mldhip_t2m_text_embed")
    cfg = _lib.Config()
    lib.mldhip_default_config(C.byref(cfg))
    assert cfg.struct_size == C.sizeof(_lib.Config)
    assert (cfg.t2m_eval, cfg.t2m_max_motions, cfg.t2m_max_words) == (0, 0, 0)
    eng = _lib.Engine(lib=lib, use_graph=0, num_layers=3, max_batch=3, max_frames=16, t2m_eval=1)
    out = np.zeros((7, 512), np.float32)
    with pytest.raises(_lib.MldHipError) as ei:                                # capacity defaults: 2 x max_batch motions (checked behind the state checks: load first)
        eng.t2m_motion_embed(np.zeros((7, 16, 263), np.float32), [16] * 7, 16, out)
    assert ei.value.code == ESTATE
    eng.close()
    # a caller built before the t2m_* fields passes the struct that ends behind clip_max_prompts: accepted, no evaluators
    cfg.struct_size = _lib.Config.t2m_eval.offset
    cfg.num_layers, cfg.max_batch, cfg.max_frames, cfg.t2m_eval = 3, 2, 16, 1
    h = C.c_void_p()
    assert lib.mldhip_create(C.byref(cfg), 0, C.byref(h)) == 0
    assert lib.mldhip_load_tensor(h, b"t2m_textencoder.hidden", np.zeros(4, np.float32).ctypes.data, (C.c_int64 * 1)(4), 1, 0, 0) == 1      # ignored
    info = _lib.NumericInfo()
    info.struct_size = _lib.NumericInfo.eval_split_ok.offset                   # ... and the numeric info that ends behind probe_err_text
    info.eval_split_ok = 77
    assert lib.mldhip_numeric_status(h, C.byref(info)) == 0 and info.eval_split_ok == 77
    lib.mldhip_destroy(h)


def scaled_engine(prec, scale):
    """engine with the probe on and the evaluator weights of t2m_ref with scale(key, value) applied"""
    e = _lib.Engine(lib=simlib.sim_library(), use_graph=0, precision=prec, **R.engine_kwargs(4, max_frames=MAX_FRAMES, max_words=6))
    for k, v in R.weights().items():
        assert e.load_tensor(k, scale(k, v))
    for k, v in zip(("mean", "std", "mean_eval", "std_eval"), R.stats()):
        e.load_tensor(k, v)
    e.set_option("range_probe", 1)
    e.finalize()
    return e


def test_probe_keeps_plain_weights_on_the_split_kernels(feats, motion_out):
    eng = scaled_engine(1, lambda k, v: v)
    ns = eng.numeric_status()
    print("probe (plain weights):", ns["probe_err_eval"])
    assert ns["probed"] == 1 and ns["eval_split_ok"] == 1 and 0 <= ns["probe_err_eval"] <= _lib.PROBE_TOL
    assert np.array_equal(motion(eng, feats, LENS), motion_out[1])             # the probe leaves nothing behind: the same rows as the unprobed handle
    eng.close()


def test_probe_falls_back_on_small_head_weights_and_then_equals_f32(feats, captions):
    """output_net.3 (weight and bias) x 2^-12 in both towers: the weights sit at 1e-5, where both halves of the split are half subnormals (absolute error 3e-8, i.e.
    ~1e-3 relative), and the embeddings ARE this layer's output, so the stage reads far above MLDHIP_PROBE_TOL, falls back, and the handle equals the F32 one to the bit."""
    scale = lambda k, v: v * np.float32(2.0 ** -12) if ".output_net.3." in k else v
    outs = {}
    for prec in (0, 1):
        e = scaled_engine(prec, scale)
        if prec == 1:
            ns = e.numeric_status()
            print("probe (output_net.3 x 2^-12):", ns["probe_err_eval"])
            assert ns["eval_split_ok"] == 0 and ns["probe_err_eval"] > _lib.PROBE_TOL
        outs[prec] = (motion(e, feats, LENS), text(e, *captions, TEXT_LENS))
        e.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


def test_probe_w_hh_scaled_down_falls_back_and_then_equals_f32(feats, captions):
    """W_hh x 2^-12 (recurrent weights near 1e-5: both halves of the split are half subnormals, ~4e-3 relative on the product h . W_hh^T).  With the input-side gate
    terms of the probe's unit-normal rows at O(1) the embeddings alone do not see it (they move by ~1e-7: 2.12e-6 against 2.16e-6 for the plain weights); the probe's
    reading of the recurrent products themselves does: the stage falls back, and the handle then equals the F32 handle to the bit."""
    scale = lambda k, v: v * np.float32(2.0 ** -12) if "weight_hh" in k else v
    outs = {}
    for prec in (0, 1):
        e = scaled_engine(prec, scale)
        if prec == 1:
            ns = e.numeric_status()
            print("probe (W_hh x 2^-12):", ns["probe_err_eval"])
            assert ns["eval_split_ok"] == 0 and ns["probe_err_eval"] > _lib.PROBE_TOL
        outs[prec] = (motion(e, feats, LENS), text(e, *captions, TEXT_LENS))
        e.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
