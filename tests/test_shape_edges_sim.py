"""Frame-length edges of the kernel selection and config 4's de-duplicated CFG layer 0, on the functional simulator (tests/hipemu).

Which attention kernel instance runs depends on the frame count T: key tiles 4 / 7 / 13 / 18 at T <= 64 / 112 / 208 / 288 (pick_nkt,
engine/path_latent.hpp), the key-blocked forms only for T <= 256, 32-key blocks in the key-blocked kernels, 16-row query tiles.  These
tests walk T across the tile edges the simulator can afford (T <= 65, one row at 209) in every attention form of both precisions, and
run config 4's sampling loop at odd batches, where layer 0 of the de-duplicated CFG batch ("cross_fold") holds an odd number of samples.
The reference is the float64 oracle throughout.  Every output buffer starts NaN-filled: a frame the kernels never write fails the
finiteness check, a padded frame must be exactly zero.  The full-length sweep (T up to 288) is tests/test_gpu_shape_edges.py.
"""
import numpy as np
import pytest

import simlib
from mld_hip import synthetic as syn
from oracle import mld_oracle as O

SIM_T = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65]
# (precision, flash_attn): F32 (flash_attn does not apply: one attention form), split-f16 whole-K/V forms, split-f16 key-blocked forms
MODES = [(0, 1), (1, 0), (1, 2)]
NOVAE_LAYERS = 2


def _ragged(T):
    """the shorter motion of a batch padded to T (not a multiple of 16 wherever T allows)"""
    return max(1, T * 5 // 8)


@pytest.fixture(scope="module")
def f64():
    ops = O.NumpyOps(np.float64)
    _, sdv = simlib.text_weights()
    sdn = syn.make_novae_denoiser_state_dict(dims=syn.ModelDims(latent_dim=512, num_layers=NOVAE_LAYERS))
    return ops, O.to_backend(ops, sdv), O.to_backend(ops, sdn)


@pytest.fixture(scope="module")
def dec_engines():
    engs = {}
    for prec, fl in MODES:
        e = simlib.sim_engine(max_batch=2, max_frames=288, precision=prec)
        e.set_option("flash_attn", fl)
        engs[prec, fl] = e
    yield engs
    for e in engs.values():
        e.close()


@pytest.fixture(scope="module")
def novae_engines():
    engs = {}
    for prec, fl in MODES:
        e = simlib.sim_novae_engine(num_layers=NOVAE_LAYERS, max_batch=2, max_frames=65, num_inference_steps=4, precision=prec)
        e.set_option("flash_attn", fl)
        engs[prec, fl] = e
    yield engs
    for e in engs.values():
        e.close()


def _decode_check(e, bv, ops, T, tag):
    lens = [T, _ragged(T)]
    z = syn._rng(21, f"edge{T}").standard_normal((2, 1, 256)).astype(np.float32)
    feats = np.full((2, T, 263), np.nan, np.float32)
    e.vae_decode(z, lens, feats)
    ref = O.vae_decode(ops, bv, z.astype(np.float64), lens)
    assert np.isfinite(feats).all(), tag
    err = float(np.abs(feats - ref).max())
    assert err < 5e-5, (tag, err)                                   # measured <= 3.6e-6 (T <= 65 and T = 209, every mode)
    assert np.all(feats[1, lens[1]:] == 0), tag


@pytest.mark.parametrize("mode", MODES, ids=["f32", "x3_wholekv", "x3_keyblocked"])
def test_vae_decode_frame_length_edges_sim(dec_engines, f64, mode):
    """Decoder self-attention at every T of SIM_T: attn_decode_kernel<4> / <7> (F32; T = 65 is the first 7-tile instance),
    attn_decode_x3_kernel<4> / <7> (flash_attn 0) and attn_flash_x3_kernel (flash_attn 2) -- query / key tiles that are empty (T = 1),
    partial (15, 17, 31, 33, 63, 65), exactly full (16, 32, 64), and a ragged second motion whose keys stop inside a tile."""
    ops, bv, _ = f64
    for T in SIM_T:
        _decode_check(dec_engines[mode], bv, ops, T, (mode, T))


def test_vae_decode_18_key_tiles_sim(dec_engines, f64):
    """T = 209: one frame past pick_nkt's 13-tile bound -- attn_decode_x3_kernel<18> (split-f16, whole-K/V form)."""
    ops, bv, _ = f64
    _decode_check(dec_engines[1, 0], bv, ops, 209, "T=209")


@pytest.mark.parametrize("mode", MODES, ids=["f32", "x3_wholekv", "x3_keyblocked"])
def test_novae_denoiser_frame_length_edges_sim(novae_engines, f64, mode):
    """trans_dec denoiser (no key mask: every one of the T frames is a key) at every T of SIM_T: attn_seq_kernel<4> / <7> (F32),
    attn_seq_x3_kernel<4, 128> / <7, 128> (flash_attn 0), attn_flash128_x3_kernel (flash_attn 2: T = 15 .. 65 end inside, or exactly at,
    a 32-key block).  R = 3: a full-length row, a ragged row and a row of length 0 (all zeros).  The T alternate between t = 999 with the
    folded cross-attention ("cross_fold") on and t = 0 with it off (the simulator's time budget: one call per T)."""
    ops, _, bd = f64
    e = novae_engines[mode]
    for k, T in enumerate(SIM_T):
        g = syn._rng(22, f"nv{T}")
        x = g.standard_normal((3, T, 263)).astype(np.float32)
        te = g.standard_normal((3, 1, 768)).astype(np.float32)
        lens = [T, _ragged(T), 0]
        t, fold = (999, 1) if k % 2 == 0 else (0, 0)
        e.set_option("cross_fold", fold)
        out = np.full((3, T, 263), np.nan, np.float32)
        e.denoiser_forward_novae(x, t, te, lens, T, out)
        ref = O.denoiser_forward_novae(ops, bd, x.astype(np.float64), t, te.astype(np.float64), lens)
        assert np.isfinite(out).all(), (mode, T, t)
        err = float(np.abs(out - ref).max())
        assert err < 5e-5, (mode, T, t, err)                   # measured <= 4.6e-6
        assert np.all(out[1, lens[1]:] == 0) and np.all(out[2] == 0), (mode, T, t)
    e.set_option("cross_fold", 1)


@pytest.mark.parametrize("B", [1, 3])
def test_novae_sample_dedup_odd_batches_sim(f64, B):
    """sample_novae in split-f16 (4 DDPM steps, in-kernel Philox noise) at odd B: with "cross_fold" on, layer 0 of the CFG batch runs on
    R0 = B samples -- attn_flash128_x3_kernel forced at 1 / 3 samples, cross2_fold_ln_kernel reading sample s's rows through
    src_mod = R0 -- and with it off, the five-launch form on all 2B rows.  Both against the oracle on the regenerated Philox stream."""
    ops, _, bd = f64
    T = 17
    lens = [17, 9, 1][:B]
    g = syn._rng(23, f"nvs{B}")
    lat0 = g.standard_normal((B, T, 263)).astype(np.float32)
    te = g.standard_normal((2 * B, 1, 768)).astype(np.float32)
    seed = 0x5EED0000 + B
    noise = np.stack([O.philox_normal(lat0.size, seed, s).reshape(B, T, 263) for s in range(4)]).astype(np.float64)
    fr = O.sample_novae(ops, bd, te.astype(np.float64), lat0.astype(np.float64), lens, noise, steps=4)
    outs = {}
    for fold in (1, 0):
        e = simlib.sim_novae_engine(num_layers=NOVAE_LAYERS, max_batch=3, max_frames=T, num_inference_steps=4, precision=1)
        e.set_option("cross_fold", fold)
        feats = np.full((B, T, 263), np.nan, np.float32)
        e.sample_novae(te, lat0, lens, None, seed, feats, None)
        e.close()
        assert np.isfinite(feats).all(), fold
        outs[fold] = float(np.abs(feats - fr).max())
    print("sim sample_novae B=%d split-f16: err vs f64 cross_fold 1 %.2e, cross_fold 0 %.2e (max|feats| %.1f)"
          % (B, outs[1], outs[0], float(np.abs(fr).max())))
    assert outs[1] < 2e-4 and outs[0] < 2e-4, outs                 # measured <= 6e-5 (|feats| ~ 30)
