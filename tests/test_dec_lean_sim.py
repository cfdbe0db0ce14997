""""dec_lean" on the functional simulator (no GPU): the decoder that skips what the joints never read against the full one, to the bit.

Shape: the smallest that reaches the fused layer tail and the final strip -- B = 5, T = 52 (48-row strips straddle sample boundaries, T is
no multiple of 16), lengths [52, 37, 52, 37, 20]: samples 2 and 3 are not their own representatives, the representative of 3 is not
sample 0, sample 4 is alone.  One sample() per setting is shared by the tests below."""
import numpy as np
import pytest

import simlib
from mld_hip import synthetic as syn

B, T, LENS = 5, 52, [52, 37, 52, 37, 20]


def _engine():
    e = simlib.sim_engine(max_batch=B, max_frames=T, num_inference_steps=2, precision=1)
    e.set_option("gemm_small_m", 0)          # the row-strip kernels at simulator-sized M
    e.set_option("ffn_strip", 3)             # 48-row strips: the fused tail
    e.set_option("flash_attn", 2)            # key-blocked attention
    return e


def _sample(e, batch, want_feats):
    lat = np.full((B, 1, 256), np.nan, np.float32)
    feats = np.full((B, T, 263), np.nan, np.float32) if want_feats else None
    joints = np.full((B, T, 22, 3), np.nan, np.float32)
    e.sample(batch.text_emb, batch.init_latents, LENS, lat, feats, joints)
    return lat, feats, joints, list(e.launch_counts()), e.numeric_status()["nonfinite_values"]


@pytest.fixture(scope="module")
def runs():
    e = _engine()
    batch = syn.make_batch(B, LENS)
    bad = syn.make_batch(B, LENS)
    bad.init_latents = np.array(bad.init_latents, np.float32, copy=True)
    bad.init_latents[1] = np.nan             # an input NaN (not a fault): sample 1's latents are NaN
    out = {}
    for lean in (0, 1):
        e.set_option("dec_lean", lean)
        out[lean] = {"joints": _sample(e, batch, False), "feats": _sample(e, batch, True), "nan": _sample(e, bad, False)}
    # ... and a NaN that does reach the joints (the split operands clamp a NaN latent away): mean[3], the root height of every frame
    mean, _ = syn.make_mean_std()
    mean = np.array(mean, np.float32, copy=True)
    mean[3] = np.nan
    e.load_tensor("mean", mean)
    e.finalize()
    for lean in (0, 1):
        e.set_option("dec_lean", lean)
        out[lean]["nan_mean"] = _sample(e, batch, False)
    e.close()
    return out


def test_joints_only_call_is_bit_identical_and_finite(runs):
    (l0, _, j0, _, n0), (l1, _, j1, _, n1) = runs[0]["joints"], runs[1]["joints"]
    assert np.array_equal(l0, l1) and np.isfinite(l1).all()
    assert np.isfinite(j1).all() and np.array_equal(j0, j1)
    assert n0 == 0 and n1 == 0


def test_padded_frames_are_unchanged(runs):
    """padded frames decode to zero features (mld_vae.py:245), so their joints are what feats2joints makes of zeros: the root keeps
    integrating mean velocities, every frame past the length equals its neighbour up to that drift -- the same values in both settings,
    and the same as the call that also returns the (zeroed) features"""
    j0, j1, jf = runs[0]["joints"][2], runs[1]["joints"][2], runs[1]["feats"][2]
    for i, n in enumerate(LENS):
        assert np.array_equal(j0[i, n:], j1[i, n:]) and np.array_equal(jf[i, n:], j1[i, n:])
        if n + 1 < T:                        # zero features: joint positions relative to the root do not depend on the frame
            rel = j1[i, n:, 1:, 1]
            assert np.all(rel == rel[0])


def test_launches(runs):
    """decode phase: init_queries is gone and the one-block representative map took its place (the counting pass that went with the
    joints was never part of launch_counts); every other launch is one for one -- the joints-only final stage replaces the full one"""
    c0, c1 = runs[0]["joints"][3], runs[1]["joints"][3]
    print("launch counts dec_lean 0 / 1:", c0, c1)
    assert c1[0] == c0[0] and c1[2] == c0[2] == 1
    assert c1[1] == c0[1]                    # - init_queries + length_reps


def test_call_that_asks_for_features_keeps_all_263_columns(runs):
    (_, f0, j0, _, _), (_, f1, j1, _, _) = runs[0]["feats"], runs[1]["feats"]
    assert np.isfinite(f1).all() and np.array_equal(f0, f1) and np.array_equal(j0, j1)
    assert np.array_equal(j1, runs[1]["joints"][2])                  # and the joints of the joints-only call are the same bits
    for i, n in enumerate(LENS):
        assert np.all(f1[i, n:] == 0)
        assert np.all(np.abs(f1[i, :n]).max(axis=0) > 0)            # every one of the 263 columns is filled


def test_nonfinite_counter_is_what_it_was(runs):
    """the counter of mldhip_numeric_status: the latents behind the loop + the joints, whether a pass of its own or the joints kernel counts them"""
    (l0, _, j0, _, n0), (l1, _, j1, _, n1) = runs[0]["nan"], runs[1]["nan"]
    assert np.isnan(l1[1]).all() and np.array_equal(l0, l1, equal_nan=True) and np.array_equal(j0, j1, equal_nan=True)
    print("NaN latent: counter", n0, n1, "non-finite joints", int((~np.isfinite(j1)).sum()))
    assert n0 == n1 == 256 + int((~np.isfinite(j1)).sum())
    (_, _, j0, _, n0), (_, _, j1, _, n1) = runs[0]["nan_mean"], runs[1]["nan_mean"]
    assert np.array_equal(j0, j1, equal_nan=True) and np.isnan(j1[:, :, 0, 1]).all()
    print("NaN mean[3]: counter", n0, n1)
    assert n0 == n1 == int((~np.isfinite(j1)).sum()) == B * T        # one value per frame, padded frames included
