"""Pin the CPU oracle at KIT-ML's width to vectors from the reference's own MldVae(nfeats=251) and recover_from_ric(., 21)
(tests/golden/kit_ops_b3.npz, written by tools/make_golden_kit.py) -- at the tolerances tests/test_oracle_golden.py has for the 263-wide twins.
The reference runs in float32 only."""
import os

import numpy as np
import pytest

from mld_hip import synthetic as syn
from oracle import mld_oracle as O

NFEATS, NJOINTS = 251, 21


@pytest.fixture(scope="module")
def kit(golden_dir):
    ops = O.NumpyOps(np.float32)
    g = np.load(os.path.join(golden_dir, "kit_ops_b3.npz"))
    return ops, O.to_backend(ops, syn.make_vae_state_dict(dims=syn.ModelDims(nfeats=NFEATS))), g


def test_kit_fixture_is_small_and_pinned(golden_dir, kit):
    _, _, g = kit
    assert os.path.getsize(os.path.join(golden_dir, "kit_ops_b3.npz")) <= os.path.getsize(os.path.join(golden_dir, "vae_decode_b3.npz"))
    assert float(g["oracle_diff_feats"]) < 2e-5 and float(g["oracle_diff_joints"]) < 1e-5
    assert float(g["oracle_diff_mu"]) < 2e-5 and float(g["oracle_diff_std"]) < 2e-5


def test_kit_vae_decode_and_joints_match_reference(kit):
    ops, bv, g = kit
    lengths = [int(x) for x in g["dec_lengths"]]
    feats = O.vae_decode(ops, bv, g["z"], lengths)
    assert feats.shape == (3, max(lengths), NFEATS)
    assert np.abs(feats - g["feats"]).max() < 2e-5
    assert (feats[1, lengths[1]:] == 0).all() and (g["feats"][1, lengths[1]:] == 0).all()      # padded frames zeroed (mld_vae.py:245)
    mean, std = syn.make_mean_std(NFEATS)
    joints = O.feats2joints(ops, g["feats"], mean, std, njoints=NJOINTS)
    assert joints.shape == (3, max(lengths), NJOINTS, 3) == g["joints"].shape
    assert np.abs(joints - g["joints"]).max() < 1e-5


def test_kit_vae_encode_matches_reference(kit):
    ops, bv, g = kit
    _, mu, lv = O.vae_encode(ops, bv, g["enc_feats"], g["enc_lengths"].tolist())
    assert np.abs(mu - g["mu"]).max() < 2e-5 and np.abs(np.sqrt(np.exp(lv)) - g["std"]).max() < 2e-5
