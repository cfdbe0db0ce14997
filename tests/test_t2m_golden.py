"""tests/t2m_ref.py (the project's own restatement of the T2M evaluator towers) in float32 against tests/golden/t2m_eval_b4.npz, which
tools/make_golden_t2m.py wrote from the reference's own MovementConvEncoder / MotionEncoderBiGRUCo / TextEncoderBiGRUCo on the same seeded weights, run as
MLD.t2m_eval runs them (renorm on every frame, sorted by length, lengths // 4): holds the restatement to the real reference, padded-frame rule included.

Bound: both sides are float32 torch on the CPU computing the same formulas (the restatement differs in the order of rows inside the packed batch only), so
they agree to a few float32 roundings of O(1) embeddings: 1e-5 absolute (measured: 0, the same kernels run on the same numbers) -- far below any structural mistake, which shows in the first digits."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import t2m_ref as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "t2m_eval_b4.npz")
TOL = 1e-5


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def fp32_motion(feats, lens, nfeats):
    _, m32 = R.models(nfeats)
    with torch.no_grad():
        return m32.motion_embed(torch.from_numpy(feats), lens, R.stats(nfeats)).numpy()


def test_motion_tower_restatement_matches_the_reference(golden):
    lens = [int(n) for n in golden["lengths"]]
    assert lens == [40, 37, 22, 5] and golden["feats"].shape == (4, 40, 263)
    out = fp32_motion(golden["feats"], lens, 263)
    err = float(np.abs(out - golden["motion_emb"]).max())
    print("motion tower restatement vs reference:", err)
    assert err <= TOL


def test_padded_frames_carry_the_renorm_constant(golden):
    """the fixture's values hold only if the frames at t >= len go through the renorm like every other frame: zeroing them behind it must miss the reference"""
    lens = [int(n) for n in golden["lengths"]]
    mean, std, mean_eval, std_eval = R.stats(263)
    g = ((golden["feats"] * std + mean - mean_eval) / std_eval).astype(np.float32)
    for b, n in enumerate(lens):
        g[b, n:] = 0.0
    _, m32 = R.models(263)
    with torch.no_grad():
        wrong = m32.motion_embed(torch.from_numpy(g), lens, None).numpy()
    diff = np.abs(wrong - golden["motion_emb"]).max(axis=1)
    assert diff[0] <= TOL                        # length 40 = T: no padded frame
    assert (diff[1:] > 100 * TOL).all(), diff    # 37, 22, 5: the last valid steps read padded frames


def test_kit_width_restatement_matches_the_reference(golden):
    lens = [int(n) for n in golden["kit_lengths"]]
    assert golden["kit_feats"].shape == (2, 24, 251)
    err = float(np.abs(fp32_motion(golden["kit_feats"], lens, 251) - golden["kit_motion_emb"]).max())
    print("motion tower restatement vs reference (251 features):", err)
    assert err <= TOL


def test_text_tower_restatement_matches_the_reference(golden):
    lens = [int(n) for n in golden["text_lengths"]]
    assert lens == [8, 3, 1]
    _, m32 = R.models()
    with torch.no_grad():
        out = m32.text_embed(torch.from_numpy(golden["word_embs"]), torch.from_numpy(golden["pos_ohot"]), lens).numpy()
        rev = m32.text_embed(torch.from_numpy(golden["word_embs"][::-1].copy()), torch.from_numpy(golden["pos_ohot"][::-1].copy()), lens[::-1]).numpy()
    err = float(np.abs(out - golden["text_emb"]).max())
    print("text tower restatement vs reference:", err)
    assert err <= TOL
    assert float(np.abs(rev[::-1] - golden["text_emb"]).max()) <= TOL      # any order in, the caller's order out
