"""tests/t2m_metrics_ref.py's float64 restatement of the three metric calls reproduces what the REFERENCE's own helpers recorded (tests/golden/t2m_metrics.npz,
written by tools/make_golden_t2m_metrics.py from mld/models/metrics/utils.py on the seeded embeddings of the recorded run): distances and statistics within
1e-5 absolute (tests/test_t2m_golden.py's bound: the recorded values are the reference's float32 / float64 results), ranks exactly."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import t2m_metrics_ref as R  # noqa: E402

ATOL = 1e-5


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "t2m_metrics.npz"))


@pytest.fixture(scope="module")
def sets(gold):
    """the three gathered sets of the recorded run: (texts, generated, ground truth) [120, 512] float32 in the recorded shuffle"""
    ups = R.golden_updates()
    idx = torch.from_numpy(gold["shuffle_idx"])
    return tuple(torch.cat([torch.flatten(u[k], start_dim=1) for u in ups])[idx].numpy() for k in range(3))


@pytest.mark.parametrize("which", ["gen", "gt"])
def test_distances_and_ranks(gold, sets, which):
    G = R.GOLD
    texts, motions = sets[0], sets[1 if which == "gen" else 2]
    d64 = R.dist_matrices(texts, motions, G["R"])
    assert d64.shape == gold[f"dist_{which}"].shape
    assert float(np.abs(d64.numpy() - gold[f"dist_{which}"]).max()) <= ATOL
    # the reference's argsort + calculate_top_k against the restatement's rank: top-k hit = rank < k (no ties on these inputs: every row counts)
    ref = R.match_reference(texts, motions, G["R"])
    assert ref["counts"].all()
    rank = ref["rank64"]
    assert np.array_equal(np.asarray([(rank <= k).sum() for k in range(G["top_k"])], np.float32), gold[f"topk_{which}"])
    assert abs(float(ref["diag64"].sum()) - float(gold[f"match_{which}"])) <= ATOL * len(rank) + 4e-4      # (+ the float32 accumulation of the recorded trace sum: 96 terms of ~30, 2 ulp of 2 900)


@pytest.mark.parametrize("which", ["gen", "gt"])
def test_statistics(gold, sets, which):
    x = sets[1 if which == "gen" else 2]
    mean, cov = (v.numpy() for v in R.stats(x))
    s = R.GOLD_COV_STEP
    assert float(np.abs(mean - gold[f"mu_{which}"]).max()) <= ATOL
    assert float(np.abs(cov[::s, ::s] - gold[f"cov_{which}_sub"]).max()) <= ATOL
    assert abs(float(np.trace(cov)) - float(gold[f"trace_{which}"])) <= ATOL * cov.shape[0]


def test_fid_of_the_restated_statistics(gold, sets):
    (mg, cg), (mt, ct) = R.stats(sets[1]), R.stats(sets[2])
    assert abs(R.fid(mt.numpy(), ct.numpy(), mg.numpy(), cg.numpy()) - float(gold["fid"])) <= R.F32_FACTOR * float(gold["fid_e32_draws"].max())
