"""HipTM2TMetrics / HipMMMetrics (mld_hip.metrics) on the functional simulator reproduce the run the REFERENCE's own helpers recorded
(tests/golden/t2m_metrics.npz) under the recorded seeds: the R-precision values exactly; the matching scores, the diversities and the multimodality under the
value rule of tests/t2m_metrics_ref.py; the FID under its FID rule with the recorded right-hand side; and the random draws consumed are the reference's (the
next draw of each generator after compute() is the recorded one, and equals a hand-driven sequence).  Also the class surface: state names, metric keys,
reset, the sanity flag, accumulation of the matching scores, the reference's asserts and the capacity error of HipMetricOps."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import simlib  # noqa: E402
import t2m_metrics_ref as R  # noqa: E402
from mld_hip import _lib  # noqa: E402
from mld_hip import engine as E  # noqa: E402
from mld_hip.evaluators import HipMetricOps  # noqa: E402
from mld_hip.metrics import HipMMMetrics, HipTM2TMetrics  # noqa: E402

G = R.GOLD
KEYS = ["Matching_score", "gt_Matching_score", "R_precision_top_1", "R_precision_top_2", "R_precision_top_3", "gt_R_precision_top_1", "gt_R_precision_top_2",
        "gt_R_precision_top_3", "FID", "Diversity", "gt_Diversity"]


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "t2m_metrics.npz"))


@pytest.fixture(scope="module")
def ops():
    eng = _lib.Engine(lib=simlib.sim_library(), use_graph=0, **R.engine_kwargs(metrics_max_rows=256))
    yield HipMetricOps(metrics_max_rows=256).use_engine(E.inject_engine(eng, "inject:t2m_metrics"))
    eng.close()


def filled(ops):
    m = HipTM2TMetrics(top_k=G["top_k"], R_size=G["R"], diversity_times=G["diversity_times"], ops=ops)
    for t, gen, gt in R.golden_updates():
        m.update(t, gen, gt, [10] * G["rows"])
    return m


@pytest.fixture(scope="module")
def computed(ops):
    m = filled(ops)
    torch.manual_seed(G["compute_seed"])
    np.random.seed(G["compute_seed"])
    out = m.compute(sanity_flag=False)
    return m, out, np.random.randint(1 << 30), int(torch.randint(1 << 30, (1,)))


def test_surface(ops):
    m = filled(ops)
    assert m.metrics == KEYS and m.name == "matching, fid, and diversity scores"
    assert int(m.count) == 3 * 10 * G["rows"] and int(m.count_seq) == 3 * G["rows"]
    assert [tuple(t.shape) for t in m.recmotion_embeddings] == [(G["rows"], G["D"])] * 3          # flattened from dim 1
    assert len(m.text_embeddings) == len(m.gtmotion_embeddings) == 3
    out = m.compute(sanity_flag=True)
    assert list(out) == KEYS and all(float(v) == 0.0 for v in out.values())
    assert m.to("cpu") is m
    m.reset()
    assert int(m.count_seq) == 0 and m.text_embeddings == [] and float(m.Matching_score) == 0.0


def test_recorded_run(gold, computed):
    _, out, _, _ = computed
    assert list(out) == KEYS
    n = G["updates"] * G["rows"] // G["R"] * G["R"]
    for k in range(G["top_k"]):                                                                   # exact
        assert float(out[f"R_precision_top_{k + 1}"]) == float(np.float32(gold["topk_gen"][k]) / n)
        assert float(out[f"gt_R_precision_top_{k + 1}"]) == float(np.float32(gold["topk_gt"][k]) / n)
    ups = R.golden_updates()
    idx = torch.from_numpy(gold["shuffle_idx"])
    texts, gen, gt = (torch.cat([torch.flatten(u[k], start_dim=1) for u in ups])[idx].numpy() for k in range(3))
    for key, motions, which in (("Matching_score", gen, "gen"), ("gt_Matching_score", gt, "gt")):
        ref = R.match_reference(texts, motions, G["R"])
        # a mean of entries that each obey the value rule obeys it; the scalar's own float32 accumulation is measured by the reference's recorded value
        r64 = float(ref["diag64"].mean())
        e32 = max(ref["e32_diag"], abs(float(gold[f"match_{which}"]) / n - r64))
        R.check_value(np.float32(out[key]), (r64, e32), key)
    np.random.seed(G["compute_seed"])
    for key, x in (("Diversity", gen), ("gt_Diversity", gt)):
        a, b = np.random.choice(len(x), G["diversity_times"], replace=False), np.random.choice(len(x), G["diversity_times"], replace=False)
        d64, e32 = R.pair_reference(x, a, b)
        R.check_value(np.float32(out[key]), (float(d64.mean()), max(e32, abs(float(gold[key.lower()]) - float(d64.mean())))), key)
    left, right = abs(float(out["FID"]) - float(gold["fid"])), float(gold["fid_e32_draws"].max())
    print(f"FID: |engine - reference| {left:.3e}  max float32 error over the 8 draws {right:.3e}")
    assert left <= R.F32_FACTOR * right


def test_draws_consumed_are_the_references(gold, computed):
    _, _, next_np, next_torch = computed
    assert next_np == int(gold["next_np"]) and next_torch == int(gold["next_torch"][0])
    # ... and equal a hand-driven sequence: one randperm; then four choices without replacement
    torch.manual_seed(G["compute_seed"])
    np.random.seed(G["compute_seed"])
    n = G["updates"] * G["rows"]
    assert np.array_equal(torch.randperm(n).numpy(), gold["shuffle_idx"])
    for _ in range(4):
        np.random.choice(n, G["diversity_times"], replace=False)
    assert np.random.randint(1 << 30) == next_np and int(torch.randint(1 << 30, (1,))) == next_torch


def test_matching_scores_accumulate_until_reset(computed):
    m, out, _, _ = computed
    first = float(m.Matching_score)
    torch.manual_seed(G["compute_seed"])
    np.random.seed(G["compute_seed"])
    again = m.compute(sanity_flag=False)
    assert float(m.Matching_score) == pytest.approx(2 * first, rel=1e-6)                           # the reference's state behaviour
    assert float(again["Matching_score"]) == pytest.approx(2 * float(out["Matching_score"]), rel=1e-6)
    assert float(again["R_precision_top_1"]) == float(out["R_precision_top_1"]) and float(again["FID"]) == float(out["FID"])


def test_the_references_asserts_and_the_capacity(ops):
    m = HipTM2TMetrics(R_size=32, diversity_times=300, ops=ops)
    t = torch.randn(32, 16, generator=torch.Generator().manual_seed(1))
    m.update(t, t, t, [5] * 32)
    with pytest.raises(AssertionError):
        m.compute(sanity_flag=False)                                                               # count_seq > R_size
    m.update(t, t, t, [5] * 32)
    with pytest.raises(AssertionError):
        m.compute(sanity_flag=False)                                                               # count_seq > diversity_times
    big = torch.zeros(257, 4)
    for call in (lambda: ops.stats(big), lambda: ops.match(big, big, 4), lambda: ops.pair_dist(big, [0], [1]), lambda: ops.pair_dist(big[:9], [0] * 257, [1] * 257)):
        with pytest.raises(ValueError, match="metrics_max_rows"):
            call()
    with pytest.raises(TypeError):
        ops.stats(big.double()[:9])


def test_multimodality_recorded_run(gold, ops):
    mm = HipMMMetrics(mm_num_times=G["mm_times"], ops=ops)
    assert mm.metrics == ["MultiModality"] and mm.name == "MultiModality scores"
    for x in R.golden_mm():
        mm.update(x, [10])
    assert int(mm.count_seq) == G["mm_texts"] and float(mm.compute(sanity_flag=True)["MultiModality"]) == 0.0
    np.random.seed(G["mm_seed"])
    out = mm.compute(sanity_flag=False)
    assert np.random.randint(1 << 30) == int(gold["next_np_mm"])                                  # two choices consumed, nothing else
    np.random.seed(G["mm_seed"])
    first, second = np.random.choice(G["mm_reps"], G["mm_times"], replace=False), np.random.choice(G["mm_reps"], G["mm_times"], replace=False)
    x = torch.cat(R.golden_mm()).reshape(-1, G["D"]).numpy()
    base = np.arange(G["mm_texts"])[:, None] * G["mm_reps"]
    d64, e32 = R.pair_reference(x, (base + first).reshape(-1), (base + second).reshape(-1))
    R.check_value(np.float32(out["MultiModality"]), (float(d64.mean()), max(e32, abs(float(gold["multimodality"]) - float(d64.mean())))), "MultiModality")
    mm.reset()
    assert mm.mm_motion_embeddings == [] and int(mm.count) == 0
