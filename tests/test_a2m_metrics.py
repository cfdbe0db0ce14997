"""mld_hip.metrics.HipHUMANACTMetrics against the reference's HUMANACTMetrics call order (tests/golden/a2m_rec.npz, tools/make_golden_a2m_rec.py):

* fed the fixture's reference logits and activations under the fixture's seeds, ``update`` reproduces the confusion matrices and accuracies exactly and
  ``compute`` the FID, diversity and multimodality (and the gt_ ones) within 1e-4 max(1, |ref|) -- the worst-case float32 rounding of the <= 300-term sums
  is 300 x 6e-8 = 1.8e-5, so the bound is about 5 x that; a wrong draw order shows as an O(1) difference;
* driven through the simulator engine under torch.manual_seed, ``update`` hands the engine the reference's four initial states (initHidden's draws) in
  the reference's order, as one call of 4B motions, and keeps the classifier's rows for the confusion matrices and the FID net's for the embeddings."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import a2m_rec_ref as R  # noqa: E402
import simlib  # noqa: E402
from mld_hip import _lib  # noqa: E402
from mld_hip import engine as _engine  # noqa: E402
from mld_hip.evaluators import HipActionRecognizer  # noqa: E402
from mld_hip.metrics import HipHUMANACTMetrics  # noqa: E402

GOLDEN = simlib.os.path.join(simlib.REPO, "tests", "golden", "a2m_rec.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


class Replay:
    """a recognizer that hands back the fixture's reference outputs of update u (rows the metric must not use are NaN) and records what it was given"""

    def __init__(self, gold):
        self.gold, self.u, self.calls = gold, 0, []

    def recognize(self, joints, lengths, h0=None):
        self.calls.append((joints.shape, list(lengths), None if h0 is None else h0.clone()))
        lo, ac = self.gold["seq_logits"][self.u], self.gold["seq_act"][self.u]
        B = lo.shape[1]
        nan_l, nan_a = np.full((2 * B, 12), np.nan, np.float32), np.full((2 * B, 30), np.nan, np.float32)
        self.u += 1
        return torch.from_numpy(np.concatenate([lo[0], lo[1], nan_l])), torch.from_numpy(np.concatenate([nan_a, ac[0], ac[1]]))


def motions(B, T):
    return torch.zeros(B, 24, 3, T), torch.zeros(B, 24, 3, T)


def test_replayed_reference_outputs_reproduce_the_metrics(gold):
    rec = Replay(gold)
    m = HipHUMANACTMetrics(recognizer=rec, diversity_times=int(gold["seq_dt"]), multimodality_times=int(gold["seq_mt"]))
    torch.manual_seed(int(gold["seq_update_seed"]))
    NU, B = gold["seq_labels"].shape
    T = int(gold["seq_lengths"].max())
    for u in range(NU):
        lens = [int(n) for n in gold["seq_lengths"][u]]
        m.update(torch.from_numpy(gold["seq_labels"][u]), *motions(B, T), lens)
    assert int(m.count) == int(gold["seq_lengths"].sum()) and int(m.count_seq) == NU * B
    assert np.array_equal(m.confusion.numpy(), gold["seq_confusion"]) and np.array_equal(m.gt_confusion.numpy(), gold["seq_gt_confusion"])
    assert all(bool(torch.isfinite(e).all()) for e in m.recmotion_embeddings + m.gtmotion_embeddings)
    sanity = m.compute(True)
    assert sorted(sanity) == sorted(HipHUMANACTMetrics.METRICS) and all(float(v) == 0.0 for v in sanity.values())
    np.random.seed(int(gold["seq_compute_seed"]))
    torch.manual_seed(int(gold["seq_compute_seed"]))
    got = m.compute(False)
    want = dict(zip([str(n) for n in gold["seq_metric_names"]], gold["seq_metric_values"]))
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        g = float(got[k])
        print(f"{k}: {g:.9f} reference {v:.9f}")
        if k in ("accuracy", "gt_accuracy"):
            assert g == float(np.float32(v)) or g == v, k
        else:
            assert abs(g - v) <= 1e-4 * max(1.0, abs(v)), (k, g, v)


def test_update_hands_the_engine_the_reference_draws(gold):
    """the simulator engine: one call of 4B motions with the four initHidden draws of the reference's first update, stacked along B in its order"""
    NU, B = gold["seq_labels"].shape
    T = 8
    eng = _lib.Engine(lib=simlib.sim_library(), use_graph=0, **R.engine_kwargs(max_batch=B, max_frames=T))
    seen = []
    real = eng.a2m_recognize

    def spy(joints, lengths, T_, h0=None, logits_out=None, act_out=None, stream=0):
        seen.append((joints.clone(), list(lengths), T_, h0.clone()))
        return real(joints, lengths, T_, h0, logits_out, act_out, stream)

    eng.a2m_recognize = spy
    mod = HipActionRecognizer(tensors=R.weights()).use_engine(_engine.inject_engine(eng, "inject:a2m_metrics"))
    m = HipHUMANACTMetrics(recognizer=mod)
    g = torch.Generator().manual_seed(3)
    rec, gt = torch.randn(B, 24, 3, T, generator=g), torch.randn(B, 24, 3, T, generator=g)
    lens = [int(n) for n in torch.randint(1, T + 1, (B,), generator=g)]
    labels = torch.from_numpy(gold["seq_labels"][0])
    torch.manual_seed(int(gold["seq_update_seed"]))
    m.update(labels, rec, gt, lens)
    assert len(seen) == 1
    joints, ln, T_, h0 = seen[0]
    assert ln == lens * 4 and T_ == T and tuple(joints.shape) == (4 * B, T, 72)
    want = torch.from_numpy(gold["seq_h0_first"])                              # [4, 2, B, 128]: classifier(rec), classifier(gt), FID(rec), FID(gt)
    assert torch.equal(h0, torch.cat(list(want), dim=1))
    jr, jg = HipActionRecognizer.to_joints(rec), HipActionRecognizer.to_joints(gt)
    assert torch.equal(joints, torch.cat([jr, jg, jr, jg]))
    # the rows the metric kept: the classifier's on its first two draws, the FID net's on the last two -- the restatement on the same draws
    x = torch.cat([jr, jg]).numpy()
    (l_rec, e_l), _ = R.reference(R.weights(), x, lens * 2, torch.cat(list(want[:2]), dim=1).numpy())
    _, (a_emb, e_a) = R.reference(R.weights(), x, lens * 2, torch.cat(list(want[2:]), dim=1).numpy())
    assert np.abs(np.concatenate([m.recmotion_embeddings[0].numpy(), m.gtmotion_embeddings[0].numpy()]) - a_emb).max() <= R.F32_FACTOR * e_a
    conf = np.zeros((12, 12), np.int64)
    gconf = np.zeros((12, 12), np.int64)
    for i, lab in enumerate(labels.numpy()):
        conf[lab, l_rec[i].argmax()] += 1
        gconf[lab, l_rec[B + i].argmax()] += 1
    R.check_gaps(l_rec)
    assert np.array_equal(m.confusion.numpy(), conf) and np.array_equal(m.gt_confusion.numpy(), gconf)
    _engine._engines.pop("inject:a2m_metrics")
    eng.close()


def test_recognizer_reads_the_tar_or_warns_and_stands_in(tmp_path):
    with pytest.warns(RuntimeWarning, match="humanact12_gru.tar"):
        syn_mod = HipActionRecognizer(str(tmp_path))
    assert syn_mod.source == "synthetic"
    sd = R.weights("rec_x3")
    torch.save({"model": {k: torch.from_numpy(v) for k, v in sd.items()}, "epoch": 3}, tmp_path / "humanact12_gru.tar")
    for where in (str(tmp_path), str(tmp_path / "humanact12_gru.tar")):
        mod = HipActionRecognizer(where)
        assert mod.source == str(tmp_path / "humanact12_gru.tar")
        got = {k: v.numpy() for k, v in mod.state_dict().items()}
        assert sorted(got) == sorted(sd) and all(np.array_equal(got[k], sd[k]) for k in sd)
        assert mod._arch == {"a2m_rec": 1} and mod._prefix == "a2m_rec."
    with pytest.raises(ValueError):
        HipActionRecognizer(tensors={**sd, "linear2.weight": np.zeros((10, 30), np.float32)})
