"""mld_hip.metrics.HipUESTCMetrics against the reference's UESTCMetrics call order (tests/golden/uestc_rec.npz, tools/make_golden_uestc_rec.py: the
sequence of tests/uestc_rec_ref.make_sequence run through the reference's own STGCN and metric helpers).

* Fed the fixture's reference yhat and features under the fixture's seeds, ``update`` reproduces the confusion matrices and accuracies exactly and
  ``compute`` all eight values within 1e-6 max(1, |ref|): the same helpers on the same float32 inputs in the same draw order, so only the order of a few
  float32 additions may differ; a wrong draw order or a wrong default (the ground-truth diversity call uses 200 / 20) shows as an O(1e-3) difference.
* Driven through the simulator engine, ``update`` makes ONE engine call per update on cat([rec, gt]); the confusion matrices equal the fixture's; the
  features lie within the restatement's float32 rule of float64 (4 x e32), and all eight values agree with the reference's within 32 x (4 + 1) x e32:
  Diversity and Multimodality are means of Euclidean distances of 256-d rows, which move by 2 sqrt(256) x the per-element error at the most (the engine is
  within 4 e32 of float64, the reference's float32 run within e32); the FIDs are sums of squared mean differences and covariance traces of the same rows,
  whose spread is ~1e-2, so the same per-element error moves them by less than it moves a distance; the accuracies are exact."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import simlib  # noqa: E402
import uestc_rec_ref as R  # noqa: E402
from mld_hip import _lib  # noqa: E402
from mld_hip import engine as _engine  # noqa: E402
from mld_hip.evaluators import HipStgcnRecognizer  # noqa: E402
from mld_hip.metrics import HipUESTCMetrics  # noqa: E402

GOLDEN = simlib.os.path.join(simlib.REPO, "tests", "golden", "uestc_rec.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


class Replay:
    """a recognizer that hands back the fixture's reference outputs of update u and records what it was given"""

    def __init__(self, gold):
        self.gold, self.u, self.calls = gold, 0, []

    def recognize(self, motion):
        self.calls.append(motion.clone())
        yh, ft = self.gold["seq_yhat"][self.u], self.gold["seq_feat"][self.u]
        self.u += 1
        return torch.from_numpy(np.concatenate([yh[0], yh[1]])), torch.from_numpy(np.concatenate([ft[0], ft[1]]))


def finish(m, gold, names, tol):
    np.random.seed(int(gold["seq_compute_seed"]))
    torch.manual_seed(int(gold["seq_compute_seed"]))
    got = m.compute(False)
    want = dict(zip([str(n) for n in gold["seq_metric_names"]], gold["seq_metric_values"]))
    assert sorted(got) == sorted(want) == sorted(HipUESTCMetrics.METRICS)
    for k in names:
        g, v = float(got[k]), float(want[k])
        print(f"{k}: {g:.9f} reference {v:.9f} (bound {tol(v):.2e})")
        if k in ("accuracy", "gt_accuracy"):
            assert g == float(np.float32(v)) or g == v, k
        else:
            assert abs(g - v) <= tol(v), (k, g, v)


def test_replayed_reference_outputs_reproduce_the_eight_values(gold):
    rec = Replay(gold)
    m = HipUESTCMetrics(recognizer=rec, diversity_times=int(gold["seq_dt"]), multimodality_times=int(gold["seq_mt"]))
    assert m.num_labels == 40
    seq = R.make_sequence()
    for lab, r, g, ln in seq:
        m.update(lab, r, g, ln)
    assert len(rec.calls) == len(seq) and all(torch.equal(c, torch.cat([r, g])) for c, (_, r, g, _) in zip(rec.calls, seq))
    assert int(m.count) == sum(sum(ln) for *_, ln in seq) and int(m.count_seq) == R.SEQ_NU * R.SEQ_B
    assert np.array_equal(m.confusion.numpy(), gold["seq_confusion"]) and np.array_equal(m.gt_confusion.numpy(), gold["seq_gt_confusion"])
    sanity = m.compute(True)
    assert sorted(sanity) == sorted(HipUESTCMetrics.METRICS) and all(float(v) == 0.0 for v in sanity.values())
    finish(m, gold, HipUESTCMetrics.METRICS, lambda v: 1e-6 * max(1.0, abs(v)))


def test_metric_on_the_simulator_engine(gold):
    eng = _lib.Engine(lib=simlib.sim_library(), use_graph=0, **R.engine_kwargs(max_batch=R.SEQ_B, max_frames=R.SEQ_T))
    seen = []
    real = eng.uestc_recognize

    def spy(x, strides, B, T, logits_out=None, feat_out=None, stream=0):
        seen.append((B, T, tuple(strides)))
        return real(x, strides, B, T, logits_out, feat_out, stream)

    eng.uestc_recognize = spy
    mod = HipStgcnRecognizer(tensors=R.weights()).use_engine(_engine.inject_engine(eng, "inject:uestc_metrics"))
    m = HipUESTCMetrics(recognizer=mod, diversity_times=int(gold["seq_dt"]), multimodality_times=int(gold["seq_mt"]))
    seq = R.make_sequence()
    e32 = 0.0
    for u, (lab, r, g, ln) in enumerate(seq):
        m.update(lab, r, g, ln)
        (rl, _), (rf, ef) = R.reference(R.weights(), torch.cat([r, g]).numpy())
        R.check_gaps(rl)
        got = np.concatenate([m.recmotion_embeddings[u].numpy(), m.gtmotion_embeddings[u].numpy()])
        R.check(got, (rf, ef), f"features of update {u} (simulator)", 0)
        e32 = max(e32, ef)
    assert seen == [(2 * R.SEQ_B, R.SEQ_T, (144 * R.SEQ_T, 6 * R.SEQ_T, R.SEQ_T, 1))] * R.SEQ_NU      # one call per update, generated + ground truth
    assert np.array_equal(m.confusion.numpy(), gold["seq_confusion"]) and np.array_equal(m.gt_confusion.numpy(), gold["seq_gt_confusion"])
    finish(m, gold, HipUESTCMetrics.METRICS, lambda v: 2 * np.sqrt(256.0) * (R.F32_FACTOR + 1) * e32)
    _engine._engines.pop("inject:uestc_metrics")
    eng.close()


def test_recognizer_reads_the_tar_or_warns_and_stands_in(tmp_path):
    with pytest.warns(RuntimeWarning, match="uestc_rot6d_stgcn.tar"):
        syn_mod = HipStgcnRecognizer(str(tmp_path))
    assert syn_mod.source == "synthetic"
    sd = R.weights("bn_x2")
    state = {k: torch.from_numpy(v) for k, v in sd.items()}
    state["data_bn.num_batches_tracked"] = torch.tensor(5)                     # the checkpoint's scalars are dropped
    state["st_gcn_networks.0.tcn.0.num_batches_tracked"] = torch.tensor(5)
    torch.save(state, tmp_path / "uestc_rot6d_stgcn.tar")
    for where in (str(tmp_path), str(tmp_path / "uestc_rot6d_stgcn.tar")):
        mod = HipStgcnRecognizer(where)
        assert mod.source == str(tmp_path / "uestc_rot6d_stgcn.tar")
        got = {k: v.numpy() for k, v in mod.state_dict().items()}
        assert sorted(got) == sorted(sd) and all(np.array_equal(got[k], sd[k]) for k in sd)
        assert mod._arch == {"uestc_rec": 1} and mod._prefix == "uestc_rec."
    seven = {**sd, "fcn.weight": sd["fcn.weight"][:7].copy(), "fcn.bias": sd["fcn.bias"][:7].copy()}
    assert HipStgcnRecognizer(tensors=seven, num_class=7)._arch == {"uestc_rec": 1, "uestc_classes": 7}
    with pytest.raises(ValueError):
        HipStgcnRecognizer(tensors={**sd, "fcn.weight": np.zeros((40, 128, 1, 1), np.float32)})
    with pytest.raises(ValueError):
        mod.recognize(torch.zeros(2, 24, 3, 4))
