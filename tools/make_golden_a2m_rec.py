"""Write tests/golden/a2m_rec.npz by running the REFERENCE's own recognition GRU and metric helpers (CPU only; needs a checkout of the reference project):

  MLD_REFERENCE=<checkout of motion-latent-diffusion> python tools/make_golden_a2m_rec.py

It imports mld/models/architectures/humanact12_gru.py and mld/models/metrics/utils.py by file path (HUMANACTMetrics itself needs torchmetrics, so the
script drives the metric's update / compute call order by hand) and runs them on the seeded stand-in weights (mld_hip.synthetic.make_a2m_rec_state_dict,
both families of tests/a2m_rec_ref.py) and seeded inputs.  The file holds no weights: they come from the seed.

  case_*          B = 17, T = 13 (tests/a2m_rec_ref.make_case): joints [B, T, 72], lengths, h0 [2, B, 128] (explicit hidden_unit), and per family the
                  reference's logits [B, 12] (MotionDiscriminator) and activations [B, 30] (MotionDiscriminatorForFID)
  seq_*           one metric run: NU updates of B motions (seeded labels covering the 12 classes, lengths, joints that are not stored) under
                  torch.manual_seed(seq_update_seed), with initHidden's draws of the first update recorded, the logits / activations of every update,
                  the confusion matrices; then compute() under np.random.seed / torch.manual_seed(seq_compute_seed) with diversity_times seq_dt,
                  multimodality_times seq_mt: the eight metric values.
The float64 restatement of tests/a2m_rec_ref.py alone satisfies the class rule on every case (asserted here)."""
import importlib.util
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "motion-latent-diffusion_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import a2m_rec_ref as R  # noqa: E402

NU, SEQ_B, SEQ_T = 3, 24, 16
UPDATE_SEED, COMPUTE_SEED, DT, MT = 21, 22, 30, 5


def load_file(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def nets(hg, sd):
    clf = hg.MotionDiscriminator(input_size=72, hidden_size=128, hidden_layer=2, output_size=12)
    fid = hg.MotionDiscriminatorForFID(input_size=72, hidden_size=128, hidden_layer=2, output_size=12)
    state = {k: torch.from_numpy(v) for k, v in sd.items()}
    for m in (clf, fid):
        m.load_state_dict(state)
        m.eval()
    return clf, fid


def to_reference(j):
    """the engine's [B, T, 72] -> the reference's [B, 24, 3, T]"""
    B, T, _ = j.shape
    return torch.from_numpy(np.ascontiguousarray(j.transpose(0, 2, 1).reshape(B, 24, 3, T)))


def main():
    ref = os.environ.get("MLD_REFERENCE") or sys.exit("set MLD_REFERENCE to a checkout of the reference project")
    hg = load_file("humanact12_gru", os.path.join(ref, "mld", "models", "architectures", "humanact12_gru.py"))
    mu = load_file("metric_utils", os.path.join(ref, "mld", "models", "metrics", "utils.py"))
    out = {}
    # ---- explicit hidden_unit: one case, both families
    j, lens, h0 = R.make_case(17, 13)
    out.update(case_joints=j, case_lengths=np.asarray(lens, np.int32), case_h0=h0)
    with torch.no_grad():
        for fam in R.FAMILIES:
            sd = R.weights(fam)
            clf, fid = nets(hg, sd)
            x, ln, h = to_reference(j), torch.tensor(lens), torch.from_numpy(h0)
            out[f"case_logits_{fam}"] = clf(x, lengths=ln, hidden_unit=h).numpy()
            out[f"case_act_{fam}"] = fid(x, lengths=ln, hidden_unit=h).numpy()
            R.check_gaps(R.reference(sd, j, lens, h0)[0][0])
    # ---- one metric run with the reference's own draws (default family)
    clf, fid = nets(hg, R.weights("default"))
    draws = []
    init = hg.MotionDiscriminator.initHidden

    def recording(self, num_samples, layer):
        h = init(self, num_samples, layer)
        draws.append(h.clone())
        return h

    hg.MotionDiscriminator.initHidden = recording
    g = np.random.default_rng(7)
    labels, lengths = [], []
    logits, acts = [], []
    confusion = torch.zeros(12, 12, dtype=torch.long)
    gt_confusion = torch.zeros(12, 12, dtype=torch.long)
    rec_emb, gt_emb, lab_emb = [], [], []
    torch.manual_seed(UPDATE_SEED)
    with torch.no_grad():
        for u in range(NU):
            lab = torch.from_numpy((np.arange(SEQ_B) + g.integers(0, 12)) % 12)
            ln = [int(n) for n in g.integers(1, SEQ_T + 1, size=SEQ_B)]
            ln[0] = SEQ_T
            rec = torch.from_numpy(g.standard_normal((SEQ_B, 24, 3, SEQ_T)).astype(np.float32))
            gt = torch.from_numpy((0.7 * g.standard_normal((SEQ_B, 24, 3, SEQ_T))).astype(np.float32))
            lt = torch.tensor(ln)
            # HUMANACTMetrics.update's order: classifier(rec), classifier(gt), confusion rows, FID net(rec), FID net(gt)
            batch_prob = clf(rec, lengths=lt)
            gt_batch_prob = clf(gt, lengths=lt)
            labels_ = lab.squeeze().long()
            for lb, pred in zip(labels_, batch_prob.max(dim=1).indices):
                confusion[lb][pred] += 1
            for lb, pred in zip(labels_, gt_batch_prob.max(dim=1).indices):
                gt_confusion[lb][pred] += 1
            r_emb = fid(rec, lengths=lt)
            g_emb = fid(gt, lengths=lt)
            lab_emb.append(labels_)
            rec_emb.append(r_emb)
            gt_emb.append(g_emb)
            labels.append(lab.numpy())
            lengths.append(ln)
            logits.append(np.stack([batch_prob.numpy(), gt_batch_prob.numpy()]))
            acts.append(np.stack([r_emb.numpy(), g_emb.numpy()]))
    hg.MotionDiscriminator.initHidden = init
    assert len(draws) == 4 * NU
    # HUMANACTMetrics.compute's order
    np.random.seed(COMPUTE_SEED)
    torch.manual_seed(COMPUTE_SEED)
    accuracy = torch.trace(confusion) / torch.sum(confusion)
    gt_accuracy = torch.trace(gt_confusion) / torch.sum(gt_confusion)
    all_labels = torch.cat(lab_emb, axis=0)
    all_gen = torch.cat(rec_emb, axis=0)
    all_gt = torch.cat(gt_emb, axis=0)
    all_gt2 = all_gt.clone()[torch.randperm(all_gt.shape[0]), :]
    genstats = mu.calculate_activation_statistics(all_gen)
    gtstats = mu.calculate_activation_statistics(all_gt)
    gtstats2 = mu.calculate_activation_statistics(all_gt2)
    div, mm = mu.calculate_diversity_multimodality(all_gen, all_labels.cpu(), 12, diversity_times=DT, multimodality_times=MT)
    gdiv, gmm = mu.calculate_diversity_multimodality(all_gt, all_labels.cpu(), 12)
    values = {"accuracy": accuracy, "gt_accuracy": gt_accuracy, "FID": mu.calculate_fid(gtstats, genstats), "gt_FID": mu.calculate_fid(gtstats, gtstats2),
              "Diversity": div, "gt_Diversity": gdiv, "Multimodality": mm, "gt_Multimodality": gmm}
    out.update(seq_labels=np.stack(labels).astype(np.int64), seq_lengths=np.asarray(lengths, np.int32), seq_logits=np.stack(logits).astype(np.float32),
               seq_act=np.stack(acts).astype(np.float32), seq_h0_first=torch.stack(draws[:4]).numpy(), seq_confusion=confusion.numpy(),
               seq_gt_confusion=gt_confusion.numpy(), seq_update_seed=np.int64(UPDATE_SEED), seq_compute_seed=np.int64(COMPUTE_SEED), seq_dt=np.int64(DT),
               seq_mt=np.int64(MT), seq_metric_names=np.asarray(list(values)), seq_metric_values=np.asarray([float(v) for v in values.values()], np.float64))
    path = os.path.join(REPO, "tests", "golden", "a2m_rec.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: round(float(v), 6) for k, v in values.items()})


if __name__ == "__main__":
    main()
