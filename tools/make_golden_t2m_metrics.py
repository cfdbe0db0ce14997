"""Write tests/golden/t2m_metrics.npz by running the REFERENCE's own metric helpers (CPU only; needs a checkout of the reference project):

  MLD_REFERENCE=<checkout of motion-latent-diffusion> python tools/make_golden_t2m_metrics.py

It imports mld/models/metrics/utils.py by file path (TM2TMetrics and MMMetrics themselves need torchmetrics, so the script drives their compute() call order
by hand, line for line: tm2t.py:89-154, mm.py:46-49) on the seeded embeddings of tests/t2m_metrics_ref.py (golden_updates / golden_mm: 3 updates of 40 rows,
D = 512, R = 32, diversity_times 30; 6 texts x 12 repeats, mm_num_times 5).  The embeddings are not stored: they come from the seed.

  shuffle_idx            torch.randperm(120) under torch.manual_seed(compute_seed)
  dist_gen / dist_gt     [3, 32, 32] float32: euclidean_distance_matrix(...).nan_to_num() of every group, text vs generated / vs ground truth
  topk_gen / topk_gt     [3] the summed calculate_top_k hits;  match_gen / match_gt: the summed traces
  mu_* [512], cov_*_sub  np.mean / np.cov of the generated / ground-truth set (every 8th row and column of the covariance), trace_*: its trace
  fid, diversity, gt_diversity, multimodality       the metric values (np.random.seed(compute_seed) before the FID part, np.random.seed(mm_seed) before MM)
  fid_e32_draws          [8] |FID(float32-CPU statistics) - FID(np.cov float64 statistics)| of the reference's calculate_frechet_distance_np on 8 further seeded sets of
                         the run's shape and distribution (tests/t2m_metrics_ref.golden_updates(1 .. 8); 120 x 512, so the covariances are singular and the
                         float32 error is that of a singular product): the right-hand side of the FID rule for the recorded run
  next_np, next_torch    the next draw of each generator after compute(): a replay that consumed other draws lands elsewhere"""
import importlib.util
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "motion-latent-diffusion_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import t2m_metrics_ref as R  # noqa: E402


def load_file(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = os.environ.get("MLD_REFERENCE") or sys.exit("set MLD_REFERENCE to a checkout of the reference project")
    mu = load_file("metric_utils", os.path.join(ref, "mld", "models", "metrics", "utils.py"))
    G = R.GOLD
    ups = R.golden_updates()
    texts = [torch.flatten(t, start_dim=1) for t, _, _ in ups]
    gens = [torch.flatten(g, start_dim=1) for _, g, _ in ups]
    gts = [torch.flatten(g, start_dim=1) for _, _, g in ups]
    count_seq, Rs, top_k = G["updates"] * G["rows"], G["R"], G["top_k"]
    out = {}
    torch.manual_seed(G["compute_seed"])
    np.random.seed(G["compute_seed"])
    shuffle_idx = torch.randperm(count_seq)
    all_texts = torch.cat(texts, axis=0).cpu()[shuffle_idx, :]
    all_gen = torch.cat(gens, axis=0).cpu()[shuffle_idx, :]
    all_gt = torch.cat(gts, axis=0).cpu()[shuffle_idx, :]
    out["shuffle_idx"] = shuffle_idx.numpy()
    for name, motions in (("gen", all_gen), ("gt", all_gt)):
        score, top_k_mat, mats = torch.tensor(0.0), torch.zeros((top_k,)), []
        for i in range(count_seq // Rs):
            group_texts = all_texts[i * Rs:(i + 1) * Rs]
            group_motions = motions[i * Rs:(i + 1) * Rs]
            dist_mat = mu.euclidean_distance_matrix(group_texts, group_motions).nan_to_num()
            score += dist_mat.trace()
            argsmax = torch.argsort(dist_mat, dim=1)
            top_k_mat += mu.calculate_top_k(argsmax, top_k=top_k).sum(axis=0)
            mats.append(dist_mat.numpy())
        out[f"dist_{name}"], out[f"topk_{name}"], out[f"match_{name}"] = np.stack(mats), top_k_mat.numpy(), score.numpy()
    all_gen, all_gt = all_gen.numpy(), all_gt.numpy()
    m, cov = mu.calculate_activation_statistics_np(all_gen)
    gt_m, gt_cov = mu.calculate_activation_statistics_np(all_gt)
    s = R.GOLD_COV_STEP
    out.update(mu_gen=m, mu_gt=gt_m, cov_gen_sub=cov[::s, ::s], cov_gt_sub=gt_cov[::s, ::s], trace_gen=np.trace(cov), trace_gt=np.trace(gt_cov))
    out["fid"] = mu.calculate_frechet_distance_np(gt_m, gt_cov, m, cov)
    out["diversity"] = mu.calculate_diversity_np(all_gen, G["diversity_times"])
    out["gt_diversity"] = mu.calculate_diversity_np(all_gt, G["diversity_times"])
    out["next_np"], out["next_torch"] = np.random.randint(1 << 30), torch.randint(1 << 30, (1,)).numpy()
    errs = []
    for k in range(1, R.FID_DRAWS + 1):
        gen = torch.cat([torch.flatten(g, start_dim=1) for _, g, _ in R.golden_updates(k)]).numpy()
        gt = torch.cat([torch.flatten(g, start_dim=1) for _, _, g in R.golden_updates(k)]).numpy()
        (mg, cg), (mt, ct) = R.stats(gen, torch.float32), R.stats(gt, torch.float32)
        f32 = mu.calculate_frechet_distance_np(mt.double().numpy(), ct.double().numpy(), mg.double().numpy(), cg.double().numpy())
        f64 = mu.calculate_frechet_distance_np(*mu.calculate_activation_statistics_np(gt.astype(np.float64)), *mu.calculate_activation_statistics_np(gen.astype(np.float64)))
        errs.append(abs(f32 - f64))
    out["fid_e32_draws"] = np.asarray(errs)
    np.random.seed(G["mm_seed"])
    all_mm = torch.cat(R.golden_mm(), axis=0).cpu().numpy()
    out["multimodality"] = mu.calculate_multimodality_np(all_mm, G["mm_times"])
    out["next_np_mm"] = np.random.randint(1 << 30)
    path = os.path.join(REPO, "tests", "golden", "t2m_metrics.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", {k: float(out[k]) for k in ("fid", "diversity", "gt_diversity", "multimodality")},
          "top-k", out["topk_gen"], out["topk_gt"], "FID float32 errors", out["fid_e32_draws"])


if __name__ == "__main__":
    main()
