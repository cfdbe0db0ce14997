"""Time one HipTM2TMetrics.compute() (mld_hip.metrics: grouped retrieval, activation statistics and pair distances in libmldhip, the matrix square root on
the host) against the same computation done the reference's way on the same box: the embeddings copied to the host, then TM2TMetrics.compute's formulas
(mld/models/metrics/tm2t.py:89-154 with utils.py's euclidean_distance_matrix / calculate_top_k / calculate_activation_statistics_np /
calculate_frechet_distance_np / calculate_diversity_np, restated here in torch-CPU / numpy as the reference runs them).

  python tools/ab_t2m_metrics.py [--out profiles/t2m_metrics_ab.json] [--repeats 7]

Shape: 4 640 x 512 embeddings resident on the GPU (the protocol's size), R = 32, top_k 3, diversity_times 300.  Both sides start from the same device tensors
under the same seeds and end with every metric on the host; wall time by time.perf_counter around a device synchronisation, the two sides alternating.  The
time inside scipy.linalg.sqrtm is listed separately on both sides (it is the same host call on both).  A RECORD, with no pass / fail threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.linalg
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "motion-latent-diffusion_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import t2m_metrics_ref as R  # noqa: E402
from mld_hip import metrics as M  # noqa: E402
from mld_hip.evaluators import HipMetricOps  # noqa: E402

N, D, RS, TOP_K, DT = 4640, 512, 32, 3, 300
_sqrtm_s = [0.0]
_sqrtm = scipy.linalg.sqrtm


def timed_sqrtm(*a, **kw):
    t0 = time.perf_counter()
    out = _sqrtm(*a, **kw)
    _sqrtm_s[0] += time.perf_counter() - t0
    return out


def host_compute(texts, gen, gt):
    """TM2TMetrics.compute the reference's way: device tensors in, every formula on the host"""
    shuffle_idx = torch.randperm(N)
    all_texts, all_gen, all_gt = (x.cpu()[shuffle_idx, :] for x in (texts, gen, gt))
    out = {}
    for name, motions in (("", all_gen), ("gt_", all_gt)):
        score, hits = torch.tensor(0.0), torch.zeros(TOP_K)
        for i in range(N // RS):
            t, m = all_texts[i * RS:(i + 1) * RS], motions[i * RS:(i + 1) * RS]
            d = torch.sqrt(-2 * torch.mm(t, m.T) + torch.sum(torch.square(t), axis=1, keepdims=True) + torch.sum(torch.square(m), axis=1)).nan_to_num()
            score += d.trace()
            order = torch.argsort(d, dim=1)
            hit = order == torch.arange(RS).unsqueeze(1)
            hits += torch.cumsum(hit[:, :TOP_K], dim=1).bool().sum(0)
        out[name + "Matching_score"] = float(score / (N // RS * RS))
        for k in range(TOP_K):
            out[f"{name}R_precision_top_{k + 1}"] = float(hits[k] / (N // RS * RS))
    g, t = all_gen.numpy(), all_gt.numpy()
    out["FID"] = float(M.calculate_frechet_distance(np.mean(t, axis=0), np.cov(t, rowvar=False), np.mean(g, axis=0), np.cov(g, rowvar=False)))
    for name, x in (("Diversity", g), ("gt_Diversity", t)):
        a, b = np.random.choice(N, DT, replace=False), np.random.choice(N, DT, replace=False)
        out[name] = float(scipy.linalg.norm(x[a] - x[b], axis=1).mean())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "t2m_metrics_ab.json"))
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ab_t2m_metrics.py measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    M.scipy.linalg.sqrtm = timed_sqrtm                      # (mld_hip.metrics and this file call the same module attribute)
    g = torch.Generator().manual_seed(9)
    texts = torch.randn(N, D, generator=g)
    gen = (0.1 * texts + torch.randn(N, D, generator=g)).to(dev)
    gt = (0.12 * texts + torch.from_numpy(R.stats_inputs(N, D, seed=10))).to(dev)
    texts = texts.to(dev)
    metric = M.HipTM2TMetrics(top_k=TOP_K, R_size=RS, diversity_times=DT, ops=HipMetricOps())
    metric.update(texts, gen, gt, [1] * N)

    def engine_side():
        metric.Matching_score, metric.gt_Matching_score = torch.tensor(0.), torch.tensor(0.)
        return {k: float(v) for k, v in metric.compute(sanity_flag=False).items()}

    sides = {"engine": engine_side, "host_reference_way": lambda: host_compute(texts, gen, gt)}
    times = {n: [] for n in sides}
    roots = {n: [] for n in sides}
    values = {}
    for rep in range(a.repeats + 1):                        # (the first round warms both sides up and is dropped)
        for n, fn in sides.items():
            torch.manual_seed(3)
            np.random.seed(3)
            torch.cuda.synchronize()
            _sqrtm_s[0] = 0.0
            t0 = time.perf_counter()
            values[n] = fn()
            torch.cuda.synchronize()
            if rep:
                times[n].append(time.perf_counter() - t0)
                roots[n].append(_sqrtm_s[0])
    res = {"shape": [N, D], "R_size": RS, "top_k": TOP_K, "diversity_times": DT, "repeats": a.repeats,
           "method": "time.perf_counter around one compute() from device-resident embeddings to host-side metric values, device synchronised on both ends; the two "
                     "sides alternate; one warm-up round dropped; seconds",
           "note": "a record, not a gate: scipy.linalg.sqrtm of the 512 x 512 product runs on the host on both sides and is listed separately"}
    for n in sides:
        rest = [t - r for t, r in zip(times[n], roots[n])]
        res[n] = {"compute_s_median": float(np.median(times[n])), "compute_s_min": float(np.min(times[n])), "compute_s_max": float(np.max(times[n])),
                  "sqrtm_s_median": float(np.median(roots[n])), "without_sqrtm_s_median": float(np.median(rest)), "values": values[n]}
    res["max_abs_difference_of_the_values"] = {k: abs(values["engine"][k] - values["host_reference_way"][k]) for k in values["engine"]}
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
