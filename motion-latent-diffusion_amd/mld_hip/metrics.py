"""``HipHUMANACTMetrics`` -- a drop-in for the reference's HUMANACTMetrics (mld/models/metrics/gru.py, selected by config_mld_humanact12's
METRIC.TYPE: ['HUMANACTMetrics']) whose recognition GRU runs in libmldhip (``HipActionRecognizer``; ``mldhip_a2m_recognize``).

It keeps the reference's surface: ``update(label, recmotion [B, 24, 3, T], gtmotion, lengths)`` / ``compute(sanity_flag)``, the state names (``count``,
``count_seq``, ``confusion``, ``gt_confusion``, ``label_embeddings``, ``recmotion_embeddings``, ``gtmotion_embeddings``) and the eight metric keys.  It is a
plain class (torchmetrics is not a dependency): states live on the object, there is no reduction across ranks.

Random draws follow the reference exactly, so under the same seeds the numbers are the reference's:
  * ``update`` draws the four initial states as the reference's four forward calls do -- torch.randn(2, B, 128) on the CPU default generator for the
    classifier on the generated motions, then on the ground truth, then the FID net on each -- and runs them as ONE engine call of 4B motions;
  * ``compute`` consumes torch.randperm and np.random in the reference's order (the ground-truth diversity / multimodality with the defaults 200 / 20).

``HipUESTCMetrics`` (at the end of this file) is the same for the reference's UESTCMetrics (mld/models/metrics/stgcn.py; METRIC.TYPE ['UESTCMetrics']) on the
recognition ST-GCN (``HipStgcnRecognizer``; ``mldhip_uestc_recognize``): the net draws nothing, so ``update`` is one engine call on cat([rec, gt]).

``HipTM2TMetrics`` / ``HipMMMetrics`` (behind it) are the text side: drop-ins for TM2TMetrics / MMMetrics (mld/models/metrics/tm2t.py, mm.py) on the embeddings of
``MLD.t2m_eval``, with the grouped retrieval, the activation statistics and the pair distances in libmldhip (``HipMetricOps``; ``mldhip_t2m_match`` /
``mldhip_act_stats`` / ``mldhip_pair_dist``)."""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import scipy.linalg
import torch
from torch import Tensor

from .evaluators import HipActionRecognizer, HipMetricOps, HipStgcnRecognizer


def calculate_activation_statistics(activations: Tensor):
    a = activations.cpu().numpy()
    return np.mean(a, axis=0), np.cov(a, rowvar=False)


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """||mu1 - mu2||^2 + Tr(C1 + C2 - 2 sqrt(C1 C2)), with the usual eps retry for a singular product and the real part of a complex root"""
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    diff = mu1 - mu2
    covmean = scipy.linalg.sqrtm(sigma1.dot(sigma2))
    if not np.isfinite(covmean).all():
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = scipy.linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError(f"Imaginary component {np.max(np.abs(covmean.imag))}")
        covmean = covmean.real
    return diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean)


def calculate_fid(statistics_1, statistics_2):
    return calculate_frechet_distance(statistics_1[0], statistics_1[1], statistics_2[0], statistics_2[1])


def calculate_diversity_multimodality(activations: Tensor, labels: Tensor, num_labels: int, diversity_times: int = 200, multimodality_times: int = 20):
    """mean distance of diversity_times random pairs; mean distance of same-label pairs, multimodality_times per label present -- drawn with
    np.random.randint in the reference's order"""
    labels = labels.long()
    n = activations.shape[0]
    first, second = np.random.randint(0, n, diversity_times), np.random.randint(0, n, diversity_times)
    diversity = 0
    for i, k in zip(first, second):
        diversity += torch.dist(activations[i, :], activations[k, :])
    diversity /= diversity_times
    multimodality = 0
    quotas = np.zeros(num_labels)
    quotas[labels.unique()] = multimodality_times
    while np.any(quotas > 0):
        i = np.random.randint(0, n)
        li = labels[i]
        if not quotas[li]:
            continue
        k = np.random.randint(0, n)
        while labels[k] != li:
            k = np.random.randint(0, n)
        quotas[li] -= 1
        multimodality += torch.dist(activations[i, :], activations[k, :])
    multimodality /= multimodality_times * num_labels
    return diversity, multimodality


class HipHUMANACTMetrics:
    METRICS = ["accuracy", "gt_accuracy", "FID", "gt_FID", "Diversity", "gt_Diversity", "Multimodality", "gt_Multimodality"]

    def __init__(self, datapath: Optional[str] = None, num_labels: int = 12, diversity_times: int = 200, multimodality_times: int = 20,
                 recognizer: Optional[HipActionRecognizer] = None, **kw):
        """``datapath``: humanact12_gru.tar (or the directory holding it; the reference passes os.path.join(model.humanact12_rec_path, 'humanact12_gru.tar')).
        ``recognizer``: an already built HipActionRecognizer (then ``datapath`` is not read).  Other keywords (dist_sync_on_step, ...) are accepted and
        ignored."""
        self.name = "matching, fid, and diversity scores"
        self.num_labels = num_labels
        self.diversity_times = diversity_times
        self.multimodality_times = multimodality_times
        self.recognizer = recognizer if recognizer is not None else HipActionRecognizer(datapath)
        self.metrics = list(self.METRICS)
        self.reset()

    def reset(self):
        self.count = torch.tensor(0)
        self.count_seq = torch.tensor(0)
        for m in self.metrics:
            setattr(self, m, torch.tensor(0.))
        self.confusion = torch.zeros(self.num_labels, self.num_labels, dtype=torch.long)
        self.gt_confusion = torch.zeros(self.num_labels, self.num_labels, dtype=torch.long)
        self.label_embeddings: List[Tensor] = []
        self.recmotion_embeddings: List[Tensor] = []
        self.gtmotion_embeddings: List[Tensor] = []

    def to(self, device):
        self.recognizer.to(device)
        return self

    def compute(self, sanity_flag):
        metrics = {m: getattr(self, m) for m in self.metrics}
        if sanity_flag:
            return metrics
        self.accuracy = torch.trace(self.confusion) / torch.sum(self.confusion)
        self.gt_accuracy = torch.trace(self.gt_confusion) / torch.sum(self.gt_confusion)
        all_labels = torch.cat(self.label_embeddings, axis=0)
        all_gen = torch.cat(self.recmotion_embeddings, axis=0)
        all_gt = torch.cat(self.gtmotion_embeddings, axis=0)
        all_gt2 = all_gt.clone()[torch.randperm(all_gt.shape[0]), :]
        genstats = calculate_activation_statistics(all_gen)
        gtstats = calculate_activation_statistics(all_gt)
        gtstats2 = calculate_activation_statistics(all_gt2)
        all_labels = all_labels.cpu()
        self.Diversity, self.Multimodality = calculate_diversity_multimodality(all_gen, all_labels, self.num_labels, diversity_times=self.diversity_times,
                                                                               multimodality_times=self.multimodality_times)
        self.gt_Diversity, self.gt_Multimodality = calculate_diversity_multimodality(all_gt, all_labels, self.num_labels)
        metrics.update({m: getattr(self, m) for m in self.metrics})
        metrics["FID"] = calculate_fid(gtstats, genstats)
        metrics["gt_FID"] = calculate_fid(gtstats, gtstats2)
        return {**metrics}

    @torch.no_grad()
    def update(self, label: Tensor, recmotion: Tensor, gtmotion: Tensor, lengths: List[int]):
        self.count += sum(lengths)
        self.count_seq += len(lengths)
        labels = label.squeeze().long()
        B = recmotion.shape[0]
        # the reference's four forward calls each draw their initial state: classifier(rec), classifier(gt), FID net(rec), FID net(gt)
        h0 = [torch.randn(2, B, 128, requires_grad=False) for _ in range(4)]
        rec, gt = HipActionRecognizer.to_joints(recmotion), HipActionRecognizer.to_joints(gtmotion)
        lens = [int(n) for n in lengths]
        logits, act = self.recognizer.recognize(torch.cat([rec, gt, rec, gt]), lens * 4, torch.cat(h0, dim=1).to(rec.device))
        batch_pred = logits[:B].max(dim=1).indices.cpu()
        gt_batch_pred = logits[B:2 * B].max(dim=1).indices.cpu()
        for lab, pred in zip(labels.cpu(), batch_pred):
            self.confusion[lab][pred] += 1
        for lab, pred in zip(labels.cpu(), gt_batch_pred):
            self.gt_confusion[lab][pred] += 1
        self.label_embeddings.append(labels)
        self.recmotion_embeddings.append(act[2 * B:3 * B])
        self.gtmotion_embeddings.append(act[3 * B:])


class HipUESTCMetrics(HipHUMANACTMetrics):
    """A drop-in for UESTCMetrics: ``update(label, recmotion [B, 24, 6, T], gtmotion, lengths)`` / ``compute(sanity_flag)``, the same state names and the
    eight metric keys.  ``compute`` is HUMANACTMetrics' own -- the reference's two classes share it line for line, the ground-truth diversity call with
    the helper's default repeat counts included -- on the 256-d features.  ``lengths`` only feed ``count``: the net has no mask (every frame counts, as
    in the reference)."""

    def __init__(self, datapath: Optional[str] = None, num_labels: int = 40, diversity_times: int = 200, multimodality_times: int = 20,
                 recognizer: Optional[HipStgcnRecognizer] = None, **kw):
        """``datapath``: uestc_rot6d_stgcn.tar or the directory holding it (cfg.model.uestc_rec_path).  ``recognizer``: an already built
        HipStgcnRecognizer (then ``datapath`` is not read).  Other keywords (cfg, dist_sync_on_step, ...) are accepted and ignored."""
        super().__init__(num_labels=num_labels, diversity_times=diversity_times, multimodality_times=multimodality_times,
                         recognizer=recognizer if recognizer is not None else HipStgcnRecognizer(datapath, num_class=num_labels))

    @torch.no_grad()
    def update(self, label: Tensor, recmotion: Tensor, gtmotion: Tensor, lengths: List[int]):
        self.count += sum(lengths)
        self.count_seq += len(lengths)
        labels = label.squeeze().long()
        B = recmotion.shape[0]
        yhat, feat = self.recognizer.recognize(torch.cat([recmotion, gtmotion]))      # generated + ground truth: one engine call
        feat = feat.reshape(2 * B, -1)
        batch_pred = yhat[:B].max(dim=1).indices.cpu()
        gt_batch_pred = yhat[B:].max(dim=1).indices.cpu()
        for lab, pred in zip(labels.cpu().reshape(-1), batch_pred):
            self.confusion[lab][pred] += 1
        for lab, pred in zip(labels.cpu().reshape(-1), gt_batch_pred):
            self.gt_confusion[lab][pred] += 1
        self.label_embeddings.append(labels)
        self.recmotion_embeddings.append(feat[:B].squeeze())
        self.gtmotion_embeddings.append(feat[B:].squeeze())


class HipTM2TMetrics:
    """A drop-in for the reference's TM2TMetrics (mld/models/metrics/tm2t.py; METRIC.TYPE ['TM2TMetrics'] of every text config): ``update(text_embeddings,
    recmotion_embeddings, gtmotion_embeddings, lengths)`` / ``compute(sanity_flag)``, the state names and the 11 metric keys (at ``top_k`` 3), on embeddings
    that stay on the device: the grouped retrieval, the activation statistics and the pair distances run in libmldhip (``HipMetricOps``; include/mldhip.h has
    the math).  A plain class (torchmetrics is not a dependency): no reduction across ranks.

    ``compute`` consumes random draws in the reference's order, so under the same seeds the numbers are the reference's: torch.randperm(count_seq) on the CPU
    generator (the three sets are gathered by it on the device); then np.random.choice(N, diversity_times, replace=False) twice for the generated set and
    twice for the ground truth.  The matrix square root of the FID stays on the host (``calculate_frechet_distance`` on the float64 casts of the statistics,
    ground truth first).  ``Matching_score`` / ``gt_Matching_score`` accumulate until ``reset()``, as the reference's states do."""

    def __init__(self, top_k: int = 3, R_size: int = 32, diversity_times: int = 300, ops=None, **kw):
        """``ops``: an already built HipMetricOps (e.g. ``MLD.metric_ops``, which shares the model's handle); None builds a stand-alone one.  Other keywords
        (dist_sync_on_step, ...) are accepted and ignored."""
        self.name = "matching, fid, and diversity scores"
        self.top_k = top_k
        self.R_size = R_size
        self.diversity_times = diversity_times
        self.ops = ops if ops is not None else HipMetricOps()
        self.Matching_metrics = ["Matching_score", "gt_Matching_score"] + [f"R_precision_top_{k}" for k in range(1, top_k + 1)] \
            + [f"gt_R_precision_top_{k}" for k in range(1, top_k + 1)]
        self.metrics = self.Matching_metrics + ["FID", "Diversity", "gt_Diversity"]
        self.reset()

    def reset(self):
        self.count = torch.tensor(0)
        self.count_seq = torch.tensor(0)
        for m in self.metrics:
            setattr(self, m, torch.tensor(0.))
        self.text_embeddings: List[Tensor] = []
        self.recmotion_embeddings: List[Tensor] = []
        self.gtmotion_embeddings: List[Tensor] = []

    def to(self, device):
        self.ops.to(device)
        for name in ("text_embeddings", "recmotion_embeddings", "gtmotion_embeddings"):
            setattr(self, name, [t.to(device) for t in getattr(self, name)])
        return self

    def _match(self, texts: Tensor, motions: Tensor):
        """(sum of the groups' traces, top-k hit counts [top_k]) of one pass of the reference's group loop"""
        rank, diag = self.ops.match(texts, motions, self.R_size)
        hits = torch.stack([(rank <= k).sum() for k in range(self.top_k)]).cpu().float()
        return diag.sum().cpu(), hits

    def _diversity(self, x: Tensor):
        n = x.shape[0]
        assert n > self.diversity_times
        first = np.random.choice(n, self.diversity_times, replace=False)
        second = np.random.choice(n, self.diversity_times, replace=False)
        return self.ops.pair_dist(x, first, second).cpu().numpy().mean()

    @torch.no_grad()
    def compute(self, sanity_flag):
        count_seq = self.count_seq.item()
        metrics = {m: getattr(self, m) for m in self.metrics}
        if sanity_flag:
            return metrics
        shuffle_idx = torch.randperm(count_seq)
        dev = self.text_embeddings[0].device
        idx = shuffle_idx.to(dev)
        all_texts = torch.cat(self.text_embeddings, axis=0).float()[idx, :].contiguous()
        all_gen = torch.cat(self.recmotion_embeddings, axis=0).float()[idx, :].contiguous()
        all_gt = torch.cat(self.gtmotion_embeddings, axis=0).float()[idx, :].contiguous()
        assert count_seq > self.R_size
        R_count = count_seq // self.R_size * self.R_size
        trace, hits = self._match(all_texts, all_gen)
        self.Matching_score = self.Matching_score + trace
        metrics["Matching_score"] = self.Matching_score / R_count
        for k in range(self.top_k):
            metrics[f"R_precision_top_{k + 1}"] = hits[k] / R_count
        trace, hits = self._match(all_texts, all_gt)
        self.gt_Matching_score = self.gt_Matching_score + trace
        metrics["gt_Matching_score"] = self.gt_Matching_score / R_count
        for k in range(self.top_k):
            metrics[f"gt_R_precision_top_{k + 1}"] = hits[k] / R_count
        mu, cov = (t.cpu().numpy().astype(np.float64) for t in self.ops.stats(all_gen))
        gt_mu, gt_cov = (t.cpu().numpy().astype(np.float64) for t in self.ops.stats(all_gt))
        metrics["FID"] = calculate_frechet_distance(gt_mu, gt_cov, mu, cov)
        assert count_seq > self.diversity_times
        metrics["Diversity"] = self._diversity(all_gen)
        metrics["gt_Diversity"] = self._diversity(all_gt)
        return {**metrics}

    @torch.no_grad()
    def update(self, text_embeddings: Tensor, recmotion_embeddings: Tensor, gtmotion_embeddings: Tensor, lengths: List[int]):
        self.count += sum(lengths)
        self.count_seq += len(lengths)
        self.text_embeddings.append(torch.flatten(text_embeddings, start_dim=1).detach())
        self.recmotion_embeddings.append(torch.flatten(recmotion_embeddings, start_dim=1).detach())
        self.gtmotion_embeddings.append(torch.flatten(gtmotion_embeddings, start_dim=1).detach())


class HipMMMetrics:
    """A drop-in for the reference's MMMetrics (mld/models/metrics/mm.py): ``update(mm_motion_embeddings [1, reps, D], lengths)`` / ``compute(sanity_flag)``
    -> {'MultiModality'}.  ``compute`` makes the reference's two np.random.choice(reps, mm_num_times, replace=False) draws and runs ONE ``mldhip_pair_dist``
    call of n x mm_num_times pairs on the flattened [n reps, D] rows."""

    def __init__(self, mm_num_times: int = 10, ops=None, **kw):
        self.name = "MultiModality scores"
        self.mm_num_times = mm_num_times
        self.ops = ops if ops is not None else HipMetricOps()
        self.metrics = ["MultiModality"]
        self.reset()

    def reset(self):
        self.count = torch.tensor(0)
        self.count_seq = torch.tensor(0)
        self.MultiModality = torch.tensor(0.)
        self.mm_motion_embeddings: List[Tensor] = []

    def to(self, device):
        self.ops.to(device)
        self.mm_motion_embeddings = [t.to(device) for t in self.mm_motion_embeddings]
        return self

    @torch.no_grad()
    def compute(self, sanity_flag):
        metrics = {m: getattr(self, m) for m in self.metrics}
        if sanity_flag:
            return metrics
        x = torch.cat(self.mm_motion_embeddings, axis=0).float()
        assert x.dim() == 3
        n, reps, D = x.shape
        assert reps > self.mm_num_times
        first = np.random.choice(reps, self.mm_num_times, replace=False)
        second = np.random.choice(reps, self.mm_num_times, replace=False)
        base = np.arange(n)[:, None] * reps
        dist = self.ops.pair_dist(x.reshape(n * reps, D).contiguous(), (base + first[None, :]).reshape(-1), (base + second[None, :]).reshape(-1))
        metrics["MultiModality"] = dist.cpu().numpy().reshape(n, self.mm_num_times).mean()
        return {**metrics}

    def update(self, mm_motion_embeddings: Tensor, lengths: List[int]):
        self.count += sum(lengths)
        self.count_seq += len(lengths)
        self.mm_motion_embeddings.append(mm_motion_embeddings)
