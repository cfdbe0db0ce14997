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
recognition ST-GCN (``HipStgcnRecognizer``; ``mldhip_uestc_recognize``): the net draws nothing, so ``update`` is one engine call on cat([rec, gt])."""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import scipy.linalg
import torch
from torch import Tensor

from .evaluators import HipActionRecognizer, HipStgcnRecognizer


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
