"""``HipT2MEvaluator`` (below), ``HipActionRecognizer`` (the HumanAct12 recognition GRU behind mld_hip.metrics.HipHUMANACTMetrics) and ``HipStgcnRecognizer``
(the UESTC recognition ST-GCN behind mld_hip.metrics.HipUESTCMetrics; both behind it), and ``HipMetricOps`` (the metric kernels behind
mld_hip.metrics.HipTM2TMetrics / HipMMMetrics; at the end of this file).

``HipT2MEvaluator`` -- the pretrained T2M evaluator nets of a checkpoint (``t2m_moveencoder`` / ``t2m_motionencoder`` / ``t2m_textencoder``:
mld/models/architectures/t2m_motionenc.py, t2m_textenc.py; instantiated at mld/models/modeltype/mld.py:110-140) as one drop-in module whose arithmetic
runs in libmldhip (``mldhip_t2m_motion_embed`` / ``mldhip_t2m_text_embed``; include/mldhip.h has the math).

Opt-in: ``load_config(overrides={"model.t2m_evaluator.target": "mld_hip.evaluators.HipT2MEvaluator"})``.  Without it ``MLD`` keeps dropping the ``t2m_*`` keys of a
checkpoint; with it ``MLD.load_state_dict`` loads them strictly and ``MLD.t2m_eval`` returns the embeddings the T2M metrics are computed from."""
from __future__ import annotations

import os
import warnings
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import engine as _engine
from . import synthetic as syn
from ._module import HipModule


class HipT2MEvaluator(HipModule):
    _prefix = ""            # the parameters carry the checkpoint's own names: t2m_moveencoder.main.0.weight, ...

    def __init__(self, nfeats: int = syn.NFEATS, seed: int = 5, **_):
        super().__init__()
        self.nfeats = int(nfeats)
        self._register_tree(syn.make_t2m_state_dict(seed, self.nfeats))     # shapes (and seeded values until a checkpoint is loaded)
        self._set_arch("text", t2m_eval=1, nfeats=self.nfeats)
        # mean_eval / std_eval belong to the motion tower's weight group (all-or-nothing with the t2m_* tensors), so this module uploads them with its parameters;
        # MLD hands over its datamodule's pair, the seeded synthetic pair stands in until then
        self.stats_eval = syn.make_mean_std_eval(self.nfeats)

    def sync_weights(self):
        eng = self.engine
        owners = eng.__dict__.setdefault("_owner", {})
        if owners.get("mean_eval/std_eval") != (id(self), id(self.stats_eval)):
            eng.load_tensor("mean_eval", self.stats_eval[0])
            eng.load_tensor("std_eval", self.stats_eval[1])
            eng._dirty = True
            owners["mean_eval/std_eval"] = (id(self), id(self.stats_eval))
        return super().sync_weights()

    @staticmethod
    def capacity(eng) -> int:
        return int(eng.cfg.t2m_max_motions) or 2 * int(eng.cfg.max_batch)

    @torch.no_grad()
    def motion_embed(self, feats: torch.Tensor, lengths: Sequence[int], renorm: bool = True) -> torch.Tensor:
        """feats [B, T, nfeats] (the model's normalisation; ``renorm=False``: already the evaluators') -> [B, 512], rows in the caller's order"""
        f = self._check(feats, "feats")
        eng = self.sync_weights()
        out = torch.empty(f.shape[0], 512, dtype=torch.float32, device=f.device)
        eng.t2m_motion_embed(f, [int(n) for n in lengths], f.shape[1], out, renorm=renorm, stream=_engine.current_stream_handle(f))
        return out

    @torch.no_grad()
    def text_embed(self, word_embs: torch.Tensor, pos_ohot: torch.Tensor, text_lengths: Sequence[int]) -> torch.Tensor:
        """word_embs [B, L, 300], pos_ohot [B, L, 15] -> [B, 512], rows in the caller's order"""
        w, p = self._check(word_embs, "word_embs"), self._check(pos_ohot, "pos_ohot")
        eng = self.sync_weights()
        out = torch.empty(w.shape[0], 512, dtype=torch.float32, device=w.device)
        eng.t2m_text_embed(w, p, [int(n) for n in text_lengths], w.shape[1], out, stream=_engine.current_stream_handle(w))
        return out


def _find_rec_file(path):
    if not path:
        return None
    if os.path.isfile(path):
        return path
    f = os.path.join(path, "humanact12_gru.tar")
    return f if os.path.isfile(f) else None


class HipActionRecognizer(HipModule):
    """The pretrained HumanAct12 recognition GRU (``humanact12_gru.tar``: MotionDiscriminator(72, 128, 2, 12) / MotionDiscriminatorForFID,
    mld/models/architectures/humanact12_gru.py) as one module whose arithmetic runs in libmldhip (``mldhip_a2m_recognize``; include/mldhip.h has the math,
    the padded-frame rule and the h0 contract).  Parameters carry the file's own names (``recurrent.weight_ih_l0``, ..., ``linear2.bias``).

    ``humanact12_rec_path`` (cfg.model.humanact12_rec_path, or the file itself) with a ``humanact12_gru.tar`` in it fills them from the file's ``model``;
    otherwise they hold ``mld_hip.synthetic.make_a2m_rec_state_dict`` -- a seeded stand-in at PyTorch's default init ranges, since no such file ships with
    this repository -- and ``source`` says which; a path that holds no such file gets a ``RuntimeWarning`` saying so."""
    _prefix = "a2m_rec."

    def __init__(self, humanact12_rec_path: Optional[str] = None, seed: int = 12, tensors: Optional[Dict[str, object]] = None, **_):
        super().__init__()
        path = _find_rec_file(humanact12_rec_path) if tensors is None else None
        if tensors is not None:
            self.source = "tensors"
        elif path is not None:
            tensors, self.source = torch.load(path, map_location="cpu")["model"], path
        else:
            if humanact12_rec_path:
                warnings.warn(f"HipActionRecognizer: no humanact12_gru.tar under humanact12_rec_path={humanact12_rec_path!r}; the weights are the seeded "
                              "synthetic stand-in (source == 'synthetic'), so its classes and activations are not the pretrained net's", RuntimeWarning, stacklevel=2)
            tensors, self.source = syn.make_a2m_rec_state_dict(seed), "synthetic"
        want = syn.make_a2m_rec_state_dict(seed)
        for k, v in want.items():
            if k not in tensors or tuple(np.shape(tensors[k])) != v.shape:
                raise ValueError(f"HipActionRecognizer: {k} {tuple(v.shape)} expected (include/mldhip.h)")
        self._register_tree({k: np.asarray(torch.as_tensor(tensors[k]).float().cpu().numpy(), np.float32) for k in want})
        self._set_arch("action", a2m_rec=1)

    @staticmethod
    def capacity(eng) -> int:
        return int(eng.cfg.a2m_max_motions) or 4 * int(eng.cfg.max_batch)

    @torch.no_grad()
    def recognize(self, joints: torch.Tensor, lengths: Sequence[int], h0: Optional[torch.Tensor] = None):
        """joints [B, T, 72] (mldhip_smpl_forward's joints, feature 3 joint + coord), lengths [B], h0 [2, B, 128] (None: zeros) -> (logits [B, 12],
        activations [B, 30]); a batch beyond the engine's capacity goes through in slices (a motion's rows do not depend on its neighbours)"""
        j = self._check(joints, "joints")
        if j.dim() != 3 or j.shape[2] != 72:
            raise ValueError(f"joints must be [B, T, 72], got {tuple(j.shape)}")
        lengths = [int(n) for n in lengths]
        B, T = j.shape[:2]
        if len(lengths) != B:
            raise ValueError("one length per motion")
        if h0 is not None:
            h0 = self._check(h0.to(j.device), "h0")
            if tuple(h0.shape) != (2, B, 128):
                raise ValueError(f"h0 must be [2, B, 128], got {tuple(h0.shape)}")
        eng = self.sync_weights()
        logits = torch.empty(B, 12, dtype=torch.float32, device=j.device)
        act = torch.empty(B, 30, dtype=torch.float32, device=j.device)
        stream = _engine.current_stream_handle(j)
        step = self.capacity(eng)
        for b0 in range(0, B, step):
            sl = slice(b0, min(B, b0 + step))
            h = None if h0 is None else (h0 if step >= B else h0[:, sl].contiguous())
            eng.a2m_recognize(j[sl], lengths[sl], T, h, logits[sl], act[sl], stream)
        return logits, act

    @staticmethod
    def to_joints(motion: torch.Tensor) -> torch.Tensor:
        """the reference's [B, 24, 3, T] -> [B, T, 72]"""
        B, J, C, T = motion.shape
        return motion.reshape(B, J * C, T).permute(0, 2, 1).float().contiguous()

    def forward(self, motion_sequence: torch.Tensor, lengths=None, hidden_unit: Optional[torch.Tensor] = None, fid: bool = False):
        """MotionDiscriminator.forward (``fid``: MotionDiscriminatorForFID.forward): motion [B, 24, 3, T], lengths [B]; without ``hidden_unit`` the initial
        state is drawn as the reference draws it, torch.randn(2, B, 128) on the CPU default generator"""
        B, T = motion_sequence.shape[0], motion_sequence.shape[3]
        if hidden_unit is None:
            hidden_unit = torch.randn(2, B, 128, requires_grad=False)
        lengths = [T] * B if lengths is None else [int(n) for n in lengths]
        logits, act = self.recognize(self.to_joints(motion_sequence), lengths, hidden_unit.float())
        return act if fid else logits


def _find_stgcn_file(path):
    if not path:
        return None
    if os.path.isfile(path):
        return path
    f = os.path.join(path, "uestc_rot6d_stgcn.tar")
    return f if os.path.isfile(f) else None


class HipStgcnRecognizer(HipModule):
    """The pretrained UESTC recognition ST-GCN (``uestc_rot6d_stgcn.tar``: STGCN(in_channels 6, num_class 40, layout 'smpl', strategy 'spatial', edge
    importance on), mld/models/architectures/uestc_stgcn.py) as one module whose arithmetic runs in libmldhip (``mldhip_uestc_recognize``; include/mldhip.h
    has the math).  Parameters carry the file's own names (``A``, ``data_bn.weight``, ``st_gcn_networks.0.gcn.conv.weight``, ..., ``fcn.bias``); the
    ``num_batches_tracked`` scalars of the file are dropped.  ``A`` is the file's registered buffer: no ``kintree_table.pkl`` is read.

    ``uestc_rec_path`` (cfg.model.uestc_rec_path, or the file itself) with a ``uestc_rot6d_stgcn.tar`` in it fills them from the file (the state dict
    itself, as the reference saves it); otherwise they hold ``mld_hip.synthetic.make_uestc_rec_state_dict`` -- a seeded stand-in, since no such file
    ships with this repository -- and ``source`` says which; a path that holds no such file gets a ``RuntimeWarning`` saying so.

    THE NET HAS NO LENGTHS (the reference leaves a "TODO: use mask"): every frame of the [B, 24, 6, T] input, padded ones included, counts."""
    _prefix = "uestc_rec."

    def __init__(self, uestc_rec_path: Optional[str] = None, seed: int = 13, num_class: int = syn.UESTC_CLASSES, tensors: Optional[Dict[str, object]] = None, **_):
        super().__init__()
        path = _find_stgcn_file(uestc_rec_path) if tensors is None else None
        if tensors is not None:
            self.source = "tensors"
        elif path is not None:
            tensors, self.source = torch.load(path, map_location="cpu"), path
            if "fcn.weight" in tensors:
                num_class = int(np.shape(tensors["fcn.weight"])[0])
        else:
            if uestc_rec_path:
                warnings.warn(f"HipStgcnRecognizer: no uestc_rot6d_stgcn.tar under uestc_rec_path={uestc_rec_path!r}; the weights are the seeded "
                              "synthetic stand-in (source == 'synthetic'), so its classes and features are not the pretrained net's", RuntimeWarning, stacklevel=2)
            tensors, self.source = syn.make_uestc_rec_state_dict(seed, num_class), "synthetic"
        want = syn.uestc_rec_shapes(num_class)
        for k, shape in want.items():
            if k not in tensors or tuple(np.shape(tensors[k])) != shape:
                raise ValueError(f"HipStgcnRecognizer: {k} {shape} expected (include/mldhip.h)")
        self.num_class = num_class
        self._register_tree({k: np.asarray(torch.as_tensor(tensors[k]).float().cpu().numpy(), np.float32) for k in want})      # (num_batches_tracked is not in `want`)
        # (the config's default 0 MEANS 40: a 40-class net asks for nothing, so it also fits an engine created with the default)
        self._set_arch("action", uestc_rec=1, **({} if num_class == syn.UESTC_CLASSES else {"uestc_classes": num_class}))

    @staticmethod
    def capacity(eng) -> int:
        return int(eng.cfg.uestc_max_motions) or 2 * int(eng.cfg.max_batch)

    @torch.no_grad()
    def recognize(self, motion: torch.Tensor):
        """motion: any 4-d float32 [B, 24, 6, T] tensor with positive strides (MLD's view of its feature rows goes in as it is: ``.stride()`` is passed
        through, nothing is copied) -> (yhat [B, NC], features [B, 256]; [256] at B = 1, the reference's ``squeeze()``); a batch beyond the engine's
        capacity goes through in slices (a motion's rows do not depend on its neighbours)"""
        if motion.dim() != 4 or motion.shape[1] != 24 or motion.shape[2] != 6:
            raise ValueError(f"motion must be [B, 24, 6, T], got {tuple(motion.shape)}")
        if motion.dtype != torch.float32:
            raise TypeError(f"motion: float32 expected, got {motion.dtype}")
        if min(motion.stride()) < 1:
            motion = motion.contiguous()      # (an expanded dimension has stride 0)
        B, T = motion.shape[0], motion.shape[3]
        eng = self.sync_weights()
        yhat = torch.empty(B, self.num_class, dtype=torch.float32, device=motion.device)
        feat = torch.empty(B, syn.UESTC_FEAT, dtype=torch.float32, device=motion.device)
        stream = _engine.current_stream_handle(motion)
        step = self.capacity(eng)
        for b0 in range(0, B, step):
            sl = slice(b0, min(B, b0 + step))
            eng.uestc_recognize(motion[sl], motion.stride(), sl.stop - b0, T, yhat[sl], feat[sl], stream)
        return yhat, feat.squeeze()

    def forward(self, motion: torch.Tensor):
        """STGCN.forward: {'output': motion, 'features': ..., 'yhat': ...}"""
        yhat, feat = self.recognize(motion)
        return {"output": motion, "features": feat, "yhat": yhat}


class HipMetricOps(HipModule):
    """The device-shaped parts of the text-to-motion metrics (``mldhip_t2m_match`` / ``mldhip_act_stats`` / ``mldhip_pair_dist``; include/mldhip.h has
    the math) on float32 embeddings that stay on the device.  A module WITHOUT weights: nothing is uploaded and nothing is finalized.

    Inside an ``MLD`` (cfg.model.metric_ops.target = mld_hip.evaluators.HipMetricOps) it shares the model's handle; stand-alone it gets a small handle of
    its own on the device of the first tensor it is given.  ``metrics_max_rows`` (0: the engine's default, 8192) is the capacity of a call: inputs beyond
    it raise ``ValueError`` -- there is no silent slicing, a covariance cannot be sliced."""
    DEFAULT_ROWS = 8192

    def __init__(self, metrics_max_rows: int = 0, **_):
        super().__init__()
        self._set_arch("text", t2m_metrics=1, **({"metrics_max_rows": int(metrics_max_rows)} if metrics_max_rows else {}))

    def engine_of(self, t: torch.Tensor):
        """the handle a call on tensor ``t`` runs on: the injected one, the model's (inside an ``MLD``), or this module's own small one on ``t``'s device"""
        if self._engine_key is not None:
            eng = _engine.get_engine(self._engine_key)
        else:
            own = {} if self._shared_arch else dict(num_layers=3, max_batch=1, max_frames=16)      # stand-alone: a small handle (the diffusion model is never loaded)
            eng = _engine.get_engine(t.device, self._variant, want={**self._shared_arch, **self._arch}, **own)
        _engine.check_arch(eng, type(self).__name__, **self._arch)
        return eng

    @staticmethod
    def capacity(eng) -> int:
        return int(eng.cfg.metrics_max_rows) or HipMetricOps.DEFAULT_ROWS

    def _rows(self, eng, x: torch.Tensor, name: str) -> torch.Tensor:
        x = self._check(x, name)
        if x.dim() != 2 or not 1 <= x.shape[1] <= 1024:
            raise ValueError(f"{name} must be [N, D] with 1 <= D <= 1024, got {tuple(x.shape)}")
        if x.shape[0] > self.capacity(eng):
            raise ValueError(f"{name}: {x.shape[0]} rows exceed the engine's metrics_max_rows={self.capacity(eng)} (mldhip_config.metrics_max_rows)")
        return x

    @torch.no_grad()
    def match(self, text: torch.Tensor, motion: torch.Tensor, R: int = 32):
        """text, motion [N, D] -> (rank [G R] int32, diag [G R] float32) with G = N // R: the rank of each row's own motion among its group's and its distance"""
        eng = self.engine_of(text)
        t, m = self._rows(eng, text, "text"), self._rows(eng, motion.to(text.device), "motion")
        if t.shape != m.shape:
            raise ValueError(f"text {tuple(t.shape)} and motion {tuple(m.shape)} must have one shape")
        N, D = t.shape
        n = N // R * R
        rank = torch.empty(n, dtype=torch.int32, device=t.device)
        diag = torch.empty(n, dtype=torch.float32, device=t.device)
        eng.t2m_match(t, m, N, D, R, rank, diag, _engine.current_stream_handle(t))
        return rank, diag

    @torch.no_grad()
    def stats(self, x: torch.Tensor):
        """x [N, D] -> (mean [D], unbiased covariance [D, D]) on the device"""
        eng = self.engine_of(x)
        x = self._rows(eng, x, "x")
        N, D = x.shape
        if N < 2:
            raise ValueError("a covariance needs at least two rows")
        mean = torch.empty(D, dtype=torch.float32, device=x.device)
        cov = torch.empty(D, D, dtype=torch.float32, device=x.device)
        eng.act_stats(x, N, D, mean, cov, _engine.current_stream_handle(x))
        return mean, cov

    @torch.no_grad()
    def pair_dist(self, x: torch.Tensor, a: Sequence[int], b: Sequence[int]):
        """x [N, D], host index lists a, b [P] -> ||x[a[p]] - x[b[p]]|| [P] on the device"""
        eng = self.engine_of(x)
        x = self._rows(eng, x, "x")
        if len(a) > self.capacity(eng):
            raise ValueError(f"{len(a)} pairs exceed the engine's metrics_max_rows={self.capacity(eng)} (mldhip_config.metrics_max_rows)")
        out = torch.empty(len(a), dtype=torch.float32, device=x.device)
        eng.pair_dist(x, x.shape[0], x.shape[1], a, b, out, _engine.current_stream_handle(x))
        return out
