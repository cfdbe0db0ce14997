"""Minimal stand-in for ``HumanML3DDataModule`` / ``KitDataModule`` (mld/data/HumanML3D.py:11-75, mld/data/Kit.py): the sampling path only needs
``nfeats``, ``njoints``, the normalisation vectors and ``feats2joints`` -- and the reference's datamodule
cannot even be constructed without the full dataset, GloVe and pytorch_lightning."""
from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch

from . import engine as _engine
from . import synthetic as syn


# name -> (nfeats, njoints, the key of its block under cfg.DATASET); the first two have recover_from_ric joints (12 x njoints - 1 features)
_LAYOUTS = {"humanml3d": (263, 22, "HUMANML3D"), "kit": (251, 21, "KIT"), "humanact12": (150, 25, "HUMANACT12")}


def _from_cfg(cfg, *path):
    try:
        for k in path:
            cfg = cfg[k]
        return cfg
    except Exception:
        return None


class HipDataModule:
    name = "humanml3d"

    def __init__(self, cfg=None, mean: Optional[np.ndarray] = None, std: Optional[np.ndarray] = None,
                 nfeats: Optional[int] = None, njoints: Optional[int] = None, engine_key: Optional[str] = None, name: Optional[str] = None,
                 nclasses: int = 12, variant: Optional[str] = None, mean_eval: Optional[np.ndarray] = None, std_eval: Optional[np.ndarray] = None):
        """name 'humanml3d' (263-d features, 22 joints), 'kit' (KIT-ML: 251-d features, 21 joints; mld/data/Kit.py) or 'humanact12' (rot6d 25x6 =
        150-d features, 12 classes; mld/data/HumanAct12.py) -- the last only carries shapes: its feats2joints needs SMPL.  What is not passed comes
        from `cfg`: the name from TEST.DATASETS[0] (how the reference's get_data.py picks the datamodule), the widths from DATASET.NFEATS / NJOINTS
        (which the reference fills from the datamodule at run time); without a cfg, the layout's own."""
        if name is None:
            ds = _from_cfg(cfg, "TEST", "DATASETS")
            name = str(ds[0]).lower() if ds and str(ds[0]).lower() in _LAYOUTS else "humanml3d"
        layout = _LAYOUTS.get(name, _LAYOUTS["humanml3d"])
        if nfeats is None:
            nfeats = _from_cfg(cfg, "DATASET", "NFEATS") or layout[0]
        if njoints is None:
            njoints = _from_cfg(cfg, "DATASET", "NJOINTS") or layout[1]
        self.name, self.nclasses = name, nclasses
        self.variant = variant          # engine registry variant; filled in by MLD when left None
        self.nfeats, self.njoints = int(nfeats), int(njoints)
        # mldhip_config fields this datamodule implies (MLD merges them into the model's shared fields): the skeleton feats2joints recovers
        self._arch = {"nfeats": self.nfeats, "njoints": self.njoints} if name != "humanact12" else {}
        if mean is None or std is None:
            root = _from_cfg(cfg, "DATASET", layout[2], "ROOT")
            if root and os.path.exists(os.path.join(root, "Mean.npy")):      # get_data.py:38-40
                mean = np.load(os.path.join(root, "Mean.npy"))
                std = np.load(os.path.join(root, "Std.npy"))
                self.stats = "dataset"
            else:
                mean, std = syn.make_mean_std(nfeats)
                self.stats = "synthetic"
        self.mean = np.asarray(mean, np.float32)
        self.std = np.asarray(std, np.float32)
        # the T2M evaluators' own statistics (get_data.py:86: get_mean_std("val", ...)): mean_eval.npy / std_eval.npy beside Mean.npy where they exist, synthetic otherwise
        if mean_eval is None or std_eval is None:
            root = _from_cfg(cfg, "DATASET", layout[2], "ROOT")
            if root and os.path.exists(os.path.join(root, "mean_eval.npy")) and os.path.exists(os.path.join(root, "std_eval.npy")):
                mean_eval, std_eval = np.load(os.path.join(root, "mean_eval.npy")), np.load(os.path.join(root, "std_eval.npy"))
            else:
                mean_eval, std_eval = syn.make_mean_std_eval(nfeats)
        self.mean_eval = np.asarray(mean_eval, np.float32)
        self.std_eval = np.asarray(std_eval, np.float32)
        self.hparams = type("H", (), {"mean": self.mean, "std": self.std, "mean_eval": self.mean_eval, "std_eval": self.std_eval})()
        self._engine_key = engine_key
        self._shared_arch = {}          # architecture fields of the model this datamodule serves (set by MLD)
        self._loaded_on = None

    def _engine(self, device):
        eng = _engine.get_engine(self._engine_key if self._engine_key is not None else device, self.variant or "text",
                                 want={**self._arch, **self._shared_arch})
        owners = eng.__dict__.setdefault("_owner", {})           # see HipModule.sync_weights: engines are shared per architecture
        if self._loaded_on is not eng or owners.get("mean/std") != id(self):
            eng.load_tensor("mean", self.mean)
            eng.load_tensor("std", self.std)
            eng._dirty = True
            self._loaded_on = eng
            owners["mean/std"] = id(self)
        return eng

    def renorm4t2m(self, features: torch.Tensor) -> torch.Tensor:
        """HumanML3D.py:54-63 / Kit.py:49-58: the model's normalisation -> the T2M evaluators', on every frame (padded ones included)"""
        mean, std = torch.from_numpy(self.mean).to(features), torch.from_numpy(self.std).to(features)
        mean_eval, std_eval = torch.from_numpy(self.mean_eval).to(features), torch.from_numpy(self.std_eval).to(features)
        return (features * std + mean - mean_eval) / std_eval

    def feats2joints(self, features: torch.Tensor, mask=None) -> torch.Tensor:
        """[B, T, nfeats] -> [B, T, njoints, 3] (HumanML3D.py:41-45 / Kit.py: recover_from_ric with the datamodule's njoints), on the tensor's device."""
        if self.name not in ("humanml3d", "kit"):
            raise NotImplementedError(f"feats2joints of '{self.name}' maps rot6d features through the SMPL body model "
                                      "(mld/transforms/rots2joints/smplh.py); SMPL is an external asset and out of scope")
        if features.dtype != torch.float32:
            raise TypeError("feats2joints expects float32 features (recover_from_ric's index_put needs fp32)")
        f = features.contiguous()
        eng = self._engine(f.device)
        _engine.finalize_if_dirty(eng, _engine.current_stream_handle(f))
        out = torch.empty(*f.shape[:2], self.njoints, 3, dtype=torch.float32, device=f.device)
        eng.feats2joints(f, f.shape[0], f.shape[1], out, _engine.current_stream_handle(f))
        return out
