"""``HipSmpl`` -- the SMPL body model behind the action path's ``feats2joints`` / ``feats2joints_eval`` (the reference's ``Rotation2xyz`` over
``smplx.SMPLLayer``: mld/transforms/rotation2xyz.py:10-114, built at mld/models/modeltype/mld.py:118-143) as one drop-in module whose arithmetic runs
in libmldhip (``mldhip_smpl_forward``; include/mldhip.h has the math, the padded-frame rule and the fixed body shape).

Opt-in: ``load_config(cfg, overrides={"model.smpl.target": "mld_hip.smpl.HipSmpl"})``.  Without it an action ``MLD`` stays as it was: features only,
``feats2joints`` raises.  With it ``MLD`` sets ``feats2joints(sample, mask)`` (vertices, no translation) and ``feats2joints_eval(sample, mask)`` (24
joints, translation) as the reference does, and ``a2m_eval`` returns the joints entries of the reference's rs_set.

The module carries smplx's five buffers as parameters (``v_template`` [V, 3], ``posedirs`` [207, 3V], ``J_regressor`` [24, V], ``lbs_weights`` [V, 24],
``parents`` [24] as float32).  ``smpl_path`` with a ``SMPL_NEUTRAL.npz`` / ``SMPL_NEUTRAL.pkl`` in it (or such a file itself) fills them from the file;
otherwise they hold ``mld_hip.synthetic.make_smpl`` -- a seeded stand-in, since no SMPL file ships with this repository -- and ``source`` says which;
a ``smpl_path`` that holds no such file gets a ``RuntimeWarning`` saying so."""
from __future__ import annotations

import os
import warnings
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import engine as _engine
from . import synthetic as syn
from ._module import HipModule

JOINTSTYPES = ("a2m", "a2mpl", "smpl", "vibe", "vertices")      # rotation2xyz.py:7


def _find_file(smpl_path: Optional[str]) -> Optional[str]:
    if not smpl_path:
        return None
    if os.path.isfile(smpl_path):
        return smpl_path
    for name in ("SMPL_NEUTRAL.npz", "SMPL_NEUTRAL.pkl"):
        if os.path.isfile(os.path.join(smpl_path, name)):
            return os.path.join(smpl_path, name)
    return None


def _dense(x) -> np.ndarray:
    """a model file's array -> numpy: plain arrays, scipy sparse matrices (J_regressor) and chumpy arrays (``.r``)"""
    if hasattr(x, "toarray"):
        x = x.toarray()
    elif hasattr(x, "r") and not isinstance(x, np.ndarray):
        x = x.r
    return np.asarray(x)


def read_smpl_file(path: str) -> Dict[str, np.ndarray]:
    """``SMPL_NEUTRAL.npz`` / ``.pkl`` -> the engine's five tensors.  The file's ``posedirs`` [V, 3, 207] becomes smplx's buffer [207, 3V] (reshape to
    [3V, 207], transpose); ``kintree_table`` [2, 24] (row 0: the parent of each joint, 2^32 - 1 for the root) becomes ``parents`` with parents[0] = -1;
    ``shapedirs`` is not read (the body shape is fixed at betas = 0: add ``shapedirs @ betas`` to ``v_template`` for another one).
    The official .pkl pickles chumpy arrays and a scipy sparse matrix: unpickling needs both packages, and a clear error says so when they are missing.
    NOT verified against a real SMPL file: none is reachable offline; the npz path is tested on a file written in the same layout."""
    if path.endswith(".npz"):
        raw = dict(np.load(path, allow_pickle=False))
    else:
        import pickle
        try:
            with open(path, "rb") as f:
                raw = pickle.load(f, encoding="latin1")       # (like any pickle, a model file can run code on load: read only files you trust)
        except ModuleNotFoundError as e:
            raise RuntimeError(f"{path}: unpickling the official SMPL model needs the `{e.name}` package (it stores chumpy arrays and a scipy sparse "
                               "J_regressor); install it, or convert the file once to an .npz holding v_template, posedirs, J_regressor, weights and "
                               "kintree_table as plain arrays") from e
    need = ("v_template", "posedirs", "J_regressor", "weights", "kintree_table")
    missing = [k for k in need if k not in raw]
    if missing:
        raise KeyError(f"{path}: not an SMPL model file, missing {missing}")
    vt = _dense(raw["v_template"]).astype(np.float32)
    V = vt.shape[0]
    pd = _dense(raw["posedirs"]).astype(np.float32)
    if pd.shape != (V, 3, 207):
        raise ValueError(f"{path}: posedirs has shape {pd.shape}, expected {(V, 3, 207)}")
    parents = _dense(raw["kintree_table"]).astype(np.int64)[0].copy()
    parents[0] = -1
    return {"v_template": vt, "posedirs": np.ascontiguousarray(pd.reshape(3 * V, 207).T), "J_regressor": _dense(raw["J_regressor"]).astype(np.float32),
            "lbs_weights": _dense(raw["weights"]).astype(np.float32), "parents": parents.astype(np.float32)}


class HipSmpl(HipModule):
    _prefix = "smpl."

    def __init__(self, smpl_path: Optional[str] = None, V: int = 6890, seed: int = 11, dense: bool = False, tensors: Optional[Dict[str, np.ndarray]] = None, **_):
        super().__init__()
        path = _find_file(smpl_path) if tensors is None else None
        if tensors is not None:
            self.source = "tensors"
        elif path is not None:
            tensors, self.source = read_smpl_file(path), path
        else:
            if smpl_path:      # the opt-in node passes DATASET.SMPL_PATH: a missing file must not pass for a body (load_state_dict never replaces it)
                warnings.warn(f"HipSmpl: no SMPL_NEUTRAL.npz / SMPL_NEUTRAL.pkl under smpl_path={smpl_path!r}; the body is the seeded synthetic stand-in "
                              "(source == 'synthetic'), so its joints and vertices are not SMPL's", RuntimeWarning, stacklevel=2)
            tensors, self.source = syn.make_smpl(V, seed=seed, dense=dense), "synthetic"
        self.V = int(tensors["v_template"].shape[0])
        if tensors["posedirs"].shape != (207, 3 * self.V) or tensors["J_regressor"].shape != (24, self.V) or tensors["lbs_weights"].shape != (self.V, 24):
            raise ValueError("HipSmpl: posedirs [207, 3V], J_regressor [24, V] and lbs_weights [V, 24] expected (include/mldhip.h)")
        self._register_tree({k: np.asarray(tensors[k], np.float32) for k in ("v_template", "posedirs", "J_regressor", "lbs_weights", "parents")})
        self._set_arch("action", smpl_verts=self.V)

    @classmethod
    def from_files(cls, smpl_path: str) -> "HipSmpl":
        """The body of ``SMPL_NEUTRAL.npz`` / ``SMPL_NEUTRAL.pkl`` under ``smpl_path`` (cfg.DATASET.SMPL_PATH; or the file itself).  See ``read_smpl_file``:
        this path cannot be verified offline against a real model file."""
        path = _find_file(smpl_path)
        if path is None:
            raise FileNotFoundError(f"no SMPL_NEUTRAL.npz / SMPL_NEUTRAL.pkl under {smpl_path!r}")
        return cls(smpl_path=path)

    # ------------------------------------------------------------------ engine calls
    def _forward(self, feats: torch.Tensor, lengths: Sequence[int], joints: bool, flags: int) -> torch.Tensor:
        f = self._check(feats, "feats")
        if f.dim() != 3 or f.shape[2] != 150:
            raise ValueError(f"feats must be [B, T, 150] rot6d features (25 slots x 6), got {tuple(f.shape)}")
        lengths = [int(n) for n in lengths]
        if len(lengths) != f.shape[0]:
            raise ValueError("one length per motion")
        eng = self.sync_weights()
        B, T = f.shape[:2]
        out = torch.empty(B, T, 24 if joints else self.V, 3, dtype=torch.float32, device=f.device)
        stream = _engine.current_stream_handle(f)
        step = int(eng.cfg.max_batch)      # (a batch beyond the engine's capacity goes through in slices: a motion's rows do not depend on its neighbours)
        for b0 in range(0, B, step):
            sl = slice(b0, min(B, b0 + step))
            eng.smpl_forward(f[sl], lengths[sl], T, out[sl] if joints else None, None if joints else out[sl], flags, stream)
        return out

    @torch.no_grad()
    def joints(self, feats: torch.Tensor, lengths: Sequence[int], vertstrans: bool = True) -> torch.Tensor:
        """feats [B, T, 150], lengths [B] -> the 24 SMPL joints [B, T, 24, 3], root-centred, zeros at t >= len; ``vertstrans``: plus trans[t] - trans[0] on
        every frame (the reference's feats2joints_eval)"""
        return self._forward(feats, lengths, True, _lib.SMPL_TRANS_JOINTS if vertstrans else 0)

    @torch.no_grad()
    def vertices(self, feats: torch.Tensor, lengths: Sequence[int], vertstrans: bool = False) -> torch.Tensor:
        """feats [B, T, 150], lengths [B] -> the body's vertices [B, T, V, 3], zeros at t >= len (the reference's feats2joints)"""
        return self._forward(feats, lengths, False, _lib.SMPL_TRANS_VERTS if vertstrans else 0)

    @torch.no_grad()
    def rot2xyz(self, x, mask, pose_rep, translation, glob, jointstype, vertstrans, betas=None, beta=0, glob_rot=None, get_rotations_back=False, **kwargs):
        """Rotation2xyz.__call__ (rotation2xyz.py:16-114) for what the model calls it with: x [B, 25, 6, T], mask [B, T] (a prefix mask: it becomes the
        lengths; None = all frames) -> [B, J, 3, T] with J = 24 ('smpl') or V ('vertices').  Everything else raises, naming itself."""
        if jointstype not in JOINTSTYPES:
            raise NotImplementedError("This jointstype is not implemented.")                      # rotation2xyz.py:41-42
        if jointstype not in ("smpl", "vertices"):
            raise NotImplementedError(f"jointstype={jointstype!r}: the vertex-regressed joint sets (a2m, a2mpl, vibe) need J_regressor_extra.npy and "
                                      "smplx's vertex-id table and have no call site in the model; 'smpl' and 'vertices' are served")
        if pose_rep != "rot6d":
            raise NotImplementedError(f"pose_rep={pose_rep!r}: only 'rot6d' is served")
        if not glob or glob_rot is not None:
            raise NotImplementedError("glob=False / glob_rot: the global orientation is slot 0 of the features")
        if betas is not None or beta != 0:
            raise NotImplementedError("betas / beta: the body shape is fixed (v_shaped = v_template); add shapedirs @ betas to v_template for another one")
        if get_rotations_back:
            raise NotImplementedError("get_rotations_back: the rotation matrices stay in the engine")
        if not translation:
            raise NotImplementedError("translation=False: the features carry the translation slot (25 slots)")
        if x.dim() != 4 or x.shape[1] != 25 or x.shape[2] != 6:
            raise ValueError(f"x must be [B, 25, 6, T], got {tuple(x.shape)}")
        B, T = x.shape[0], x.shape[3]
        if mask is None:
            lengths = [T] * B
        else:
            m = mask.to(torch.bool).cpu()
            lengths = m.sum(dim=1).tolist()
            if tuple(m.shape) != (B, T) or not torch.equal(m, torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]) or min(lengths) < 1:
                raise ValueError("mask must be a [B, T] prefix mask with at least one frame per motion (lengths_to_mask's): it becomes the engine's lengths")
        feats = x.permute(0, 3, 2, 1).reshape(B, T, 150).float()                                  # the inverse of sample.view(..., 6, 25).permute(0, 3, 2, 1)
        out = self.joints(feats, lengths, bool(vertstrans)) if jointstype == "smpl" else self.vertices(feats, lengths, bool(vertstrans))
        return out.permute(0, 2, 3, 1).contiguous()                                               # rotation2xyz.py:97
