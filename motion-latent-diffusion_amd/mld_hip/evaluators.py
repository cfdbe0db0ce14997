"""``HipT2MEvaluator`` -- the pretrained T2M evaluator nets of a checkpoint (``t2m_moveencoder`` / ``t2m_motionencoder`` / ``t2m_textencoder``:
mld/models/architectures/t2m_motionenc.py, t2m_textenc.py; instantiated at mld/models/modeltype/mld.py:110-140) as one drop-in module whose arithmetic
runs in libmldhip (``mldhip_t2m_motion_embed`` / ``mldhip_t2m_text_embed``; include/mldhip.h has the math).

Opt-in: ``load_config(overrides={"model.t2m_evaluator.target": "mld_hip.evaluators.HipT2MEvaluator"})``.  Without it ``MLD`` keeps dropping the ``t2m_*`` keys of a
checkpoint; with it ``MLD.load_state_dict`` loads them strictly and ``MLD.t2m_eval`` returns the embeddings the T2M metrics are computed from."""
from __future__ import annotations

from typing import Sequence

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
