"""Text encoders at the INPUT boundary of the hot path.

``MldTextEncoder`` keeps the frozen CLIP ViT-L/14 text tower on PyTorch-ROCm exactly as the reference does
(mld/models/architectures/mld_clip.py:17-90) -- it is not part of the HIP engine (BASELINE.json:
"the frozen CLIP text encoder run once on PyTorch-ROCm").  It also absorbs the transformers>=5 API
change (``get_text_features`` returns a ModelOutput there, which breaks the reference's ``.unsqueeze(1)``).

``HipMldTextEncoder`` is the same adapter with the tower itself inside the HIP engine (``mldhip_text_encode``, include/mldhip.h): the
tokenizer stays in transformers on the CPU, the token ids go to the engine, the embeddings come back as a device tensor on the
caller's stream.  Opt-in: override ``model.text_encoder.target`` with ``mld_hip.text_encoder.HipMldTextEncoder``.

``SyntheticTextEncoder`` exists because no CLIP weights are reachable offline: a deterministic stand-in
with CLIP-like statistics so ``MLD.forward({"text": ..., "length": ...})`` can be exercised end to end.
"""
from __future__ import annotations

import logging
import os
import zlib
from typing import Dict, List, Optional

import numpy as np
import torch
from torch import nn


class MldTextEncoder(nn.Module):
    def __init__(self, modelpath: str, finetune: bool = False, last_hidden_state: bool = False,
                 latent_dim: list = [1, 256]) -> None:
        super().__init__()
        if last_hidden_state:
            raise NotImplementedError("last_hidden_state=True (token-level CLIP states) is not used by the MLD configs")
        if not os.path.isdir(modelpath):
            raise FileNotFoundError(f"CLIP weights not found at {modelpath!r} (configs/assets.yaml model.clip_path). "
                                    "Offline runs can pass text_encoder=SyntheticTextEncoder() to mld_hip.MLD.")
        from transformers import AutoModel, AutoTokenizer
        self.latent_dim = latent_dim
        self.tokenizer = AutoTokenizer.from_pretrained(modelpath)
        self.text_model = AutoModel.from_pretrained(modelpath)
        if not finetune:
            self.text_model.eval()
            for p in self.text_model.parameters():
                p.requires_grad = False
        self.max_length = self.tokenizer.model_max_length
        self.text_encoded_dim = self.text_model.config.text_config.hidden_size
        self.name = "clip"

    @torch.no_grad()
    def forward(self, texts: List[str]):
        ids = self.tokenizer(texts, padding="max_length", truncation=True, max_length=self.max_length,
                             return_tensors="pt").input_ids[:, : self.tokenizer.model_max_length]
        out = self.text_model.get_text_features(ids.to(next(self.text_model.parameters()).device))
        if not torch.is_tensor(out):                       # transformers >= 5: BaseModelOutputWithPooling
            out = out.pooler_output if getattr(out, "pooler_output", None) is not None else out[0]
        return out.unsqueeze(1).float()                    # [B, 1, 768]


class HipMldTextEncoder(MldTextEncoder):
    """``MldTextEncoder`` with the CLIP text tower in libmldhip: same constructor, same ``forward(texts) -> [B, 1, 768]``.

    The tower shares the model's ONE engine (its architecture fields join the denoiser's and the VAE's, ``MLD.__init__``); its tensors are
    copied into that handle once.  A tower the engine is not built for (``hidden_act`` other than quick_gelu, head dim other than 64, widths
    other than 768 / 3072) runs on the parent's PyTorch path, with one log line."""
    _prefix = "text_encoder."

    def __init__(self, modelpath: str, finetune: bool = False, last_hidden_state: bool = False, latent_dim: list = [1, 256]) -> None:
        super().__init__(modelpath, finetune=finetune, last_hidden_state=last_hidden_state, latent_dim=latent_dim)
        tc = self.text_model.config.text_config
        why = []
        if getattr(tc, "hidden_act", None) != "quick_gelu":
            why.append(f"hidden_act={getattr(tc, 'hidden_act', None)!r} (built: quick_gelu)")
        if tc.hidden_size % tc.num_attention_heads or tc.hidden_size // tc.num_attention_heads != 64:
            why.append(f"head dim {tc.hidden_size / tc.num_attention_heads:g} (built: 64)")
        if tc.hidden_size != 768 or tc.intermediate_size != 3072 or tc.max_position_embeddings > 80:
            why.append(f"widths {tc.hidden_size} / {tc.intermediate_size}, context {tc.max_position_embeddings} (built: 768 / 3072, <= 80)")
        if int(self.text_model.config.projection_dim) != tc.hidden_size:
            why.append(f"projection_dim {self.text_model.config.projection_dim} != hidden_size")
        self.hip_tower = not why
        if why:
            logging.getLogger(__name__).warning("HipMldTextEncoder: the text tower stays on PyTorch: %s", "; ".join(why))
        self._variant = "text"
        self._arch: Dict[str, object] = {}
        self._shared_arch: Dict[str, object] = {}
        self._engine_key: Optional[str] = None
        self._synced_sig = None
        if self.hip_tower:
            self._arch = dict(text_dim=int(tc.hidden_size), clip_layers=int(tc.num_hidden_layers), clip_heads=int(tc.num_attention_heads),
                              clip_ff=int(tc.intermediate_size), clip_vocab=int(tc.vocab_size), clip_ctx=int(tc.max_position_embeddings))
        self.eos_token_id = int(tc.eos_token_id)

    def use_engine(self, key: str):
        self._engine_key = key
        self._synced_sig = None
        return self

    def _tower_parameters(self):
        for name, p in self.text_model.named_parameters():
            if name.startswith("text_model.") or name == "text_projection.weight":
                yield "text_model." + name, p

    def sync_weights(self):
        """The engine of this model with the tower's tensors in it (uploaded once; again only if they changed or another module overwrote them)."""
        from . import engine as _engine
        dev = next(self.text_model.parameters()).device
        eng = _engine.get_engine(self._engine_key) if self._engine_key is not None else \
            _engine.get_engine(dev, self._variant, want={**self._shared_arch, **self._arch})
        _engine.check_arch(eng, type(self).__name__, **self._arch)
        sig = (id(eng), tuple((p.data_ptr(), p._version) for _, p in self._tower_parameters()))
        owners = eng.__dict__.setdefault("_owner", {})
        if sig != self._synced_sig or owners.get(self._prefix) != (id(self), sig):
            for name, p in self._tower_parameters():
                eng.load_tensor(self._prefix + name, p.data)
            eng._dirty = True
            self._synced_sig = sig
            owners[self._prefix] = (id(self), sig)
        return eng, dev

    def eos_positions(self, ids: torch.Tensor) -> torch.Tensor:
        """The pooling position of transformers' CLIPTextTransformer: argmax(ids) under the legacy eos_token_id == 2, else the first EOS token."""
        if self.eos_token_id == 2:
            return ids.to(torch.int).argmax(dim=-1)
        return (ids.to(torch.int) == self.eos_token_id).int().argmax(dim=-1)

    @torch.no_grad()
    def forward(self, texts: List[str]):
        if not self.hip_tower:
            return super().forward(texts)
        from . import engine as _engine
        ids = self.tokenizer(texts, padding="max_length", truncation=True, max_length=self.max_length,
                             return_tensors="pt").input_ids[:, : self.tokenizer.model_max_length]
        eng, dev = self.sync_weights()
        anchor = next(self.text_model.parameters())
        stream = _engine.current_stream_handle(anchor)
        _engine.finalize_if_dirty(eng, stream)
        out = torch.empty(ids.shape[0], 1, self.text_encoded_dim, device=dev, dtype=torch.float32)
        eng.text_encode(ids.numpy(), self.eos_positions(ids).numpy(), out, stream)
        return out


class SyntheticTextEncoder(nn.Module):
    """Deterministic text -> [B, 1, 768] embedding (hash-seeded N(0, 0.5^2)); "" maps to one fixed vector."""

    def __init__(self, text_encoded_dim: int = 768, seed: int = 1234):
        super().__init__()
        self.text_encoded_dim = text_encoded_dim
        self.seed = seed
        self.register_buffer("_anchor", torch.zeros(1), persistent=False)   # follows .to(device)
        self.name = "synthetic"

    def forward(self, texts: List[str]):
        rows = []
        for t in texts:
            g = np.random.Generator(np.random.PCG64([self.seed, zlib.crc32(t.encode())]))
            rows.append((0.5 * g.standard_normal(self.text_encoded_dim)).astype(np.float32))
        return torch.from_numpy(np.stack(rows)[:, None, :]).to(self._anchor.device)
