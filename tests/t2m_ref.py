"""Shared pieces of the T2M evaluator tests (tests/test_t2m_golden.py against the fixture, tests/test_t2m_sim.py on the simulator,
tests/test_gpu_t2m.py on the MI355X): the project's own restatement of the two evaluator towers on ``torch.nn`` modules, in float64 or float32
on the CPU, the seeded inputs, and the tolerance rule.

The restatement: ``nn.Conv1d(C, 512, 4, 2, 1)`` / LeakyReLU(0.2) / ``nn.Conv1d(512, 512, 4, 2, 1)`` / LeakyReLU(0.2) / ``nn.Linear(512, 512)``, then
``nn.Linear`` -> bidirectional ``nn.GRU`` over a ``pack_padded_sequence`` (sorted by length internally, rows returned in the caller's order) ->
``cat(h_fwd, h_bwd)`` -> Linear, LayerNorm, LeakyReLU(0.2), Linear; the text tower adds ``word + nn.Linear(15, 300)(pos)`` in front.  Parameters are
loaded from the checkpoint's own key names (``mld_hip.synthetic.make_t2m_state_dict``).  The renorm (``(f std + mean - mean_eval) / std_eval`` on ALL T
frames, padded ones included) is part of ``motion_embed``.

Tolerance (``tests/clip_tower_ref.py``'s rule, not a new number): e32 = max|torch-fp32-CPU - torch-fp64-CPU| on the same inputs; MLDHIP_PREC_F32 must be
within 4 x e32 of fp64, MLDHIP_PREC_F16X3 within 16 x e32."""
import numpy as np
import torch
from torch import nn
from torch.nn.utils.rnn import pack_padded_sequence

from mld_hip import synthetic as syn

F32_FACTOR, X3_FACTOR = 4.0, 16.0
UNIT_LEN = 4
SEED = 5

_cache = {}


class _Tower(nn.Module):
    """input_emb -> bidirectional GRU over packed rows -> output_net (both evaluator encoders share this shape)"""

    def __init__(self, n_in, hidden, n_out=512):
        super().__init__()
        self.input_emb = nn.Linear(n_in, hidden)
        self.gru = nn.GRU(hidden, hidden, batch_first=True, bidirectional=True)
        self.output_net = nn.Sequential(nn.Linear(2 * hidden, hidden), nn.LayerNorm(hidden), nn.LeakyReLU(0.2), nn.Linear(hidden, n_out))
        self.hidden = nn.Parameter(torch.zeros(2, 1, hidden))

    def forward(self, x, lens):
        lens = torch.as_tensor(lens, dtype=torch.int64)
        order = torch.argsort(lens, descending=True, stable=True)      # pack_padded_sequence wants descending lengths; rows come back in the caller's order
        emb = self.input_emb(x[order])
        packed = pack_padded_sequence(emb, lens[order], batch_first=True)
        _, last = self.gru(packed, self.hidden.repeat(1, x.shape[0], 1))
        out = self.output_net(torch.cat([last[0], last[1]], dim=-1))
        back = torch.empty_like(order)
        back[order] = torch.arange(len(order))
        return out[back]


class Evaluators(nn.Module):
    def __init__(self, nfeats):
        super().__init__()
        self.t2m_moveencoder = nn.Module()
        self.t2m_moveencoder.main = nn.Sequential(nn.Conv1d(nfeats - 4, 512, 4, 2, 1), nn.Identity(), nn.LeakyReLU(0.2),
                                                  nn.Conv1d(512, 512, 4, 2, 1), nn.Identity(), nn.LeakyReLU(0.2))
        self.t2m_moveencoder.out_net = nn.Linear(512, 512)
        self.t2m_motionencoder = _Tower(512, 1024)
        self.t2m_textencoder = _Tower(300, 512)
        self.t2m_textencoder.pos_emb = nn.Linear(15, 300)

    def motion_embed(self, feats, lens, stats=None):
        """feats [B, T, nfeats], lens [B]; stats = (mean, std, mean_eval, std_eval) applies renorm4t2m to every frame first"""
        if stats is not None:
            mean, std, mean_eval, std_eval = (torch.as_tensor(s, dtype=feats.dtype) for s in stats)
            feats = (feats * std + mean - mean_eval) / std_eval
        mov = self.t2m_moveencoder.main(feats[..., :-4].permute(0, 2, 1)).permute(0, 2, 1)
        mov = self.t2m_moveencoder.out_net(mov)
        return self.t2m_motionencoder(mov, [int(n) // UNIT_LEN for n in lens])

    def text_embed(self, word_embs, pos_ohot, text_lens):
        return self.t2m_textencoder(word_embs + self.t2m_textencoder.pos_emb(pos_ohot), text_lens)


def weights(nfeats=syn.NFEATS, seed=SEED):
    """{checkpoint key: float32 numpy} of the synthetic evaluators (cached: ~60 MB per feature width)"""
    key = ("w", nfeats, seed)
    if key not in _cache:
        _cache[key] = syn.make_t2m_state_dict(seed, nfeats)
    return _cache[key]


def models(nfeats=syn.NFEATS, seed=SEED):
    """(fp64, fp32) restatements holding the same parameters, loaded strictly from the checkpoint key names"""
    key = ("m", nfeats, seed)
    if key not in _cache:
        sd = {k: torch.from_numpy(v) for k, v in weights(nfeats, seed).items()}
        m32 = Evaluators(nfeats).eval()
        m32.load_state_dict(sd, strict=True)
        m64 = Evaluators(nfeats).double().eval()
        m64.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
        _cache[key] = (m64, m32)
    return _cache[key]


def stats(nfeats=syn.NFEATS):
    """(mean, std, mean_eval, std_eval) float32 numpy"""
    return (*syn.make_mean_std(nfeats), *syn.make_mean_std_eval(nfeats))


def make_motions(lens, T, nfeats=syn.NFEATS, seed=0):
    """[B, T, nfeats] float32: unit-normal rows in the model's normalisation, zeros at t >= len (what the decoder leaves there)"""
    g = np.random.default_rng([seed, T, nfeats])
    f = g.standard_normal((len(lens), T, nfeats)).astype(np.float32)
    for b, n in enumerate(lens):
        f[b, n:] = 0.0
    return f


def make_captions(text_lens, L, seed=0):
    """(word_embs [B, L, 300], pos_ohot [B, L, 15]) float32: GloVe-like rows, one-hot POS tags; rows at l >= len are zero like the dataloader's padding"""
    g = np.random.default_rng([seed, L, 300])
    w = (0.4 * g.standard_normal((len(text_lens), L, 300))).astype(np.float32)
    p = np.zeros((len(text_lens), L, 15), np.float32)
    tags = g.integers(0, 15, size=(len(text_lens), L))
    for b, n in enumerate(text_lens):
        p[b, np.arange(L), tags[b]] = 1.0
        w[b, n:] = 0.0
        p[b, n:] = 0.0
    return w, p


def reference_motion(feats, lens, nfeats=syn.NFEATS, renorm=True):
    """(fp64 [B, 512] as float64 numpy, e32) of the motion tower on these rows"""
    m64, m32 = models(nfeats)
    st = stats(nfeats) if renorm else None
    with torch.no_grad():
        r64 = m64.motion_embed(torch.from_numpy(feats).double(), lens, st).numpy()
        r32 = m32.motion_embed(torch.from_numpy(feats), lens, st).double().numpy()
    return r64, float(np.abs(r32 - r64).max())


def reference_text(word_embs, pos_ohot, text_lens):
    m64, m32 = models()
    with torch.no_grad():
        r64 = m64.text_embed(torch.from_numpy(word_embs).double(), torch.from_numpy(pos_ohot).double(), text_lens).numpy()
        r32 = m32.text_embed(torch.from_numpy(word_embs), torch.from_numpy(pos_ohot), text_lens).double().numpy()
    return r64, float(np.abs(r32 - r64).max())


def load_evaluators(eng, nfeats=syn.NFEATS, finalize=True, groups=("motion", "text")):
    """Loads the synthetic evaluator weights (+ mean / std, mean_eval / std_eval) into an engine created with t2m_eval=1; returns the ignored keys"""
    ignored = []
    for k, v in weights(nfeats).items():
        want = "text" if k.startswith("t2m_textencoder.") else "motion"
        if want in groups and not eng.load_tensor(k, v):
            ignored.append(k)
    mean, std, mean_eval, std_eval = stats(nfeats)
    eng.load_tensor("mean", mean)
    eng.load_tensor("std", std)
    if "motion" in groups:
        eng.load_tensor("mean_eval", mean_eval)
        eng.load_tensor("std_eval", std_eval)
    if finalize:
        eng.finalize()
    return ignored


def engine_kwargs(max_motions, max_frames=16, max_words=8, **extra):
    """mldhip_config fields of a small engine that carries the evaluators (the diffusion model is the 3-layer stack, never loaded)"""
    return dict(num_layers=3, max_batch=2, max_frames=max_frames, t2m_eval=1, t2m_max_motions=max_motions, t2m_max_words=max_words, **extra)
