"""Shared pieces of the HumanAct12 recognition-GRU tests (tests/test_a2m_rec_golden.py, tests/test_a2m_rec_sim.py, tests/test_a2m_metrics.py on the CPU,
tests/test_gpu_a2m_rec.py on the MI355X; tools/ab_a2m_rec.py times ``forward`` under eager PyTorch): the project's own restatement of MotionDiscriminator /
MotionDiscriminatorForFID (nn.GRU(72, 128, 2) + Linear(128 -> 30) + tanh + Linear(30 -> 12); the math written out in include/mldhip.h) in float64 or
float32, the seeded inputs and weights, and the two rules.

The restatement is pinned to the reference's own modules by tests/golden/a2m_rec.npz (tools/make_golden_a2m_rec.py).

Tolerance rule (``tests/smpl_ref.py``'s / ``tests/t2m_ref.py``'s, not a new number): err = max|engine - float64 restatement| over the logits and over the
activations; e32 = the float32-CPU error of the same restatement on the same inputs; e32 > 0 and err <= 4 e32 in both precision modes (exact fp32 in
both, and the two modes are bit-equal).
Class rule: the predicted class equals the float64 argmax on every row whose float64 top-two logit gap is >= 1e-4; at most one row per case has a
smaller gap (the seeds below are chosen so that the float64 restatement alone satisfies this: ``check_gaps``)."""
import numpy as np
import torch
from torch import nn

from mld_hip import synthetic as syn

F32_FACTOR = 4.0
GAP = 1e-4
H = 128

# the weight families: PyTorch's default init, and the same with the four recurrent matrices x 3 (saturated gates)
FAMILIES = {"default": dict(seed=12, rec_gain=1.0), "rec_x3": dict(seed=12, rec_gain=3.0)}

_cache = {}


def weights(family="default"):
    """{key: float32 numpy} of a weight family, keys without the a2m_rec. prefix (cached)"""
    if family not in _cache:
        _cache[family] = syn.make_a2m_rec_state_dict(**FAMILIES[family])
    return _cache[family]


def modules(sd, dtype=torch.float64, device="cpu"):
    """(nn.GRU, linear1, linear2) holding ``sd``, in ``dtype`` on ``device``"""
    gru, l1, l2 = nn.GRU(72, H, 2), nn.Linear(H, 30), nn.Linear(30, 12)
    owner = {"recurrent": gru, "linear1": l1, "linear2": l2}
    with torch.no_grad():
        for k, v in sd.items():
            head, name = k.split(".", 1)
            getattr(owner[head], name).copy_(torch.from_numpy(v))
    return tuple(m.to(device=device, dtype=dtype).eval() for m in (gru, l1, l2))


def forward(mods, joints, lens, h0):
    """joints [B, T, 72] (the engine's layout), lens [B], h0 [2, B, 128], all of the modules' dtype / device -> (logits [B, 12], act [B, 30])"""
    gru, l1, l2 = mods
    B = joints.shape[0]
    o, _ = gru(joints.permute(1, 0, 2), h0)                                       # [T, B, 128]
    lens = torch.as_tensor(lens, device=joints.device)
    out = o[lens - 1, torch.arange(B, device=joints.device)]
    act = torch.tanh(l1(out))
    return l2(act), act


def reference(sd, joints, lens, h0):
    """((logits64, e32_logits), (act64, e32_act)): float64 numpy + the float32-CPU error of each output"""
    with torch.no_grad():
        j, h = torch.from_numpy(np.ascontiguousarray(joints)), torch.from_numpy(np.ascontiguousarray(h0))
        r64 = forward(modules(sd, torch.float64), j.double(), lens, h.double())
        r32 = forward(modules(sd, torch.float32), j.float(), lens, h.float())
    return [(a.numpy(), float((b.double() - a).abs().max())) for a, b in zip(r64, r32)]


def to_engine(x):
    """the reference's [B, 24, 3, T] -> the engine's [B, T, 72] (feature 3 joint + coord)"""
    B, J, C, T = x.shape
    return np.ascontiguousarray(np.asarray(x).reshape(B, J * C, T).transpose(0, 2, 1))


def make_case(B, T, scale=1.0, seed=None, pad=0.0, lens=None):
    """seeded joints [B, T, 72] float32 (N(0, scale^2)), lengths in 1 .. T (the first motion T, the last 1; or ``lens``) and h0 [2, B, 128] N(0, 1);
    frames t >= len hold ``pad``"""
    g = torch.Generator().manual_seed(B if seed is None else seed)
    x = torch.randn(B, 24, 3, T, generator=g) * scale
    drawn = torch.randint(1, T + 1, (B,), generator=g)
    drawn[0], drawn[-1] = T, 1
    h0 = torch.randn(2, B, H, generator=g)
    j = to_engine(x.numpy())
    lens = [int(n) for n in (drawn if lens is None else lens)]
    for b, n in enumerate(lens):
        j[b, n:] = pad
    return j, lens, h0.numpy()


def gaps(logits64):
    s = np.sort(logits64, axis=1)
    return s[:, -1] - s[:, -2]


def check_gaps(logits64):
    """the class rule's premise on the float64 restatement alone: at most one row below GAP"""
    assert int((gaps(logits64) < GAP).sum()) <= 1


def check_classes(logits, logits64):
    """the class rule: every row with a float64 top-two gap >= GAP predicts the float64 argmax"""
    ok = gaps(logits64) >= GAP
    assert int((~ok).sum()) <= 1
    assert np.array_equal(np.asarray(logits).argmax(1)[ok], logits64.argmax(1)[ok])


def load(eng, sd, finalize=True, skip=()):
    """puts a weight family under its a2m_rec. keys into an engine created with a2m_rec = 1; returns the ignored keys"""
    ignored = [k for k, v in sd.items() if k not in skip and not eng.load_tensor("a2m_rec." + k, v)]
    if finalize:
        eng.finalize()
    return ignored


def engine_kwargs(max_batch=5, max_frames=16, **extra):
    """mldhip_config fields of a small engine that carries the recognizer (the diffusion model is the 3-layer text stack, never loaded)"""
    return dict(num_layers=3, max_batch=max_batch, max_frames=max_frames, a2m_rec=1, **extra)
