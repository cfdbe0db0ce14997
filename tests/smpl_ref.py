"""Shared pieces of the SMPL body-model tests (tests/test_smpl_sim.py and tests/test_smpl_host.py on the simulator, tests/test_gpu_smpl.py on the
MI355X; tools/ab_smpl.py times ``forward`` under eager PyTorch): the project's own restatement of Rotation2xyz over smplx's SMPLLayer at betas = 0
(the math written out in include/mldhip.h) on torch tensors, in float64 or float32, the seeded inputs, a loader that puts
``mld_hip.synthetic.make_smpl`` into an engine, and the tolerance rule.

There is NO reference fixture behind this file: the reference's SMPL path imports ``smplx``, which is not installed here, and no SMPL file is
reachable, so parity is against this restatement alone.  It is unpinned, like the schedulers' restatements.

The restatement follows smplx's ``lbs`` step by step: pytorch3d's ``rotation_6d_to_matrix`` (F.normalize with eps 1e-12, rows b1, b2, b3), the pose
feature ``(R[1:] - I).view(207)``, ``pose_offsets = pf @ posedirs``, ``J = J_regressor @ v_template``, ``batch_rigid_transform`` (4 x 4 chain over
the parents, then the rest joints taken out of the translations), ``T = W @ A`` and the homogeneous product; then rotation2xyz.py:88-109: the mask,
the root-centring of the joints and the translation term (added to every frame, padded ones included).

Tolerance (``tests/clip_tower_ref.py``'s / ``tests/t2m_ref.py``'s rule, not a new number): e32 = max|float32-CPU restatement - float64 restatement|
on the same inputs; the engine must be within 4 x e32 of float64 in BOTH precision modes (its arithmetic is exact fp32 in both)."""
import numpy as np
import torch
import torch.nn.functional as F

from mld_hip import synthetic as syn

F32_FACTOR = 4.0
TRANS_JOINTS, TRANS_VERTS = 1, 2
# frames per pass of forward()'s vertex stage.  Its last product is a batch of (frames x V) 3 x 3 matrix-vector products.  In one piece a HumanAct12
# batch (2 592 valid frames) makes that 17.9 M > 2^24 batches, and the stage under eager PyTorch-ROCm on the MI355X returned wrong vertices (up to 1.8 off
# on values of 2.35) where the engine matched float64; in chunks of 512 frames (3.5 M) it matches float64 too (profiles/smpl_ab.json).  Which operation
# of the one-piece form went wrong was not isolated.
VERT_CHUNK = 512

_cache = {}


def body(V, dense=False, seed=11):
    """{key: float32 numpy} of the synthetic body (cached)"""
    key = (V, dense, seed)
    if key not in _cache:
        _cache[key] = syn.make_smpl(V, seed=seed, dense=dense)
    return _cache[key]


def make_feats(lens, T, seed=0, pad=0.0):
    """[B, T, 150] float32 rot6d features: per (frame, joint) rows 1-2 of a random rotation plus 0.1 N(0, 1), times a random scale in [0.5, 2] (the decoder's
    output is not normalised; this stays well conditioned); translations N(0, 1); frames at t >= len hold `pad` (0: what the decoder leaves there)."""
    g = np.random.default_rng([seed, T, len(lens)])
    B = len(lens)
    q = g.standard_normal((B, T, 24, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    r1 = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1)
    r2 = np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1)
    six = np.concatenate([r1, r2], -1) + 0.1 * g.standard_normal((B, T, 24, 6))
    six *= g.uniform(0.5, 2.0, size=(B, T, 24, 1))
    slots = np.zeros((B, T, 6, 25))
    slots[..., :24] = six.transpose(0, 1, 3, 2)
    slots[:, :, :3, 24] = g.standard_normal((B, T, 3))
    f = slots.reshape(B, T, 150).astype(np.float32)
    for b, n in enumerate(lens):
        f[b, n:] = pad
    return f


def rot6d_to_matrix(d6):
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = F.normalize(a1, dim=-1)
    b2 = F.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1, dim=-1)
    return torch.stack((b1, b2, torch.cross(b1, b2, dim=-1)), dim=-2)


def forward(model, feats, lens, flags=0, want_verts=True):
    """model: {key: tensor} of one dtype / device; feats [B, T, 150] of the same -> (joints [B, T, 24, 3], vertices [B, T, V, 3] or None)"""
    B, T = feats.shape[:2]
    dt, dev = feats.dtype, feats.device
    x = feats.reshape(B, T, 6, 25)
    trans = x[:, :, :3, 24]
    mask = torch.arange(T, device=dev)[None, :] < torch.as_tensor(lens, device=dev)[:, None]
    R = rot6d_to_matrix(x[..., :24].permute(0, 1, 3, 2)[mask])                   # [N, 24, 3, 3], valid frames only (rotation2xyz.py:61)
    N = R.shape[0]
    parents = [int(p) for p in model["parents"].tolist()]
    vt = model["v_template"]
    Jr = model["J_regressor"] @ vt                                              # [24, 3]
    rel = Jr.clone()
    rel[1:] = Jr[1:] - Jr[parents[1:]]
    tm = torch.zeros(N, 24, 4, 4, dtype=dt, device=dev)
    tm[:, :, :3, :3] = R
    tm[:, :, :3, 3] = rel
    tm[:, :, 3, 3] = 1
    chain = [tm[:, 0]]
    for i in range(1, 24):
        chain.append(chain[parents[i]] @ tm[:, i])
    G = torch.stack(chain, dim=1)
    posed = G[:, :, :3, 3]
    joints = torch.zeros(B, T, 24, 3, dtype=dt, device=dev)
    joints[mask] = posed
    joints = joints - joints[:, :, :1]
    shift = trans - trans[:, :1]
    if flags & TRANS_JOINTS:
        joints = joints + shift[:, :, None]
    if not want_verts:
        return joints, None
    Jh = torch.cat([Jr, torch.zeros(24, 1, dtype=dt, device=dev)], dim=1)
    A = G.clone()
    A[:, :, :, 3] = G[:, :, :, 3] - (G @ Jh[None, :, :, None])[..., 0]
    vs = []
    for n0 in range(0, N, VERT_CHUNK):           # (a frame's vertices do not depend on the chunk: every product below is per frame)
        Rc, Ac = R[n0:n0 + VERT_CHUNK], A[n0:n0 + VERT_CHUNK]
        n = Rc.shape[0]
        pf = (Rc[:, 1:] - torch.eye(3, dtype=dt, device=dev)).reshape(n, 207)
        vp = vt[None] + (pf @ model["posedirs"]).reshape(n, -1, 3)
        Tm = (model["lbs_weights"] @ Ac.reshape(n, 24, 16)).reshape(n, -1, 4, 4)
        vs.append((Tm[:, :, :3, :3] @ vp[..., None])[..., 0] + Tm[:, :, :3, 3])
    v = torch.cat(vs)
    verts = torch.zeros(B, T, vt.shape[0], 3, dtype=dt, device=dev)
    verts[mask] = v
    if flags & TRANS_VERTS:
        verts = verts + shift[:, :, None]
    return joints, verts


def as_model(bd, dtype, device="cpu"):
    return {k: torch.from_numpy(v).to(device=device, dtype=dtype) for k, v in bd.items()}


def reference(bd, feats, lens, flags=0, want_verts=True):
    """((joints64, e32_joints), (verts64, e32_verts)) as float64 numpy + the float32-CPU error of each output"""
    out = []
    with torch.no_grad():
        r64 = forward(as_model(bd, torch.float64), torch.from_numpy(feats).double(), lens, flags, want_verts)
        r32 = forward(as_model(bd, torch.float32), torch.from_numpy(feats), lens, flags, want_verts)
    for a, b in zip(r64, r32):
        if a is None:
            out.append((None, 0.0))
            continue
        assert torch.isfinite(b).all()
        out.append((a.numpy(), float((b.double() - a).abs().max())))
    return out


def reference_per_motion(bd, feats, lens, flags=0):
    """``reference`` of a batch computed one motion at a time (a motion's outputs do not depend on its neighbours; it keeps the float64 vertex stage of a
    64-motion batch small): the stitched float64 outputs and the largest float32-CPU error over the motions, for joints and vertices"""
    parts = [reference(bd, feats[b:b + 1], lens[b:b + 1], flags) for b in range(len(lens))]
    return [(np.concatenate([p[i][0] for p in parts]), max(p[i][1] for p in parts)) for i in range(2)]


def humanact12_batch(B=64, T=60):
    """one HumanAct12-sized batch (tools/ab_smpl.py's and tests/test_gpu_smpl.py's): B motions of T frames, ragged lengths 20 .. T (the first one full)"""
    rng = np.random.default_rng(0)
    lens = [int(x) for x in rng.integers(20, T + 1, size=B)]
    lens[0] = T
    return make_feats(lens, T, seed=7), lens


def load_body(eng, bd, finalize=True, skip=()):
    """Loads the body's five tensors under their ``smpl.`` keys into an engine created with smpl_verts = V; returns the ignored keys"""
    ignored = [k for k, v in bd.items() if k not in skip and not eng.load_tensor("smpl." + k, v)]
    if finalize:
        eng.finalize()
    return ignored


def engine_kwargs(V, max_batch=5, max_frames=16, **extra):
    """mldhip_config fields of a small engine that carries the body model (the diffusion model is the 3-layer text stack, never loaded)"""
    return dict(num_layers=3, max_batch=max_batch, max_frames=max_frames, nfeats=150, smpl_verts=V, **extra)
