"""Shared pieces of the UESTC recognition ST-GCN tests (tests/test_uestc_rec_golden.py, tests/test_uestc_rec_sim.py, tests/test_uestc_metrics.py on the CPU,
tests/test_gpu_uestc_rec.py on the MI355X; tools/ab_uestc_rec.py times ``forward`` under eager PyTorch): the project's own restatement of STGCN in eval mode
(the math written out in include/mldhip.h) with plain torch ops in float64 or float32, the seeded inputs, the weight families and the rules.

The restatement is pinned to the reference's own module by tests/golden/uestc_rec.npz (tools/make_golden_uestc_rec.py).

Tolerance rule (``tests/t2m_ref.py``'s pair, not a new number): err = max|engine - float64 restatement| over the logits and over the features; e32 = the
float32-CPU error of the same restatement on the same inputs; e32 > 0; err <= 4 e32 on MLDHIP_PREC_F32 handles and <= 16 e32 on MLDHIP_PREC_F16X3 handles.
Class rule (``tests/a2m_rec_ref.py``'s): the predicted class equals the float64 argmax on every row whose float64 top-two logit gap is >= 1e-4; at most one
row per case has a smaller gap (the seeds are chosen so that the float64 restatement alone satisfies this: ``check_gaps``)."""
import numpy as np
import torch
import torch.nn.functional as F

from mld_hip import synthetic as syn

F32_FACTOR, X3_FACTOR = 4.0, 16.0
GAP = 1e-4
EPS = 1e-5
NC = syn.UESTC_CLASSES

# the weight families: the seeded default; BN gammas x 2 (activations that grow with depth); and one whose inputs leave the half range (the probe's fallback)
FAMILIES = {"default": dict(seed=13), "bn_x2": dict(seed=13, bn_gain=2.0)}
OVERFLOW = dict(seed=13, in_gain=1e6)

_cache = {}


def weights(family="default"):
    """{key: float32 numpy} of a weight family, keys without the uestc_rec. prefix (cached)"""
    if family not in _cache:
        _cache[family] = syn.make_uestc_rec_state_dict(**(OVERFLOW if family == "overflow" else FAMILIES[family]))
    return _cache[family]


def tensors(sd, dtype=torch.float64, device="cpu"):
    return {k: torch.from_numpy(np.asarray(v)).to(device=device, dtype=dtype) for k, v in sd.items()}


def _bn(x, w, p, dim):
    """eval-mode BatchNorm over dimension ``dim`` of x from the running statistics"""
    shape = [1] * x.dim()
    shape[dim] = -1
    s = w[p + ".weight"] / torch.sqrt(w[p + ".running_var"] + EPS)
    return (x - w[p + ".running_mean"].view(shape)) * s.view(shape) + w[p + ".bias"].view(shape)


def forward(w, motion):
    """motion [B, 24, 6, T] (any strides) of the tensors' dtype -> (yhat [B, NC], features [B, 256]); every frame counts: the net has no lengths"""
    B, V, C, T = motion.shape
    x = _bn(motion.reshape(B, V * C, T), w, "data_bn", 1).reshape(B, V, C, T).permute(0, 2, 3, 1)      # [n, c, t, v]
    for i, (cin, cout, stride) in enumerate(syn.UESTC_BLOCKS):
        p = f"st_gcn_networks.{i}"
        y = F.conv2d(x, w[p + ".gcn.conv.weight"], w[p + ".gcn.conv.bias"])
        y = y.view(B, 3, cout, y.shape[2], V)
        g = torch.einsum("nkctv,kvw->nctw", y, w["A"] * w[f"edge_importance.{i}"])
        h = torch.relu(_bn(g, w, p + ".tcn.0", 1))
        h = _bn(F.conv2d(h, w[p + ".tcn.2.weight"], w[p + ".tcn.2.bias"], stride=(stride, 1), padding=(4, 0)), w, p + ".tcn.3", 1)
        if i == 0:
            res = 0
        elif cin == cout and stride == 1:
            res = x
        else:
            res = _bn(F.conv2d(x, w[p + ".residual.0.weight"], w[p + ".residual.0.bias"], stride=(stride, 1)), w, p + ".residual.1", 1)
        x = torch.relu(h + res)
    feat = x.mean(dim=(2, 3))
    yhat = feat @ w["fcn.weight"].view(-1, syn.UESTC_FEAT).t() + w["fcn.bias"]
    return yhat, feat


def reference(sd, motion):
    """((yhat64, e32_yhat), (feat64, e32_feat)): float64 numpy + the float32-CPU error of each output"""
    with torch.no_grad():
        m = torch.from_numpy(np.ascontiguousarray(motion))
        r64 = forward(tensors(sd, torch.float64), m.double())
        r32 = forward(tensors(sd, torch.float32), m.float())
    return [(a.numpy(), float((b.double() - a).abs().max())) for a, b in zip(r64, r32)]


def make_case(B, T, seed=None):
    """seeded motion [B, 24, 6, T] float32, N(0, 1) (rot6d components are O(1))"""
    g = torch.Generator().manual_seed(1000 * T + B if seed is None else seed)
    return torch.randn(B, 24, 6, T, generator=g).numpy()


def feature_rows(motion):
    """the same values as MLD holds them: feature rows [B, T, 150] = [B, T, 6, 25] with a 25th (translation) slot; returns (rows, view) where view is the
    [B, 24, 6, T] strided view m.view(B, T, 6, 25).permute(0, 3, 2, 1)[:, :-1] of the rows"""
    B, V, C, T = motion.shape
    rows = torch.zeros(B, T, 6, 25)
    rows[..., :24] = torch.from_numpy(np.ascontiguousarray(motion)).permute(0, 3, 2, 1)
    rows[..., 24] = 7.0      # (never read)
    rows = rows.reshape(B, T, 150).contiguous()
    return rows, rows.view(B, T, 6, 25).permute(0, 3, 2, 1)[:, :-1]


# the metric sequence of tests/golden/uestc_rec.npz and tests/test_uestc_metrics.py: NU updates of B motions of T frames (small: the simulator runs it)
SEQ_NU, SEQ_B, SEQ_T, SEQ_COMPUTE_SEED, SEQ_DT, SEQ_MT = 2, 3, 5, 23, 12, 3


def make_sequence():
    """[(label [B, 1], recmotion [B, 24, 6, T], gtmotion, lengths)] per update, seeded; labels cover three of the 40 classes, each twice -- 32 is the class the default family predicts on these
    motions (its logits hardly move with the input), so the confusion matrices have diagonal hits and both accuracies are 1 / 3"""
    g = np.random.default_rng(17)
    seq = []
    for u in range(SEQ_NU):
        lab = torch.from_numpy(np.asarray([32, 17, 39], np.int64)[(np.arange(SEQ_B) + u) % 3].reshape(SEQ_B, 1))
        ln = [int(n) for n in g.integers(1, SEQ_T + 1, size=SEQ_B)]
        rec = torch.from_numpy(g.standard_normal((SEQ_B, 24, 6, SEQ_T)).astype(np.float32))
        gt = torch.from_numpy((0.7 * g.standard_normal((SEQ_B, 24, 6, SEQ_T))).astype(np.float32))
        seq.append((lab, rec, gt, ln))
    return seq


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


def check(out, ref, what, prec):
    """the tolerance rule on one output; prints the reading before it asserts; returns (err, e32)"""
    r64, e32 = ref
    err = float(np.abs(np.asarray(out, np.float64) - r64).max())
    factor = X3_FACTOR if prec == 1 else F32_FACTOR
    print(f"{what}: mode {prec}  err {err:.3e}  e32 {e32:.3e}  ratio {err / e32:.2f}  (bound {factor:.0f})")
    assert e32 > 0 and np.isfinite(np.asarray(out)).all()
    assert err <= factor * e32, (what, prec, err, e32)
    return err, e32


def load(eng, sd, finalize=True, skip=()):
    """puts a weight family under its uestc_rec. keys into an engine created with uestc_rec = 1; returns the ignored keys"""
    ignored = [k for k, v in sd.items() if k not in skip and not eng.load_tensor("uestc_rec." + k, v)]
    if finalize:
        eng.finalize()
    return ignored


def engine_kwargs(max_batch=3, max_frames=16, **extra):
    """mldhip_config fields of a small engine that carries the net (the diffusion model is the 3-layer text stack, never loaded)"""
    return dict(num_layers=3, max_batch=max_batch, max_frames=max_frames, uestc_rec=1, **extra)
