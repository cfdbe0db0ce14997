"""Shared pieces of the action-condition edge tests (tests/test_gpu_action_edges.py on the MI355X, tests/test_action_edges_sim.py on the simulator): the
HumanAct12 / UESTC variant -- labels instead of text rows (action_rows_kernel), a time embedding of width 256, the ActorVae -- on every reverse-loop family
and serving entry, modelled on tests/batch_edges_ref.py.

Reference.  One batch of `bmax` motions per (weights, steps): labels cycling through all classes from a seeded offset (neighbouring motions differ),
unit-normal start latents, every length 8.  It is run once on the three backends of tests/config_envelope_ref.py by action_trace, the loop of
O.sample_action keeping every step; the motions of a call are independent, so a call of B motions is the first B motions of the batch and its reference the
first B rows (prefix).  `rot` rotates every label by that many classes: the same start latents under other labels.  Tolerances are the project's own:
config_envelope_ref.Record.rule for eta = 0 latents and sampled features, config_envelope_ref.OP_TOL for single decode / encode calls against fp64, and
batch_edges_ref.ETA_TOL for stochastic, source and guided calls, whose reference is the float32 numpy loop of tests/sample_from_ref.py."""
import numpy as np

import config_envelope_ref as R
from batch_edges_ref import ETA_TOL  # noqa: F401  (re-exported: the test files name it through this module)
from mld_hip import _lib
from mld_hip import synthetic as syn
from oracle import mld_oracle as O
from sample_from_ref import NONE, reverse_from_np

f32 = np.float32
GUIDANCE = 7.5
NCLASSES = 12
MAX_FRAMES, LENGTH = 16, 8          # latents-only calls: the decoder is not part of them
DEN_LAYERS, VAE_LAYERS = 5, 3       # 3 ActorVae layers: the plain stack ends in Ha after visiting Hb (tests/test_gpu_config_envelope.py covers 2 and 5)
ENGINE_CFG = dict(condition=_lib.COND_ACTION, nclasses=NCLASSES, vae_arch=_lib.VAE_ACTOR, vae_num_layers=VAE_LAYERS, num_layers=DEN_LAYERS, nfeats=150,
                  guidance_scale=GUIDANCE)

_ref = {}


def weights():
    """(denoiser, ActorVae) state dicts of the MI355X tests"""
    return R.action_weights(DEN_LAYERS, VAE_LAYERS, NCLASSES)


def batch(bmax, rot=0, seed=141):
    """(labels [bmax] int32, start latents [bmax, 1, 256]) of the reference batch"""
    key = ("batch", bmax, seed)
    if key not in _ref:
        g = syn._rng(seed, "action_edges%d" % bmax)
        off = int(g.integers(0, NCLASSES))
        lat0 = g.standard_normal((bmax, 1, 256)).astype(f32)
        lat0.setflags(write=False)
        _ref[key] = (off, lat0)
    off, lat0 = _ref[key]
    return ((off + rot + np.arange(bmax)) % NCLASSES).astype(np.int32), lat0


def action_trace(ops, sd, acts, lat0, steps, guidance=GUIDANCE, nhead=4):
    """the loop of O.sample_action (mld.py:710-735), which keeps no trace, keeping every step: prev_sample of every scheduler step, [steps, B, 256] numpy"""
    sch = O.DDIMSchedule()
    acts = np.asarray(acts, np.int64).reshape(-1)
    B = len(acts)
    cond = np.concatenate([np.zeros_like(acts), acts])
    x = ops.asarray(lat0) * sch.init_noise_sigma
    tr = []
    for t in sch.set_timesteps(steps):
        eps = O.denoiser_forward_action(ops, sd, ops.cat([x, x], 0), t, cond, nhead, guidance)
        u, c = eps[:B], eps[B:]
        x = sch.step(u + guidance * (c - u), t, x)
        tr.append(np.asarray(ops.to_numpy(x)).reshape(B, -1).copy())
    return np.stack(tr)


def loop_reference(w, steps, bmax, rot=0, n=None, tag="gpu"):
    """the latents after every step [steps, n, 256] of the first n (default: all) motions of the batch of bmax, labels rotated by rot:
    [fp64, NumpyOps(float32), TorchOps('float32')] as float64, computed once"""
    n = bmax if n is None else n
    key = ("loop", tag, steps, bmax, rot, n)
    if key not in _ref:
        acts, lat0 = batch(bmax, rot)
        outs = [action_trace(ops, O.to_backend(ops, w[0]), acts[:n], lat0[:n], steps).astype(np.float64) for ops in R.backends()]
        for o in outs:
            o.setflags(write=False)
        _ref[key] = outs
    return _ref[key]


def prefix(outs, B, step=-1, lo=0):
    """(fp64 latents [B, 256], e32) of motions lo .. lo + B - 1 after scheduler step `step`"""
    r64 = outs[0][step, lo:lo + B]
    return r64, max(float(np.abs(o[step, lo:lo + B] - r64).max()) for o in outs[1:])


def feats_reference(w, outs, idx, lengths, tag):
    """O.actor_decode of the final latents of motions idx on each backend: (fp64 features [len(idx), max(lengths), nfeats], e32) -- the error of a float32
    sample, loop and decode, against the float64 one"""
    key = ("feats", tag, tuple(idx), tuple(lengths))
    if key not in _ref:
        res = []
        for k, ops in enumerate(R.backends()):
            lat = np.ascontiguousarray(outs[k][-1][list(idx)][:, None, :]).astype(np.float64 if k == 0 else f32)
            f = O.actor_decode(ops, O.to_backend(ops, w[1]), ops.asarray(lat), list(lengths))
            res.append(np.asarray(f if isinstance(f, np.ndarray) else ops.to_numpy(f), np.float64))
        _ref[key] = (res[0], max(float(np.abs(r - res[0]).max()) for r in res[1:]))
    return _ref[key]


def sanity(outs, B=None):
    """what makes the relative rule mean something: finite references, e32 > 0, and the float32 backends themselves inside F32_FACTOR x e32 (true by the
    definition of e32 -- unless the batch is degenerate).  Returns e32 of the final latents."""
    r64, e32 = prefix(outs, B or outs[0].shape[1])
    assert all(np.isfinite(o).all() for o in outs) and np.abs(r64).max() > 0
    assert e32 > 0
    for o in outs[1:]:
        assert np.abs(o[-1][:len(r64)] - r64).max() <= R.FACTOR[0] * e32
    return e32


def garray(gs):
    """[B, 1, 1] float32 scales for reverse_from_np: None or a negative entry is the handle's own"""
    return np.asarray([GUIDANCE if g is None or g < 0 else g for g in gs], f32).reshape(-1, 1, 1)


def numpy_loop(w, acts, lat0, steps, starts=None, eta=0.0, keys_per_motion=None, gs=None, tag=None):
    """the float32 numpy loop of tests/sample_from_ref.py on the action condition: (trajectory [steps, B, 256] with NaN where a row is not written, latents
    [B, 256]).  starts: per motion (kind, first_step, source [1, 256] or None); keys_per_motion: (seed, index) of the Philox draws (eta > 0); gs: a
    guidance scale per motion"""
    key = ("np", tag)
    if tag is None or key not in _ref:
        ops = O.NumpyOps(f32)
        sd = O.to_backend(ops, w[0])
        acts = np.asarray(acts, np.int64).reshape(-1)
        B = len(acts)
        cond = np.concatenate([np.zeros_like(acts), acts])
        out = reverse_from_np(sd, None, np.asarray(lat0, f32), starts or [(NONE, 0, None)] * B, steps, eta, keys_per_motion,
                              guidance=GUIDANCE if gs is None else garray(gs), denoise=lambda x2, t: O.denoiser_forward_action(ops, sd, x2, t, cond, 4, GUIDANCE))
        if tag is None:
            return out
        _ref[key] = out
    return _ref[key]
