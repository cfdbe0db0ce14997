"""Shared pieces of the configuration-envelope tests (tests/test_gpu_config_envelope.py on the MI355X, tests/test_config_envelope_sim.py on
the simulator): synthetic weights by model dimensions, the float64 / float32 references and the tolerance rule.

Tolerance.  Single-call outputs (a denoiser call, decode features, encode mu / logvar, joints from given features) keep the absolute bound
their entry point has in tests/test_gpu_shape_edges.py: OP_TOL; joints of every case JOINT_TOL, the contract.  What comes out of a reverse
loop scales with the guidance and the step count, so it follows the relative rule of tests/clip_tower_ref.py: max|engine - fp64| must be
<= F32_FACTOR x e32 on an MLDHIP_PREC_F32 handle and <= X3_FACTOR x e32 on an MLDHIP_PREC_F16X3 one, e32 = the error of a float32 CPU
evaluation of the same case against fp64 -- the larger of NumpyOps(float32) and TorchOps("float32"): two summation orders give a steadier
estimate over many steps.  Every comparison goes into a record (Record) that the test files write to the file an environment variable names."""
import json
import os

import numpy as np

from clip_tower_ref import F32_FACTOR, X3_FACTOR
from mld_hip import synthetic as syn
from oracle import mld_oracle as O

FACTOR = {0: F32_FACTOR, 1: X3_FACTOR}
OP_TOL, JOINT_TOL = 1e-4, 1e-3
MODE = {0: "f32", 1: "f16x3"}

_weights = {}


def text_weights(**dims):
    """(denoiser, MldVae) synthetic state dicts of the text model with the given ModelDims fields"""
    key = ("text",) + tuple(sorted(dims.items()))
    if key not in _weights:
        d = syn.ModelDims(**dims)
        _weights[key] = (syn.make_denoiser_state_dict(dims=d), syn.make_vae_state_dict(dims=d))
    return _weights[key]


def action_weights(num_layers, vae_layers, nclasses, nfeats=150):
    key = ("action", num_layers, vae_layers, nclasses, nfeats)
    if key not in _weights:
        d = syn.ModelDims(num_layers=num_layers, nfeats=nfeats)
        _weights[key] = (syn.make_denoiser_state_dict(seed=3, dims=d, condition="action", nclasses=nclasses),
                         syn.make_actor_vae_state_dict(dims=d, num_layers=vae_layers))
    return _weights[key]


def novae_weights(num_layers, ff_size):
    key = ("novae", num_layers, ff_size)
    if key not in _weights:
        _weights[key] = syn.make_novae_denoiser_state_dict(dims=syn.ModelDims(latent_dim=512, num_layers=num_layers, ff_size=ff_size))
    return _weights[key]


def backends():
    """the reference first, then the two float32 evaluations whose larger error is e32"""
    return [O.TorchOps("float64"), O.NumpyOps(np.float32), O.TorchOps("float32")]


def reference(fn):
    """fn(ops, W) -> array or tuple of arrays, W(state dict) = the dict on that backend.  Returns ([fp64 results], [e32 of each])."""
    outs = []
    for ops in backends():
        r = fn(ops, lambda sd, ops=ops: O.to_backend(ops, sd))
        r = list(r) if isinstance(r, (list, tuple)) else [r]
        outs.append([np.asarray(x if isinstance(x, np.ndarray) else ops.to_numpy(x), np.float64) for x in r])
    r64 = outs[0]
    e32 = [max(float(np.abs(o[i] - r64[i]).max()) for o in outs[1:]) for i in range(len(r64))]
    return r64, e32


def reference64(fn):
    """the fp64 results alone (single-call outputs with an absolute bound)"""
    ops = O.TorchOps("float64")
    r = fn(ops, lambda sd: O.to_backend(ops, sd))
    r = list(r) if isinstance(r, (list, tuple)) else [r]
    return [np.asarray(x if isinstance(x, np.ndarray) else ops.to_numpy(x), np.float64) for x in r]


class Record:
    """every comparison of a test file: name -> e32 / err / ratio (relative rule) or err / bound (absolute bound)"""

    def __init__(self, env):
        self.env, self.cases, self.bad = env, {}, []

    def rule(self, name, got, r64, e32, prec):
        """the relative rule; a miss is remembered (failures) so that a test measures all its cases before it fails"""
        got = np.asarray(got, np.float64)
        finite = bool(np.isfinite(got).all())
        err = float(np.abs(got - r64).max()) if finite else float("inf")
        ratio = err / e32 if e32 > 0 else (0.0 if err == 0 else float("inf"))
        ok = finite and err <= FACTOR[prec] * e32
        self.cases[name] = {"e32": e32, "err": err, "ratio": ratio, "factor": FACTOR[prec], "max_abs_reference": float(np.abs(r64).max())}
        print("%s: err %.3e  e32 %.3e  ratio %.2f (factor %g)%s" % (name, err, e32, ratio, FACTOR[prec], "" if ok else "  <-- MISS"))
        if not ok:
            self.bad.append((name, err, e32, ratio))
        return ok

    def bound(self, name, got, r64, tol):
        got = np.asarray(got, np.float64)
        finite = bool(np.isfinite(got).all())
        err = float(np.abs(got - r64).max()) if finite else float("inf")
        ok = finite and err < tol
        self.cases[name] = {"err": err, "bound": tol}
        print("%s: err %.3e (bound %g)%s" % (name, err, tol, "" if ok else "  <-- MISS"))
        if not ok:
            self.bad.append((name, err, tol))
        return ok

    def failures(self):
        """the misses since the last call"""
        bad, self.bad = self.bad, []
        return bad

    def dump(self, **header):
        out = os.environ.get(self.env)
        if out and self.cases:
            with open(out, "w") as f:
                json.dump({**header, "f32_factor": F32_FACTOR, "x3_factor": X3_FACTOR, "op_tol": OP_TOL, "joint_tol": JOINT_TOL,
                           "cases": self.cases}, f, indent=1, sort_keys=True)


def chain_launches(steps, num_layers):
    """launches of a reverse loop on the per-launch families (engine/path_latent.hpp enqueue_sample): the condition rows, init_chain, and per step
    four per layer (engine/path_loop.hpp denoiser_body), one per skip linear and the final-norm + scheduler step"""
    return 2 + steps * (4 * num_layers + (num_layers - 1) // 2 + 1)


def split_cfg(cfg):
    """(engine fields, DDIMSchedule arguments, guidance the oracle uses) of a case.  guidance_scale <= 1: the reference runs the conditional batch
    alone (mld.py:300,316-340) -- u + 1 x (c - u) on the [2B] batch the C ABI still takes"""
    sch = {k: cfg[k] for k in ("steps_offset", "set_alpha_to_one", "beta_start", "beta_end") if k in cfg}
    if "set_alpha_to_one" in sch:
        sch["set_alpha_to_one"] = bool(sch["set_alpha_to_one"])
    g = cfg.get("guidance_scale", 7.5)
    return cfg, sch, (g if g > 1.0 else 1.0)
