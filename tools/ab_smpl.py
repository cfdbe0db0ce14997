"""Time the SMPL body model of the engine (mldhip_smpl_forward) against the float32 torch restatement of tests/smpl_ref.py under eager PyTorch-ROCm on
the same GPU (the baseline: the parent commit has no body model, and ``smplx`` is not installed).

  python tools/ab_smpl.py [--out profiles/smpl_ab.json] [--repeats 5]

Shape: one HumanAct12 batch, B = 64 motions x T = 60 frames (ragged lengths 20 .. 60), V = 6890 -- joints only (the chain kernel) and with vertices (the
whole call).  Timing: device events around windows of back-to-back calls on one stream after a warm-up of the same calls, engine and eager windows
alternating, `repeats` windows each; the median and the spread (min, max) of the per-call time are written.  The operations and bytes a call needs are
computed from the shapes here, and the share of the hardware's least time (fp32 matrix peak 157.3 TFLOP/s, 6.3 TB/s achievable HBM) is derived from
them.  The outputs of every side on the timed inputs are compared with the float64 restatement (one motion at a time on the CPU) under the tests' rule,
within 4 x the float32-CPU error; the tool fails, after writing its figures, when one side misses it.  The eager side runs its vertex stage in chunks of
smpl_ref.VERT_CHUNK frames (why: there)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "motion-latent-diffusion_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import smpl_ref as R  # noqa: E402
from mld_hip import _lib  # noqa: E402

B, T, V = 64, 60, 6890
PEAK_F32_MATRIX, HBM = 157.3e12, 6.3e12


def window(fn, calls):
    """ms per call over `calls` back-to-back calls, by device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def stats(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(np.min(xs)), "max_ms": float(np.max(xs)), "windows": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "smpl_ab.json"))
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ab_smpl.py measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    feats_np, lens = R.humanact12_batch(B, T)
    valid = int(sum(lens))
    feats = torch.from_numpy(feats_np).to(dev)
    bd = R.body(V)
    m32 = R.as_model(bd, torch.float32, dev)
    res = {"shape": {"B": B, "T": T, "V": V, "frames": B * T, "valid_frames": valid},
           "method": "device events around windows of back-to-back calls after a warm-up, engine / eager windows alternating; ms per call",
           "note": "eager = tests/smpl_ref.py forward(), float32, PyTorch-ROCm on the same GPU; it computes valid frames only, the engine every frame of the [B, T] grid"}
    # what a call needs, from the shapes: the engine multiplies every frame of the grid (padded ones ride along as zero rows of their tiles)
    flop_blend = 2.0 * B * T * 208 * 3 * V
    flop_skin = 2.0 * B * T * 24 * 12 * V + 2.0 * 12 * B * T * V
    bytes_out = 4.0 * B * T * V * 3
    res["needs"] = {"blend_flop": flop_blend, "skinning_flop": flop_skin, "vertex_bytes": bytes_out,
                    "least_ms": 1e3 * max((flop_blend + flop_skin) / PEAK_F32_MATRIX, bytes_out / HBM),
                    "bound": "compute" if (flop_blend + flop_skin) / PEAK_F32_MATRIX > bytes_out / HBM else "memory"}
    engs = {}
    for prec, name in ((0, "engine_f32"), (1, "engine_f16x3")):
        engs[name] = _lib.Engine(device=0, precision=prec, **R.engine_kwargs(V, max_batch=B, max_frames=T))
        R.load_body(engs[name], bd)
    s = torch.cuda.current_stream().cuda_stream
    j = torch.empty(B, T, 24, 3, device=dev)
    v = torch.empty(B, T, V, 3, device=dev)
    legs = {
        "joints_only": {**{n: (lambda e=e: e.smpl_forward(feats, lens, T, j, None, 1, s)) for n, e in engs.items()},
                        "eager_fp32": lambda: R.forward(m32, feats, lens, 1, want_verts=False)},
        "with_vertices": {**{n: (lambda e=e: e.smpl_forward(feats, lens, T, j, v, 1, s)) for n, e in engs.items()},
                          "eager_fp32": lambda: R.forward(m32, feats, lens, 1, want_verts=True)},
    }
    calls = {"joints_only": 200, "with_vertices": 20}
    with torch.no_grad():
        for leg, fns in legs.items():
            for fn in fns.values():                                            # warm-up: code objects, allocator, library algorithm picks
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            ts = {n: [] for n in fns}
            for _ in range(a.repeats):
                for n, fn in fns.items():
                    ts[n].append(window(fn, calls[leg]))
            row = {n: stats(x) for n, x in ts.items()}
            for n in engs:
                row["ratio_eager_over_" + n] = row["eager_fp32"]["median_ms"] / row[n]["median_ms"]
            if leg == "with_vertices":
                row["engine_f32_share_of_least_time"] = res["needs"]["least_ms"] / row["engine_f32"]["median_ms"]
            res[leg] = row
            print(leg, json.dumps(row))
        # both sides against the float64 restatement (one motion at a time on the CPU), under the tests' rule: within 4 x e32, the float32-CPU error
        (rj, e32j), (rv, e32v) = R.reference_per_motion(bd, feats_np, lens, 1)
        out = {"rule": "err = max|output - float64 restatement|, e32 = max|float32-CPU restatement - float64 restatement|; both sides within 4 x e32",
               "e32_joints": e32j, "e32_vertices": e32v, "max_abs_vertices": float(np.abs(rv).max())}
        sides = {n: (lambda e=e: e.smpl_forward(feats, lens, T, j, v, 1, s) or (j, v)) for n, e in engs.items()}
        sides["eager_fp32"] = lambda: R.forward(m32, feats, lens, 1)
        ok = True
        for n, fn in sides.items():
            oj, ov = fn()
            torch.cuda.synchronize()
            ej = float(np.abs(oj.cpu().double().numpy() - rj).max())
            ev = float(np.abs(ov.cpu().double().numpy() - rv).max())
            out[n] = {"err_joints": ej, "err_vertices": ev, "ratio_joints": ej / e32j, "ratio_vertices": ev / e32v}
            ok = ok and ej <= R.F32_FACTOR * e32j and ev <= R.F32_FACTOR * e32v
        out["nonfinite"] = engs["engine_f32"].numeric_status()["nonfinite_values"] + engs["engine_f16x3"].numeric_status()["nonfinite_values"]
        res["outputs"] = out
        print("outputs", json.dumps(out))
    for e in engs.values():
        e.close()
    json.dump(res, open(a.out, "w"), indent=1)
    assert ok and out["nonfinite"] == 0, "the engine and the eager restatement must both match the float64 restatement within 4 x e32 (see outputs)"


if __name__ == "__main__":
    main()
