"""Time the UESTC recognition ST-GCN of the engine (mldhip_uestc_recognize), both arithmetic modes, against the project's restatement of the same net
(tests/uestc_rec_ref.py forward(): conv2d / einsum / BatchNorm affines) under eager PyTorch-ROCm, float32, on the same GPU in the same process (the
baseline: the parent commit has no such net).

  python tools/ab_uestc_rec.py [--out profiles/uestc_rec_ab.json] [--repeats 21]

Shapes: 2 x 64 and 2 x 512 motions (generated + ground truth of one metric update) at T = 60 frames, the default weight family.  First every side is
compared with the float64 restatement on the CPU under the tests' rule (F32 engine and eager within 4 x, F16X3 engine within 16 x the float32-CPU
error; logits and features) on the FIRST 16 MOTIONS of its full-batch output -- a motion's outputs do not depend on the rest of the batch, and float64
on the CPU costs 3 GFLOP per motion; the tool stops, after writing its figures, when one side misses it.  Timing: wall-clock time of windows of
back-to-back calls on one stream after a warm-up, each window closed by a device synchronisation, the three sides alternating, `repeats` windows
each; the median and the spread (min, max) of the per-call time are written.  The per-stage split (GEMMs / mix / staging / head) comes from a kernel
trace of this tool's --one-call mode (6 calls of the F32 engine at 2 x 64 motions and nothing else), summed by kernel name."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "motion-latent-diffusion_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import uestc_rec_ref as R  # noqa: E402
from mld_hip import _lib  # noqa: E402

T = 60
SHAPES = (128, 1024)
CALLS = 5
CHECK = 16


def window(fn, calls):
    """wall-clock ms per call over `calls` back-to-back calls, closed by a device synchronisation"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def stats(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(np.min(xs)), "max_ms": float(np.max(xs)), "windows": len(xs)}


def engine(prec, B):
    eng = _lib.Engine(device=0, precision=prec, **R.engine_kwargs(max_batch=B // 2, max_frames=T))
    R.load(eng, R.weights("default"))
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "uestc_rec_ab.json"))
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--one-call", action="store_true", help="one warm call and 5 calls of the F32 engine at 2 x 64 motions, nothing else (for a kernel trace)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ab_uestc_rec.py measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    if a.one_call:
        B = SHAPES[0]
        eng = engine(0, B)
        m = torch.from_numpy(R.make_case(B, T)).to(dev)
        lo, fe = torch.empty(B, R.NC, device=dev), torch.empty(B, 256, device=dev)
        for _ in range(6):
            eng.uestc_recognize(m, m.stride(), B, T, lo, fe, s)
        torch.cuda.synchronize()
        eng.close()
        return
    assert a.repeats >= 20, "at least 20 alternated windows per side"
    sd = R.weights("default")
    w32 = R.tensors(sd, torch.float32, dev)
    res = {"T": T, "calls_per_window": CALLS,
           "method": "wall clock around windows of back-to-back calls after a warm-up, each closed by a device synchronisation, the sides alternating; ms per call, median over the windows",
           "note": "eager = tests/uestc_rec_ref.py forward(): conv2d / einsum / BatchNorm affines, float32, PyTorch-ROCm on the same GPU in the same process"}
    ok = True
    for B in SHAPES:
        mn = R.make_case(B, T)
        (rl, el), (rf, ef) = R.reference(sd, mn[:CHECK])
        m = torch.from_numpy(mn).to(dev)
        engs = {"engine_f32": engine(0, B), "engine_f16x3": engine(1, B)}
        bufs = {n: (torch.empty(B, R.NC, device=dev), torch.empty(B, 256, device=dev)) for n in engs}
        fns = {n: (lambda n=n: engs[n].uestc_recognize(m, m.stride(), B, T, bufs[n][0], bufs[n][1], s)) for n in engs}
        fns["eager_fp32"] = lambda: R.forward(w32, m)
        row = {"B": B, "rule": f"err = max|output - float64 restatement| on the first {CHECK} motions, e32 = max|float32-CPU restatement - float64 restatement|; "
                               "F32 engine and eager within 4 x e32, F16X3 engine within 16 x e32", "e32_logits": el, "e32_feat": ef,
               "probe_err_uestc": engs["engine_f16x3"].numeric_status()["probe_err_uestc"], "uestc_split_ok": engs["engine_f16x3"].numeric_status()["uestc_split_ok"]}
        with torch.no_grad():
            outs = {n: (fns[n]() or bufs[n]) for n in engs}
            outs["eager_fp32"] = fns["eager_fp32"]()
            torch.cuda.synchronize()
            for n, (ol, of) in outs.items():
                errl = float(np.abs(ol[:CHECK].cpu().double().numpy() - rl).max())
                errf = float(np.abs(of[:CHECK].cpu().double().numpy() - rf).max())
                f = R.X3_FACTOR if n == "engine_f16x3" else R.F32_FACTOR
                row[n + "_parity"] = {"err_logits": errl, "err_feat": errf, "ratio_logits": errl / el, "ratio_feat": errf / ef, "bound": f}
                ok = ok and errl <= f * el and errf <= f * ef
            row["engine_nonfinite"] = sum(e.numeric_status()["nonfinite_values"] for e in engs.values())
            ok = ok and row["engine_nonfinite"] == 0
            if ok:
                for fn in fns.values():                                    # warm-up: code objects, allocator, library algorithm picks
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                ts = {n: [] for n in fns}
                for _ in range(a.repeats):
                    for n, fn in fns.items():
                        ts[n].append(window(fn, CALLS))
                row.update({n: stats(x) for n, x in ts.items()})
                for n in engs:
                    row[f"ratio_eager_over_{n}"] = row["eager_fp32"]["median_ms"] / row[n]["median_ms"]
        for e in engs.values():
            e.close()
        res[f"B{B}"] = row
        print(f"B {B}", json.dumps(row))
        if not ok:
            break
    json.dump(res, open(a.out, "w"), indent=1)
    assert ok, "every side must match the float64 restatement within its bound (see the parity entries)"


if __name__ == "__main__":
    main()
