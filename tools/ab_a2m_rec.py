"""Time the HumanAct12 recognition GRU of the engine (mldhip_a2m_recognize) against the project's restatement (tests/a2m_rec_ref.py: nn.GRU(72, 128, 2) +
Linear + tanh + Linear) under eager PyTorch-ROCm, float32, on the same GPU in the same process (the baseline: the parent commit has no recognizer).

  python tools/ab_a2m_rec.py [--out profiles/a2m_rec_ab.json] [--repeats 21]

Shapes: B = 128 rows (one metric update's four passes over 32 motions) and B = 1 024 rows, T = 60 frames, ragged lengths (tests/a2m_rec_ref.make_case),
PyTorch's default-init weight family.  First both sides are compared with the float64 restatement on the CPU under the tests' rule (within 4 x the
float32-CPU error, logits and activations); the tool stops, after writing its figures, when one side misses it.  Timing: device events around windows
of back-to-back calls on one stream after a warm-up, engine and eager windows alternating, `repeats` windows each; the median and the spread (min,
max) of the per-call time are written."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "motion-latent-diffusion_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import a2m_rec_ref as R  # noqa: E402
from mld_hip import _lib  # noqa: E402

T = 60
SHAPES = (128, 1024)
CALLS = 10


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "a2m_rec_ab.json"))
    ap.add_argument("--repeats", type=int, default=21)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ab_a2m_rec.py measures on the GPU; there is nothing to report without one"
    assert a.repeats >= 20, "at least 20 alternated windows per side"
    dev = torch.device("cuda:0")
    sd = R.weights("default")
    mods = R.modules(sd, torch.float32, dev)
    s = torch.cuda.current_stream().cuda_stream
    res = {"T": T, "calls_per_window": CALLS,
           "method": "device events around windows of back-to-back calls after a warm-up, engine / eager windows alternating; ms per call, median over the windows",
           "note": "eager = tests/a2m_rec_ref.py forward(): nn.GRU + Linears, float32, PyTorch-ROCm on the same GPU in the same process"}
    ok = True
    for B in SHAPES:
        jn, lens, h0n = R.make_case(B, T)
        (rl, el), (ra, ea) = R.reference(sd, jn, lens, h0n)
        j, h0 = torch.from_numpy(jn).to(dev), torch.from_numpy(h0n).to(dev)
        eng = _lib.Engine(device=0, precision=0, **R.engine_kwargs(max_batch=B // 4, max_frames=T))
        R.load(eng, sd)
        lo, ac = torch.empty(B, 12, device=dev), torch.empty(B, 30, device=dev)
        fns = {"engine": lambda: eng.a2m_recognize(j, lens, T, h0, lo, ac, s),
               "eager_fp32": lambda: R.forward(mods, j, lens, h0)}
        row = {"B": B, "rule": "err = max|output - float64 restatement|, e32 = max|float32-CPU restatement - float64 restatement|; both sides within 4 x e32",
               "e32_logits": el, "e32_act": ea}
        with torch.no_grad():
            outs = {"engine": (fns["engine"]() or (lo, ac)), "eager_fp32": fns["eager_fp32"]()}
            torch.cuda.synchronize()
            for n, (ol, oa) in outs.items():
                errl = float(np.abs(ol.cpu().double().numpy() - rl).max())
                erra = float(np.abs(oa.cpu().double().numpy() - ra).max())
                row[n + "_parity"] = {"err_logits": errl, "err_act": erra, "ratio_logits": errl / el, "ratio_act": erra / ea}
                ok = ok and errl <= R.F32_FACTOR * el and erra <= R.F32_FACTOR * ea
            row["engine_nonfinite"] = eng.numeric_status()["nonfinite_values"]
            ok = ok and row["engine_nonfinite"] == 0
            if ok:
                for fn in fns.values():                                    # warm-up: code objects, allocator, library algorithm picks
                    for _ in range(5):
                        fn()
                torch.cuda.synchronize()
                ts = {n: [] for n in fns}
                for _ in range(a.repeats):
                    for n, fn in fns.items():
                        ts[n].append(window(fn, CALLS))
                row.update({n: stats(x) for n, x in ts.items()})
                row["ratio_eager_over_engine"] = row["eager_fp32"]["median_ms"] / row["engine"]["median_ms"]
        eng.close()
        res[f"B{B}"] = row
        print(f"B {B}", json.dumps(row))
        if not ok:
            break
    json.dump(res, open(a.out, "w"), indent=1)
    assert ok, "the engine and the eager restatement must both match the float64 restatement within 4 x e32 (see the parity entries)"


if __name__ == "__main__":
    main()
