"""Time the T2M evaluator towers of the engine against the same nets under eager PyTorch-ROCm (tests/t2m_ref.py's modules in float32 on the same GPU: the
baseline -- the parent commit has no evaluator), and as a share of a 1 280-motion sample_many + embed.

  python tools/ab_t2m_eval.py [--out profiles/t2m_eval_ab.json] [--iters 5]

Shapes: the motion tower at 64 and at 1 280 motions x 196 frames, the text tower at 1 280 captions x 20 words, both arithmetic modes.  The per-stage split of
the motion tower (convolutions / linears + input GEMM / recurrence / head) is read from the engine by timing calls that stop early: motions of ONE GRU step
(lengths 4..7) run everything but 48 of the 49 recurrence launches, so recurrence ~ full - one-step; the eager baseline is split the same way."""
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
import t2m_ref as R  # noqa: E402
from mld_hip import _lib  # noqa: E402
from mld_hip import synthetic as syn  # noqa: E402


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "t2m_eval_ab.json"))
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"unit": "ms per call, median of %d" % a.iters, "shapes": {}, "note": "eager = tests/t2m_ref.py modules, float32, PyTorch-ROCm on the same GPU"}
    _, m32 = R.models()
    m32 = m32.to(dev)
    st = tuple(torch.from_numpy(s).to(dev) for s in R.stats())
    rng = np.random.default_rng(0)
    for B in (64, 1280):
        lens = [int(x) for x in 4 * rng.integers(10, 50, size=B)]
        lens[0] = 196
        feats = torch.from_numpy(R.make_motions(lens, 196, seed=B)).to(dev)
        short = [4 + (i % 4) for i in range(B)]
        out = torch.empty(B, 512, device=dev)
        row = {}
        with torch.no_grad():
            row["eager_fp32"] = timed(lambda: m32.motion_embed(feats, lens, st), a.iters)
            row["eager_fp32_one_step"] = timed(lambda: m32.motion_embed(feats, short, st), a.iters)
        for prec, name in ((0, "engine_f32"), (1, "engine_f16x3")):
            eng = _lib.Engine(device=0, precision=prec, **R.engine_kwargs(1280, max_frames=196, max_words=20))
            R.load_evaluators(eng)
            s = torch.cuda.current_stream().cuda_stream
            row[name] = timed(lambda: eng.t2m_motion_embed(feats, lens, 196, out, stream=s), a.iters)
            row[name + "_one_step"] = timed(lambda: eng.t2m_motion_embed(feats, short, 196, out, stream=s), a.iters)
            row[name + "_recurrence_share"] = 1.0 - row[name + "_one_step"] / row[name]
            if B == 1280:
                tl = [int(x) for x in rng.integers(1, 21, size=B)]
                w, p = R.make_captions(tl, 20, seed=1)
                wd, pd = torch.from_numpy(w).to(dev), torch.from_numpy(p).to(dev)
                trow = res["shapes"].setdefault("text 1280 x 20", {})
                trow[name] = timed(lambda: eng.t2m_text_embed(wd, pd, tl, 20, out, s), a.iters)
                if prec == 0:
                    with torch.no_grad():
                        trow["eager_fp32"] = timed(lambda: m32.text_embed(wd, pd, tl), a.iters)
                trow[name + "_numeric"] = eng.numeric_status()
            eng.close()
        row["ratio_eager_over_engine_f16x3"] = row["eager_fp32"] / row["engine_f16x3"]
        row["ratio_eager_over_engine_f32"] = row["eager_fp32"] / row["engine_f32"]
        res["shapes"]["motion %d x 196" % B] = row
        print("motion %d x 196:" % B, json.dumps(row))
    print("text:", json.dumps(res["shapes"]["text 1280 x 20"], default=str))
    json.dump(res, open(a.out, "w"), indent=1, default=str)

    # the towers as a share of a 1 280-motion sample_many + embed (F16X3, the serving mode): 20 requests of 64 motions, then ONE embed of the 1 280 generated motions
    eng = _lib.Engine(device=0, precision=1, max_batch=1280, max_frames=196, t2m_eval=1, t2m_max_motions=1280)
    eng.load_state_dict(syn.make_denoiser_state_dict(), "denoiser.")
    eng.load_state_dict(syn.make_vae_state_dict(), "vae.")
    R.load_evaluators(eng)
    reqs, lens_all = [], []
    for i in range(20):
        b = syn.make_batch(64, "ragged", seed=100 + i)
        T = max(b.lengths)
        reqs.append(dict(text_emb=torch.from_numpy(b.text_emb).to(dev), init_latents=torch.from_numpy(b.init_latents).to(dev), lengths=b.lengths,
                         feats_out=torch.zeros(64, T, 263, device=dev)))
        lens_all += b.lengths
    allf = torch.zeros(1280, 196, 263, device=dev)
    out = torch.empty(1280, 512, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    t_sample = timed(lambda: eng.sample_many(reqs, s), 3)
    for i, q in enumerate(reqs):
        allf[64 * i:64 * i + 64, :q["feats_out"].shape[1]] = q["feats_out"]
    t_embed = timed(lambda: eng.t2m_motion_embed(allf, lens_all, 196, out, stream=s), 3)
    res["sample_many_1280_plus_embed"] = {"sample_many_ms": t_sample, "motion_embed_ms": t_embed, "embed_share": t_embed / (t_sample + t_embed)}
    print("share:", json.dumps(res["sample_many_1280_plus_embed"]))
    eng.close()
    json.dump(res, open(a.out, "w"), indent=1, default=str)


if __name__ == "__main__":
    main()
