"""A/B of the CLIP text tower: PyTorch-ROCm eager (timed exactly as bench.py's bench_text_encoder times it) against the engine's
mldhip_text_encode in MLDHIP_PREC_F16X3 and MLDHIP_PREC_F32, in ONE process, at the bench's shape: 12 layers, 128 prompts of 77
ids, random-init weights (the same tensors in both towers).  Three prompt sets:
  (a) like for like: 128 distinct prompts with EOS at 76;
  (b) a real CFG batch: 64 "" prompts + 64 distinct prompts (EOS at 76);
  (c) short prompts: the batch of (b) with EOS positions drawn uniformly from 5..25 (fixed seed).
The torch tower always runs the padded [128][77] batch (that is what it does).  Run by hand on the GPU, under a time limit:
  timeout 600 python tools/ab_text_tower.py --out profiles/text_tower_ab.json
Interleaved rounds, median of the rounds per arm, every arm warmed up; a result is a "win" only if the ranges of the rounds do not overlap."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "motion-latent-diffusion_amd"))
from mld_hip import _lib  # noqa: E402

P, CTX, VOCAB, EOS = 128, 77, 49408, 49407


def prompt_sets():
    rng = np.random.default_rng(2024)

    def build(eos_pos, empty):
        ids = np.full((P, CTX), EOS, dtype=np.int64)
        for p, e in enumerate(eos_pos):
            ids[p, 0] = EOS - 1
            if not empty[p]:
                ids[p, 1:e] = rng.integers(0, EOS - 1, size=e - 1)
        return ids, np.asarray(eos_pos, dtype=np.int32)
    none, half = [False] * P, [True] * (P // 2) + [False] * (P // 2)
    short = [1] * (P // 2) + [int(x) for x in rng.integers(5, 26, size=P // 2)]
    return {"a_distinct_eos76": build([76] * P, none), "b_cfg_eos76": build([1] * (P // 2) + [76] * (P // 2), half),
            "c_cfg_short_5_25": build(short, half)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "text_tower_ab.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--hip-only", action="store_true", help="one warmed F16X3 pass per prompt set and nothing else (for rocprofv3 --kernel-trace --stats)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    cfg = CLIPTextConfig(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, projection_dim=768,
                         vocab_size=VOCAB, max_position_embeddings=CTX)
    torch.manual_seed(0)
    model = CLIPTextModelWithProjection(cfg).eval().to(dev)
    tensors = {"text_encoder.text_model." + k: v for k, v in model.state_dict().items() if v.dtype.is_floating_point}
    engines = {}
    for name, prec in (("hip_f16x3", 1), ("hip_f32", 0)):
        if a.hip_only and prec == 0:
            continue
        eng = _lib.Engine(device=0, precision=prec, num_layers=3, max_batch=64, max_frames=16, clip_layers=12, clip_max_prompts=P)
        for k, v in tensors.items():
            eng.load_tensor(k, v)
        eng.finalize()
        engines[name] = eng
    sets = prompt_sets()
    out = torch.empty(P, 1, 768, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def time_arm(fn, iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e3

    result = {"shape": {"prompts": P, "ctx": CTX, "layers": 12, "width": 768, "ff": 3072}, "rounds": a.rounds, "iters_per_round": a.iters,
              "method": "one process, arms interleaved round by round, 3 warm-up calls per arm, wall clock around `iters` back-to-back calls + device sync "
                        "(bench.py bench_text_encoder's method for the torch arm); median [min, max] of the rounds, ms per 128 prompts; the HIP arms include "
                        "the host-side dedupe, the table upload and the launches of the call", "sets": {}}
    for sname, (ids, eos) in sets.items():
        tid = torch.from_numpy(ids).to(dev)
        arms = {"torch_f32": lambda: model(input_ids=tid)}
        for name, eng in engines.items():
            arms[name] = (lambda e: (lambda: e.text_encode(ids, eos, out, stream)))(eng)
        if a.hip_only:
            arms.pop("torch_f32")
        with torch.no_grad():
            for fn in arms.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            if a.hip_only:
                continue
            samples = {k: [] for k in arms}
            for _ in range(a.rounds):
                for k, fn in arms.items():
                    samples[k].append(time_arm(fn, a.iters))
        uniq = {tuple(ids[p, :eos[p] + 1]) for p in range(P)}
        rec = {"unique_prompts": len(uniq), "token_rows": int(sum(len(u) for u in uniq)), "padded_rows": P * CTX}
        for k, v in samples.items():
            rec[k] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
        # parity of the arms on this set (random-init weights; the tolerance tests live in tests/test_gpu_text_tower.py)
        with torch.no_grad():
            ref = model(input_ids=tid).text_embeds
        for name, eng in engines.items():
            eng.text_encode(ids, eos, out, stream)
            torch.cuda.synchronize()
            rec[name]["max_abs_vs_torch"] = float((out[:, 0] - ref).abs().max())
        for name in engines:
            rec[name]["verdict_vs_torch"] = ("faster (ranges do not overlap)" if rec[name]["max_ms"] < rec["torch_f32"]["min_ms"] else
                                             "slower (ranges do not overlap)" if rec[name]["min_ms"] > rec["torch_f32"]["max_ms"] else "tie (ranges overlap)")
        result["sets"][sname] = rec
        print(sname, json.dumps(rec))
    if a.hip_only:
        torch.cuda.synchronize()
        return
    json.dump(result, open(a.out, "w"), indent=1)
    print("wrote", a.out)
    for eng in engines.values():
        eng.close()


if __name__ == "__main__":
    main()
