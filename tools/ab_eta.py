"""Cost of stochastic DDIM: eta 0 against eta 0.5 on one box, same weights, same inputs, interleaved rounds.
  python tools/ab_eta.py [--rounds 7] [--out profiles/ab_eta.json]
Shapes: one bs-64 request (the cluster loop, F16X3) and 1 280 motions per call (the sample-major persistent loop).  Reported per shape and eta: ms
per reverse loop (latents out only) and per full call (decode + joints), median / min over the rounds; the eta 0.5 engine samples through
mldhip_sample_many_seeded (its keys are uploaded every call), the eta 0 engine through mldhip_sample_many."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "motion-latent-diffusion_amd")]
import numpy as np
import torch
from mld_hip import _lib, synthetic as syn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ab_eta.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5, help="calls per timed sample")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sdd, sdv = syn.make_denoiser_state_dict(), syn.make_vae_state_dict()
    mean, std = syn.make_mean_std()
    out = {"what": __doc__.split("\n")[0], "rounds": a.rounds, "reps": a.reps, "shapes": {}}
    for name, B, T in (("bs64_cluster", 64, 196), ("b1280_persistent", 1280, 196)):
        bb = syn.make_batch(B, [T] * B)
        te, x0 = torch.from_numpy(bb.text_emb).to(dev), torch.from_numpy(bb.init_latents).to(dev)
        engines = {}
        for eta in (0.0, 0.5):
            e = _lib.Engine(device=0, max_batch=B, max_frames=T, precision=1, eta=eta)
            e.load_state_dict(sdd, "denoiser."); e.load_state_dict(sdv, "vae."); e.load_tensor("mean", mean); e.load_tensor("std", std); e.finalize()
            lat, j = torch.empty(B, 1, 256, device=dev), torch.empty(B, T, 22, 3, device=dev)
            rl = dict(text_emb=te, init_latents=x0, lengths=bb.lengths, latents_out=lat)
            rf = dict(rl, joints_out=j)

            def call(r, e=e, eta=eta, k=[0]):
                k[0] += 1
                if eta == 0.0:
                    e.sample_many([r])
                else:
                    e.sample_many_seeded([r], [(k[0], 0)])                # a new seed every call: replays the captured graph
            call(rl); call(rf); torch.cuda.synchronize()
            engines[eta] = (e, call, rl, rf, [], [])
        for _ in range(a.rounds):
            for eta, (e, call, rl, rf, tl, tf) in engines.items():
                for r, acc in ((rl, tl), (rf, tf)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.reps):
                        call(r)
                    torch.cuda.synchronize()
                    acc.append((time.perf_counter() - t0) * 1e3 / a.reps)
        res = {"motions": B, "frames": T}
        for eta, (e, call, rl, rf, tl, tf) in engines.items():
            res["eta_%g" % eta] = {"loop_ms_median": float(np.median(tl)), "loop_ms_min": float(np.min(tl)), "full_ms_median": float(np.median(tf)),
                                   "full_ms_min": float(np.min(tf)), "launches": e.launch_counts(), "numeric": e.numeric_status()}
        z, h = res["eta_0"], res["eta_0.5"]
        res["cost_loop_pct_median"] = 100.0 * (h["loop_ms_median"] / z["loop_ms_median"] - 1.0)
        res["cost_loop_pct_min"] = 100.0 * (h["loop_ms_min"] / z["loop_ms_min"] - 1.0)
        res["cost_full_pct_median"] = 100.0 * (h["full_ms_median"] / z["full_ms_median"] - 1.0)
        print(name, json.dumps(res), flush=True)
        out["shapes"][name] = res
        for e, *_ in engines.values():
            e.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("->", a.out)


if __name__ == "__main__":
    main()
