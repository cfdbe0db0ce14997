"""sha256 of every output of the decoder / encoder row-strip kernels over a fixed list of cases: the bit identity of two BUILDS of the library.
  python tools/decoder_digests.py --lib PATH [--sim] --out FILE
Run it on the library of the parent commit and on this tree's and compare the two files (`cmp`, or --against FILE: exit status 1 when a digest
differs).  A change that reorders no sum must leave every digest as it is, on the GPU and in the simulator (--sim: PATH is a `make sim` build,
the suite's 3-layer model of tests/simlib.py).

Cases: split-f16 precision, "gemm_small_m" 0, synthetic weights, seeded inputs, B = 3, lengths [T, 1, 5T/8]:
  T = 16   48 rows: exactly one 48-row strip, a partial 64- and 96-row strip
  T = 49   147 rows: a partial last strip at every height, strips that straddle two samples (the per-row sample index, the cvec row)
  T = 196  588 rows: the length-1 sample leaves 48-, 64- and 96-row strips made only of padded frames (the uniform exit at every height)
each under ("strip_gemm", "ffn_strip", "dec_tail", "dec_lean") = (1,6,1,1) (1,4,1,1) (1,3,1,1) (1,3,1,0) (1,3,0,1), and "dec_half" 4 / 6 / 2 on
(1,3,1,1) (numeric_status recorded: a veto of finalize's probe is visible as decode_half_ok 0, and the case then runs the fp32 form; 2 = the half
form forced, 64-row strips, which no probe can veto).  Per case: a joints-only sample call of 2 steps (the only entry that ends in
final_joints_x3_kernel, under "dec_lean"; its digest covers the two denoiser steps as well), vae_decode to features (final_strip_x3_kernel) and from
them feats2joints, vae_encode (the K = 512 skip linear), and the handle's launch counts.  launch_counts() counts launches, it names no kernel: to see
WHICH kernels a run launched, run this tool under a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/decoder_digests.py ...).  Which instantiation a case reaches (engine/path_vae.hpp): 96-row forms under "ffn_strip" 6, 64-row forms under 4 and -- at these row
counts -- for the GEMMs under 3; the fused tail and its layer-0 form under (.,3,1,1), the plain tail under (.,3,1,0), ffn_strip_x3_kernel<3> and the
LayerNorm GEMM under (.,3,0,.); strip_inproj_h_kernel<4 / 6> under "dec_half" 4 / 6."""
import argparse, hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "motion-latent-diffusion_amd")]
import numpy as np
from mld_hip import _lib, synthetic as syn

OPTION_SETS = ((1, 6, 1, 1), (1, 4, 1, 1), (1, 3, 1, 1), (1, 3, 1, 0), (1, 3, 0, 1))
OPTION_NAMES = ("strip_gemm", "ffn_strip", "dec_tail", "dec_lean")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--sim", action="store_true", help="--lib is the simulator build: host memory, the 3-layer model")
    ap.add_argument("--out", required=True)
    ap.add_argument("--against", help="a file written by an earlier run: compare every digest")
    a = ap.parse_args()
    lib = _lib.load_library(os.path.abspath(a.lib))
    if a.sim:
        dims = syn.ModelDims(num_layers=3)
        dev_of = lambda x: np.ascontiguousarray(x)
        empty = lambda *s: np.full(s, np.nan, np.float32)
        host, sync = (lambda x: x), (lambda: None)
    else:
        import torch
        dims = syn.ModelDims()
        dev = torch.device("cuda:0")
        dev_of = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        empty = lambda *s: torch.full(s, float("nan"), device=dev)
        host, sync = (lambda x: x.cpu().numpy()), torch.cuda.synchronize
    sdd, sdv = syn.make_denoiser_state_dict(dims=dims), syn.make_vae_state_dict(dims=dims)
    mean, std = syn.make_mean_std()
    sha = lambda x: hashlib.sha256(np.ascontiguousarray(host(x)).tobytes()).hexdigest()
    out = {"what": __doc__.split("\n")[0], "simulator": bool(a.sim), "cases": {}}
    for T in (16, 49, 196):
        lens = [T, 1, 5 * T // 8]
        b = syn.make_batch(3, lens, seed=100 + T)
        g = syn._rng(200 + T, "decoder_digests")
        z = g.standard_normal((3, 1, 256)).astype(np.float32)
        fin = g.standard_normal((3, T, 263)).astype(np.float32)
        eps = g.standard_normal((3, 256)).astype(np.float32)
        for dh in (0, 4, 6, 2):
            extra = dict(use_graph=0, num_layers=3) if a.sim else {}
            e = _lib.Engine(lib=lib, device=0, precision=1, max_batch=4, max_frames=T, num_inference_steps=2, **extra)
            e.load_state_dict(sdd, "denoiser."); e.load_state_dict(sdv, "vae.")
            e.load_tensor("mean", mean); e.load_tensor("std", std)
            e.set_option("gemm_small_m", 0)
            if dh:
                e.set_option("dec_half", dh)
            e.finalize()
            for opts in (OPTION_SETS if dh == 0 else ((1, 3, 1, 1),)):
                for k, v in zip(OPTION_NAMES, opts):
                    e.set_option(k, v)
                lat, joints, feats = empty(3, 1, 256), empty(3, T, 22, 3), empty(3, T, 263)
                el, mu, lv = empty(3, 1, 256), empty(3, 1, 256), empty(3, 1, 256)
                counts = {}                                 # launch_counts() holds the last call's launches (denoiser, decoder, encoder)
                e.sample(dev_of(b.text_emb), dev_of(b.init_latents), lens, lat, None, joints)
                counts["sample"] = e.launch_counts()
                e.vae_decode(dev_of(z), lens, feats)
                counts["decode"] = e.launch_counts()
                dj = empty(3, T, 22, 3)
                e.feats2joints(feats, 3, T, dj)
                e.vae_encode(dev_of(fin), lens, T, dev_of(eps), el, mu, lv)
                counts["encode"] = e.launch_counts()
                sync()
                case = {"launches": counts,
                        "sha256": {"sample_latents": sha(lat), "sample_joints": sha(joints), "decode_feats": sha(feats), "decode_joints": sha(dj), "encode_latent": sha(el),
                                   "encode_mu": sha(mu), "encode_logvar": sha(lv)}}
                if dh:
                    s = e.numeric_status()
                    case["numeric_status"] = {k: s[k] for k in ("decode_half_ok", "probe_err_decode_half", "decode_split_ok")}
                name = "T%d opts%s dec_half%d" % (T, "".join(map(str, opts)), dh)
                out["cases"][name] = case
                print(name, counts["sample"], counts["decode"], counts["encode"], case["sha256"]["sample_joints"][:12], case["sha256"]["decode_feats"][:12], case["sha256"]["encode_mu"][:12], flush=True)
            e.close()
    json.dump(out, open(a.out, "w"), indent=1, sort_keys=True)
    print("->", a.out)
    if a.against:
        old = json.load(open(a.against))["cases"]
        bad = [k for k, c in out["cases"].items() if old.get(k, {}).get("sha256") != c["sha256"] or old.get(k, {}).get("launches") != c["launches"]]
        print("against", a.against, ":", "%d of %d cases differ %s" % (len(bad), len(out["cases"]), bad) if bad else "every case equal")
        if bad or set(old) != set(out["cases"]):
            sys.exit(1)


if __name__ == "__main__":
    main()
