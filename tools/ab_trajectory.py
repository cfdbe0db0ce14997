"""Cost of the per-step trajectory (mldhip_sample_many_traj) on one box: the no-trajectory headline of the parent commit against this tree, and
one bs-64 call with a trajectory against the same call without one.
  python tools/ab_trajectory.py --parent DIR [--runs 3] [--append] [--out profiles/traj_ab.json]
DIR is a built checkout of the parent commit (its own libmldhip.so beside its bench.py).  Three legs:
- headline: `bench.py --gpus 1 --steps 20 --warmup 5`, --runs times per tree, alternating parent / branch, each run a fresh process; the verdict is
  whether the branch's median lies inside the parent's min..max of this session (exit status 1 when not).  --append keeps the sessions --out already
  holds and adds this one: every session made is kept, whatever its verdict.
- bs-64 parent against branch: one F16X3 request of 64 motions, T = 196 (the cluster loop) through sample_many on each tree's library, --runs fresh
  processes each, alternating.  Reported only.
- bs-64 pair: the same request on ONE handle of this tree, interleaved rounds of sample_many_traj with and without a [50, 64, 256] traj_out (both
  graphs captured before timing); ms per reverse loop (latents out only) and per full call.  Reported only."""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "motion-latent-diffusion_amd")]
import numpy as np


def headline(tree, timeout):
    """one bench.py run of `tree` in a child process -> its result line"""
    env = dict(os.environ, MLD_BENCH_EVIDENCE=os.devnull)
    r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=tree, env=env,
                       capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.exit("bench.py of %s ended with %d:\n%s" % (tree, r.returncode, r.stderr[-2000:]))
    line = json.loads(r.stdout.strip().splitlines()[-1])
    return {"value": line["value"], "ms_per_step": line["ms_per_step"]}


def bs64_plain(tree, rounds, reps):
    """--child: one bs-64 request without a trajectory on the library of `tree` -> ms per reverse loop (latents out only) and per full call"""
    sys.path[:0] = [tree, os.path.join(tree, "motion-latent-diffusion_amd")]
    import torch
    from mld_hip import _lib, synthetic as syn
    assert os.path.abspath(_lib.DEFAULT_LIB).startswith(tree + os.sep), _lib.DEFAULT_LIB
    dev = torch.device("cuda:0")
    B, T = 64, 196
    e = _lib.Engine(device=0, max_batch=B, max_frames=T, precision=1)
    e.load_state_dict(syn.make_denoiser_state_dict(), "denoiser."); e.load_state_dict(syn.make_vae_state_dict(), "vae.")
    mean, std = syn.make_mean_std()
    e.load_tensor("mean", mean); e.load_tensor("std", std); e.finalize()
    bb = syn.make_batch(B, [T] * B)
    rl = dict(text_emb=torch.from_numpy(bb.text_emb).to(dev), init_latents=torch.from_numpy(bb.init_latents).to(dev), lengths=bb.lengths,
              latents_out=torch.empty(B, 1, 256, device=dev))
    rf = dict(rl, joints_out=torch.empty(B, T, 22, 3, device=dev))
    e.sample_many([rl]); e.sample_many([rf]); torch.cuda.synchronize()
    tl, tf = [], []
    for _ in range(rounds):
        for r, acc in ((rl, tl), (rf, tf)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                e.sample_many([r])
            torch.cuda.synchronize()
            acc.append((time.perf_counter() - t0) * 1e3 / reps)
    res = {"loop_ms_median": float(np.median(tl)), "loop_ms_min": float(np.min(tl)), "full_ms_median": float(np.median(tf)), "full_ms_min": float(np.min(tf)),
           "launches": e.launch_counts(), "cluster_loop": e.numeric_status()["cluster_loop"]}
    e.close()
    return res


def bs64_trees(parent, runs, rounds, reps, timeout):
    out = {"what": "one bs-64 request WITHOUT a trajectory (sample_many, cluster loop), parent tree against this tree, %d fresh processes each, alternating" % runs,
           "parent": [], "branch": []}
    for i in range(runs):
        for name, tree in (("parent", parent), ("branch", ROOT)):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, "--rounds", str(rounds), "--reps", str(reps)], cwd=tree,
                               capture_output=True, text=True, timeout=timeout)
            if r.returncode != 0:
                sys.exit("bs-64 child of %s ended with %d:\n%s" % (tree, r.returncode, r.stderr[-2000:]))
            out[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print("bs64", name, i, json.dumps(out[name][-1]), flush=True)
    for k in ("loop_ms_median", "full_ms_median"):
        pm, bm = float(np.median([h[k] for h in out["parent"]])), float(np.median([h[k] for h in out["branch"]]))
        out[k] = {"parent": pm, "branch": bm, "branch_over_parent": bm / pm}
    return out


def bs64_pair(rounds, reps):
    import torch
    from mld_hip import _lib, synthetic as syn
    dev = torch.device("cuda:0")
    B, T, n = 64, 196, 50
    e = _lib.Engine(device=0, max_batch=B, max_frames=T, precision=1)
    e.load_state_dict(syn.make_denoiser_state_dict(), "denoiser."); e.load_state_dict(syn.make_vae_state_dict(), "vae.")
    mean, std = syn.make_mean_std()
    e.load_tensor("mean", mean); e.load_tensor("std", std); e.finalize()
    bb = syn.make_batch(B, [T] * B)
    rl = dict(text_emb=torch.from_numpy(bb.text_emb).to(dev), init_latents=torch.from_numpy(bb.init_latents).to(dev), lengths=bb.lengths,
              latents_out=torch.empty(B, 1, 256, device=dev))
    rf = dict(rl, joints_out=torch.empty(B, T, 22, 3, device=dev))
    traj = torch.empty(n, B, 256, device=dev)
    legs = {"without": ({}, [], []), "with": ({"traj_out": traj}, [], [])}
    for extra, _, _ in legs.values():
        for r in (rl, rf):
            e.sample_many_traj([dict(r, **extra)])
    torch.cuda.synchronize()
    launches = {}
    for _ in range(rounds):
        for name, (extra, tl, tf) in legs.items():
            for r, acc in ((rl, tl), (rf, tf)):
                q = [dict(r, **extra)]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    e.sample_many_traj(q)
                torch.cuda.synchronize()
                acc.append((time.perf_counter() - t0) * 1e3 / reps)
            launches[name] = e.launch_counts()
    same = bool(torch.equal(traj[n - 1], rl["latents_out"][:, 0]))
    res = {"motions": B, "frames": T, "steps": n, "trajectory_bytes": n * B * 256 * 4, "rounds": rounds, "calls_per_timed_sample": reps,
           "last_row_equals_latents": same, "numeric": e.numeric_status()}
    for name, (_, tl, tf) in legs.items():
        res[name] = {"loop_ms_median": float(np.median(tl)), "loop_ms_min": float(np.min(tl)), "full_ms_median": float(np.median(tf)),
                     "full_ms_min": float(np.min(tf)), "launches": launches[name]}
    res["cost_loop_pct_median"] = 100.0 * (res["with"]["loop_ms_median"] / res["without"]["loop_ms_median"] - 1.0)
    res["cost_loop_pct_min"] = 100.0 * (res["with"]["loop_ms_min"] / res["without"]["loop_ms_min"] - 1.0)
    res["cost_full_pct_median"] = 100.0 * (res["with"]["full_ms_median"] / res["without"]["full_ms_median"] - 1.0)
    e.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--child", metavar="TREE", help=argparse.SUPPRESS)
    ap.add_argument("--append", action="store_true", help="keep the sessions --out already holds and add this one")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "traj_ab.json"))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5, help="calls per timed sample of the bs-64 pair")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per bench.py run")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(bs64_plain(os.path.abspath(a.child), a.rounds, a.reps)), flush=True)
        return
    if not a.parent:
        ap.error("--parent is required")
    parent = os.path.abspath(a.parent)
    out = {"what": __doc__.split("\n")[0], "command": "bench.py --gpus 1 --steps 20 --warmup 5, alternating parent / branch, a fresh process per run", "sessions": []}
    if a.append and os.path.exists(a.out):
        out["sessions"] = json.load(open(a.out)).get("sessions", [])
    ses = {"runs_per_tree": a.runs, "order": [], "parent": [], "branch": []}
    for i in range(a.runs):
        for name, tree in (("parent", parent), ("branch", ROOT)):
            h = headline(tree, a.timeout)
            ses[name].append(h)
            ses["order"].append(name)
            print(name, i, json.dumps(h), flush=True)
    pv, bv = [h["value"] for h in ses["parent"]], [h["value"] for h in ses["branch"]]
    med = float(np.median(bv))
    ses["headline"] = {"unit": "motions/s", "parent_min": min(pv), "parent_max": max(pv), "parent_median": float(np.median(pv)), "branch_min": min(bv),
                       "branch_max": max(bv), "branch_median": med, "branch_over_parent_median": med / float(np.median(pv)),
                       "branch_median_inside_parent_min_max": bool(min(pv) <= med <= max(pv)), "branch_median_not_below_parent_min": bool(med >= min(pv))}
    print("headline", json.dumps(ses["headline"]), flush=True)
    out["sessions"].append(ses)
    pa, ba = ([h["value"] for s in out["sessions"] for h in s[k]] for k in ("parent", "branch"))
    out["verdict"] = {"rule": "the branch's median headline lies inside the parent's min..max of the session",
                      "per_session": [s["headline"]["branch_median_inside_parent_min_max"] for s in out["sessions"]],
                      "pooled": {"runs_per_tree": len(pa), "parent_median": float(np.median(pa)), "branch_median": float(np.median(ba)),
                                 "branch_over_parent_median": float(np.median(ba) / np.median(pa))}}
    out["bs64_no_trajectory_parent_vs_branch"] = bs64_trees(parent, a.runs, a.rounds, a.reps, a.timeout)
    out["bs64_trajectory_pair"] = bs64_pair(a.rounds, a.reps)     # (after the children: this process opens the GPU only now)
    print("bs64", json.dumps(out["bs64_trajectory_pair"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("->", a.out)
    if not ses["headline"]["branch_median_inside_parent_min_max"]:
        sys.exit("the branch's median headline lies outside the parent's min..max of this session")


if __name__ == "__main__":
    main()
