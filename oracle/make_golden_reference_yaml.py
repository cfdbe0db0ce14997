"""Fixture of the reference's experiment / module YAMLs, the values tests/test_host_mirror.py compares the drop-in configs with:

    MLD_REFERENCE=<checkout of motion-latent-diffusion> python oracle/make_golden_reference_yaml.py   ->   tests/golden/reference_yaml.json

Per module file the `params:` block of each hot-path part (plus `num_inference_timesteps` / `eta` where the part has them); per experiment file
the model keys the drop-ins must keep, TRAIN.ABLATION and TEST.CHECKPOINTS.  Keyed by the file's path inside the reference checkout."""
import json
import os
import sys

import yaml

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "reference_yaml.json")
MODULES = {"modules": ("denoiser", "motion_vae", "scheduler"), "modules_humanact12": ("denoiser", "motion_vae", "scheduler"),
           "modules_novae": ("denoiser", "scheduler")}
EXPERIMENTS = ("config_mld_humanml3d.yaml", "config_mld_humanact12.yaml", "config_novae_humanml3d.yaml")
MODEL_KEYS = ("latent_dim", "ff_size", "num_layers", "num_head", "guidance_scale", "guidance_uncondp", "condition", "vae", "vae_type")


def main():
    ref = os.environ.get("MLD_REFERENCE") or sys.exit("set MLD_REFERENCE to a checkout of the reference project")
    out = {}
    for d, parts in MODULES.items():
        for part in parts:
            rel = "configs/%s/%s.yaml" % (d, part)
            blk = yaml.safe_load(open(os.path.join(ref, rel)))[part]
            out[rel] = {part: {k: blk[k] for k in ("params", "num_inference_timesteps", "eta") if k in blk}}
    for fn in EXPERIMENTS:
        rel = "configs/" + fn
        exp = yaml.safe_load(open(os.path.join(ref, rel)))
        out[rel] = {"model": {k: exp["model"][k] for k in MODEL_KEYS if k in exp["model"]},
                    "TRAIN": {"ABLATION": exp["TRAIN"]["ABLATION"]}, "TEST": {"CHECKPOINTS": exp["TEST"]["CHECKPOINTS"]}}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d files" % (OUT, len(out)))


if __name__ == "__main__":
    main()
