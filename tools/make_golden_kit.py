"""Write tests/golden/kit_ops_b3.npz: the REFERENCE's own MldVae at KIT-ML's width (nfeats 251) and recover_from_ric with 21 joints, on the seeded
synthetic weights of mld_hip.synthetic -- the 251-wide twin of vae_decode_b3.npz / vae_encode_b3.npz (oracle/make_golden.py).

  python tools/make_golden_kit.py --reference <checkout of motion-latent-diffusion>      (CPU, a few seconds; or MLD_REFERENCE in the environment)

Data only: decode features of B = 3 ragged motions (T <= 32), the joints recovered from them, encode mu / std of B = 3 motions (T <= 24), and the
oracle-vs-reference differences measured while writing.  tests/test_kit_golden.py holds oracle/mld_oracle.py to it."""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import oracle._paths  # noqa: E402,F401
from mld_hip import synthetic as syn  # noqa: E402
from oracle import mld_oracle as O  # noqa: E402

NFEATS, NJOINTS = 251, 21
DEC_LENS, ENC_LENS = [32, 17, 1], [24, 13, 5]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("MLD_REFERENCE"))
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "kit_ops_b3.npz"))
    a = ap.parse_args()
    if not a.reference:
        ap.error("--reference (or MLD_REFERENCE): the checkout of the reference project")
    sys.path.insert(0, a.reference)
    from mld.data.humanml.scripts.motion_process import recover_from_ric
    from mld.models.architectures.mld_vae import MldVae

    class Abl:      # TRAIN.ABLATION of the MLD experiment files
        SKIP_CONNECT = True
        VAE_TYPE = "mld"
        PE_TYPE = "mld"
        DIFF_PE_TYPE = "mld"
        MLP_DIST = False

    torch.manual_seed(0)
    vae = MldVae(ablation=Abl, nfeats=NFEATS, latent_dim=[1, 256], ff_size=1024, num_layers=9, num_heads=4, dropout=0.1, arch="encoder_decoder",
                 normalize_before=False, activation="gelu", position_embedding="learned").eval()
    sdv = syn.make_vae_state_dict(dims=syn.ModelDims(nfeats=NFEATS))
    vae.load_state_dict({k: torch.from_numpy(v) for k, v in sdv.items()}, strict=True)
    mean, std = syn.make_mean_std(NFEATS)
    ops = O.NumpyOps(np.float32)
    bv = O.to_backend(ops, sdv)

    z = syn._rng(7, "golden_kit_z").standard_normal((3, 1, 256)).astype(np.float32)
    with torch.no_grad():
        feats = vae.decode(torch.from_numpy(z).permute(1, 0, 2), DEC_LENS).numpy()
        joints = recover_from_ric(torch.from_numpy(feats) * torch.from_numpy(std) + torch.from_numpy(mean), NJOINTS).numpy()
    fm = O.vae_decode(ops, bv, z, DEC_LENS)
    jm = O.feats2joints(ops, feats, mean, std, njoints=NJOINTS)

    fe = syn._rng(9, "golden_kit_feats").standard_normal((3, max(ENC_LENS), NFEATS)).astype(np.float32)
    for i, n in enumerate(ENC_LENS):
        fe[i, n:] = 0
    with torch.no_grad():
        _, dist = vae.encode(torch.from_numpy(fe), ENC_LENS)
    mu_r, std_r = dist.loc.permute(1, 0, 2).numpy(), dist.scale.permute(1, 0, 2).numpy()
    _, mu_o, lv_o = O.vae_encode(ops, bv, fe, ENC_LENS)

    diffs = dict(oracle_diff_feats=np.abs(feats - fm).max(), oracle_diff_joints=np.abs(joints - jm).max(),
                 oracle_diff_mu=np.abs(mu_r - mu_o).max(), oracle_diff_std=np.abs(std_r - np.sqrt(np.exp(lv_o))).max())
    np.savez_compressed(a.out, z=z, dec_lengths=np.array(DEC_LENS), feats=feats, joints=joints, enc_feats=fe, enc_lengths=np.array(ENC_LENS),
                        mu=mu_r, std=std_r, **diffs)
    print("kit_ops_b3 oracle-vs-reference:", {k: float(v) for k, v in diffs.items()}, "->", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
