"""Write tests/golden/t2m_eval_b4.npz: the REFERENCE's own T2M evaluators (MovementConvEncoder, MotionEncoderBiGRUCo, TextEncoderBiGRUCo at the released
widths of its configs/base.yaml) on the seeded synthetic weights of mld_hip.synthetic.make_t2m_state_dict, run the way MLD.t2m_eval runs them: renorm4t2m on
every frame, columns [..., :-4], the batch sorted by length (descending) for pack_padded_sequence and m_lens = lengths // 4.

  python tools/make_golden_t2m.py --reference <checkout of motion-latent-diffusion>      (CPU, a few seconds; or MLD_REFERENCE in the environment)

Data only: features of B = 4 motions (T = 40, lengths 40 / 37 / 22 / 5, nfeats 263), of B = 2 motions (T = 24, nfeats 251), captions of B = 3 (L = 8, lengths
8 / 3 / 1), and the three sets of embeddings in the caller's (unsorted) order.  tests/test_t2m_golden.py holds tests/t2m_ref.py to it."""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import oracle._paths  # noqa: E402,F401
import t2m_ref as R  # noqa: E402

LENS, T = [40, 37, 22, 5], 40
KIT_LENS, KIT_T, KIT_NFEATS = [24, 10], 24, 251
TEXT_LENS, L = [8, 3, 1], 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("MLD_REFERENCE"))
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "t2m_eval_b4.npz"))
    a = ap.parse_args()
    if not a.reference:
        ap.error("--reference (or MLD_REFERENCE): the checkout of the reference project")
    sys.path.insert(0, a.reference)
    from mld.models.architectures import t2m_motionenc, t2m_textenc

    def evaluators(nfeats):
        sd = {k: torch.from_numpy(v) for k, v in R.weights(nfeats).items()}
        mods = {"t2m_moveencoder": t2m_motionenc.MovementConvEncoder(input_size=nfeats - 4, hidden_size=512, output_size=512),
                "t2m_motionencoder": t2m_motionenc.MotionEncoderBiGRUCo(input_size=512, hidden_size=1024, output_size=512),
                "t2m_textencoder": t2m_textenc.TextEncoderBiGRUCo(word_size=300, pos_size=15, hidden_size=512, output_size=512)}
        for name, m in mods.items():
            m.load_state_dict({k[len(name) + 1:]: v for k, v in sd.items() if k.startswith(name + ".")}, strict=True)
            m.eval()
        return mods

    def motion_embed(mods, feats, lens, nfeats):
        mean, std, mean_eval, std_eval = (torch.from_numpy(s) for s in R.stats(nfeats))
        f = (torch.from_numpy(feats) * std + mean - mean_eval) / std_eval            # renorm4t2m, on every frame
        order = np.argsort(lens)[::-1].copy()                                          # align_idx of MLD.t2m_eval
        m_lens = torch.div(torch.tensor(lens)[order], 4, rounding_mode="floor")
        with torch.no_grad():
            emb = mods["t2m_motionencoder"](mods["t2m_moveencoder"](f[order][..., :-4]).detach(), m_lens).numpy()
        out = np.empty_like(emb)
        out[order] = emb
        return out

    mods = evaluators(263)
    feats = R.make_motions(LENS, T, seed=21)
    emb = motion_embed(mods, feats, LENS, 263)
    w, p = R.make_captions(TEXT_LENS, L, seed=22)                                      # (already in descending order of length, as the dataloader's collate leaves them)
    with torch.no_grad():
        temb = mods["t2m_textencoder"](torch.from_numpy(w), torch.from_numpy(p), torch.tensor(TEXT_LENS)).numpy()
    kit_feats = R.make_motions(KIT_LENS, KIT_T, nfeats=KIT_NFEATS, seed=23)
    kit_emb = motion_embed(evaluators(KIT_NFEATS), kit_feats, KIT_LENS, KIT_NFEATS)
    np.savez_compressed(a.out, feats=feats, lengths=np.array(LENS), motion_emb=emb, word_embs=w, pos_ohot=p, text_lengths=np.array(TEXT_LENS), text_emb=temb,
                        kit_feats=kit_feats, kit_lengths=np.array(KIT_LENS), kit_motion_emb=kit_emb)
    print("t2m_eval_b4 ->", a.out, os.path.getsize(a.out), "bytes; max|emb|", float(np.abs(emb).max()), float(np.abs(temb).max()), float(np.abs(kit_emb).max()))


if __name__ == "__main__":
    main()
