"""MLD.t2m_eval end to end on the MI355X: a synthetic batch (B = 4, two DDIM steps, the 3-layer model) through sampling, decode, renorm and both evaluator
towers of ONE engine.  Its lat_rm equals mldhip_t2m_motion_embed of its own m_rst to the bit, its lat_m / lat_t are within tests/t2m_ref.py's tolerance of the
float64 restatement on m_ref / the captions, everything comes back in the reference's align_idx order, and a checkpoint's t2m_* keys load strictly."""
import faulthandler

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import simlib  # noqa: E402
import t2m_ref as R  # noqa: E402
from mld_hip import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(180, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def test_t2m_eval_end_to_end():
    from mld_hip import config as C
    from mld_hip import engine as E
    from mld_hip.datamodule import HipDataModule
    from mld_hip.evaluators import HipT2MEvaluator
    from mld_hip.mld import MLD
    from mld_hip.text_encoder import SyntheticTextEncoder

    dev = torch.device("cuda:0")
    E.drop_engines()
    E.configure(max_batch=4, max_frames=64)
    over = {"model.denoiser.params.num_layers": simlib.SIM_LAYERS, "model.motion_vae.params.num_layers": simlib.SIM_LAYERS,
            "model.scheduler.num_inference_timesteps": 2}
    plain = MLD(C.load_config(overrides=over), HipDataModule(), text_encoder=SyntheticTextEncoder())
    assert plain.t2m_evaluator is None and not any(k.startswith("t2m_") for k in plain.state_dict())
    with pytest.raises(RuntimeError):
        plain.t2m_eval({})
    cfg = C.load_config(overrides={**over, "model.t2m_evaluator.target": "mld_hip.evaluators.HipT2MEvaluator"})
    model = MLD(cfg, HipDataModule(cfg), text_encoder=SyntheticTextEncoder())
    assert isinstance(model.t2m_evaluator, HipT2MEvaluator)
    # a checkpoint: the model's own keys + the evaluator nets under their checkpoint names, loaded strictly
    ckpt = {k: v for k, v in model.state_dict().items() if not k.startswith("t2m_evaluator.")}
    ckpt.update({k: torch.from_numpy(v) for k, v in R.weights().items()})
    model.load_state_dict(ckpt, strict=True)
    with pytest.raises(RuntimeError):
        model.load_state_dict({k: v for k, v in ckpt.items() if k != "t2m_textencoder.hidden"}, strict=True)
    model = model.to(dev).eval()

    lengths, text_lens, L = [24, 40, 9, 40], [3, 5, 1, 2], 5
    motion = torch.from_numpy(R.make_motions(lengths, 40, seed=31)).to(dev)
    w, p = R.make_captions(text_lens, L, seed=32)
    batch = {"text": ["a person walks.", "someone jumps twice.", "a man waves.", "a person sits down."], "motion": motion, "length": lengths,
             "word_embs": torch.from_numpy(w).to(dev), "pos_ohot": torch.from_numpy(p).to(dev), "text_len": torch.tensor(text_lens)}
    lat0 = torch.from_numpy(syn.make_batch(4, lengths).init_latents).to(dev)
    rs = model.t2m_eval(batch, init_latents=lat0)
    torch.cuda.synchronize()
    assert set(rs) == {"m_ref", "m_rst", "lat_t", "lat_m", "lat_rm", "joints_ref", "joints_rst"}
    order = np.argsort(lengths)[::-1].copy()                                   # the reference's align_idx
    sorted_lens = [lengths[i] for i in order]
    assert tuple(rs["lat_rm"].shape) == (4, 512) and tuple(rs["joints_rst"].shape) == (4, 40, 22, 3)
    assert torch.equal(rs["m_ref"], model.datamodule.renorm4t2m(motion)[torch.from_numpy(order).to(dev)])
    # lat_rm IS the motion tower on m_rst (rows already in the evaluators' normalisation), to the bit; so is lat_m on m_ref
    ev = model.t2m_evaluator
    assert torch.equal(ev.motion_embed(rs["m_rst"].contiguous(), sorted_lens, renorm=False), rs["lat_rm"])
    assert torch.equal(ev.motion_embed(rs["m_ref"].contiguous(), sorted_lens, renorm=False), rs["lat_m"])
    # ... and the engine's own renorm (renorm = 1 on the model's rows) lands within the tolerance of the same reference
    r64, e32 = R.reference_motion(R.make_motions(lengths, 40, seed=31), lengths)
    err = float(np.abs(rs["lat_m"].cpu().numpy().astype(np.float64) - r64[order]).max())
    err1 = float(np.abs(ev.motion_embed(motion, lengths, renorm=True).cpu().numpy().astype(np.float64) - r64).max())
    t64, te32 = R.reference_text(w, p, text_lens)
    terr = float(np.abs(rs["lat_t"].cpu().numpy().astype(np.float64) - t64[order]).max())
    print(f"MLD.t2m_eval: lat_m err {err:.3e} (engine renorm {err1:.3e})  e32 {e32:.3e};  lat_t err {terr:.3e}  e32 {te32:.3e}")
    assert err <= R.F32_FACTOR * e32 and err1 <= R.F32_FACTOR * e32 and terr <= R.F32_FACTOR * te32
    assert np.isfinite(rs["lat_rm"].cpu().numpy()).all() and np.isfinite(rs["joints_rst"].cpu().numpy()).all()
    E.drop_engines()
