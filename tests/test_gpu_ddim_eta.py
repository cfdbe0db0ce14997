"""Stochastic DDIM (eta > 0) on an MI355X: full 9-layer synthetic weights, 50 steps, against the numpy oracle loop fed the same Philox draws
(include/mldhip.h "Noise contract"), across the reverse-loop families, in the pipelined mode of mldhip_sample_many_seeded, and through MLD.forward.

Tolerances are those of tests/test_gpu_parity.py: joints 1e-3, final latents 5e-3."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from mld_hip import _lib  # noqa: E402
from mld_hip import synthetic as syn  # noqa: E402
from oracle import mld_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


def _load(eng):
    eng.load_state_dict(syn.make_denoiser_state_dict(), "denoiser.")
    eng.load_state_dict(syn.make_vae_state_dict(), "vae.")
    mean, std = syn.make_mean_std()
    eng.load_tensor("mean", mean)
    eng.load_tensor("std", std)
    eng.finalize()


def _cuda(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def oracle_eta(text_emb, init_latents, lengths, eta, seed, indices, steps=50, guidance=7.5):
    """numpy: the reverse loop with DDIMScheduler.step(eta) and z of motion m = Philox(seed, step) elements [indices[m] * 256, + 256), then decode + joints"""
    ops = O.NumpyOps(f32)
    sd = O.to_backend(ops, syn.make_denoiser_state_dict())
    sch = O.DDIMSchedule()
    lat = init_latents.astype(f32)
    B = lat.shape[0]
    for i, t in enumerate(sch.set_timesteps(steps)):
        e = np.asarray(O.denoiser_forward(ops, sd, np.concatenate([lat, lat], 0), t, text_emb, 4))
        u, c = e[:B], e[B:]
        eps = u + f32(guidance) * (c - u)
        z = np.stack([O.philox_normal(256, seed, i, first=int(k) * 256) for k in indices]).reshape(B, 1, 256)
        prev = int(t) - sch.num_train_timesteps // steps
        a_t = f32(sch.alphas_cumprod[int(t)])
        a_p = f32(sch.alphas_cumprod[prev]) if prev >= 0 else f32(sch.final_alpha_cumprod)
        var = f32(f32(f32(1) - a_p) / f32(f32(1) - a_t)) * f32(f32(1) - f32(a_t / a_p))
        sg = f32(f32(eta) * np.sqrt(var, dtype=f32))
        ce = np.sqrt(max(f32(f32(f32(1) - a_p) - f32(sg * sg)), f32(0)), dtype=f32)
        x0 = (lat - np.sqrt(f32(1) - a_t, dtype=f32) * eps) / np.sqrt(a_t, dtype=f32)
        lat = (np.sqrt(a_p, dtype=f32) * x0 + ce * eps + sg * z).astype(f32)
    sv = O.to_backend(ops, syn.make_vae_state_dict())
    mean, std = syn.make_mean_std()
    feats = np.asarray(O.vae_decode(ops, sv, lat, lengths, 4))
    return lat, np.asarray(O.feats2joints(ops, feats, mean, std))


def _req(b, dev, sl=slice(None)):
    B = len(b.lengths[sl])
    n = b.init_latents.shape[0]
    te = np.concatenate([b.text_emb[:n][sl], b.text_emb[n:][sl]], 0)
    T = max(b.lengths[sl])
    return dict(text_emb=_cuda(te, dev), init_latents=_cuda(b.init_latents[sl], dev), lengths=b.lengths[sl],
                latents_out=torch.full((B, 1, 256), float("nan"), device=dev), joints_out=torch.full((B, T, 22, 3), float("nan"), device=dev))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.mark.parametrize("eta", [0.5, 1.0])
def test_cluster_loop_bs64_eta_matches_oracle(dev, eta):
    """One bs-64 request, ragged lengths up to T = 196, on the cluster loop (the default for one F16X3 request): joints within 1e-3 of the oracle
    loop with the same Philox draws; and far from the eta = 0 joints."""
    e = _lib.Engine(device=0, max_batch=64, max_frames=196, precision=1, eta=eta)
    _load(e)
    b = syn.make_batch(64, "ragged", seed=71)
    q = _req(b, dev)
    seed = 0xC0FFEE + int(eta * 10)
    e.sample_many_seeded([q], [(seed, 3)])
    torch.cuda.synchronize()
    assert e.launch_counts()[0] == 2                           # condition rows + one cluster launch
    lr, jr = oracle_eta(b.text_emb, b.init_latents, b.lengths, eta, seed, [3 + m for m in range(64)])
    j = q["joints_out"].cpu().numpy()
    assert np.abs(q["latents_out"].cpu().numpy() - lr).max() < 5e-3
    assert np.abs(j - jr).max() < 1e-3
    ns = e.numeric_status()
    assert ns["nonfinite_values"] == 0 and ns["cluster_loop"] == 1, ns
    e0 = _lib.Engine(device=0, max_batch=64, max_frames=196, precision=1)
    _load(e0)
    q0 = _req(b, dev)
    e0.sample_many([q0])
    torch.cuda.synchronize()
    assert (q0["joints_out"] - q["joints_out"]).abs().max().item() > 1e-2
    e0.close()
    e.close()


def test_persistent_loop_1280_motions_eta(dev):
    """1 280 motions per call on the sample-major persistent loop: a spread subset of motions against the oracle loop (the motions of a call are
    independent; each one's noise is a function of its key alone)."""
    B = 1280
    e = _lib.Engine(device=0, max_batch=B, max_frames=48, precision=1, eta=0.5)
    _load(e)
    b = syn.make_batch(B, "ragged", seed=72, max_len=48)
    q = _req(b, dev)
    seed = 4242
    e.sample_many_seeded([q], [(seed, 100)])
    torch.cuda.synchronize()
    assert e.launch_counts()[0] == 2                           # condition rows + one persistent launch
    sub = [0, 7, 8, 333, 640, 901, 1272, 1279]
    te = np.concatenate([b.text_emb[:B][sub], b.text_emb[B:][sub]], 0)
    lens = [b.lengths[i] for i in sub]
    lr, jr = oracle_eta(te, b.init_latents[sub], lens, 0.5, seed, [100 + i for i in sub])
    lat = q["latents_out"].cpu().numpy()[sub]
    joints = q["joints_out"].cpu().numpy()[sub][:, :max(lens)]
    assert np.abs(lat - lr).max() < 5e-3
    assert np.abs(joints - jr).max() < 1e-3
    assert e.numeric_status()["nonfinite_values"] == 0
    e.close()


def test_families_agree_and_pipelined_seeded_calls_are_bit_identical(dev):
    """The same keys on the latency, strip, persistent and cluster families give the same motions within the mode's tolerance; "many_pipeline" 1 with
    mixed, ragged requests is bit-identical to one-request seeded calls with the same keys."""
    e = _lib.Engine(device=0, max_batch=64, max_frames=196, precision=1, max_in_flight=2, eta=0.5)
    _load(e)
    b = syn.make_batch(24, "ragged", seed=73)
    out = {}
    for fam in (1, 2, 3, 4):
        e.set_option("loop_kernel", fam)
        q = _req(b, dev)
        e.sample_many_seeded([q], [(9, 0)])
        torch.cuda.synchronize()
        out[fam] = (q["latents_out"].cpu().numpy(), q["joints_out"].cpu().numpy())
    for fam in (1, 2, 3):
        assert np.abs(out[fam][0] - out[4][0]).max() < 5e-3, fam
        assert np.abs(out[fam][1] - out[4][1]).max() < 1e-3, fam
    e.set_option("loop_kernel", 0)
    batches = [syn.make_batch(64, "ragged" if i % 2 else None, seed=400 + i) for i in range(3)] + [syn.make_batch(40, "ragged", seed=404)]
    keys = [(1000 + i, 64 * i) for i in range(4)]
    solo = []
    for bb, k in zip(batches, keys):
        q = _req(bb, dev)
        e.sample_many_seeded([q], [k])
        solo.append(q)
    torch.cuda.synchronize()
    e.set_option("many_pipeline", 1)
    for _ in range(2):                                          # the second call replays the captured graphs with the uploaded keys
        reqs = [_req(bb, dev) for bb in batches]
        e.sample_many_seeded(reqs, keys)
        torch.cuda.synchronize()
        for q, s in zip(reqs, solo):
            assert torch.equal(q["latents_out"], s["latents_out"]) and torch.equal(q["joints_out"], s["joints_out"])
    assert e.numeric_status()["nonfinite_values"] == 0
    e.close()


def test_mld_forward_with_scheduler_eta(dev):
    """cfg.model.scheduler.eta = 0.5 through MLD.forward: torch.manual_seed makes a run reproducible, another seed gives other joints, and the
    reference's modular loop (drop-in scheduler.step with variance_noise) fed the engine's Philox draws agrees with the fused path."""
    from mld_hip import config as C
    from mld_hip import engine as E
    from mld_hip.datamodule import HipDataModule
    from mld_hip.mld import MLD
    from mld_hip.text_encoder import SyntheticTextEncoder

    E.drop_engines()
    cfg = C.load_config(overrides={"model.scheduler.eta": 0.5})
    E.configure(max_batch=8, max_frames=196)
    model = MLD(cfg, HipDataModule(cfg), text_encoder=SyntheticTextEncoder()).to(dev).eval()
    assert model.fused and model.eta == 0.5
    texts = ["a man kicks with something or someone with his left leg.", "A person is skipping rope.", "a person walks backward slowly."]
    lengths = [50, 100, 100]
    lat0 = _cuda(syn.make_batch(3, lengths).init_latents, dev)
    batch = {"text": texts, "length": lengths}
    torch.manual_seed(5)
    j1 = model(batch, init_latents=lat0)
    torch.manual_seed(5)
    j2 = model(batch, init_latents=lat0)
    torch.manual_seed(6)
    j3 = model(batch, init_latents=lat0)
    assert all(torch.equal(a, b) for a, b in zip(j1, j2))
    assert max((a - c).abs().max().item() for a, c in zip(j1, j3)) > 1e-2
    seed = 31337
    jf = model(batch, init_latents=lat0, seed=seed)
    emb = model.text_encoder([""] * 3 + texts)
    steps = cfg.model.scheduler.num_inference_timesteps
    noise = torch.stack([torch.from_numpy(O.philox_normal(3 * 256, seed, i).reshape(3, 1, 256)) for i in range(steps)]).to(dev)
    z = model._diffusion_reverse(emb, lengths, init_latents=lat0, step_noise=noise)
    feats = model.vae.decode(z.contiguous(), lengths)
    jm = model.feats2joints(feats).cpu().numpy()
    for i, n in enumerate(lengths):
        assert np.abs(jm[i, :n] - jf[i].numpy()).max() < 1e-3
    E.drop_engines()
