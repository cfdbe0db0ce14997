""""loop_lean" on the MI355X: the persistent reverse loop whose last denoiser layer works on the latent token's row tile only (kernels/loop_fused.hpp `full`)
against "loop_lean" 0, to the bit -- latents and joints, the same launches.

"loop_kernel" 3 on a max_batch 24 handle, 2 steps, T = 52, modes F32 and F16X3: a sample_many of two requests (5 + 3 motions: one workgroup, rows beyond
B repeat motion B - 1), one call of 17 motions (three workgroups, the last with one real motion), the from-form (a request that enters at step 1 beside one that
starts at 0, with trajectories) and, on an eta 0.5 handle, the seeded form.  The simulator twin with the fp64 check is tests/test_loop_lean_sim.py."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from mld_hip import _lib  # noqa: E402
from mld_hip import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu

T, STEPS = 52, 2
LENS_A, LENS_B = [52, 37, 52, 37, 20], [52, 20, 37]
LENS_17 = [52, 37, 20, 45, 29, 52, 16, 33, 52, 41, 8, 37, 52, 24, 49, 20, 37]


def _engine(prec, eta=0.0):
    assert torch.cuda.is_available()
    e = _lib.Engine(device=0, precision=prec, max_batch=24, max_frames=T, num_inference_steps=STEPS, eta=eta)
    e.load_state_dict(syn.make_denoiser_state_dict(), "denoiser.")
    e.load_state_dict(syn.make_vae_state_dict(), "vae.")
    mean, std = syn.make_mean_std()
    e.load_tensor("mean", mean)
    e.load_tensor("std", std)
    e.finalize()
    e.set_option("loop_kernel", 3)
    return e


@pytest.fixture(scope="module", params=[0, 1], ids=["f32", "f16x3"])
def eng(request):
    e = _engine(request.param)
    yield request.param, e
    e.close()


def _request(lens, seed, traj=False):
    dev = torch.device("cuda:0")
    b = syn.make_batch(len(lens), lens, seed=seed)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    q = {"lengths": lens, "text_emb": torch.from_numpy(np.ascontiguousarray(b.text_emb)).to(dev),
         "init_latents": torch.from_numpy(np.ascontiguousarray(b.init_latents)).to(dev),
         "latents_out": nan(len(lens), 1, 256), "joints_out": nan(len(lens), max(lens), 22, 3)}
    if traj:
        q["traj_out"] = nan(STEPS, len(lens), 256)
    return q


def _both(e, run):
    """run() -> requests, under "loop_lean" 0 and 1: the same bits in every output, finite latents and joints, the same launch counts"""
    out, counts = [], []
    for lean in (0, 1):
        e.set_option("loop_lean", lean)
        out.append(run())
        torch.cuda.synchronize()
        counts.append(e.launch_counts())
    assert counts[0] == counts[1], counts
    for qa, qb in zip(*out):
        for k in ("latents_out", "joints_out"):
            assert torch.isfinite(qb[k]).all() and torch.equal(qa[k], qb[k]), k
        if "traj_out" in qa:
            assert torch.equal(torch.nan_to_num(qa["traj_out"], nan=-7.0), torch.nan_to_num(qb["traj_out"], nan=-7.0))
    assert e.numeric_status()["nonfinite_values"] == 0
    return out[1]


def test_sample_many_of_two_requests(eng):
    _, e = eng

    def run():
        rq = [_request(LENS_A, 11), _request(LENS_B, 12)]
        e.sample_many(rq)
        return rq
    _both(e, run)
    assert e.launch_counts()[0] == 2                     # condition rows + ONE loop launch


def test_one_call_of_17_motions(eng):
    _, e = eng

    def run():
        q = _request(LENS_17, 13)
        e.sample(q["text_emb"], q["init_latents"], LENS_17, q["latents_out"], None, q["joints_out"])
        return [q]
    _both(e, run)


def test_from_form(eng):
    """den_loop_kernel<*, kLoopFrom>: the second request enters at step 1 from a clean source; its step-0 trajectory row keeps the NaN fill"""
    _, e = eng
    src = torch.from_numpy(np.random.default_rng(5).standard_normal((len(LENS_B), 1, 256)).astype(np.float32) * np.float32(0.7)).to("cuda:0")

    def run():
        rq = [_request(LENS_A, 11, traj=True), _request(LENS_B, 12, traj=True)]
        rq[1].update(src_latents=src, first_step=1, noised=0)
        e.sample_many_from(rq, None)
        return rq
    on = _both(e, run)
    assert bool(torch.isnan(on[1]["traj_out"][0]).all()) and torch.equal(on[1]["traj_out"][-1], on[1]["latents_out"][:, 0])
    assert torch.equal(on[0]["traj_out"][-1], on[0]["latents_out"][:, 0])


def test_eta_form():
    """den_loop_kernel<true, kLoopEta>: eta 0.5, one key per request"""
    e = _engine(1, eta=0.5)
    try:
        def run():
            rq = [_request(LENS_A, 11), _request(LENS_B, 12)]
            e.sample_many_seeded(rq, [(0x1EA4, 3), (0x1EA4, 40)])
            return rq
        _both(e, run)
    finally:
        e.close()
