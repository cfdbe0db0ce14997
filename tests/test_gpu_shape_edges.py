"""Frame-length edges of the kernel selection, and config 4's served mode over many steps, on the MI355X against the float64 oracle.

Which kernel instance runs depends on the frame count T (engine/path_latent.hpp, engine/path_novae.hpp):
  pick_nkt                 key tiles 4 / 7 / 13 / 18 for T <= 64 / 112 / 208 / 288 (whole-K/V attention kernels)
  dec_attention            attn_flash_x3_kernel (key-blocked, 16 query tiles per workgroup) only for T <= 256
  novae_self_attention     attn_flash128_x3_kernel only for T <= 256, else attn_seq_x3_kernel<18, 128>
  attn_seq* grid           (nqt + 7) / 8 workgroups in y: the edge is at T = 128 / 129
  joints_body              feats2joints_kernel<256> / <512> at T = 256 / 257 (4 or 8 frames per lane of the wave scan)
  mldhip_vae_encode        T + 2 tokens: every edge above sits 2 frames lower
Section A walks T across all of them in four modes: F32, split-f16 (auto), split-f16 with the key-blocked forms forced
(flash_attn 2) and with the whole-K/V forms forced (flash_attn 0).  Section B runs config 4 as it is served -- split-f16, B = 64,
T = 196, in-kernel Philox noise, CFG halves de-duplicated in front of layer 0 -- for 20 DDPM steps.

The reference is always the float64 oracle.  Output buffers start NaN-filled (a value the kernels never write fails the finiteness
check); padded frames must be exactly zero where the contract says so.  Each bound is the one of the existing test of the same entry
point; the value beside it is the largest error measured over the test on an MI355X.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from mld_hip import _lib  # noqa: E402
from mld_hip import synthetic as syn  # noqa: E402
from oracle import mld_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

NOVAE_CFG = dict(latent_dim=512, vae_arch=_lib.VAE_NONE, denoiser_arch=_lib.ARCH_TRANS_DEC, scheduler_type=_lib.SCHED_DDPM,
                 steps_offset=0)
TS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 112, 113, 128, 129, 196, 197, 208, 209, 255, 256, 257, 287, 288]
ENC_TS = [1, 14, 15, 30, 62, 110, 126, 127, 206, 254, 255, 286]
F2J_TS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 288]
# name -> (precision, flash_attn or None for the handle's default)
MODES = {"f32": (0, None), "x3": (1, None), "x3_keyblocked": (1, 2), "x3_wholekv": (1, 0)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def f64():
    ops = O.TorchOps("float64")
    return (ops, O.to_backend(ops, syn.make_denoiser_state_dict()), O.to_backend(ops, syn.make_vae_state_dict()),
            O.to_backend(ops, syn.make_novae_denoiser_state_dict()))


@pytest.fixture(scope="module")
def cache():
    return {}          # float64 oracle results shared by the four modes


def _cuda(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _ragged(T):
    """the shorter motion of a batch padded to T (not a multiple of 16 wherever T allows)"""
    return max(1, T * 5 // 8)


def _text_engine(mode, **cfg):
    prec, flash = MODES[mode]
    e = _lib.Engine(device=0, precision=prec, **cfg)
    e.load_state_dict(syn.make_denoiser_state_dict(), "denoiser.")
    e.load_state_dict(syn.make_vae_state_dict(), "vae.")
    mean, std = syn.make_mean_std()
    e.load_tensor("mean", mean)
    e.load_tensor("std", std)
    e.finalize()
    if flash is not None:
        e.set_option("flash_attn", flash)
    return e


def _novae_engine(prec, flash=None, **cfg):
    e = _lib.Engine(device=0, precision=prec, **{**NOVAE_CFG, **cfg})
    e.load_state_dict(syn.make_novae_denoiser_state_dict(), "denoiser.")
    mean, std = syn.make_mean_std()
    e.load_tensor("mean", mean)
    e.load_tensor("std", std)
    e.finalize()
    if flash is not None:
        e.set_option("flash_attn", flash)
    return e


@pytest.fixture(scope="module", params=list(MODES))
def teng(request, dev):
    e = _text_engine(request.param, max_batch=2, max_frames=288, num_inference_steps=4)
    yield request.param, e
    e.close()


def _report(name, errs):
    worst = max(errs, key=errs.get)
    print("%s: max err %.3e at %s" % (name, errs[worst], worst))
    return errs[worst]


# ------------------------------------------------------------------ A. frame-length sweep (T up to 288)
def test_vae_decode_frame_length_sweep(teng, dev, f64, cache):
    """MldVae.decode at every T of TS, a full motion next to a ragged one.  Instances reached: attn_decode_kernel<4 / 7 / 13 / 18> (F32,
    T = 1 .. 64 / 65 .. 112 / 113 .. 208 / 209 .. 288); attn_decode_x3_kernel<4 / 7 / 13 / 18> (flash_attn 0 at the same T; auto mode
    at T = 257, 287, 288, where the key-blocked form does not apply); attn_flash_x3_kernel (flash_attn 2 at T <= 256, 16 query tiles per
    workgroup exactly full at 256, partial at 197 .. 255).  Layer 0's once-per-call projection ("dec_l0_once") and the fused tail
    ("dec_tail") are also switched off one at a time at T = 197, 257 and 288.  (attn_decode_x3_kernel<18> asked for 164 KiB of LDS until
    this test ran it: every split-f16 decode of more than 256 frames, or of 209 .. 256 frames in the whole-K/V form, was refused.)"""
    mode, e = teng
    ops, _, bv, _ = f64
    errs = {}
    for T in TS:
        lens = [T, _ragged(T)]
        z = syn._rng(31, f"edge{T}").standard_normal((2, 1, 256)).astype(np.float32)
        if ("dec", T) not in cache:
            cache["dec", T] = ops.to_numpy(O.vae_decode(ops, bv, ops.asarray(z), lens))
        variants = [(1, 1)] + ([(0, 1), (1, 0), (0, 0)] if T in (197, 257, 288) else [])
        for l0, tail in variants:
            e.set_option("dec_l0_once", l0)
            e.set_option("dec_tail", tail)
            feats = _nan(dev, 2, T, 263)
            e.vae_decode(_cuda(z, dev), lens, feats)
            torch.cuda.synchronize()
            f = feats.cpu().numpy()
            assert np.isfinite(f).all(), (mode, T, l0, tail)
            assert np.all(f[1, lens[1]:] == 0), (mode, T, l0, tail)
            errs[T, l0, tail] = float(np.abs(f - cache["dec", T]).max())
    e.set_option("dec_l0_once", 1)
    e.set_option("dec_tail", 1)
    assert _report(f"vae_decode {mode}", errs) < 1e-4                 # measured 2.8e-6 (split-f16, T = 288), 2.5e-6 (F32)


def test_vae_encode_frame_length_sweep(teng, dev, f64, cache):
    """MldVae.encode at the T of ENC_TS, where the T + 2 tokens cross the tile edges (16, 17, 32, 64, 112, 128, 129, 208, 256, 257, 288
    tokens): mu, logvar and the latent with a fixed eps.  T = 287 is refused with MLDHIP_EINVAL: the handle takes 288 frames, the
    encoder's attention 288 tokens."""
    mode, e = teng
    ops, _, bv, _ = f64
    errs = {"mu": {}, "logvar": {}, "latent": {}}
    for T in ENC_TS:
        lens = [T, _ragged(T)]
        g = syn._rng(32, f"enc{T}")
        fe = g.standard_normal((2, T, 263)).astype(np.float32)
        fe[1, lens[1]:] = 0
        eps = g.standard_normal((2, 1, 256)).astype(np.float32)
        if ("enc", T) not in cache:
            cache["enc", T] = [ops.to_numpy(x) for x in O.vae_encode(ops, bv, ops.asarray(fe), lens, ops.asarray(eps))]
        lr, mr, lvr = cache["enc", T]
        lat, mu, lv = (_nan(dev, 2, 1, 256) for _ in range(3))
        e.vae_encode(_cuda(fe, dev), lens, T, _cuda(eps, dev), lat, mu, lv)
        torch.cuda.synchronize()
        for name, got, ref in (("mu", mu, mr), ("logvar", lv, lvr), ("latent", lat, lr)):
            got = got.cpu().numpy()
            assert np.isfinite(got).all(), (mode, T, name)
            errs[name][T] = float(np.abs(got - ref).max())
    fe = np.zeros((2, 287, 263), np.float32)
    out = [_nan(dev, 2, 1, 256) for _ in range(3)]
    with pytest.raises(_lib.MldHipError) as ei:
        e.vae_encode(_cuda(fe, dev), [287, 100], 287, None, *out)
    assert ei.value.code == -1                                     # MLDHIP_EINVAL: 289 tokens
    em, el, et = (_report(f"vae_encode {mode} {k}", errs[k]) for k in ("mu", "logvar", "latent"))
    assert em < 1e-4 and el < 1e-4 and et < 5e-4                    # measured mu 3.7e-6, logvar 4.8e-6, latent 1.3e-5


def test_feats2joints_frame_length_sweep(teng, dev, f64):
    """recover_from_ric at the T of F2J_TS on O(1) random-walk features: feats2joints_kernel<256> (T <= 256; 4 frames per lane, the last
    lane partial or idle at T = 1 .. 5, 63 .. 65, 255) and feats2joints_kernel<512> (T = 257, 288: 8 frames per lane)."""
    mode, e = teng
    ops = f64[0]
    mean, std = syn.make_mean_std()
    errs = {}
    for T in F2J_TS:
        f = syn._rng(33, f"f2j{T}").standard_normal((2, T, 263)).astype(np.float32)
        joints = _nan(dev, 2, T, 22, 3)
        e.feats2joints(_cuda(f, dev), 2, T, joints)
        torch.cuda.synchronize()
        j = joints.cpu().numpy()
        assert np.isfinite(j).all(), (mode, T)
        ref = ops.to_numpy(O.feats2joints(ops, ops.asarray(f), ops.asarray(mean), ops.asarray(std)))
        errs[T] = float(np.abs(j - ref).max())
    assert _report(f"feats2joints {mode}", errs) < 1e-4               # measured 4.6e-7


@pytest.fixture(scope="module", params=list(MODES))
def neng(request, dev):
    prec, flash = MODES[request.param]
    e = _novae_engine(prec, flash, max_batch=2, max_frames=288, num_inference_steps=10)
    yield request.param, e
    e.close()


def test_novae_denoiser_frame_length_sweep(neng, dev, f64, cache):
    """Config 4's trans_dec denoiser (every frame a key) at every T of TS, R = 4 ragged, t = 999 and 0, "cross_fold" 1 and 0.
    Instances reached: attn_seq_kernel<4 / 7 / 13 / 18, 128> (F32); attn_seq_x3_kernel<4 / 7 / 13 / 18, 128> (flash_attn 0 at every T,
    auto at every T: 16 (sample, head) pairs are below its 512 threshold), grid y = 1 / 2 at T = 128 / 129; attn_flash128_x3_kernel (flash_attn
    2, T <= 256: the last 32-key block partial or full); attn_seq_x3_kernel<18, 128> again for flash_attn 2 at T = 257, 287, 288.
    Row 2 is then given length 0: it must come out all zeros and the other rows bit-identical (same R: the same launches)."""
    mode, e = neng
    ops, _, _, bn = f64
    errs = {}
    for T in TS:
        g = syn._rng(34, f"nvedge{T}")
        x = g.standard_normal((4, T, 263)).astype(np.float32)
        te = (0.5 * g.standard_normal((4, 1, 768))).astype(np.float32)
        lens = [T, _ragged(T), max(1, T // 3), max(1, T - 1)]
        lens0 = lens[:2] + [0] + lens[3:]
        for t in (999, 0):
            if ("nv", T, t) not in cache:
                cache["nv", T, t] = ops.to_numpy(O.denoiser_forward_novae(ops, bn, ops.asarray(x), t, ops.asarray(te), lens))
            for fold in (1, 0):
                e.set_option("cross_fold", fold)
                out, out0 = _nan(dev, 4, T, 263), _nan(dev, 4, T, 263)
                e.denoiser_forward_novae(_cuda(x, dev), t, _cuda(te, dev), lens, T, out)
                e.denoiser_forward_novae(_cuda(x, dev), t, _cuda(te, dev), lens0, T, out0)
                torch.cuda.synchronize()
                o, o0 = out.cpu().numpy(), out0.cpu().numpy()
                assert np.isfinite(o).all() and np.isfinite(o0).all(), (mode, T, t, fold)
                for i, n in enumerate(lens):
                    assert np.all(o[i, n:] == 0), (mode, T, t, fold, i)
                assert np.all(o0[2] == 0), (mode, T, t, fold)
                assert np.array_equal(o0[[0, 1, 3]], o[[0, 1, 3]]), (mode, T, t, fold)
                errs[T, t, fold] = float(np.abs(o - cache["nv", T, t]).max())
    e.set_option("cross_fold", 1)
    # measured 6.0e-6 (F32), 6.1e-6 (split-f16)
    assert _report(f"denoiser_forward_novae {mode}", errs) < (1e-4 if MODES[mode][0] == 0 else 3e-4)


@pytest.mark.parametrize("mode", ["x3", "f32"])
def test_sample_longest_and_shortest_motion(dev, f64, mode):
    """The capacity envelope end to end, in F32 and in split-f16 (the headline mode): a 288-frame motion (18 key tiles, the whole-K/V
    decoder attention attn_decode_x3_kernel<18> in split-f16) next to a 1-frame one, and a batch of one 1-frame motion; 4 DDIM steps."""
    ops, bd, bv, _ = f64
    mean, std = syn.make_mean_std()
    e = _text_engine(mode, max_batch=2, max_frames=288, num_inference_steps=4)
    for lens in ([288, 1], [1]):
        b = syn.make_batch(len(lens), lens, seed=55)
        B, T = len(lens), max(lens)
        joints, feats = _nan(dev, B, T, 22, 3), _nan(dev, B, T, 263)
        e.sample(_cuda(b.text_emb, dev), _cuda(b.init_latents, dev), lens, None, feats, joints)
        torch.cuda.synchronize()
        jr, fr, _ = O.sample(ops, bd, bv, ops.asarray(b.text_emb), ops.asarray(b.init_latents), lens, ops.asarray(mean), ops.asarray(std),
                             steps=4, return_intermediates=True)
        jr, fr = ops.to_numpy(jr), ops.to_numpy(fr)
        f, j = feats.cpu().numpy(), joints.cpu().numpy()
        assert np.isfinite(f).all() and np.isfinite(j).all()
        ef = float(np.abs(f - fr).max())
        ej = max(float(np.abs(j[i, :n] - jr[i, :n]).max()) for i, n in enumerate(lens))
        print("sample %s lengths %s: feats err %.3e joints err %.3e" % (mode, lens, ef, ej))
        assert ef < 1e-4 and ej < 1e-3                                 # measured feats 4.7e-6, joints 8.8e-6 (both modes)
        for i, n in enumerate(lens):
            assert np.all(f[i, n:] == 0)
    e.close()


# ------------------------------------------------------------------ B. config 4 as served: split-f16, B = 64, T = 196, 20 DDPM steps
SEED = 0x00C0FFEE12345678


def _served_batch():
    """64 motions with the realistic length mix (uniform in {40 .. 196 step 4}, one at 196), lat0 ~ N(0, 1)"""
    rng = np.random.Generator(np.random.PCG64(1234))
    lens = [int(v) for v in rng.choice(np.arange(40, 197, 4), 64)]
    lens[0] = 196
    b = syn.make_batch(64, lens, seed=1234)
    lat0 = syn._rng(35, "served").standard_normal((64, 196, 263)).astype(np.float32)
    return lens, b.text_emb, lat0


def _subset(lens):
    """about six motions spread over the batch: motion 0, the shortest, odd indices, the last"""
    idx = [0, int(np.argmin(lens)), 17, 32, 47, 63]
    return sorted(set(idx))


def _oracle_novae(f64, text, lat0, lens, idx, steps, seed):
    """float64 sample_novae on the motions idx of a call (they are independent: attention stays within a sample, no key mask), with
    the call's in-kernel Philox draws regenerated and sliced per motion"""
    ops, _, _, bn = f64
    B = len(lens)
    noise = np.stack([O.philox_normal(lat0.size, seed, s).reshape(lat0.shape)[idx] for s in range(steps)])
    te = np.concatenate([text[idx], text[[B + i for i in idx]]])
    fr = O.sample_novae(ops, bn, ops.asarray(te), ops.asarray(lat0[idx]), [lens[i] for i in idx], ops.asarray(noise), steps=steps)
    return ops.to_numpy(fr)


def _run_novae(e, dev, text, lat0, lens, seed):
    feats = _nan(dev, len(lens), lat0.shape[1], 263)
    e.sample_novae(_cuda(text, dev), _cuda(lat0, dev), lens, None, seed, feats, None)
    torch.cuda.synchronize()
    f = feats.cpu().numpy()
    assert np.isfinite(f).all()
    return f


def test_novae_served_mode_20_steps_vs_f64_oracle(dev, f64):
    """Config 4 as the benchmark runs it: split-f16, default options (cross_fold on, so layer 0 runs on the de-duplicated CFG half with
    attn_flash128_x3_kernel forced at R0 = 64 samples and cross2_fold_ln_kernel reading through src_mod = 64), 64 motions of the realistic
    length mix, in-kernel Philox noise, 20 DDPM steps.  All 196 rows of six motions against the float64 oracle; the same inputs with
    cross_fold 0 (no fold, no de-duplication) and on an F32 handle within the same bound.  A second call with the same seed replays the
    captured graphs and must be bit-identical; another seed must not be."""
    lens, text, lat0 = _served_batch()
    idx = _subset(lens)
    fr = _oracle_novae(f64, text, lat0, lens, idx, 20, SEED)
    scale = float(np.abs(fr).max())
    errs = {}
    e = _novae_engine(1, max_batch=64, max_frames=196, num_inference_steps=20)
    f = _run_novae(e, dev, text, lat0, lens, SEED)
    errs["split"] = float(np.abs(f[idx] - fr).max())
    f2 = _run_novae(e, dev, text, lat0, lens, SEED)
    assert np.array_equal(f, f2)                                   # graph replay: bit-identical
    f3 = _run_novae(e, dev, text, lat0, lens, SEED + 1)
    assert not np.array_equal(f, f3)
    e.set_option("cross_fold", 0)
    errs["split, cross_fold 0"] = float(np.abs(_run_novae(e, dev, text, lat0, lens, SEED)[idx] - fr).max())
    e.close()
    e = _novae_engine(0, max_batch=64, max_frames=196, num_inference_steps=20)
    errs["f32"] = float(np.abs(_run_novae(e, dev, text, lat0, lens, SEED)[idx] - fr).max())
    e.close()
    print("config 4 served mode, 20 steps, motions %s, max|feats| %.1f: err vs float64  %s"
          % (idx, scale, "  ".join("%s %.3e" % kv for kv in errs.items())))
    # measured 2.1e-4 split, 2.2e-4 cross_fold 0, 2.2e-4 F32 at max|feats| 100; the bound is test_novae_pipeline_vs_golden's (|feats| 67)
    assert max(errs.values()) < 2e-3, errs


@pytest.mark.parametrize("B", [1, 33])
def test_novae_dedup_odd_batches_vs_f64_oracle(dev, f64, B):
    """Odd B with the CFG halves de-duplicated: layer 0 on R0 = B samples (odd), attn_flash128_x3_kernel forced at 1 / 33 samples,
    cross2_fold_ln_kernel's src_mod = B wrapping the second half onto the first; split-f16, T = 196, 5 DDPM steps."""
    lens, text, lat0 = _served_batch()
    sel = list(range(B))
    lens, lat0 = [lens[i] for i in sel], np.ascontiguousarray(lat0[sel])
    text = np.concatenate([text[sel], text[[64 + i for i in sel]]])
    idx = sorted({0, int(np.argmin(lens)), min(17, B - 1), B - 1})      # B = 33: the first, an odd one, the shortest and last
    fr = _oracle_novae(f64, text, lat0, lens, idx, 5, SEED)
    e = _novae_engine(1, max_batch=B, max_frames=196, num_inference_steps=5)
    f = _run_novae(e, dev, text, lat0, lens, SEED)
    e.close()
    err = float(np.abs(f[idx] - fr).max())
    print("config 4 split-f16, B = %d, 5 steps, motions %s: err vs float64 %.3e (max|feats| %.1f)" % (B, idx, err, float(np.abs(fr).max())))
    assert err < 2e-3                                               # measured 8.0e-5 (B = 1), 1.1e-4 (B = 33) at max|feats| 40 - 42
