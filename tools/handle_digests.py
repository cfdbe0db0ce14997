"""What the HOST layer of the library decides and computes, over a fixed list of handles: the bit identity of two BUILDS across a host-only change.
  python tools/handle_digests.py --lib PATH [--sim] --out FILE
Run it on the library of the parent commit and on this tree's and compare the two files (`cmp`, or --against FILE: exit status 1 on a difference).
Every handle is finalized with "range_probe" 1.  Recorded per handle (one line of the file each): missing_keys() before any tensor is loaded (count
and sha256 of the sorted names), the keys mldhip_load_tensor ignored, every field of numeric_status() (floats as hex), the bytes
mldhip_numeric_status writes into a struct cut to each accepted prefix size (unwritten bytes stay 0x77), and per entry point the handle has one
small call: launch_counts() and the sha256 of its outputs.

GPU list (max_batch 8, max_frames 64, synthetic weights of mld_hip/synthetic.py): the default text handle in F32 and F16X3, both again with
"dec_half" 1, the HumanAct12 action handle, a diffusion-only handle at num_layers 2, one F16X3 handle with every optional module on (CLIP tower at
clip_layers 2, evaluators, UESTC and HumanAct12 recognizers, smpl_verts 64, metric kernels; nfeats 150, as the body model asks), and a UESTC handle
whose weights overflow the half range (in_gain 1e6: that verdict is a fallback).
--sim (PATH is a `make sim` build; a probe costs minutes there): the text tower, evaluator and UESTC stages only, on handles of the sizes the
simulator suite probes (num_layers 3, max_batch <= 3, max_frames 16, no diffusion weights)."""
import argparse, ctypes as C, hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "motion-latent-diffusion_amd")]
import numpy as np
from mld_hip import _lib, synthetic as syn

NI = _lib.NumericInfo
INFO_SIZES = sorted({getattr(NI, f).offset + getattr(NI, f).size for f in ("reserved", "probe_err_text", "probe_err_eval")} | {C.sizeof(NI)})


def clip_tower(layers, vocab, ctx, W=768, F=3072, seed=21):
    """seeded tensors under the keys the engine declares for the tower (transformers' CLIPModel names)"""
    g = syn._rng(seed, "handle_digests.clip")
    mat = lambda *s: (0.02 * g.standard_normal(s)).astype(np.float32)
    gain = lambda: (1.0 + 0.05 * g.standard_normal(W)).astype(np.float32)
    p, sd = "text_encoder.text_model.text_model.", {}
    sd[p + "embeddings.token_embedding.weight"], sd[p + "embeddings.position_embedding.weight"] = mat(vocab, W), mat(ctx, W)
    for i in range(layers):
        q = p + "encoder.layers.%d." % i
        for n in ("layer_norm1", "layer_norm2"):
            sd[q + n + ".weight"], sd[q + n + ".bias"] = gain(), mat(W)
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            sd[q + "self_attn." + n + ".weight"], sd[q + "self_attn." + n + ".bias"] = mat(W, W), mat(W)
        sd[q + "mlp.fc1.weight"], sd[q + "mlp.fc1.bias"], sd[q + "mlp.fc2.weight"], sd[q + "mlp.fc2.bias"] = mat(F, W), mat(F), mat(W, F), mat(W)
    sd[p + "final_layer_norm.weight"], sd[p + "final_layer_norm.bias"] = gain(), mat(W)
    sd["text_encoder.text_model.text_projection.weight"] = mat(W, W)
    return sd


def handles(sim):
    """(name, mldhip_config overrides, {key: tensor}, {option: value})"""
    t2m = lambda nf: {**syn.make_t2m_state_dict(nfeats=nf), **dict(zip(("mean_eval", "std_eval"), syn.make_mean_std_eval(nf)))}
    stats = lambda nf: dict(zip(("mean", "std"), syn.make_mean_std(nf)))
    pre = lambda p, sd: {p + k: v for k, v in sd.items()}
    uestc = lambda **kw: pre("uestc_rec.", syn.make_uestc_rec_state_dict(seed=13, **kw))
    if sim:
        small = dict(use_graph=0, num_layers=3, max_frames=16, precision=1)
        return [("clip", dict(small, max_batch=2, clip_layers=1, clip_vocab=64, clip_max_prompts=6), clip_tower(1, 64, 77), {}),
                ("t2m_eval", dict(small, max_batch=2, t2m_eval=1, t2m_max_motions=4, t2m_max_words=6), {**t2m(syn.NFEATS), **stats(syn.NFEATS)}, {}),
                ("uestc", dict(small, max_batch=3, uestc_rec=1), uestc(), {}),
                ("uestc overflow", dict(small, max_batch=3, uestc_rec=1), uestc(in_gain=1e6), {})]
    base = dict(max_batch=8, max_frames=64)
    text = {**pre("denoiser.", syn.make_denoiser_state_dict()), **pre("vae.", syn.make_vae_state_dict()), **stats(syn.NFEATS)}
    out = [("text prec%d dec_half%d" % (p, dh), dict(base, precision=p), text, {"dec_half": dh}) for dh in (0, 1) for p in (0, 1)]
    adims = syn.ModelDims(num_layers=15, nfeats=150)
    out.append(("action", dict(base, precision=1, condition=_lib.COND_ACTION, nclasses=12, vae_arch=_lib.VAE_ACTOR, vae_num_layers=6, num_layers=15, nfeats=150),
                {**pre("denoiser.", syn.make_denoiser_state_dict(seed=3, dims=adims, condition="action", nclasses=12)), **pre("vae.", syn.make_actor_vae_state_dict())}, {}))
    out.append(("novae", dict(base, precision=1, latent_dim=512, vae_arch=_lib.VAE_NONE, denoiser_arch=_lib.ARCH_TRANS_DEC, scheduler_type=_lib.SCHED_DDPM, steps_offset=0,
                              num_layers=2, num_inference_steps=10),
                {**pre("denoiser.", syn.make_novae_denoiser_state_dict(dims=syn.ModelDims(latent_dim=512, num_layers=2))), **stats(syn.NFEATS)}, {}))
    d150 = syn.ModelDims(nfeats=150)
    out.append(("all modules", dict(base, precision=1, nfeats=150, clip_layers=2, clip_vocab=512, t2m_eval=1, uestc_rec=1, a2m_rec=1, smpl_verts=64, t2m_metrics=1),
                {**pre("denoiser.", syn.make_denoiser_state_dict(dims=d150)), **pre("vae.", syn.make_vae_state_dict(dims=d150)), **stats(150), **clip_tower(2, 512, 77), **t2m(150),
                 **uestc(), **pre("a2m_rec.", syn.make_a2m_rec_state_dict()), **pre("smpl.", syn.make_smpl(64))}, {}))
    out.append(("uestc overflow", dict(base, precision=1, num_layers=3, uestc_rec=1), uestc(in_gain=1e6), {}))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--sim", action="store_true", help="--lib is the simulator build: host memory, the simulator suite's handle sizes")
    ap.add_argument("--out", required=True)
    ap.add_argument("--against", help="a file written by an earlier run: compare")
    a = ap.parse_args()
    lib = _lib.load_library(os.path.abspath(a.lib))
    if a.sim:
        dev_of, empty, host, sync = np.ascontiguousarray, (lambda *s: np.full(s, np.nan, np.float32)), (lambda x: x), (lambda: None)
    else:
        import torch
        dev = torch.device("cuda:0")
        dev_of = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        empty = lambda *s: torch.full(s, float("nan"), device=dev)
        host, sync = (lambda x: x.cpu().numpy()), torch.cuda.synchronize
    g = syn._rng(300, "handle_digests")
    normal = lambda *s: g.standard_normal(s).astype(np.float32)
    result = {"what": __doc__.split("\n")[0], "simulator": bool(a.sim), "handles": {}}
    for name, cfg, tensors, options in handles(a.sim):
        e = _lib.Engine(lib=lib, device=0, **cfg)
        keys = lambda ks: {"count": len(ks), "sha256": hashlib.sha256("\n".join(sorted(ks)).encode()).hexdigest()}
        rec = {"missing_before_load": keys(e.missing_keys()), "calls": {}}
        ignored = [k for k, v in tensors.items() if not e.load_tensor(k, v)]
        e.set_option("range_probe", 1)
        for k, v in options.items():
            e.set_option(k, v)
        e.finalize()
        rec["ignored"], rec["missing_after_load"] = ignored, keys(e.missing_keys())
        rec["numeric_status"] = {k: (float(v).hex() if isinstance(v, float) else v) for k, v in e.numeric_status().items()}
        rec["numeric_status_prefix"] = {}
        for size in INFO_SIZES:
            buf = (C.c_ubyte * C.sizeof(NI))(*([0x77] * C.sizeof(NI)))
            info = NI.from_buffer(buf)
            info.struct_size = size
            e._check(lib.mldhip_numeric_status(e._h, C.byref(info)))
            rec["numeric_status_prefix"][str(size)] = bytes(buf).hex()
        c = e.cfg

        def call(what, fn, *outs):
            fn()
            sync()
            rec["calls"][what] = {"launches": e.launch_counts(), "sha256": [hashlib.sha256(np.ascontiguousarray(host(o)).tobytes()).hexdigest() for o in outs]}
            print(name, "|", what, rec["calls"][what]["launches"], [s[:12] for s in rec["calls"][what]["sha256"]], flush=True)

        B, T, NF, D = 3, 40, c.nfeats, c.latent_dim
        lens = [24, 40, 33]
        have = lambda p: any(k.startswith(p) for k in tensors)
        if have("denoiser.") and c.vae_arch == _lib.VAE_NONE:
            feats, joints, o = empty(B, T, NF), empty(B, T, c.njoints, 3), empty(2 * B, T, NF)
            call("sample_novae", lambda: e.sample_novae(dev_of(normal(2 * B, 1, c.text_dim)), dev_of(normal(B, T, NF)), lens, None, 5, feats, joints), feats, joints)
            call("denoiser_forward_novae", lambda: e.denoiser_forward_novae(dev_of(normal(2 * B, T, NF)), 999, dev_of(normal(2 * B, 1, c.text_dim)), lens + lens, T, o), o)
        elif have("denoiser."):
            lat, feats, joints, o = empty(B, 1, D), empty(B, T, NF), empty(B, T, c.njoints, 3), empty(2 * B, 1, D)
            if c.condition == _lib.COND_ACTION:
                call("sample_action", lambda: e.sample_action([0, 5, 11], dev_of(normal(B, 1, D)), lens, lat, feats), lat, feats)
                call("denoiser_forward_action", lambda: e.denoiser_forward_action(dev_of(normal(2 * B, 1, D)), 981, [0, 5, 11, 1, 2, 3], o), o)
            else:
                call("sample", lambda: e.sample(dev_of(normal(2 * B, 1, c.text_dim)), dev_of(normal(B, 1, D)), lens, lat, feats, joints), lat, feats, joints)
                call("denoiser_forward", lambda: e.denoiser_forward(dev_of(normal(2 * B, 1, D)), 981, dev_of(normal(2 * B, 1, c.text_dim)), 2 * B, o), o)
                mu, lv, dj = empty(B, 1, D), empty(B, 1, D), empty(B, T, c.njoints, 3)
                call("vae_encode", lambda: e.vae_encode(dev_of(normal(B, T, NF)), lens, T, dev_of(normal(B, D)), lat, mu, lv), lat, mu, lv)
                call("feats2joints", lambda: e.feats2joints(feats, B, T, dj), dj)
            call("vae_decode", lambda: e.vae_decode(dev_of(normal(B, 1, D)), lens, feats), feats)
        if c.clip_layers > 0:
            ids = g.integers(0, c.clip_vocab, (3, c.clip_ctx)).astype(np.int32)
            o = empty(3, 1, c.text_dim)
            call("text_encode", lambda: e.text_encode(ids, [1, 16, 32], o), o)
        if c.t2m_eval:
            Te, L, o, o2 = 16, min(6, c.t2m_max_words or 32), empty(2, 512), empty(2, 512)      # (Engine.cfg keeps the caller's 0 = default)
            pos = np.zeros((2, L, 15), np.float32)
            pos[:, :, 3] = 1.0
            call("t2m_motion_embed", lambda: e.t2m_motion_embed(dev_of(normal(2, Te, NF)), [16, 9], Te, o, True), o)
            call("t2m_text_embed", lambda: e.t2m_text_embed(dev_of(normal(2, L, 300)), dev_of(pos), [L, 2], L, o2), o2)
        if c.uestc_rec:
            x, lo, fe = normal(2, 24, 6, 8), empty(2, max(c.uestc_classes, syn.UESTC_CLASSES)), empty(2, 256)
            call("uestc_recognize", lambda: e.uestc_recognize(dev_of(x), (24 * 6 * 8, 6 * 8, 8, 1), 2, 8, lo, fe), lo, fe)
        if c.a2m_rec:
            lo, act = empty(2, 12), empty(2, 30)
            call("a2m_recognize", lambda: e.a2m_recognize(dev_of(normal(2, 16, 72)), [16, 7], 16, None, lo, act), lo, act)
        if c.smpl_verts > 0:
            jo, vo = empty(2, 8, 24, 3), empty(2, 8, c.smpl_verts, 3)
            call("smpl_forward", lambda: e.smpl_forward(dev_of(0.5 * normal(2, 8, 150)), [8, 3], 8, jo, vo), jo, vo)
        if c.t2m_metrics:
            x, y = dev_of(normal(64, 32)), dev_of(normal(64, 32))
            if a.sim:
                rank, diag, mean, cov, dist = np.zeros(64, np.int32), empty(64), empty(32), empty(32, 32), empty(5)
            else:
                rank, diag, mean, cov, dist = torch.zeros(64, dtype=torch.int32, device=dev), empty(64), empty(32), empty(32, 32), empty(5)
            call("t2m_match", lambda: e.t2m_match(x, y, 64, 32, 32, rank, diag), rank, diag)
            call("act_stats", lambda: e.act_stats(x, 64, 32, mean, cov), mean, cov)
            call("pair_dist", lambda: e.pair_dist(x, 64, 32, [0, 1, 2, 3, 63], [5, 4, 3, 2, 0], dist), dist)
        rec["numeric_status_after"] = {k: (float(v).hex() if isinstance(v, float) else v) for k, v in e.numeric_status().items()}
        e.close()
        result["handles"][name] = rec
        print(name, "|", rec["numeric_status"], flush=True)
    with open(a.out, "w") as f:      # one line per handle: two builds' files compare with cmp / diff
        f.write(json.dumps({k: v for k, v in result.items() if k != "handles"}, sort_keys=True) + "\n")
        for name, rec in sorted(result["handles"].items()):
            f.write(json.dumps({name: rec}, sort_keys=True) + "\n")
    print("->", a.out)
    if a.against:
        same = open(a.against).read() == open(a.out).read()
        print("against", a.against, ":", "equal" if same else "DIFFERENT")
        sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
