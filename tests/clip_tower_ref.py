"""Shared pieces of the text-tower tests (tests/test_text_tower_sim.py on the simulator, tests/test_gpu_text_tower.py on the MI355X):
the reference -- transformers' own ``CLIPTextModelWithProjection``, random-init under a fixed seed, in float64 and float32 on the CPU --
the prompt sets, the key mapping into ``mldhip_load_tensor`` and the tolerance rule.

Tolerance (measured per prompt set, not guessed): e32 = max|torch-fp32-CPU - torch-fp64-CPU| of the same model on the same ids;
MLDHIP_PREC_F32 must be within 4 x e32 of fp64 (the margin covers summation order), MLDHIP_PREC_F16X3 within 16 x e32 (4 x for 22
against 24 mantissa bits, 4 x margin).  The rule is applied per row wherever rows are compared (row_ratios).

Every token row: the tower is causal and pools at the eos_pos the caller passes (ids behind it are never read), so the output for (ids, eos_pos = k) is
row k of the full sequence -- prefix_call builds P prompts from one id row and reference_rows gives all rows from one forward pass.

Weight regimes (VARIANTS; applied to the fp32 model before the fp64 copy is made).  Notes on three of them, measured on the one-layer simulator tower,
rows n = 1 / 17 / 33, worst row in units of e32:
  "small_w" (fc1 x 64, fc2 x 1/64): F32 1.7, F16X3 left on the split kernels 63 (finite, non-finite counter 0; probe reading 4.4e-5 against 2.8e-6 for the
      plain weights).  Neither factor does it alone: fc1 x 64 alone ends at 3.0 (probe 2.5e-6), fc2 x 1/64 alone at 3.9 (probe 2.6e-6).  The error is made by the
      fc2-down half -- fc2's weights land at |w| ~ 3e-4, where the low half of the split is a half subnormal (absolute error 3e-8, i.e. 1e-4 relative) -- but alone
      it also shrinks the MLP's share of the residual stream 64-fold, and the error with it; fc1 x 64 restores the share and makes it visible.
  "overflow": fc1 x 2^16.  2^14 does not do what the name says on this initialisation: fc1's output has a standard deviation of 0.7, its largest value
      over two layers x 77 rows is 3.6, so x 2^14 peaks at 5.9e4 < 65 504; x 2^16 peaks at 2.4e5 (mlp_peaks; the tests assert it).
  "gelu_tails" (fc1 x 8) reaches |x| = 29, short of where expf(-1.702 x) overflows (|x| > 52); "gelu_overflow" (x 32, |x| = 115) is the case that does."""
import numpy as np
import torch

WIDTH, HEADS, FF, CTX, VOCAB = 768, 12, 3072, 77, 64
BOS, EOS = VOCAB - 2, VOCAB - 1          # the EOS id is the largest: argmax(ids) and "first EOS" name the same position
KEY_PREFIX = "text_encoder.text_model."  # MldTextEncoder.text_model is a CLIPModel: its text_model.* / text_projection.* sit under this prefix
F32_FACTOR, X3_FACTOR = 4.0, 16.0

_models = {}


def _scale(params, f):
    for p in params:
        p.mul_(f)


def _sharp(m):
    for layer in m.text_model.encoder.layers:
        a = layer.self_attn
        _scale((a.q_proj.weight, a.q_proj.bias, a.k_proj.weight, a.k_proj.bias), 4.0)


SINK_LOGIT = 30.0


def _sink(m):
    """Released CLIP towers park most of every row's attention on the BOS key.  On top of "sharp": a fixed vector of 20 x N(0, 1) added to the BOS
    token embedding -- row 0 of the residual stream is that vector in every layer, so its LayerNorm-ed row and hence key 0 are known from the
    weights alone -- and, because with random weights the bias is the only part of q that all query rows share, every layer's q bias moved along
    its own key 0 (per head) by what adds SINK_LOGIT to the key-0 logit of every row."""
    _sharp(m)
    hd = WIDTH // HEADS
    u = 20.0 * torch.randn(WIDTH, generator=torch.Generator().manual_seed(99))
    m.text_model.embeddings.token_embedding.weight[BOS] += u
    un = (u - u.mean()) / u.std(unbiased=False)
    for layer in m.text_model.encoder.layers:
        a = layer.self_attn
        k0 = (a.k_proj.weight @ (layer.layer_norm1.weight * un + layer.layer_norm1.bias) + a.k_proj.bias).reshape(HEADS, hd)
        a.q_proj.bias += (SINK_LOGIT * hd ** 0.5 * k0 / (k0 * k0).sum(dim=1, keepdim=True)).reshape(WIDTH)


def _outlier(m):
    e = m.text_model.embeddings
    for col, off in ((5, 40.0), (300, -25.0), (767, 60.0)):
        e.token_embedding.weight[:, col] += off
    e.position_embedding.weight[0] *= 30.0


def _fc1(f):
    def apply(m):
        for layer in m.text_model.encoder.layers:
            _scale((layer.mlp.fc1.weight, layer.mlp.fc1.bias), f)
    return apply


def _fc2(f):
    def apply(m):
        for layer in m.text_model.encoder.layers:
            _scale((layer.mlp.fc2.weight, layer.mlp.fc2.bias), f)
    return apply


def _small_w(m):
    _fc1(64.0)(m)
    _fc2(1.0 / 64.0)(m)


# named in-place weight transformations of the fp32 model (the fp64 copy is made afterwards: both see the same numbers)
VARIANTS = {
    "plain": lambda m: None,
    "sharp": _sharp,                    # q_proj / k_proj weight and bias x 4: logits x 16
    "sink": _sink,
    "outlier": _outlier,                # three embedding channels far off, position 0 x 30: LayerNorm rows with outlier channels
    "gelu_tails": _fc1(8.0),            # fc1 weight and bias x 8: pre-activations reach |x| ~ 25 (far tails of the sigmoid, no overflow yet)
    "gelu_overflow": _fc1(32.0),        # ... x 32: |x| ~ 100, where expf(-1.702 x) overflows inside quick_gelu (module docstring)
    "small_w": _small_w,                # fc1 x 64, fc2 x 1/64: the split-f16 mode's small-operand limit (module docstring)
    "small_w_fc1": _fc1(64.0),          # the two halves of "small_w" alone (attribution only)
    "small_w_fc2": _fc2(1.0 / 64.0),
    "overflow": _fc1(2.0 ** 16),        # the hidden activation passes 65 504, the largest half (module docstring: why not 2^14)
}


def reference_model(layers, ctx=CTX, variant="plain"):
    """(fp64 model, fp32 model) with identical parameters; cached per (depth, context length, variant).  The 1-D parameters (biases, LayerNorm
    affine) are drawn too: transformers initialises them to 0 / 1, which would hide a dropped bias.  ``variant`` names one of VARIANTS."""
    key = (layers, ctx, variant)
    if key not in _models:
        from transformers import CLIPTextConfig, CLIPTextModelWithProjection
        cfg = CLIPTextConfig(vocab_size=VOCAB, hidden_size=WIDTH, intermediate_size=FF, num_hidden_layers=layers, num_attention_heads=HEADS,
                             max_position_embeddings=ctx, projection_dim=WIDTH, hidden_act="quick_gelu", bos_token_id=BOS, eos_token_id=EOS,
                             pad_token_id=EOS)
        torch.manual_seed(1234)
        m32 = CLIPTextModelWithProjection(cfg).eval()
        g = torch.Generator().manual_seed(4321)
        with torch.no_grad():
            for name, p in m32.named_parameters():
                if p.dim() == 1:
                    p.copy_((1.0 if "norm" in name and name.endswith("weight") else 0.0) + 0.1 * torch.randn(p.shape, generator=g))
            VARIANTS[variant](m32)
        import copy
        m64 = copy.deepcopy(m32).double().eval()
        _models[key] = (m64, m32)
    return _models[key]


def make_ids(eos_positions, seed=0, ctx=CTX):
    """[P, CTX] int64 ids as the tokenizer pads them: BOS, random word ids, EOS at eos_positions[p], EOS (= pad) behind it.  Position 1 is the "" prompt."""
    rng = np.random.default_rng(seed)
    ids = np.full((len(eos_positions), ctx), EOS, dtype=np.int64)
    for p, e in enumerate(eos_positions):
        ids[p, 0] = BOS
        ids[p, 1:e] = rng.integers(0, BOS, size=max(e - 1, 0))
        ids[p, e] = EOS
    return ids


def reference_embeddings(layers, ids):
    """(fp64 [P, WIDTH] as float64 numpy, e32) on these ids"""
    m64, m32 = reference_model(layers)
    t = torch.from_numpy(np.asarray(ids, dtype=np.int64))
    with torch.no_grad():
        r64 = m64(input_ids=t).text_embeds.numpy()
        r32 = m32(input_ids=t).text_embeds.double().numpy()
    return r64, float(np.abs(r32 - r64).max())


def reference_rows(layers, ids_row, ctx=CTX, variant="plain"):
    """(r64, r32), both float64 numpy [ctx, WIDTH]: EVERY token row of the tower on one id row -- final_layer_norm's output times
    text_projection^T, from one forward pass in float64 and one in float32.  Row k is what the engine returns for (ids_row, eos_pos = k): the
    tower is causal and pools at the eos_pos the caller passes."""
    m64, m32 = reference_model(layers, ctx, variant)
    t = torch.from_numpy(np.asarray(ids_row, dtype=np.int64).reshape(1, ctx))
    with torch.no_grad():
        r64 = (m64.text_model(input_ids=t).last_hidden_state[0] @ m64.text_projection.weight.T).numpy()
        r32 = (m32.text_model(input_ids=t).last_hidden_state[0] @ m32.text_projection.weight.T).double().numpy()
    return r64, r32


def prefix_call(ids_row, lengths):
    """(ids [P, ctx] int64, eos_pos [P]): the same id row P times, prompt p ending at token lengths[p] - 1"""
    ids_row = np.asarray(ids_row, dtype=np.int64)
    return np.repeat(ids_row[None], len(lengths), axis=0), [int(n) - 1 for n in lengths]


def row_ratios(out, r64, r32, lengths):
    """(per-row max|out - r64| over the rows n - 1 of ``lengths``, e32 over the same rows)"""
    rows = [int(n) - 1 for n in lengths]
    err = np.abs(np.asarray(out, dtype=np.float64) - r64[rows]).max(axis=1)
    return err, float(np.abs(r32[rows] - r64[rows]).max())


def attention_shape(layers, ids_row, ctx=CTX, variant="plain"):
    """(largest softmax weight of the LAST query row in any head, share of (head, query row >= 1) pairs whose largest weight sits on key 0), layer 0
    of the fp64 model -- a small eager causal attention on the model's own parameters (transformers' sdpa path returns no attentions)"""
    m64, _ = reference_model(layers, ctx, variant)
    t = torch.from_numpy(np.asarray(ids_row, dtype=np.int64).reshape(1, ctx))
    hd = WIDTH // HEADS
    with torch.no_grad():
        layer = m64.text_model.encoder.layers[0]
        x = layer.layer_norm1(m64.text_model.embeddings(input_ids=t))[0]
        q = layer.self_attn.q_proj(x).reshape(ctx, HEADS, hd).permute(1, 0, 2)
        k = layer.self_attn.k_proj(x).reshape(ctx, HEADS, hd).permute(1, 2, 0)
        s = (q @ k) * hd ** -0.5 + torch.triu(torch.full((ctx, ctx), float("-inf"), dtype=torch.float64), 1)
        w = torch.softmax(s, dim=-1)
    return float(w[:, -1].max()), float((w[:, 1:].argmax(dim=-1) == 0).double().mean())


def mlp_peaks(layers, ids_row, ctx=CTX, variant="plain"):
    """(max|fc1 output|, max|quick_gelu output|) over every layer and row of the fp64 model: what the "gelu_tails" / "overflow" variants must reach"""
    m64, _ = reference_model(layers, ctx, variant)
    pre, act = [], []
    hooks = []
    for layer in m64.text_model.encoder.layers:
        hooks.append(layer.mlp.fc1.register_forward_hook(lambda mod, a, out: pre.append(float(out.abs().max()))))
        hooks.append(layer.mlp.fc2.register_forward_pre_hook(lambda mod, a: act.append(float(a[0].abs().max()))))
    try:
        with torch.no_grad():
            m64.text_model(input_ids=torch.from_numpy(np.asarray(ids_row, dtype=np.int64).reshape(1, ctx)))
    finally:
        for h in hooks:
            h.remove()
    return max(pre), max(act)


def tower_tensors(layers, ctx=CTX, variant="plain"):
    """{mldhip_load_tensor key: float32 numpy} of the reference model: the tower's weight group"""
    _, m32 = reference_model(layers, ctx, variant)
    return {KEY_PREFIX + k: v.detach().numpy() for k, v in m32.state_dict().items() if v.dtype.is_floating_point}


def engine_kwargs(layers, max_prompts, ctx=CTX, **extra):
    """mldhip_config fields of a small engine that carries this tower (the diffusion model is the 3-layer stack, never loaded)"""
    return dict(num_layers=3, max_batch=2, max_frames=16, clip_layers=layers, clip_heads=HEADS, clip_ff=FF, clip_vocab=VOCAB, clip_ctx=ctx,
                clip_max_prompts=max_prompts, **extra)


def load_tower(eng, layers, ctx=CTX, variant="plain"):
    ignored = [k for k, v in tower_tensors(layers, ctx, variant).items() if not eng.load_tensor(k, v)]
    eng.finalize()
    return ignored


def make_clip_dir(root, layers):
    """A throw-away CLIP directory (random-init CLIPModel at the text tower's real widths + a minimal CLIPTokenizer vocabulary) for the
    adapter classes of mld_hip.text_encoder; "clip" in the path, as the reference requires (mld_clip.py:39)."""
    import json
    import os
    from transformers import CLIPConfig, CLIPModel, CLIPTokenizer
    d = os.path.join(str(root), "clip-vit-random")
    os.makedirs(d, exist_ok=True)
    chars = list("abcdefghijklmnopqrstuvwxyz0123456789.,!?'")
    vocab = {}
    for c in chars:
        vocab[c] = len(vocab)
    for c in chars:
        vocab[c + "</w>"] = len(vocab)
    vocab["<|startoftext|>"] = len(vocab)
    vocab["<|endoftext|>"] = len(vocab)
    json.dump(vocab, open(os.path.join(d, "vocab.json"), "w"))
    open(os.path.join(d, "merges.txt"), "w").write("#version: 0.2\n")
    CLIPTokenizer(os.path.join(d, "vocab.json"), os.path.join(d, "merges.txt"), model_max_length=CTX).save_pretrained(d)
    eos = vocab["<|endoftext|>"]
    cfg = CLIPConfig(text_config=dict(vocab_size=len(vocab), hidden_size=WIDTH, intermediate_size=FF, num_hidden_layers=layers,
                                      num_attention_heads=HEADS, max_position_embeddings=CTX, projection_dim=WIDTH,
                                      bos_token_id=vocab["<|startoftext|>"], eos_token_id=eos, pad_token_id=eos),
                     vision_config=dict(hidden_size=32, intermediate_size=32, num_hidden_layers=1, num_attention_heads=2, image_size=32,
                                        patch_size=16, projection_dim=WIDTH),
                     projection_dim=WIDTH)
    torch.manual_seed(0)
    CLIPModel(cfg).save_pretrained(d)
    return d, vocab
