"""Shared pieces of the text-tower tests (tests/test_text_tower_sim.py on the simulator, tests/test_gpu_text_tower.py on the MI355X):
the reference -- transformers' own ``CLIPTextModelWithProjection``, random-init under a fixed seed, in float64 and float32 on the CPU --
the prompt sets, the key mapping into ``mldhip_load_tensor`` and the tolerance rule.

Tolerance (measured per prompt set, not guessed): e32 = max|torch-fp32-CPU - torch-fp64-CPU| of the same model on the same ids;
MLDHIP_PREC_F32 must be within 4 x e32 of fp64 (the margin covers summation order), MLDHIP_PREC_F16X3 within 16 x e32 (4 x for 22
against 24 mantissa bits, 4 x margin)."""
import numpy as np
import torch

WIDTH, HEADS, FF, CTX, VOCAB = 768, 12, 3072, 77, 64
BOS, EOS = VOCAB - 2, VOCAB - 1          # the EOS id is the largest: argmax(ids) and "first EOS" name the same position
KEY_PREFIX = "text_encoder.text_model."  # MldTextEncoder.text_model is a CLIPModel: its text_model.* / text_projection.* sit under this prefix
F32_FACTOR, X3_FACTOR = 4.0, 16.0

_models = {}


def reference_model(layers):
    """(fp64 model, fp32 model) with identical parameters; cached per depth.  The 1-D parameters (biases, LayerNorm affine) are drawn too:
    transformers initialises them to 0 / 1, which would hide a dropped bias."""
    if layers not in _models:
        from transformers import CLIPTextConfig, CLIPTextModelWithProjection
        cfg = CLIPTextConfig(vocab_size=VOCAB, hidden_size=WIDTH, intermediate_size=FF, num_hidden_layers=layers, num_attention_heads=HEADS,
                             max_position_embeddings=CTX, projection_dim=WIDTH, hidden_act="quick_gelu", bos_token_id=BOS, eos_token_id=EOS,
                             pad_token_id=EOS)
        torch.manual_seed(1234)
        m32 = CLIPTextModelWithProjection(cfg).eval()
        g = torch.Generator().manual_seed(4321)
        with torch.no_grad():
            for name, p in m32.named_parameters():
                if p.dim() == 1:
                    p.copy_((1.0 if "norm" in name and name.endswith("weight") else 0.0) + 0.1 * torch.randn(p.shape, generator=g))
        import copy
        m64 = copy.deepcopy(m32).double().eval()
        _models[layers] = (m64, m32)
    return _models[layers]


def make_ids(eos_positions, seed=0):
    """[P, CTX] int64 ids as the tokenizer pads them: BOS, random word ids, EOS at eos_positions[p], EOS (= pad) behind it.  Position 1 is the "" prompt."""
    rng = np.random.default_rng(seed)
    ids = np.full((len(eos_positions), CTX), EOS, dtype=np.int64)
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


def tower_tensors(layers):
    """{mldhip_load_tensor key: float32 numpy} of the reference model: the tower's weight group"""
    _, m32 = reference_model(layers)
    return {KEY_PREFIX + k: v.detach().numpy() for k, v in m32.state_dict().items() if v.dtype.is_floating_point}


def engine_kwargs(layers, max_prompts, **extra):
    """mldhip_config fields of a small engine that carries this tower (the diffusion model is the 3-layer stack, never loaded)"""
    return dict(num_layers=3, max_batch=2, max_frames=16, clip_layers=layers, clip_heads=HEADS, clip_ff=FF, clip_vocab=VOCAB, clip_ctx=CTX,
                clip_max_prompts=max_prompts, **extra)


def load_tower(eng, layers):
    ignored = [k for k, v in tower_tensors(layers).items() if not eng.load_tensor(k, v)]
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
