"""The fixture of the text tower's operand-policy tests: OpenCLIP text towers on UNROUNDED fp32 synthetic weights (and on their fp16
roundings), built in code; "truth" = a float64 restatement of the published block (LayerNorm, packed in_proj, causal softmax,
out_proj, erf-GELU MLP, ln_final — the architecture oracle/clip_oracle.py restates in fp32, to which tests/test_text_tower_precision.py
holds this restatement); e32 = max|clip_oracle fp32 - truth|, the fp32 evaluation's own distance from truth.

The end-to-end bound of `precise-full` is 16 e32, the first stage's gate (tests/first_stage_w32.py) for the same operand format: a
split pair carries about 22 bits against fp32's 24, four times fp32's rounding, and another factor of four covers the dropped lo.lo
products and a summation order other than the oracle's.  Nothing in it comes from this project's own output."""
import functools

import torch
import torch.nn.functional as F

from oracle import clip_oracle
from panacea_amd import conditioner as C

FACTOR = 16.0
VOCAB = 500
PROMPTS, TOKENS = 2, 77
SMALL, DEEP = (128, 3, 2), (128, 24, 2)          # (width, layers, heads); the deep one: depth does not eat the margin


def _embedder(width, layers, heads, precision=None, arch="custom", layer="penultimate"):
    kw = {} if precision is None else dict(precision=precision)
    return C.FrozenOpenCLIPEmbedder(arch=arch, width=width, layers=layers, heads=heads, vocab_size=VOCAB, layer=layer, **kw)


@functools.lru_cache(maxsize=None)
def weights(width, layers, heads, rounded=False):
    """the synthetic state dict of a tower: unrounded fp32 values of useful scale, or their fp16 roundings"""
    g = torch.Generator().manual_seed(7 + 1000 * width + 10 * layers + heads)
    sd = {}
    for n, p in _embedder(width, layers, heads).state_dict().items():
        r = torch.randn(p.shape, generator=g)
        if p.dim() >= 2 and "embedding" not in n:
            w = r * (p.shape[-1] ** -0.5)
        elif "ln_" in n and n.endswith("weight"):
            w = 1 + 0.1 * r
        else:
            w = 0.05 * r
        sd[n] = w.half().float() if rounded else w
    return sd


def tokens(prompts=PROMPTS):
    return torch.randint(0, VOCAB, (prompts, TOKENS), generator=torch.Generator().manual_seed(4))


def tower(dims, precision=None, rounded=False, device=None, arch="custom"):
    emb = _embedder(*dims, precision=precision, arch=arch)
    emb.load_state_dict(weights(*dims, rounded), strict=True)
    return emb if device is None else emb.to(device)


def truth(sd, tok, heads, layer="penultimate", prefix="model."):
    """float64: token + positional embedding -> the residual attention blocks under the causal mask -> ln_final; [B, L, W]"""
    g = lambda k: sd[prefix + k].double()   # noqa: E731
    x = g("token_embedding.weight")[tok] + g("positional_embedding")
    B, L, W = x.shape
    rb = prefix + "transformer.resblocks."
    n_layers = 1 + max(int(k[len(rb):].split(".")[0]) for k in sd if k.startswith(rb))
    above = torch.ones(L, L, dtype=torch.bool).triu_(1)          # key j > query i
    for i in range(n_layers - (1 if layer == "penultimate" else 0)):
        b = f"transformer.resblocks.{i}."
        h = F.layer_norm(x, (W,), g(b + "ln_1.weight"), g(b + "ln_1.bias"), 1e-5)
        qkv = h @ g(b + "attn.in_proj_weight").t() + g(b + "attn.in_proj_bias")
        q, k, v = (t.reshape(B, L, heads, W // heads).transpose(1, 2) for t in qkv.split(W, dim=-1))
        s = (q @ k.transpose(2, 3)) * (W // heads) ** -0.5
        p = torch.softmax(s.masked_fill(above, -float("inf")), dim=-1)
        a = (p @ v).transpose(1, 2).reshape(B, L, W)
        x = x + a @ g(b + "attn.out_proj.weight").t() + g(b + "attn.out_proj.bias")
        h = F.layer_norm(x, (W,), g(b + "ln_2.weight"), g(b + "ln_2.bias"), 1e-5)
        h = F.gelu(h @ g(b + "mlp.c_fc.weight").t() + g(b + "mlp.c_fc.bias"))
        x = x + h @ g(b + "mlp.c_proj.weight").t() + g(b + "mlp.c_proj.bias")
    return F.layer_norm(x, (W,), g("ln_final.weight"), g("ln_final.bias"), 1e-5)


@functools.lru_cache(maxsize=None)
def fixture(dims, rounded=False, prompts=PROMPTS):
    """-> tokens, truth (float64), ref32 (clip_oracle, fp32), e32 = max|ref32 - truth| of the tower `dims` on the given weights"""
    sd, tok = weights(*dims, rounded), tokens(prompts)
    t = truth(sd, tok, dims[2])
    r = clip_oracle.text_tower(sd, tok, heads=dims[2], layer="penultimate")
    return dict(tokens=tok, truth=t, ref32=r, e32=(r.double() - t).abs().max().item())


def err(got, t):
    return (got.detach().cpu().double() - t).abs().max().item()
