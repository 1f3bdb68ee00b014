"""Plain-torch restatement of the reference's FrozenOpenCLIPEmbedder.encode_with_transformer
(ldm/modules/encoders/modules.py:216-233) over an open_clip-named state dict, runnable in any dtype, plus the seeded
test tower. Shared by tests/test_text_cpu.py and tests/test_text_gpu.py; a helper, not a test, and no device code.

open_clip's text tower per block (ResidualAttentionBlock): x = x + attn(ln_1(x), attn_mask); x = x + mlp(ln_2(x)),
attn = nn.MultiheadAttention (in_proj -> heads -> softmax(q k^T / sqrt(dh) + mask) v -> out_proj), mlp = c_fc ->
nn.GELU (exact erf) -> c_proj; attn_mask = build_attention_mask: -inf above the diagonal, no padding mask."""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

PREFIX = "cond_stage_model.model."


def text_cfg(width=128, layers=4, vocab=512, context=77, mlp=None, layer="penultimate"):
    """The fields of rdeic_amd.text.TextConfig, restated (heads = width / 64)."""
    return SimpleNamespace(width=width, heads=width // 64, layers=layers, vocab=vocab, context=context,
                           mlp=mlp or 4 * width, layer=layer)


def seeded_text_state_dict(cfg, seed: int = 0, prefix: str = PREFIX) -> dict:
    """fp32 weights from a seeded CPU generator: linears ~ N(0, 1 / fan_in) (scores O(1) after LayerNorm), LayerNorm
    gammas near 1, small biases and embeddings; plus the three entries a loader must ignore."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g)  # noqa: E731
    w, m = cfg.width, cfg.mlp
    sd = {prefix + "token_embedding.weight": rn(cfg.vocab, w) * 0.05,
          prefix + "positional_embedding": rn(cfg.context, w) * 0.02}
    for i in range(cfg.layers):
        b = f"{prefix}transformer.resblocks.{i}."
        for ln in ("ln_1", "ln_2"):
            sd[b + ln + ".weight"] = 1.0 + 0.1 * rn(w)
            sd[b + ln + ".bias"] = 0.05 * rn(w)
        sd[b + "attn.in_proj_weight"] = rn(3 * w, w) / w ** 0.5
        sd[b + "attn.in_proj_bias"] = 0.05 * rn(3 * w)
        sd[b + "attn.out_proj.weight"] = rn(w, w) / w ** 0.5
        sd[b + "attn.out_proj.bias"] = 0.05 * rn(w)
        sd[b + "mlp.c_fc.weight"] = rn(m, w) / w ** 0.5
        sd[b + "mlp.c_fc.bias"] = 0.05 * rn(m)
        sd[b + "mlp.c_proj.weight"] = rn(w, m) / m ** 0.5
        sd[b + "mlp.c_proj.bias"] = 0.05 * rn(w)
    sd[prefix + "ln_final.weight"] = 1.0 + 0.1 * rn(w)
    sd[prefix + "ln_final.bias"] = 0.05 * rn(w)
    sd[prefix + "text_projection"] = rn(w, w) / w ** 0.5
    sd[prefix + "logit_scale"] = torch.tensor(4.6052)
    sd[prefix + "attn_mask"] = torch.full((cfg.context, cfg.context), float("-inf")).triu_(1)
    return sd


def seeded_tokens(batch: int, cfg, seed: int = 1) -> torch.Tensor:
    """[batch, context] int64: SOT-like first id, a random body of a different length per row, zero padding (token
    rows as the tokenizer makes them, inside the test vocabulary)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.zeros((batch, cfg.context), dtype=torch.int64)
    for b in range(batch):
        n = int(torch.randint(1, cfg.context - 2, (1,), generator=g))
        t[b, 0] = cfg.vocab - 2
        t[b, 1:1 + n] = torch.randint(1, cfg.vocab - 2, (n,), generator=g)
        t[b, 1 + n] = cfg.vocab - 1
    return t


def encode_with_transformer(sd: dict, tokens: torch.Tensor, heads: int, dtype=torch.float64, causal: bool = True,
                            skip_last: int = 1, prefix: str = PREFIX, eps: float = 1e-5) -> torch.Tensor:
    """[B, L] tokens -> [B, L, width] in `dtype` (every tensor and every product in that dtype). skip_last: how
    many trailing blocks are left out (1 = "penultimate", 0 = "last"); causal=False drops the mask."""
    p = lambda n: sd[prefix + n].to(dtype)  # noqa: E731
    head = prefix + "transformer.resblocks."
    layers = len({k[len(head):].split(".", 1)[0] for k in sd if k.startswith(head)})
    x = p("token_embedding.weight")[tokens] + p("positional_embedding")
    B, L, Wd = x.shape
    dh = Wd // heads
    mask = torch.full((L, L), float("-inf"), dtype=dtype).triu_(1) if causal else None
    for i in range(layers - skip_last):
        b = f"transformer.resblocks.{i}."
        h = F.layer_norm(x, (Wd,), p(b + "ln_1.weight"), p(b + "ln_1.bias"), eps)
        qkv = F.linear(h, p(b + "attn.in_proj_weight"), p(b + "attn.in_proj_bias"))
        q, k, v = (t.reshape(B, L, heads, dh).transpose(1, 2) for t in qkv.chunk(3, dim=-1))
        s = (q @ k.transpose(-1, -2)) * dh ** -0.5
        if mask is not None:
            s = s + mask
        o = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, L, Wd)
        x = x + F.linear(o, p(b + "attn.out_proj.weight"), p(b + "attn.out_proj.bias"))
        h = F.layer_norm(x, (Wd,), p(b + "ln_2.weight"), p(b + "ln_2.bias"), eps)
        h = F.gelu(F.linear(h, p(b + "mlp.c_fc.weight"), p(b + "mlp.c_fc.bias")))
        x = x + F.linear(h, p(b + "mlp.c_proj.weight"), p(b + "mlp.c_proj.bias"))
    return F.layer_norm(x, (Wd,), p("ln_final.weight"), p("ln_final.bias"), eps)


def rel_l2(a: torch.Tensor, ref: torch.Tensor) -> float:
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).norm() / ref.norm())
