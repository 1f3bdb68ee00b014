"""OpenCLIP text tower on the device: the reference's FrozenOpenCLIPEmbedder.encode_with_transformer
(ldm/modules/encoders/modules.py:174-236; ViT-H/14 text, layer "penultimate" in configs/model/rdeic.yaml:96-100).

    x = token_embedding[tokens] + positional_embedding
    per block:  x += out_proj(causal_attention(in_proj(ln_1 x)));  x += c_proj(gelu(c_fc(ln_2 x)))
    the first `layers - 1` blocks for "penultimate", all for "last"; then ln_final

The attention mask is open_clip's build_attention_mask: causal, no padding mask (padding tokens attend and are
attended like any other). The tower is frozen (cond_stage_trainable: false): inference only, no backward.
Every linear runs on the MFMA GEMM (ops.linear; bias, exact-erf GELU and the residual in its epilogue), in_proj
as one GEMM whose three column slices are q | k | v, the attention on rdeic_attention_causal. Per-image launch
choices (images=B) and a per-(batch, head) attention keep a caption's context the same bits alone and inside
any batch.

Weights carry the checkpoint's own names under `cond_stage_model.model.`; text_projection, logit_scale and the
attn_mask buffer are ignored.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from . import ops
from . import weights as W

PREFIX = "cond_stage_model.model."
SOT, EOT = 49406, 49407
HEAD_DIM = 64  # rdeic_attention_causal's head dim: ViT-H/14 text is 16 heads of 64


@dataclass
class TextConfig:
    width: int = 1024
    heads: int = 16
    layers: int = 24
    vocab: int = 49408
    context: int = 77
    mlp: int = 4096
    layer: str = "penultimate"

    @staticmethod
    def from_state_dict(sd: Dict[str, torch.Tensor], prefix: str = PREFIX, layer: str = "penultimate") -> "TextConfig":
        """Infer the configuration from the shapes of an open_clip-named dict (heads = width / 64)."""
        pos = sd[prefix + "positional_embedding"]
        tok = sd[prefix + "token_embedding.weight"]
        context, width = int(pos.shape[0]), int(pos.shape[1])
        head = prefix + "transformer.resblocks."
        blocks = {int(k[len(head):].split(".", 1)[0]) for k in sd if k.startswith(head)}
        if not blocks or blocks != set(range(len(blocks))):
            raise ValueError(f"text tower: resblocks {sorted(blocks)[:8]} are not 0..n-1")
        if width % HEAD_DIM:
            raise ValueError(f"text tower width {width} is not a multiple of the head dim {HEAD_DIM}")
        mlp = int(sd[head + "0.mlp.c_fc.weight"].shape[0])
        return TextConfig(width=width, heads=width // HEAD_DIM, layers=len(blocks), vocab=int(tok.shape[0]),
                          context=context, mlp=mlp, layer=layer)

    def blocks_run(self) -> int:
        if self.layer == "penultimate":
            return self.layers - 1
        if self.layer == "last":
            return self.layers
        raise ValueError(f"layer {self.layer!r} (last | penultimate)")


def has_tower(sd: Dict[str, torch.Tensor], prefix: str = PREFIX) -> bool:
    head = prefix + "transformer."
    return any(k.startswith(head) for k in sd)


def param_shapes(cfg: TextConfig) -> Dict[str, Tuple[int, ...]]:
    """name (without prefix) -> shape of every tensor the tower reads."""
    w, m = cfg.width, cfg.mlp
    s: Dict[str, Tuple[int, ...]] = {"token_embedding.weight": (cfg.vocab, w), "positional_embedding": (cfg.context, w)}
    for i in range(cfg.layers):
        b = f"transformer.resblocks.{i}."
        s.update({b + "ln_1.weight": (w,), b + "ln_1.bias": (w,), b + "attn.in_proj_weight": (3 * w, w),
                  b + "attn.in_proj_bias": (3 * w,), b + "attn.out_proj.weight": (w, w), b + "attn.out_proj.bias": (w,),
                  b + "ln_2.weight": (w,), b + "ln_2.bias": (w,), b + "mlp.c_fc.weight": (m, w),
                  b + "mlp.c_fc.bias": (m,), b + "mlp.c_proj.weight": (w, m), b + "mlp.c_proj.bias": (w,)})
    s.update({"ln_final.weight": (w,), "ln_final.bias": (w,)})
    return s


def init_spec(name: str, shape: Tuple[int, ...]) -> Tuple[float, float]:
    """(scale, offset) of the synthetic tower, uniform in [offset - scale, offset + scale): linears ~ 1/sqrt(fan_in)
    (unit-variance outputs from LayerNorm'd inputs keep the scores O(1)), LayerNorm gammas near 1, small biases and
    embeddings. The names differ from every other parameter's, so no existing seed or value moves."""
    if name.endswith("token_embedding.weight"):
        return 0.05, 0.0
    if name.endswith("positional_embedding"):
        return 0.02, 0.0
    if len(shape) == 2:
        return math.sqrt(3.0 / shape[1]), 0.0
    if "ln_" in name and name.endswith(".weight"):
        return 0.1, 1.0
    return 0.05, 0.0


@dataclass
class _Block:
    ln1: Tuple[torch.Tensor, torch.Tensor]
    in_proj: ops.ConvParams
    out_proj: ops.ConvParams
    ln2: Tuple[torch.Tensor, torch.Tensor]
    c_fc: ops.ConvParams
    c_proj: ops.ConvParams


class OpenCLIPTextEncoder:
    def __init__(self, cfg: Optional[TextConfig] = None, compute_dtype=torch.bfloat16, device="cuda"):
        self.cfg = cfg or TextConfig()
        if self.cfg.width != self.cfg.heads * HEAD_DIM:
            raise ValueError(f"text tower: width {self.cfg.width} != heads {self.cfg.heads} x {HEAD_DIM} "
                             "(the causal attention kernel is built for 64-wide heads)")
        self.cfg.blocks_run()  # validates `layer`
        self.compute_dtype = compute_dtype
        self.device = torch.device(device)
        self.shapes = param_shapes(self.cfg)
        self.blocks: List[_Block] = []
        self.tok: Optional[torch.Tensor] = None
        self._empty: Optional[torch.Tensor] = None  # cached context of [""]

    # ------------------------------------------------------------------ weights
    def _f32(self, t: torch.Tensor) -> torch.Tensor:
        return t.detach().to(device=self.device, dtype=torch.float32).contiguous()

    def _install(self, get) -> None:
        """Pack the tower from get(name) -> fp32 tensor (any device); linears packed as ParamStore packs them
        (rdeic_pack_conv_weight, K padded to 64), embeddings and LayerNorm parameters kept in fp32."""
        cfg, dt = self.cfg, self.compute_dtype
        self.tok = self._f32(get("token_embedding.weight"))
        self.pos = self._f32(get("positional_embedding"))
        self.blocks = []
        for i in range(cfg.blocks_run()):
            b = f"transformer.resblocks.{i}."
            def pack(w: str, bias: str, b: str = b) -> ops.ConvParams:
                return ops.ConvParams.pack(self._f32(get(b + w)), self._f32(get(b + bias)), dtype=dt)

            self.blocks.append(_Block(
                ln1=(self._f32(get(b + "ln_1.weight")), self._f32(get(b + "ln_1.bias"))),
                in_proj=pack("attn.in_proj_weight", "attn.in_proj_bias"),
                out_proj=pack("attn.out_proj.weight", "attn.out_proj.bias"),
                ln2=(self._f32(get(b + "ln_2.weight")), self._f32(get(b + "ln_2.bias"))),
                c_fc=pack("mlp.c_fc.weight", "mlp.c_fc.bias"),
                c_proj=pack("mlp.c_proj.weight", "mlp.c_proj.bias")))
        self.ln_final = (self._f32(get("ln_final.weight")), self._f32(get("ln_final.bias")))
        self._empty = None

    def load_state_dict(self, sd: Dict[str, torch.Tensor], prefix: str = PREFIX):
        """Load the checkpoint's own names (`prefix` + token_embedding.weight, positional_embedding,
        transformer.resblocks.{i}.*, ln_final.*). Every tensor the tower reads must be present with its shape;
        text_projection, logit_scale and attn_mask are ignored."""
        missing = [n for n in self.shapes if prefix + n not in sd]
        if missing:
            raise KeyError(f"text tower: missing parameters: {missing[:8]}{' ...' if len(missing) > 8 else ''}")
        for n, shape in self.shapes.items():
            if tuple(sd[prefix + n].shape) != shape:
                raise ValueError(f"{prefix + n}: checkpoint shape {tuple(sd[prefix + n].shape)} != {shape}")
        self._install(lambda n: sd[prefix + n])
        return self

    def init_synthetic(self, seed: Optional[int] = None, prefix: str = PREFIX):
        """Seeded weights generated on the device by name (rdeic_fill_uniform, as the rest of the model's)."""
        seed = W.GLOBAL_SEED if seed is None else seed

        def gen(n: str) -> torch.Tensor:
            shape = self.shapes[n]
            scale, offset = init_spec(n, shape)
            t = torch.empty(shape, dtype=torch.float32, device=self.device)
            return ops.fill_uniform(t, W.param_seed(prefix + n, seed), scale, offset)

        self._install(gen)
        return self

    # ------------------------------------------------------------------ forward
    def check_tokens(self, tokens: torch.Tensor) -> torch.Tensor:
        """Host-side validation before any launch: integer [B, context], 0 <= id < vocab. Returns CPU int64."""
        if tokens.dtype not in (torch.int64, torch.int32, torch.int16, torch.uint8):
            raise TypeError(f"token ids must be an integer tensor, got {tokens.dtype}")
        t = tokens.detach().to("cpu", torch.int64)
        if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] != self.cfg.context:
            raise ValueError(f"tokens must be [B, {self.cfg.context}], got {tuple(t.shape)}")
        lo, hi = int(t.min()), int(t.max())
        if lo < 0 or hi >= self.cfg.vocab:
            raise ValueError(f"token id out of range: min {lo}, max {hi}, vocabulary {self.cfg.vocab}")
        return t

    @torch.no_grad()
    def encode_tokens(self, tokens: torch.Tensor) -> torch.Tensor:
        """tokens [B, context] -> [B, context, width] in the compute dtype (encode_with_transformer)."""
        if self.tok is None:
            raise RuntimeError("text tower has no weights: load_state_dict or init_synthetic first")
        cfg = self.cfg
        t = self.check_tokens(tokens)
        B, L, Wd = t.shape[0], cfg.context, cfg.width
        tok = t.to(torch.int32).to(self.device)
        x = ops.embed_tokens(self.tok, self.pos, tok, self.compute_dtype)
        rows = B * L
        o = torch.empty((rows, Wd), dtype=self.compute_dtype, device=self.device)
        scale = HEAD_DIM ** -0.5
        for blk in self.blocks:
            n1 = ops.layer_norm(x, blk.ln1[0], blk.ln1[1], eps=1e-5)
            qkv = ops.linear(n1, blk.in_proj, images=B)
            ops.attention_causal(qkv[:, :Wd], qkv[:, Wd:2 * Wd], qkv[:, 2 * Wd:], o, batch=B, heads=cfg.heads, l=L,
                                 dh=HEAD_DIM, scale=scale)
            x = ops.linear(o, blk.out_proj, res=x, images=B)
            n2 = ops.layer_norm(x, blk.ln2[0], blk.ln2[1], eps=1e-5)
            hid = ops.linear(n2, blk.c_fc, act=ops.GELU, images=B)
            x = ops.linear(hid, blk.c_proj, res=x, images=B)
        x = ops.layer_norm(x, self.ln_final[0], self.ln_final[1], eps=1e-5)
        return x.view(B, L, Wd)

    def encode_empty(self) -> torch.Tensor:
        """The context of [""] ([1, context, width]), computed once per loaded tower."""
        if self._empty is None:
            t = torch.zeros((1, self.cfg.context), dtype=torch.int64)
            t[0, 0], t[0, 1] = SOT, EOT
            self._empty = self.encode_tokens(t)
        return self._empty
