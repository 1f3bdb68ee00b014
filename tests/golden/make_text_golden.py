"""Golden for the text tower: the reference's own FrozenOpenCLIPEmbedder.encode_with_transformer /
text_transformer_forward (ldm/modules/encoders/modules.py:216-233) over the seeded 128-wide, 4-layer test tower
(tests/text_ref.py), in both layer modes. Writes tests/golden/text_tower.npz: the tokens, the two fp32 outputs and a
checksum of the regenerated weights (the weights themselves are regenerated from the seed by the test).

open_clip is absent, so a stub module provides what FrozenOpenCLIPEmbedder.__init__ asks of it: a text model with
open_clip's attribute names (token_embedding, positional_embedding, transformer.resblocks, ln_final, attn_mask)
whose blocks are open_clip's ResidualAttentionBlock restated on torch's own nn.MultiheadAttention. kornia, which
modules.py imports for its image embedders only, is stubbed empty. Run from the repository root:

    python tests/golden/make_text_golden.py
"""
import hashlib
import os
import sys
import types
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import text_ref as R  # noqa: E402
from tests.golden import refload  # noqa: E402

SEED, TOKEN_SEED, BATCH = 7, 8, 2
CFG = R.text_cfg(width=128, layers=4, vocab=512)


class ResidualAttentionBlock(nn.Module):
    """open_clip.transformer.ResidualAttentionBlock (LND layout, no layer scale)."""

    def __init__(self, width, heads, mlp):
        super().__init__()
        self.ln_1 = nn.LayerNorm(width)
        self.attn = nn.MultiheadAttention(width, heads)
        self.ln_2 = nn.LayerNorm(width)
        self.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(width, mlp)), ("gelu", nn.GELU()),
                                              ("c_proj", nn.Linear(mlp, width))]))

    def forward(self, x, attn_mask=None):
        h = self.ln_1(x)
        x = x + self.attn(h, h, h, need_weights=False, attn_mask=attn_mask)[0]
        return x + self.mlp(self.ln_2(x))


class Transformer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.grad_checkpointing = False
        self.resblocks = nn.ModuleList([ResidualAttentionBlock(cfg.width, cfg.heads, cfg.mlp)
                                        for _ in range(cfg.layers)])


class StubCLIP(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.visual = nn.Identity()  # FrozenOpenCLIPEmbedder deletes it
        self.token_embedding = nn.Embedding(cfg.vocab, cfg.width)
        self.positional_embedding = nn.Parameter(torch.empty(cfg.context, cfg.width))
        self.transformer = Transformer(cfg)
        self.ln_final = nn.LayerNorm(cfg.width)
        self.text_projection = nn.Parameter(torch.empty(cfg.width, cfg.width))
        self.logit_scale = nn.Parameter(torch.ones([]))
        # open_clip.CLIP.build_attention_mask
        self.register_buffer("attn_mask", torch.full((cfg.context, cfg.context), float("-inf")).triu_(1))


def main():
    oc = types.ModuleType("open_clip")
    oc.create_model_and_transforms = lambda arch, device=None, pretrained=None: (StubCLIP(CFG), None, None)
    sys.modules["open_clip"] = oc
    if "kornia" not in sys.modules:
        try:
            import kornia  # noqa: F401
        except ImportError:
            sys.modules["kornia"] = types.ModuleType("kornia")
    refload.load()  # puts the reference on sys.path with its other stubs
    from ldm.modules.encoders.modules import FrozenOpenCLIPEmbedder

    sd = R.seeded_text_state_dict(CFG, SEED)
    tokens = R.seeded_tokens(BATCH, CFG, TOKEN_SEED)
    out = {}
    for layer in ("penultimate", "last"):
        emb = FrozenOpenCLIPEmbedder(layer=layer)
        emb.load_state_dict({k[len("cond_stage_model."):]: v for k, v in sd.items()}, strict=True)
        with torch.no_grad():
            out[layer] = emb.encode_with_transformer(tokens).float().numpy()
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].contiguous().numpy().tobytes())
    path = os.path.join(HERE, "text_tower.npz")
    np.savez_compressed(path, tokens=tokens.numpy(), penultimate=out["penultimate"], last=out["last"],
                        seed=np.int64(SEED), weights_sha256=np.array(h.hexdigest()))
    for layer in out:
        ref = R.encode_with_transformer(sd, tokens, CFG.heads, torch.float64, skip_last=int(layer == "penultimate"))
        print(layer, "rel L2 vs the fp64 restatement:", R.rel_l2(torch.from_numpy(out[layer]), ref))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
