"""Host side of the text conditioning (rdeic_amd/text.py, rdeic_amd/tokenizer.py): the plain-torch restatement of
encode_with_transformer (tests/text_ref.py) against an independent implementation (transformers.CLIPTextModel) and
against the reference's own module (tests/golden/text_tower.npz), the tokenizer's mechanics, the configuration
inferred from a state dict, and the start-up refusals of the partition CLI. No device code runs here."""
import gzip
import hashlib
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import text_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "text_tower.npz")


# ---------------------------------------------------------------------------------------------- restatement
def _hf_model(sd, cfg):
    """transformers.CLIPTextModel in float64 holding the open_clip-named weights of sd."""
    transformers = pytest.importorskip("transformers")
    hc = transformers.CLIPTextConfig(vocab_size=cfg.vocab, hidden_size=cfg.width, intermediate_size=cfg.mlp,
                                     num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads,
                                     max_position_embeddings=cfg.context, hidden_act="gelu", layer_norm_eps=1e-5,
                                     attention_dropout=0.0, pad_token_id=0, bos_token_id=cfg.vocab - 2,
                                     eos_token_id=cfg.vocab - 1)
    model = transformers.CLIPTextModel(hc).double().eval()
    p = R.PREFIX
    w = cfg.width
    hf = {"text_model.embeddings.token_embedding.weight": sd[p + "token_embedding.weight"],
          "text_model.embeddings.position_embedding.weight": sd[p + "positional_embedding"],
          "text_model.final_layer_norm.weight": sd[p + "ln_final.weight"],
          "text_model.final_layer_norm.bias": sd[p + "ln_final.bias"]}
    for i in range(cfg.layers):
        b, h = f"{p}transformer.resblocks.{i}.", f"text_model.encoder.layers.{i}."
        for j, name in enumerate(("q_proj", "k_proj", "v_proj")):
            hf[h + f"self_attn.{name}.weight"] = sd[b + "attn.in_proj_weight"][j * w:(j + 1) * w]
            hf[h + f"self_attn.{name}.bias"] = sd[b + "attn.in_proj_bias"][j * w:(j + 1) * w]
        for src, dst in (("attn.out_proj", "self_attn.out_proj"), ("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"),
                         ("mlp.c_fc", "mlp.fc1"), ("mlp.c_proj", "mlp.fc2")):
            hf[h + dst + ".weight"] = sd[b + src + ".weight"]
            hf[h + dst + ".bias"] = sd[b + src + ".bias"]
    own = model.state_dict()
    want = {k for k in own if not k.endswith("position_ids")}
    # transformers 5 drops the `text_model.` level on some releases: accept either spelling
    if not want <= set(hf):
        hf = {k[len("text_model."):]: v for k, v in hf.items()}
    assert want <= set(hf), sorted(want - set(hf))[:4]
    model.load_state_dict({k: v.double() for k, v in hf.items()}, strict=False)
    return model


def test_restatement_matches_transformers_clip_text_model():
    cfg = R.text_cfg(width=128, layers=3, vocab=512)
    sd = R.seeded_text_state_dict(cfg, seed=3)
    tokens = R.seeded_tokens(2, cfg, seed=4)
    model = _hf_model(sd, cfg)
    with torch.no_grad():
        out = model(input_ids=tokens, output_hidden_states=True)
        hf_last = out.last_hidden_state
        hf_pen = model.text_model.final_layer_norm(out.hidden_states[-2]) if hasattr(model, "text_model") \
            else model.final_layer_norm(out.hidden_states[-2])
    for skip, want in ((0, hf_last), (1, hf_pen)):
        got = R.encode_with_transformer(sd, tokens, cfg.heads, torch.float64, skip_last=skip)
        err = float((got - want).abs().max())
        print(f"skip_last={skip}: max |restatement - transformers| = {err:.3g}")
        assert err <= 1e-12
    # the mask and the layer break are visible to this check: dropping either moves the output
    assert R.rel_l2(R.encode_with_transformer(sd, tokens, cfg.heads, causal=False), hf_pen) > 0.05
    assert R.rel_l2(hf_last, hf_pen) > 0.05


def test_restatement_matches_reference_module_golden():
    """tests/golden/text_tower.npz (make_text_golden.py): the reference's FrozenOpenCLIPEmbedder.
    encode_with_transformer / text_transformer_forward over the seeded 128-wide, 4-layer tower, both layer modes.
    Pins the reference's layer break and ln_final against the restatement."""
    g = np.load(GOLDEN)
    cfg = R.text_cfg(width=128, layers=4, vocab=512)
    sd = R.seeded_text_state_dict(cfg, seed=int(g["seed"]))
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].contiguous().numpy().tobytes())
    assert h.hexdigest() == str(g["weights_sha256"]), "the seeded test tower changed: regenerate the golden"
    tokens = torch.from_numpy(g["tokens"])
    for skip, key in ((1, "penultimate"), (0, "last")):
        got = R.encode_with_transformer(sd, tokens, cfg.heads, torch.float32, skip_last=skip)
        err = R.rel_l2(got, torch.from_numpy(g[key]))
        print(f"{key}: rel L2 restatement (fp32) vs reference module (fp32) = {err:.3g}")
        assert err <= 1e-5  # two fp32 evaluations of the same function; a wrong layer break is ~0.5


# ---------------------------------------------------------------------------------------------- tokenizer
def _toy_vocab(tmp_path) -> str:
    # header line, then merges in rank order: ids 512 ("ab"), 513 ("abc</w>"), 514 ("bc</w>")
    path = tmp_path / "toy_bpe.txt.gz"
    with gzip.open(path, "wb") as f:
        f.write('"#version: toy\na b\nab c</w>\nb c</w>\n'.encode())
    return str(path)


def test_tokenizer_empty_text_needs_no_vocabulary(monkeypatch):
    from rdeic_amd import tokenizer as T
    monkeypatch.delenv(T.VOCAB_ENV, raising=False)
    t = T.tokenize(["", "   "])
    assert t.dtype == torch.int64 and tuple(t.shape) == (2, 77)
    for row in t:
        assert row[:2].tolist() == [49406, 49407] and int(row[2:].abs().sum()) == 0
    with pytest.raises(FileNotFoundError, match="bpe_simple_vocab_16e6.txt.gz"):
        T.tokenize(["a photo"])


def test_tokenizer_bpe_mechanics_on_a_toy_vocabulary(tmp_path):
    from rdeic_amd import tokenizer as T
    v = _toy_vocab(tmp_path)
    # byte table: '!'..'~' are ids 0..93 in order, so 'a' = 97 - 33 = 64, 'b' = 65, 'c' = 66, '!' = 0, '&' = 5;
    # the word-final forms are + 256; merges follow from 512
    t = T.tokenize(["abc", "bc", "cab", "ABC  bc!", "a &amp; b"], vocab_path=v)
    exp = [[513],                  # a b -> ab (rank 0), ab c</w> -> abc</w> (rank 1)
           [514],                  # b c</w> -> bc</w> (rank 2)
           [66, 64, 65 + 256],     # no pair of c a b</w> is a merge
           [513, 514, 0 + 256],    # lower-cased, whitespace collapsed, punctuation its own word
           [64 + 256, 5 + 256, 65 + 256]]  # html-unescaped
    for row, body in zip(t, exp):
        want = [49406] + body + [49407]
        assert row[:len(want)].tolist() == want and int(row[len(want):].abs().sum()) == 0
    long = T.tokenize(["cab " * 100], vocab_path=v)[0]
    assert long[0] == 49406 and long[-1] == 49407 and long[1:4].tolist() == [66, 64, 321]
    assert int((long == 49407).sum()) == 1
    short = T.tokenize(["cab"], vocab_path=v, context=4)[0]
    assert short.tolist() == [49406, 66, 64, 49407]  # cut to the context, EOT forced last


# ---------------------------------------------------------------------------------------------- configuration
def test_config_is_inferred_from_the_state_dict():
    from rdeic_amd.text import TextConfig, has_tower, param_shapes
    cfg = R.text_cfg(width=192, layers=5, vocab=300, context=33, mlp=256)
    sd = R.seeded_text_state_dict(cfg)
    got = TextConfig.from_state_dict(sd)
    assert (got.width, got.heads, got.layers, got.vocab, got.context, got.mlp, got.layer) == \
        (192, 3, 5, 300, 33, 256, "penultimate")
    assert has_tower(sd) and not has_tower({"model.diffusion_model.out.2.weight": torch.zeros(1)})
    shapes = param_shapes(got)
    ignored = {R.PREFIX + n for n in ("text_projection", "logit_scale", "attn_mask")}
    assert {R.PREFIX + n for n in shapes} == set(sd) - ignored
    assert all(tuple(sd[R.PREFIX + n].shape) == s for n, s in shapes.items())
    d = TextConfig()
    assert (d.width, d.heads, d.layers, d.vocab, d.context, d.mlp, d.layer) == \
        (1024, 16, 24, 49408, 77, 4096, "penultimate")
    assert d.blocks_run() == 23 and TextConfig(layer="last").blocks_run() == 24


def test_state_dict_without_tower_keys_leaves_no_tower():
    from rdeic_amd.rdeic import RDEIC
    m = RDEIC(device="cpu")
    assert m.cond_stage_model is None
    m.load_state_dict({}, strict=False)
    assert m.cond_stage_model is None and m.session().cond_stage_model is None
    with pytest.raises(RuntimeError, match="no text tower"):
        m.get_learned_conditioning([""])


# ---------------------------------------------------------------------------------------------- CLI refusals
def test_partition_cli_refuses_captions_without_vocabulary_or_tower(tmp_path, monkeypatch, capsys):
    import inference_partition as P
    monkeypatch.delenv("RDEIC_CLIP_VOCAB", raising=False)
    src = tmp_path / "in"
    src.mkdir()
    caps = tmp_path / "caps.json"
    caps.write_text(json.dumps({"a.png": "abc"}))
    base = ["--input", str(src), "--output", str(tmp_path / "out"), "--captions_file", str(caps)]
    with pytest.raises(SystemExit):
        P.parse_args(base)
    assert "bpe_simple_vocab_16e6.txt.gz" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        P.parse_args(base + ["--clip_vocab", str(tmp_path / "missing.gz")])
    with pytest.raises(SystemExit):
        P.parse_args(["--input", str(src), "--captions_file", str(tmp_path / "missing.json"), "--clip_vocab",
                      _toy_vocab(tmp_path)])
    v = _toy_vocab(tmp_path)
    monkeypatch.setenv("RDEIC_CLIP_VOCAB", v)
    assert P.parse_args(base).clip_vocab == v  # the environment variable serves as the flag
    # a model without the tower: refused before any image is read
    monkeypatch.setattr(P, "_load", lambda args: SimpleNamespace(cond_stage_model=None, device="cpu"))
    with pytest.raises(SystemExit, match="text tower"):
        P.main(base)
    assert not (tmp_path / "out").exists()
    with pytest.raises(SystemExit, match="Qwen2-VL"):  # the captioner stays refused, with its message
        P.main(["--input", str(src), "--use_captions"])
