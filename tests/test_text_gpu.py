"""The OpenCLIP text tower on the MI355X (rdeic_amd/text.py): against the float64 restatement of
encode_with_transformer (tests/text_ref.py) on the same seeded weights, batch invariance bit for bit, the RDEIC
integration at the real width (load_state_dict builds the tower, get_learned_conditioning, the cached "" context,
the UNet running on it), and the partition CLI's --captions_file.

Bounds. fp32 mode: relative L2 <= 1e-4, the project's fp32-against-fp64 bound. bf16 mode: no
more than twice the relative L2 of the same restatement run by torch on the CPU entirely in bfloat16 (computed
here; the factor covers the different rounding points: fp32 accumulation and fp32 LayerNorm statistics on the
device against bf16 everywhere on the CPU). A missing mask moves the output by ~0.3 and the wrong layer by ~0.5."""
import csv
import gzip
import json
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import text_ref as R

pytestmark = pytest.mark.gpu

CONFIGS = {"w128": dict(width=128, layers=4, vocab=512, batch=3),
           "w1024": dict(width=1024, layers=3, vocab=1024, batch=2)}  # the real linears' shapes
SKIP = {"penultimate": 1, "last": 0}


@lru_cache(maxsize=None)
def _case(name):
    c = CONFIGS[name]
    cfg = R.text_cfg(width=c["width"], layers=c["layers"], vocab=c["vocab"])
    sd = R.seeded_text_state_dict(cfg, seed=21)
    tokens = R.seeded_tokens(c["batch"], cfg, seed=22)
    return cfg, sd, tokens


@lru_cache(maxsize=None)
def _reference(name, layer):
    """(float64 restatement, relative L2 of the all-bf16 CPU restatement against it); computed once, read-only."""
    cfg, sd, tokens = _case(name)
    ref = R.encode_with_transformer(sd, tokens, cfg.heads, torch.float64, skip_last=SKIP[layer])
    cpu16 = R.encode_with_transformer(sd, tokens, cfg.heads, torch.bfloat16, skip_last=SKIP[layer])
    return ref, R.rel_l2(cpu16, ref)


@lru_cache(maxsize=None)
def _tower(name, layer, dtype):
    from rdeic_amd.text import OpenCLIPTextEncoder, TextConfig
    _, sd, _ = _case(name)
    return OpenCLIPTextEncoder(TextConfig.from_state_dict(sd, layer=layer), dtype, "cuda").load_state_dict(sd)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("layer", ["penultimate", "last"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_tower_against_float64_restatement(gpu, name, layer, dtype):
    cfg, _, tokens = _case(name)
    ref, cpu16 = _reference(name, layer)
    out = _tower(name, layer, dtype).encode_tokens(tokens)
    torch.cuda.synchronize()
    assert out.dtype == dtype and tuple(out.shape) == (tokens.shape[0], cfg.context, cfg.width)
    err = R.rel_l2(out, ref)
    bound = 1e-4 if dtype == torch.float32 else 2 * cpu16
    print(f"{name} {layer} {dtype}: rel L2 = {err:.3g} (bound {bound:.3g}; all-bf16 CPU restatement {cpu16:.3g})")
    assert err <= bound


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_batch_invariance_bitwise(gpu, name, dtype):
    _, _, tokens = _case(name)
    tower = _tower(name, "penultimate", dtype)
    both = torch.cat([tokens, tokens[:1]])[:3]  # three rows in either configuration
    full = tower.encode_tokens(both)
    for b in range(3):
        assert torch.equal(tower.encode_tokens(both[b:b + 1])[0], full[b]), b
    assert torch.equal(tower.encode_tokens(both), full)


def test_token_ids_are_validated_on_the_host(gpu):
    cfg, _, tokens = _case("w128")
    tower = _tower("w128", "penultimate", torch.float32)
    bad = tokens.clone()
    bad[1, 5] = cfg.vocab
    with pytest.raises(ValueError, match="out of range"):
        tower.encode_tokens(bad)
    bad[1, 5] = -1
    with pytest.raises(ValueError, match="out of range"):
        tower.encode_tokens(bad)
    with pytest.raises(ValueError):
        tower.encode_tokens(tokens[:, :50])
    with pytest.raises(TypeError):
        tower.encode_tokens(tokens.float())


# ---------------------------------------------------------------------------------------------- integration
@pytest.fixture(scope="module")
def real_width():
    """The fp32 model with seeded weights plus a state dict holding a 1024-wide, 2-layer, full-vocabulary tower."""
    from rdeic_amd.rdeic import RDEIC
    cfg = R.text_cfg(width=1024, layers=2, vocab=49408)
    sd = R.seeded_text_state_dict(cfg, seed=31)
    model = RDEIC(compute_dtype=torch.float32).init_synthetic()
    assert model.cond_stage_model is None
    model.load_state_dict(sd, strict=False)
    model.preprocess_model.update(force=True)
    return model, cfg, sd


def test_integration_at_the_real_width(gpu, real_width):
    from rdeic_amd import _lib
    model, cfg, sd = real_width
    tower = model.cond_stage_model
    assert tower is not None and (tower.cfg.width, tower.cfg.heads, tower.cfg.layers, tower.cfg.vocab) == \
        (1024, 16, 2, 49408)
    assert model.session().cond_stage_model is tower  # sessions share the tower
    empty = torch.zeros((1, 77), dtype=torch.int64)
    empty[0, 0], empty[0, 1] = 49406, 49407
    ctx = model.get_learned_conditioning([""])
    assert ctx.dtype == torch.float32 and tuple(ctx.shape) == (1, 77, 1024) and ctx.is_cuda
    assert torch.equal(ctx, tower.encode_tokens(empty))
    assert torch.equal(ctx, model.get_learned_conditioning(empty))
    ref = R.encode_with_transformer(sd, empty, cfg.heads, torch.float64, skip_last=1)
    err = R.rel_l2(ctx, ref)
    print(f'"" context at width 1024, fp32: rel L2 = {err:.3g}')
    assert err <= 1e-4
    _lib.RECORDER = calls = []  # every library call is appended while this is a list
    try:
        assert model.get_learned_conditioning([""]) is ctx  # cached: the same tensor, nothing launched
    finally:
        _lib.RECORDER = None
    assert calls == []
    # the UNet takes the new context
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 16, 16, 4, generator=g).cuda()
    hint = torch.randn(1, 16, 16, 256, generator=g).cuda()
    t = torch.full((1,), 151, dtype=torch.long, device="cuda")
    with torch.no_grad():
        e = model.eps_nhwc(x, t, hint, ctx)
    assert tuple(e.shape) == (1, 16, 16, 4) and bool(torch.isfinite(e).all())
    # a reload builds a new tower and drops the cached context
    model.load_state_dict(sd, strict=False)
    model.preprocess_model.update(force=True)
    assert model.cond_stage_model is not tower
    ctx2 = model.get_learned_conditioning([""])
    assert ctx2 is not ctx and torch.equal(ctx2, ctx)


def test_model_without_tower_keys_has_no_tower(gpu):
    from rdeic_amd.rdeic import RDEIC
    m = RDEIC(compute_dtype=torch.bfloat16)
    m.load_state_dict({}, strict=False)
    assert m.cond_stage_model is None
    with pytest.raises(RuntimeError, match="no text tower"):
        m.get_learned_conditioning([""])
    from rdeic_amd.text import TextConfig
    m.init_text_synthetic(TextConfig(width=128, heads=2, layers=2, mlp=512))
    out = m.get_learned_conditioning([""])
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (1, 77, 128) and bool(torch.isfinite(out.float()).all())


# ---------------------------------------------------------------------------------------------- partition CLI
def test_partition_cli_captions(gpu, real_width, tmp_path, monkeypatch):
    import inference_partition as P
    from PIL import Image
    from rdeic_amd.synthetic import synth_image
    model, _, _ = real_width
    monkeypatch.setattr(P, "_load", lambda args: model)
    monkeypatch.delenv("RDEIC_CLIP_VOCAB", raising=False)
    src = tmp_path / "in"
    src.mkdir()
    Image.fromarray(synth_image(64, 64, 41)).save(src / "a.png")
    Image.fromarray(synth_image(64, 64, 42)).save(src / "b.png")
    vocab = tmp_path / "toy_bpe.txt.gz"
    with gzip.open(vocab, "wb") as f:
        f.write('"#version: toy\na b\nab c</w>\nb c</w>\n'.encode())
    caps = tmp_path / "caps.json"
    caps.write_text(json.dumps({"a.png": "abc bc cab", "b.png": "a cab!"}))
    none = tmp_path / "none.json"
    none.write_text("{}")
    base = ["--input", str(src), "--sampler", "ddim", "--steps", "2", "--batch_size", "2"]

    def pixels(d):
        return [np.array(Image.open(tmp_path / d / f"{n}.png")) for n in "ab"]

    def bodies(d):
        return [(tmp_path / d / "data" / n).read_bytes() for n in "ab"]

    rec = P.main(base + ["--output", str(tmp_path / "cap"), "--captions_file", str(caps), "--clip_vocab", str(vocab),
                         "--guidance_scale", "2"])
    assert [r["caption"] for r in rec] == ["abc bc cab", "a cab!"]
    with open(tmp_path / "cap" / "metrics.csv") as f:
        rows = list(csv.DictReader(f))
    assert [r["caption"] for r in rows] == ["abc bc cab", "a cab!"] and all(np.isfinite(float(r["psnr"])) for r in rows)
    plain = P.main(base + ["--output", str(tmp_path / "plain")])
    assert all("caption" not in r for r in plain)
    with open(tmp_path / "plain" / "metrics.csv") as f:
        assert "caption" not in f.readline()
    # the captions reach the pixels; the bitstreams carry no text
    assert bodies("cap") == bodies("plain")
    assert any(not np.array_equal(a, b) for a, b in zip(pixels("cap"), pixels("plain")))
    # no captions and guidance 1: the run without the flag, bytes and pixels
    P.main(base + ["--output", str(tmp_path / "empty"), "--captions_file", str(none), "--clip_vocab", str(vocab),
                   "--guidance_scale", "1"])
    assert bodies("empty") == bodies("plain")
    for a, b in zip(pixels("empty"), pixels("plain")):
        assert np.array_equal(a, b)
