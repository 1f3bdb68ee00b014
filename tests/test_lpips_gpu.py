"""LPIPS on the device (rdeic_amd/lpips.py, csrc/lpips.hip) against the CPU restatement of the reference's
model/lpips.py (tests/lpips_ref.py): the three kernels on their own, the metric end to end with a seeded
backbone and the published heads, its batch / chunk invariance, and the CLI / robustness wiring.

End-to-end tolerance, 1e-4 relative to the fp64 restatement: the fp32 conv sums have K <= 3456 terms
(3x3x384), so a feature carries about sqrt(K) 2^-24 = 3.5e-6 of relative error; the five-layer
normalise-and-difference keeps that at the 1e-5 level; 1e-4 is one decade of margin and keeps every digit
the CLI prints (:.4f) for scores up to 1. The fp32 CPU restatement itself sits near 1e-6.

Layer-distance tolerance, 1e-4 relative to the fp64 formula on the same fp32 inputs: with u = 2^-24 the norm
of c <= 512 values is within (c/2 + 2) u, a quotient within (c/2 + 3) u; for independent non-negative maps
|a/na| + |b/nb| is about 3 |a/na - b/nb|, and squaring doubles it: 2 * 3 * 259 u = 9.3e-5 in the worst case
(the random-sign typical figure is two decades smaller)."""
import csv
import os
from functools import lru_cache

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import lpips_ref as R

pytestmark = pytest.mark.gpu

RTOL = 1e-4


@lru_cache(maxsize=None)
def _model(net):
    from rdeic_amd.lpips import LPIPS
    return LPIPS(net, backbone=R.seeded_backbone(net), lin=R.LIN_NPZ)


# ------------------------------------------------------------------ 1. prep
def test_prep_is_bit_exact(gpu):
    g = torch.Generator().manual_seed(7)
    img = torch.randint(0, 256, (2, 35, 47, 3), generator=g, dtype=torch.uint8)
    img[0, 0, :, 0] = torch.arange(47, dtype=torch.uint8) * 5  # and every level somewhere
    img[1].view(-1)[:256] = torch.arange(256, dtype=torch.uint8)
    want = R.scaling_layer(img.numpy(), torch.float32).permute(0, 2, 3, 1).contiguous()  # CPU fp32, true divisions
    got = _model("alex").prep(img.cuda()).cpu()
    assert got.shape == (2, 35, 47, 4) and got.dtype == torch.float32
    assert torch.equal(got[..., :3].contiguous().view(torch.int32), want.view(torch.int32))
    assert (got[..., 3].view(torch.int32) == 0).all()


# ------------------------------------------------------------------ 2. max pool
@pytest.mark.parametrize("shape,k,ld_in,ld_out", [
    ((2, 15, 15, 64), 3, 64, 64), ((2, 23, 19, 64), 3, 64, 64), ((1, 8, 11, 192), 3, 192, 192),
    ((1, 7, 5, 64), 2, 64, 64), ((2, 15, 15, 64), 3, 80, 72), ((2, 9, 10, 64), 2, 67, 65), ((1, 7, 7, 3), 3, 3, 3)])
def test_max_pool_is_bit_exact(gpu, shape, k, ld_in, ld_out):
    from rdeic_amd.lpips import max_pool
    n, h, w, c = shape
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randn((n, h, w, ld_in), generator=g)
    want = F.max_pool2d(x[..., :c].permute(0, 3, 1, 2), kernel_size=k, stride=2).permute(0, 2, 3, 1)
    ho, wo = (h - k) // 2 + 1, (w - k) // 2 + 1
    assert want.shape == (n, ho, wo, c)
    buf = torch.full((n, ho, wo, ld_out), -7.0, device="cuda")
    got = max_pool(x.cuda()[..., :c], k, 2, out=buf[..., :c])
    assert torch.equal(got.cpu(), want.contiguous())
    assert (buf[..., c:] == -7.0).all()  # nothing written past the channels
    if ld_in == c:
        assert torch.equal(max_pool(x.cuda(), k, 2).cpu(), want.contiguous())


def _max_pool_rule(x, k, s):
    """The documented rule: row-major scan of the window, strict >, a NaN wins and stays."""
    n, h, w, c = x.shape
    out = np.empty((n, (h - k) // s + 1, (w - k) // s + 1, c), np.float32)
    for i, oy, ox, ch in np.ndindex(*out.shape):
        m = x[i, oy * s, ox * s, ch]
        for dy, dx in np.ndindex(k, k):
            v = x[i, oy * s + dy, ox * s + dx, ch]
            if v > m or v != v:
                m = v
        out[i, oy, ox, ch] = m
    return out


@pytest.mark.parametrize("shape,k,ld", [((1, 3, 3, 4), 3, 4), ((2, 7, 9, 6), 3, 7), ((1, 5, 5, 64), 2, 64)])
def test_max_pool_special_values(gpu, shape, k, ld):
    """Signed zeros, an all -inf window and a NaN before a larger element, on the vector path (c, ld % 4 == 0) and
    the scalar one: the bits of the rule above, and of F.max_pool2d."""
    from rdeic_amd.lpips import max_pool
    n, h, w, c = shape
    g = torch.Generator().manual_seed(c * 10 + k)
    x = torch.randn((n, h, w, ld), generator=g)
    win = x[0, :k, :k]  # the first window, one case per channel
    win[..., 0] = -5.0
    win[0, 1, 0], win[1, 0, 0] = -0.0, 0.0  # -0.0 comes first and stays
    win[..., 1] = -5.0
    win[0, 1, 1], win[1, 0, 1] = 0.0, -0.0  # +0.0 comes first and stays
    win[..., 2] = float("-inf")
    win[0, 1, 3], win[k - 1, k - 1, 3] = float("nan"), 100.0  # a NaN, then the window's largest element
    want = _max_pool_rule(x[..., :c].numpy(), k, 2)
    nan = np.isnan(want)
    assert nan[0, 0, 0, 3] and nan.sum() == 1 and want[0, 0, 0, 2] == float("-inf")
    assert want.view(np.int32)[0, 0, 0, 0] == np.float32(-0.0).view(np.int32) and want.view(np.int32)[0, 0, 0, 1] == 0
    got = max_pool(x.cuda()[..., :c], k, 2).cpu().numpy()
    ref = F.max_pool2d(x[..., :c].permute(0, 3, 1, 2), kernel_size=k, stride=2).permute(0, 2, 3, 1).contiguous().numpy()
    for name, other in (("rule", want), ("F.max_pool2d", ref)):
        assert got.shape == other.shape and np.array_equal(np.isnan(got), np.isnan(other)), name
        assert np.array_equal(got.view(np.int32)[~nan], other.view(np.int32)[~nan]), name


# ------------------------------------------------------------------ 3. layer distance
@lru_cache(maxsize=None)
def _taps(c, h, w):
    """Two random non-negative [3, h, w, c] maps, a few pixels all-zero in one, the other, both; lin >= 0."""
    g = torch.Generator().manual_seed(c * 1000 + h * 31 + w)
    f0, f1 = torch.rand((3, h, w, c), generator=g), torch.rand((3, h, w, c), generator=g)
    f0, f1 = F.relu(f0 - 0.3), F.relu(f1 - 0.3)  # post-ReLU: about a third of the channels are zero
    hw = h * w
    f0.view(3, hw, c)[0, 0] = 0
    f1.view(3, hw, c)[1, hw - 1] = 0
    f0.view(3, hw, c)[2, hw // 2] = 0
    f1.view(3, hw, c)[2, hw // 2] = 0
    if hw > 64:  # and a whole wave's worth in a later block
        f0.view(3, hw, c)[1, 64:70] = 0
        f1.view(3, hw, c)[1, 66:72] = 0
    lin = torch.rand(c, generator=g) * 0.1
    want = R.layer_distance(f0.double().permute(0, 3, 1, 2), f1.double().permute(0, 3, 1, 2), lin.double()).numpy()
    return f0, f1, lin, want


@pytest.mark.parametrize("hw", [(1, 2), (3, 3), (15, 15), (23, 19)])
@pytest.mark.parametrize("c", [64, 192, 384, 512])
def test_layer_distance(gpu, c, hw):
    from rdeic_amd.lpips import layer_distance
    f0, f1, lin, want = _taps(c, *hw)
    a, b, l = f0.cuda(), f1.cuda(), lin.cuda()
    got = layer_distance(a, b, l)
    g = got.cpu().double().numpy()
    rel = np.abs(g - want) / want
    print(f"c={c} hw={hw}: got {g}, fp64 {want}, rel {rel.max():.3e}")
    assert np.isfinite(g).all() and (want > 0).all()
    assert rel.max() <= RTOL
    assert torch.equal(layer_distance(a, b, l), got)  # repeatable bit for bit
    for i in range(3):  # an image alone scores what it scores in the batch
        assert torch.equal(layer_distance(a[i:i + 1], b[i:i + 1], l), got[i:i + 1]), i
    acc = got.clone()
    layer_distance(b, a, l, out=acc, accumulate=True)  # second call adds
    assert torch.equal(acc, got + layer_distance(b, a, l))
    assert float(layer_distance(a, a, l).abs().max()) == 0.0  # identical maps, zero pixels included


@pytest.mark.parametrize("c,ld", [(512, 516), (512, 513), (384, 386), (384, 385), (192, 200)])
def test_layer_distance_pixel_stride(gpu, c, ld):
    """A channel slice of a wider buffer (ld > c), aligned for the wide loads or not, scores the same bits."""
    from rdeic_amd.lpips import layer_distance
    f0, f1, lin, _ = _taps(c, 15, 15)
    a, b, l = f0.cuda(), f1.cuda(), lin.cuda()
    wa = torch.full((3, 15, 15, ld), float("nan"), device="cuda")
    wb = torch.full((3, 15, 15, ld), float("nan"), device="cuda")
    wa[..., :c], wb[..., :c] = a, b
    assert torch.equal(layer_distance(wa[..., :c], wb[..., :c], l), layer_distance(a, b, l))


# ------------------------------------------------------------------ 4. / 5. end to end
@lru_cache(maxsize=None)
def _pairs(net, h, w):
    """(pred [2], target [2], fp64 restatement [2]): image + sigma-12 noise, and two unrelated images."""
    b, a = R.noisy_pair(h, w, 11)
    other = R.noisy_pair(h, w, 12)[1]
    pred, tgt = np.stack([b, other]), np.stack([a, a])
    return pred, tgt, R.lpips(net, R.seeded_backbone(net), pred, tgt)


@pytest.mark.parametrize("h,w", [(64, 64), (96, 80), (35, 47)])
def test_lpips_alex_matches_restatement(gpu, h, w):
    from rdeic_amd import metrics
    m = _model("alex")
    pred, tgt, want = _pairs("alex", h, w)
    p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(tgt).cuda()
    got = metrics.lpips(p, t, m)
    rel = np.abs(got - want) / want
    print(f"alex {h}x{w}: got {got}, fp64 {want}, rel {rel}")
    assert got.dtype == np.float64 and got.shape == (2,) and np.isfinite(got).all()
    assert want[0] < 0.05 < want[1]  # a small and a large score are both covered
    assert rel.max() <= RTOL
    assert (m(t, t) == 0.0).all()  # identical images: exactly zero
    swapped = m(t, p)
    print(f"  swapped rel {np.abs(swapped - got) / got}")
    assert (np.abs(swapped - got) <= RTOL * got).all()
    for i in range(2):  # batch of 2 against each pair alone
        assert m(p[i:i + 1], t[i:i + 1])[0] == got[i], i
    assert np.array_equal(m(p, t), got)


def test_lpips_vgg_matches_restatement(gpu):
    m = _model("vgg")
    pred, tgt, want = _pairs("vgg", 32, 48)
    p, t = torch.from_numpy(pred[:1]).cuda(), torch.from_numpy(tgt[:1]).cuda()
    got = m(p, t)
    rel = np.abs(got - want[:1]) / want[:1]
    print(f"vgg 32x48: got {got}, fp64 {want[:1]}, rel {rel}")
    assert rel.max() <= RTOL
    assert (m(t, t) == 0.0).all()


def test_lpips_size_and_input_checks(gpu):
    m = _model("alex")
    small = torch.zeros((1, 30, 64, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        m(small, small)
    ok = torch.zeros((1, 31, 31, 3), dtype=torch.uint8, device="cuda")
    assert m(ok, ok)[0] == 0.0
    with pytest.raises(ValueError):
        m(ok, ok.float())
    with pytest.raises(ValueError):
        m(ok, torch.zeros((1, 31, 32, 3), dtype=torch.uint8, device="cuda"))


# ------------------------------------------------------------------ 6. chunking
def test_chunking_does_not_change_scores(gpu, monkeypatch):
    from rdeic_amd import lpips as L
    m = _model("alex")
    pred, tgt, _ = _pairs("alex", 96, 80)
    p = torch.from_numpy(np.concatenate([pred, tgt[:1]])).cuda()
    t = torch.from_numpy(np.concatenate([tgt, pred[:1]])).cuda()
    whole = m(p, t)
    assert np.array_equal(m(p, t, chunk=1), whole) and np.array_equal(m(p, t, chunk=2), whole)
    monkeypatch.setattr(L, "chunk_pairs", lambda net, h, w: 1)  # the rule itself
    assert np.array_equal(m(p, t), whole)
    monkeypatch.setattr(L, "split_pair", lambda net, h, w: True)  # prediction and target in launches of their own
    assert np.array_equal(m(p, t), whole)


# ------------------------------------------------------------------ 7. CLI
def test_partition_cli_fills_lpips(gpu, tmp_path, capsys):
    import inference_partition as P
    from PIL import Image
    from rdeic_amd import metrics
    from rdeic_amd.synthetic import synth_image
    src = tmp_path / "in"
    os.makedirs(src)
    img = synth_image(128, 128, 11)
    Image.fromarray(img).save(src / "a.png")
    bb = str(tmp_path / "alexnet.pth")
    torch.save(R.seeded_backbone("alex"), bb)
    base = ["--input", str(src), "--sampler", "ddim", "--steps", "2"]
    P.main(base + ["--output", str(tmp_path / "o1"), "--lpips_backbone", bb, "--lpips_lin", R.LIN_NPZ])
    printed = capsys.readouterr().out
    with open(tmp_path / "o1" / "metrics.csv") as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 1 and np.isfinite(float(rows[0]["lpips"]))
    png = np.array(Image.open(tmp_path / "o1" / "a.png"))
    want = metrics.lpips(torch.from_numpy(png[None]).cuda(), torch.from_numpy(img[None]).cuda(), _model("alex"))[0]
    print(f"cli lpips {rows[0]['lpips']}, direct {want}")
    assert f"{float(rows[0]['lpips']):.4f}" == f"{want:.4f}" and want > 0
    assert f"LPIPS {want:.4f}" in printed
    P.main(base + ["--output", str(tmp_path / "o2")])  # without the flags nothing changes
    with open(tmp_path / "o2" / "metrics.csv") as f:
        rows2 = list(csv.DictReader(f))
    assert rows2[0]["lpips"] == "nan"
    assert np.array_equal(np.array(Image.open(tmp_path / "o2" / "a.png")), png)
    assert {k: v for k, v in rows2[0].items() if k != "lpips"} == {k: v for k, v in rows[0].items() if k != "lpips"}


# ------------------------------------------------------------------ 8. robustness harness
def test_robustness_rows_carry_lpips(gpu):
    from rdeic_amd import robustness as RB
    from rdeic_amd.rdeic import RDEIC
    from rdeic_amd.synthetic import synth_context, synth_image
    model = RDEIC().init_synthetic(rate_gain=0.4)
    img = torch.from_numpy(np.stack([synth_image(128, 128, 231)])).cuda()
    ctx = synth_context().cuda()
    kw = dict(rates=[0.0, 0.02], seeds=[1, 2], steps=2)
    plain = RB.run_bitstream_robustness(model, img, ctx, "random", **kw)
    scored = RB.run_bitstream_robustness(model, img, ctx, "random", lpips=_model("alex"), **kw)
    assert len(plain) == len(scored) == 4 and not scored[0]["decode_failed"]
    for a, b in zip(plain, scored):
        assert {k: v for k, v in a.items() if k != "lpips"} == {k: v for k, v in b.items() if k != "lpips"}
        if a["decode_failed"]:
            assert a["lpips"] == 1.0 and b["lpips"] == 1.0
        else:
            assert a["lpips"] is None  # as before
            assert isinstance(b["lpips"], float) and np.isfinite(b["lpips"]) and b["lpips"] > 0
