"""DISTS on the device (rdeic_amd/dists.py, csrc/dists.hip) against the CPU restatement (tests/dists_ref.py) in
float64: the kernels on their own, the metric end to end with a seeded backbone and seeded weights, its exact
properties, and the CLI / out-of-domain / robustness wiring.

L2 pool, 1e-6 relative: nine non-negative fp32 products (the weights are powers of two), 9 * 2^-24 = 5.4e-7,
halved by the square root.
Moments: means 1e-6 relative, second moments 1e-5 of max(vx, vy). A thread's fp32 run is 8 terms
(8 * 2^-24 = 4.8e-7 at worst); every other sum is fp64, and the second moments are taken about the mean.
End to end, 1e-5 absolute: ten times below the last digit the CLIs print; the float32 CPU restatement sits at
1.5e-7 on these sizes and pairs."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from rdeic_amd import dists as D
from tests import dists_ref as R

pytestmark = pytest.mark.gpu

SIZES = [(16, 16), (32, 48), (37, 51), (64, 64)]
KINDS = ("noisy copy", "unrelated", "flat grey target", "black / black")


@lru_cache(maxsize=None)
def _model():
    return D.DISTS(R.seeded_weights(), backbone=R.seeded_backbone())


@lru_cache(maxsize=None)
def _want(h, w):
    pred, tgt = R.pairs(h, w)
    return R.dists(R.seeded_backbone(), R.seeded_weights(), pred, tgt)


def _dev(h, w):
    pred, tgt = R.pairs(h, w)
    return torch.from_numpy(pred).cuda(), torch.from_numpy(tgt).cuda()


# ------------------------------------------------------------------ 1. prep
def test_prep_is_bit_exact(gpu):
    g = torch.Generator().manual_seed(7)
    img = torch.randint(0, 256, (2, 35, 47, 3), generator=g, dtype=torch.uint8)
    img[1].view(-1)[:256] = torch.arange(256, dtype=torch.uint8)  # every level somewhere
    x = img.to(torch.float32) / 255  # CPU fp32, true divisions
    want = (x - torch.tensor(R.MEAN)) / torch.tensor(R.STD)
    raw, norm = D.prep(img.cuda())
    for got, ref in ((raw.cpu(), x), (norm.cpu(), want)):
        assert got.shape == (2, 35, 47, 4) and got.dtype == torch.float32
        assert torch.equal(got[..., :3].contiguous().view(torch.int32), ref.contiguous().view(torch.int32))
        assert (got[..., 3].view(torch.int32) == 0).all()


# ------------------------------------------------------------------ 2. L2 pool
@pytest.mark.parametrize("shape,ld_in,ld_out", [
    ((2, 37, 51, 64), 64, 64),     # odd sizes: the far-side padding is read
    ((1, 36, 50, 128), 128, 128),  # even sizes: it is not
    ((1, 16, 16, 512), 512, 512), ((1, 1, 1, 128), 128, 128),
    ((1, 2, 3, 4), 6, 5),          # ld > c, no 16-byte alignment: the scalar path
    ((1, 2, 3, 4), 8, 12),         # ld > c on the float4 path
    ((2, 5, 4, 3), 3, 3)])
def test_l2_pool_matches_restatement(gpu, shape, ld_in, ld_out):
    n, h, w, c = shape
    g = torch.Generator().manual_seed(h * 100 + w + c)
    x = torch.randn((n, h, w, ld_in), generator=g)
    want = R.l2_pool(x[..., :c].double().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    ho, wo = (h + 1) // 2, (w + 1) // 2
    assert want.shape == (n, ho, wo, c)
    buf = torch.full((n, ho, wo, ld_out), -7.0, device="cuda")
    got = D.l2_pool(x.cuda()[..., :c], out=buf[..., :c]).cpu().double()
    rel = ((got - want).abs() / want).max().item()
    print(f"l2 pool {shape} ld {ld_in}->{ld_out}: rel {rel:.3e}")
    assert rel <= 1e-6
    assert (buf[..., c:] == -7.0).all()  # nothing written past the channels
    const = torch.full((1, h, w, c), 3.0, device="cuda")  # the known answers: 16/16, 12/16, 9/16, 4/16 of a^2 in bounds
    y = D.l2_pool(const).cpu().double()
    fy = torch.tensor([(1 if 2 * i - 1 < 0 else 0) + (1 if 2 * i + 1 >= h else 0) for i in range(ho)])
    fx = torch.tensor([(1 if 2 * j - 1 < 0 else 0) + (1 if 2 * j + 1 >= w else 0) for j in range(wo)])
    frac = (torch.tensor([1.0, 0.75, 0.5])[fy][:, None] * torch.tensor([1.0, 0.75, 0.5])[fx][None, :]).double()
    assert ((y - torch.sqrt(frac * 9.0 + 1e-12)[None, :, :, None]).abs() <= 1e-6 * 3.0).all()


# ------------------------------------------------------------------ 3. moments
@lru_cache(maxsize=None)
def _maps(c, hw, offset):
    g = torch.Generator().manual_seed(c * 10000 + hw + offset)
    if offset:  # a variance of 1e-4 under a mean of 100
        x = 100 + 0.01 * torch.randn((3, hw, 1, c), generator=g)
        y = 100 + 0.01 * torch.randn((3, hw, 1, c), generator=g)
    else:
        x = torch.relu(torch.randn((3, hw, 1, c), generator=g) + 0.5)
        y = torch.relu(x + 0.3 * torch.randn((3, hw, 1, c), generator=g))  # taps are non-negative: no mean near 0
    xd, yd = x.numpy().astype(np.float64)[:, :, 0], y.numpy().astype(np.float64)[:, :, 0]
    mx, my = xd.mean(1), yd.mean(1)
    want = np.stack([mx, my, ((xd - mx[:, None]) ** 2).mean(1), ((yd - my[:, None]) ** 2).mean(1),
                     ((xd - mx[:, None]) * (yd - my[:, None])).mean(1)], axis=1)  # [3, 5, c]
    return x, y, want


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("hw", [1, 7, 2601])
@pytest.mark.parametrize("c", [4, 64, 512])
def test_moments(gpu, c, hw, offset):
    x, y, want = _maps(c, hw, offset)
    a, b = x.cuda(), y.cuda()
    got_d = D.moments(a, b)
    got = got_d.cpu().numpy()
    assert got.shape == (3, 5, c) and got.dtype == np.float64 and np.isfinite(got).all()
    mean_rel = (np.abs(got[:, :2] - want[:, :2]) / np.abs(want[:, :2]).clip(1e-30)).max()
    scale = np.maximum(want[:, 2], want[:, 3])[:, None]
    second = np.abs(got[:, 2:] - want[:, 2:])
    print(f"c={c} hw={hw} offset={offset}: mean rel {mean_rel:.3e}, second / max(vx, vy) "
          f"{(second / scale.clip(1e-30)).max():.3e}")
    assert (np.abs(got[:, :2] - want[:, :2]) <= 1e-6 * np.abs(want[:, :2])).all()
    assert (second <= 1e-5 * scale).all()
    if hw == 1:
        assert (got[:, 2:] == 0).all()
    assert torch.equal(D.moments(a, b), got_d)  # repeatable bit for bit
    for i in range(3):  # an image alone gets what it gets in the batch
        assert torch.equal(D.moments(a[i:i + 1], b[i:i + 1]), got_d[i:i + 1]), i
    same = D.moments(a, a)  # two identical maps: vx == vy == cxy bitwise
    assert torch.equal(same[:, 2], same[:, 3]) and torch.equal(same[:, 2], same[:, 4])
    assert torch.equal(same[:, 0], same[:, 1]) and torch.equal(same[:, 2], got_d[:, 2])
    swapped = D.moments(b, a)
    assert torch.equal(swapped[:, [1, 0, 3, 2, 4]], got_d)


@pytest.mark.parametrize("c,ld", [(64, 68), (64, 65), (4, 6), (3, 3)])
def test_moments_pixel_stride(gpu, c, ld):
    """A channel slice of a wider buffer (ld > c), aligned for the wide loads or not, gives the same bits."""
    g = torch.Generator().manual_seed(c + ld)
    x, y = torch.randn((2, 9, 11, c), generator=g).cuda(), torch.randn((2, 9, 11, c), generator=g).cuda()
    wx = torch.full((2, 9, 11, ld), float("nan"), device="cuda")
    wy = torch.full((2, 9, 11, ld), float("nan"), device="cuda")
    wx[..., :c], wy[..., :c] = x, y
    got = D.moments(wx[..., :c], wy[..., :c])
    assert torch.equal(got, D.moments(x, y)) and torch.isfinite(got).all()
    xd = x.cpu().double().reshape(2, 99, c)
    assert torch.allclose(got[:, 0].cpu(), xd.mean(1), rtol=1e-6, atol=1e-7)
    assert torch.allclose(got[:, 2].cpu(), xd.var(1, unbiased=False), rtol=1e-5, atol=0)


# ------------------------------------------------------------------ 4. end to end
@pytest.mark.parametrize("h,w", SIZES)
def test_dists_matches_restatement(gpu, h, w):
    from rdeic_amd import metrics
    m = _model()
    want = _want(h, w)
    p, t = _dev(h, w)
    got = metrics.dists(p, t, m)
    err = np.abs(got - want)
    for k, kind in enumerate(KINDS):
        print(f"dists {h}x{w} {kind}: got {got[k]:.9f}, fp64 {want[k]:.9f}, abs err {err[k]:.3e}")
    assert got.dtype == np.float64 and got.shape == (4,) and np.isfinite(got).all()
    assert want[0] < want[1] and want[2] > 0 and abs(want[3]) < 1e-12
    assert err.max() <= 1e-5


# ------------------------------------------------------------------ 5. exact properties
@pytest.mark.parametrize("h,w", [(37, 51), (16, 16)])
def test_exact_properties(gpu, h, w):
    m = _model()
    p, t = _dev(h, w)
    got = m(p, t)
    assert np.abs(m(t, t)).max() <= 1e-12 and np.abs(m(p, p)).max() <= 1e-12  # identical pairs
    assert abs(got[3]) <= 1e-12  # black against black
    assert np.array_equal(m(t, p), got)  # swapping the arguments changes no bit
    assert np.array_equal(m(p, t), got)
    for i in range(4):  # alone, inside a batch of 3, and chunked
        assert m(p[i:i + 1], t[i:i + 1])[0] == got[i], i
        j = [(i + 1) % 4, i, (i + 2) % 4]
        assert m(p[j], t[j])[1] == got[i], i
    assert np.array_equal(m(p, t, chunk=1), got) and np.array_equal(m(p, t, chunk=3), got)


def test_split_pair_and_input_checks(gpu, monkeypatch):
    m = _model()
    p, t = _dev(32, 48)
    got = m(p, t)
    monkeypatch.setattr(D, "chunk_pairs", lambda h, w: 1)
    assert np.array_equal(m(p, t), got)
    monkeypatch.setattr(D, "split_pair", lambda h, w: True)  # prediction and target in launches of their own
    assert np.array_equal(m(p, t), got)
    monkeypatch.undo()
    one = torch.full((1, 1, 1, 3), 9, dtype=torch.uint8, device="cuda")  # the minimum size
    assert abs(m(one, one)[0]) <= 1e-12 and np.isfinite(m(one, one + 100)).all()
    with pytest.raises(ValueError):
        m(p, t.float())
    with pytest.raises(ValueError):
        m(p, t[:, :, :40])
    with pytest.raises(ValueError):
        m(p[:, :0], t[:, :0])


# ------------------------------------------------------------------ 6. wiring
def test_cli_and_ood_scoring_carry_dists(gpu):
    import inference_partition as P
    from rdeic_amd import ood
    m = _model()
    pred, tgt = R.pairs(64, 64)
    want = m(torch.from_numpy(pred[:1]).cuda(), torch.from_numpy(tgt[:1]).cuda())[0]
    vals = P.compute_metrics(pred[0], tgt[0], None, m)
    assert vals["dists"] == want and want > 0
    plain = P.compute_metrics(pred[0], tgt[0], None)
    assert "dists" not in plain and {k: v for k, v in vals.items() if k != "dists"}.keys() == plain.keys()
    assert plain["psnr"] == vals["psnr"] and np.isnan(plain["lpips"])
    p1, t1 = torch.from_numpy(pred[:1]).cuda(), torch.from_numpy(tgt[:1]).cuda()
    scored = ood.score_image(p1, t1, dists=m)
    assert scored["dists"] == want
    unscored = ood.score_image(p1, t1)
    assert "dists" not in unscored and list(unscored) == [k for k in scored if k != "dists"]


def test_robustness_rows_carry_dists(gpu):
    from rdeic_amd import robustness as RB
    from rdeic_amd.rdeic import RDEIC
    from rdeic_amd.synthetic import synth_context, synth_image
    model = RDEIC().init_synthetic(rate_gain=0.4)
    img = torch.from_numpy(np.stack([synth_image(128, 128, 231)])).cuda()
    ctx = synth_context().cuda()
    kw = dict(rates=[0.0, 0.02], seeds=[1, 2], steps=2)
    plain = RB.run_bitstream_robustness(model, img, ctx, "random", **kw)
    scored = RB.run_bitstream_robustness(model, img, ctx, "random", dists=_model(), **kw)
    assert len(plain) == len(scored) == 4 and not scored[0]["decode_failed"]
    for a, b in zip(plain, scored):
        assert "dists" not in a and {k: v for k, v in b.items() if k != "dists"} == a
        if b["decode_failed"]:
            assert b["dists"] == 1.0
        else:
            assert isinstance(b["dists"], float) and np.isfinite(b["dists"]) and b["dists"] > 0
