"""FID / KID on the device (rdeic_amd/fid.py, csrc/fid.hip) against the CPU restatement (tests/fid_ref.py) in
float64: the four kernels on their own, each Inception block and the whole tower on seeded weights, the set
statistics end to end, and the CLI wiring.

Prep, 1e-6 absolute: the source index and weight are fp32 by definition (the restatement computes them the same
way); what is left is a handful of fp32 products and adds on values in [-1, 1], under 8 * 2^-24.
Average pool, 1e-6 of the mean |x| over the window: nine adds and a divide, 10 * 2^-24. Max pool: bit-exact.
Global average pool, 1e-6 relative on non-negative input: an fp64 sum rounded to fp32 once, 2^-24.
Moments, 1e-12 * sum_k |x_ki| |x_kj| per element: fixed-order fp64 sums of exact products, rows * 2^-53.
Blocks and tower: 4x the worst error of the float32 CPU restatement (the margin is for another summation order).
Measured on MI355X: see the docstrings of test_blocks and test_tower.
Statistics and self-FID: 1e-6 of the trace sum (the eigen-decomposition routes agree to 2e-8 of it on the CPU)."""
import csv
import functools
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rdeic_amd import fid as FID
from tests import fid_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fid_tower.npz")


@functools.lru_cache(maxsize=None)
def _sd():
    return FID.seeded_inception(0)


@functools.lru_cache(maxsize=None)
def _tower():
    return FID.InceptionV3(_sd())


def _images(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)


def _strided(x, ld):
    """x [..., c] as a channel slice of a buffer with pixel stride ld (the rest is NaN)."""
    buf = torch.full(x.shape[:-1] + (ld,), float("nan"), dtype=x.dtype)
    buf[..., :x.shape[-1]] = x
    return buf.cuda()[..., :x.shape[-1]]


# ------------------------------------------------------------------ 1. prep
@pytest.mark.parametrize("src,dst", [((1, 1), (5, 5)), ((7, 5), (13, 11)), ((33, 64), (16, 9)), ((299, 299), (299, 299)),
                                     ((64, 48), (299, 299))])
def test_prep(gpu, src, dst):
    img = _images(2, src[0], src[1], 11)
    got = FID.prep(img.cuda(), dst).cpu()
    assert got.shape == (2, dst[0], dst[1], 4) and got.dtype == torch.float32
    assert (got[..., 3].contiguous().view(torch.int32) == 0).all()
    want = R.prep(img, dst, torch.float64).permute(0, 2, 3, 1)
    err = (got[..., :3].double() - want).abs().max().item()
    print(f"prep {src} -> {dst}: worst abs err {err:.3e}")
    assert err <= 1e-6
    if src == dst:  # bit-exact v / 255 * 2 - 1 (CPU fp32, true divisions)
        exact = img.float() / 255 * 2 - 1
        assert torch.equal(got[..., :3].contiguous().view(torch.int32), exact.view(torch.int32))
    if src == (7, 5):  # the clamp at 0 and at in - 1: the corners are the corner pixels themselves
        corner = img[:, [0, 0, -1, -1], [0, -1, 0, -1]].double() / 255 * 2 - 1
        assert (got[:, [0, 0, -1, -1], [0, -1, 0, -1], :3].double() - corner).abs().max() <= 1e-6


# ------------------------------------------------------------------ 2. pools
@pytest.mark.parametrize("c,ld", [(4, 4), (68, 72), (192, 192), (6, 7)])  # (6, 7): the scalar path
@pytest.mark.parametrize("h,w", [(1, 1), (2, 3), (8, 8), (17, 17), (35, 35)])
def test_pool2d(gpu, h, w, c, ld):
    from rdeic_amd import lpips as L
    g = torch.Generator().manual_seed(h * 100 + c)
    x = torch.randn((2, h, w, c), generator=g) - 1.0  # mostly negative: a zero used as padding would win a max
    xd = _strided(x, ld)
    xn = x.permute(0, 3, 1, 2)
    cases = [("max", 3, 1, 1)] + ([("max", 3, 2, 0)] if min(h, w) >= 3 else [])
    for mode, k, s, p in cases:
        out = torch.full((2, (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1, ld), 7.0, device="cuda")
        got = FID.pool2d(xd, k, s, p, mode, out=out[..., :c])
        want = F.max_pool2d(xn, k, s, p).permute(0, 2, 3, 1).contiguous()
        assert torch.equal(got.cpu().contiguous().view(torch.int32), want.view(torch.int32)), (mode, k, s, p)
        assert (out[..., c:] == 7.0).all()  # nothing written past the slice
        if p == 0:
            assert torch.equal(got.contiguous().view(torch.int32), L.max_pool(xd, k, s).contiguous().view(torch.int32))
    got = FID.pool2d(xd, 3, 1, 1, "avg").cpu().double()
    x64 = xn.double()
    want = F.avg_pool2d(x64, 3, 1, 1, count_include_pad=False).permute(0, 2, 3, 1)
    bound = 1e-6 * F.avg_pool2d(x64.abs(), 3, 1, 1, count_include_pad=False).permute(0, 2, 3, 1)
    worst = ((got - want).abs() / bound).max().item()
    print(f"avg pool {h}x{w} c {c}: worst err / bound {worst:.3f}")
    assert ((got - want).abs() <= bound).all()


def test_avg_pool_divisor_is_the_number_of_taps_inside(gpu):
    for h, w in ((8, 8), (1, 1)):
        got = FID.pool2d(torch.full((1, h, w, 4), 3.0, device="cuda"), 3, 1, 1, "avg").cpu()
        assert got.shape == (1, h, w, 4)
        # 12 / 4 at a corner, 18 / 6 on an edge, 27 / 9 inside, 3 / 1 on the 1 x 1 map: exact in fp32
        assert (got == 3.0).all(), got[0, :, :, 0]
    ramp = torch.arange(64, dtype=torch.float32).reshape(1, 8, 8, 1).expand(1, 8, 8, 4).contiguous()
    got = FID.pool2d(ramp.cuda(), 3, 1, 1, "avg").cpu()[0, :, :, 0]
    assert got[0, 0] == (0 + 1 + 8 + 9) / 4 and got[0, 3] == (2 + 3 + 4 + 10 + 11 + 12) / 6 and got[3, 3] == 27.0


@pytest.mark.parametrize("c", [4, 2048, 6])
@pytest.mark.parametrize("h,w", [(1, 1), (1, 7), (8, 8)])
def test_global_avgpool(gpu, h, w, c):
    g = torch.Generator().manual_seed(h * w + c)
    x = torch.rand((2, h, w, c), generator=g)
    got = FID.global_avgpool(x.cuda()).cpu().double()
    want = x.double().mean((1, 2))
    assert got.shape == (2, c)
    rel = ((got - want).abs() / want).max().item()
    print(f"global avg pool hw {h * w} c {c}: worst rel err {rel:.3e}")
    assert rel <= 1e-6
    assert torch.equal(FID.global_avgpool(torch.cat([x[1:], x]).cuda())[1:].cpu().double(), got)  # batch-invariant


# ------------------------------------------------------------------ 3. moments
@pytest.mark.parametrize("rows,c,ld", [(1, 4, 4), (7, 64, 64), (3, 100, 104), (130, 2048, 2048)])
def test_feat_moments(gpu, rows, c, ld):
    g = torch.Generator().manual_seed(rows + c)
    x = torch.randn((rows, c), generator=g) * 2 + 0.5
    xd = _strided(x, ld)
    x64 = x.double().numpy()
    want_sum, want_outer = R.moments(x64)
    b_sum, b_outer = 1e-12 * np.abs(x64).sum(0), 1e-12 * (np.abs(x64).T @ np.abs(x64))

    def run(parts):
        total = torch.full((c,), float("nan"), dtype=torch.float64, device="cuda")
        outer = torch.full((c, c), float("nan"), dtype=torch.float64, device="cuda")
        for i, part in enumerate(parts):
            FID.feat_moments(part, total, outer, accumulate=i > 0)
        return total, outer

    total, outer = run([xd])
    assert torch.equal(outer, outer.T)  # bitwise: the mirror is the same register
    t, o = total.cpu().numpy(), outer.cpu().numpy()
    print(f"moments {rows}x{c}: worst err / bound sum {(np.abs(t - want_sum) / b_sum).max():.3e}, "
          f"outer {(np.abs(o - want_outer) / b_outer).max():.3e}")
    assert (np.abs(t - want_sum) <= b_sum).all() and (np.abs(o - want_outer) <= b_outer).all()
    t2, o2 = run([xd])
    assert torch.equal(t2, total) and torch.equal(o2, outer)  # a repeat run: the same bits
    if rows >= 2:  # two accumulating calls on halves
        th, oh = run([xd[:rows // 2], xd[rows // 2:]])
        assert torch.equal(oh, oh.T)
        assert (np.abs(th.cpu().numpy() - want_sum) <= b_sum).all()
        assert (np.abs(oh.cpu().numpy() - want_outer) <= b_outer).all()
    else:  # one row onto what is already there
        th, oh = run([xd, xd])
        assert (np.abs(th.cpu().numpy() - 2 * want_sum) <= 2 * b_sum).all()
        assert (np.abs(oh.cpu().numpy() - 2 * want_outer) <= 2 * b_outer).all()


def test_feature_stats_mean_cov_merge(gpu):
    g = torch.Generator().manual_seed(4)
    x = torch.randn((23, 64), generator=g) + 3.0
    a, b, whole = FID.FeatureStats(64), FID.FeatureStats(64), FID.FeatureStats(64)
    a.update(x[:10].cuda()), a.update(x[10:15].cuda()), b.update(x[15:].cuda()), whole.update(x.cuda())
    a.merge(b)
    assert a.n == whole.n == 23
    mu, cov = R.mean_cov(x.double().numpy())
    for s in (a, whole):
        assert np.abs(s.mean() - mu).max() <= 1e-12 and np.abs(s.cov() - cov).max() <= 1e-10  # |x|^2 ~ 10: n eps
    with pytest.raises(ValueError):
        FID.FeatureStats(64).cov()


# ------------------------------------------------------------------ 4. blocks
@pytest.mark.parametrize("name,cin,size,out", [
    ("Mixed_5b", 192, 5, (5, 256)), ("Mixed_6a", 288, 5, (2, 768)), ("Mixed_6b", 768, 7, (7, 768)),
    ("Mixed_7a", 768, 5, (2, 1280)), ("Mixed_7b", 1280, 3, (3, 2048)), ("Mixed_7c", 2048, 3, (3, 2048))])
def test_blocks(gpu, name, cin, size, out):
    """Measured on MI355X, device error / float32 CPU yardstick (x4 is the bound), both over the block's largest
    output: Mixed_5b 5.84e-7 / 4.39e-7 (1.33x), Mixed_6a 5.15e-7 / 3.28e-7 (1.57x), Mixed_6b 7.66e-7 / 3.76e-7
    (2.04x), Mixed_7a 5.30e-7 / 3.34e-7 (1.59x), Mixed_7b 5.10e-7 / 3.79e-7 (1.35x), Mixed_7c 6.68e-7 / 4.52e-7
    (1.48x).
    With every conv as one k chain (no split-K) Mixed_6a sat at 1.448e-6 (4.41x) and Mixed_7c at 1.893e-6 (4.19x),
    past the bound: a chain of 2592 to 4032 signed products rounds several times worse than the CPU's blocked sum
    (restated on the CPU for Mixed_6a.branch3x3 alone: 1.39e-6 against 2.2e-7). fid.conv_splits cuts the chains of
    the layers past 1024 products to 512 at most."""
    from rdeic_amd import ops
    g = torch.Generator().manual_seed(cin + size)
    x = torch.randn((2, cin, size, size), generator=g)
    with torch.no_grad():
        want = R.block(name, x.double(), _sd())
        yard = (R.block(name, x, _sd()).double() - want).abs().max().item()
    with ops.splitk_as((False, False)):
        got = _tower().block(name, x.permute(0, 2, 3, 1).contiguous().cuda())
    assert got.shape == (2, out[0], out[0], out[1]) and got.is_contiguous()
    err = (got.cpu().double().permute(0, 3, 1, 2) - want).abs().max().item()
    top = want.abs().max().item()
    print(f"{name} at {size}x{size}: device err {err / top:.3e}, float32 CPU yardstick {yard / top:.3e} "
          f"(of the largest output {top:.3f})")
    assert err / top <= 4 * yard / top


# ------------------------------------------------------------------ 5. tower
def test_tower(gpu):
    """Measured on MI355X: worst absolute feature error 1.12e-6 against the golden's float32 yardstick of 9.80e-7
    (bound 3.92e-6), largest feature 3.21 (1.62e-6 before the long k chains were split)."""
    z = np.load(GOLDEN)
    img = torch.from_numpy(z["images"]).cuda()
    yard, top = float(z["f32_max_abs_err"]), float(z["max_abs_feature"])
    t = _tower()
    got = t.features(img)
    assert got.shape == (2, 2048) and got.dtype == torch.float32
    err = np.abs(got.cpu().double().numpy() - z["features"]).max()
    print(f"tower: device worst abs err {err:.3e}, float32 CPU yardstick {yard:.3e}, largest |feature| {top:.3f}")
    assert err <= 4 * yard
    alone = t.features(img[:1])
    three = t.features(torch.cat([img[1:], img[:1], img[1:]]))
    assert torch.equal(alone[0], got[0]) and torch.equal(three[1], got[0]) and torch.equal(three[0], got[1])
    assert torch.equal(t.features(img, chunk=1), got)  # the chunked path


# ------------------------------------------------------------------ 6. end to end
def test_statistics_and_self_fid(gpu):
    from rdeic_amd import metrics
    t = _tower()
    img = _images(6, 64, 64, 21).cuda()
    f = t.features(img)
    a, b = FID.FeatureStats(), FID.FeatureStats()
    a.update(f[:3]), b.update(f[3:])
    fa, fb = f[:3].cpu().double().numpy(), f[3:].cpu().double().numpy()
    got, want, tr = FID.fid(a, b), R.fid(fa, fb), R.trace_sum(fa, fb)
    print(f"fid {got:.9g}, restatement on the same features {want:.9g}, |diff| / trace sum {abs(got - want) / tr:.2e}")
    assert want > 0 and abs(got - want) <= 1e-6 * tr
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # 6 samples: the KID subset size is clamped
        r = metrics.fid_kid([img[:4], img[4:]], [img[:4], img[4:]], t, patch=0, kid_subsets=3)
    fall = f.cpu().double().numpy()
    print(f"self fid {r['fid']:.3e} of trace sum {R.trace_sum(fall, fall):.6g}; kid {r['kid_mean']:.3e}")
    assert r["n_images"] == r["n_patches"] == 6 and abs(r["fid"]) <= 1e-6 * R.trace_sum(fall, fall)
    assert np.isfinite(r["kid_mean"]) and np.isfinite(r["kid_std"])


# ------------------------------------------------------------------ 7. CLIs
@pytest.fixture(scope="module")
def inception_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("fid") / "inception.pth")
    torch.save(_sd(), path)
    return path


@pytest.fixture()
def one_model(monkeypatch):
    """The runs of one test share one synthetic codec (the load dominates a tiny run)."""
    import inference
    import inference_partition as P
    cached = functools.lru_cache(maxsize=None)(inference.load_model)
    monkeypatch.setattr(inference, "load_model", cached)
    monkeypatch.setattr(P, "load_model", cached)


def _fid_rows(path):
    with open(path) as f:
        r = csv.reader(f)
        header = next(r)
        return header, [dict(zip(header, row)) for row in r]


def test_partition_cli_writes_fid_kid(gpu, tmp_path, capsys, inception_file, one_model):
    import inference_partition as P
    from PIL import Image
    from rdeic_amd.synthetic import synth_image
    src = tmp_path / "in"
    os.makedirs(src)
    Image.fromarray(synth_image(128, 128, 11)).save(src / "a.png")
    base = ["--input", str(src), "--sampler", "ddim", "--steps", "2"]
    P.main(base + ["--output", str(tmp_path / "o1"), "--fid_inception", inception_file, "--fid_patch", "64"])
    printed = capsys.readouterr().out
    header, rows = _fid_rows(tmp_path / "o1" / "fid_kid.csv")
    assert header == FID.CSV_COLUMNS and len(rows) == 1
    assert rows[0]["set"] == "all" and rows[0]["n_images"] == "1" and rows[0]["n_patches"] == "5"  # 2 x 2 + 1 shifted
    vals = [float(rows[0][k]) for k in ("fid", "kid_mean", "kid_std")]
    assert all(np.isfinite(v) for v in vals) and vals[0] > 0
    assert FID.summary_line({k: float(v) if k != "set" and "n_" not in k else v for k, v in rows[0].items()}) in printed
    P.main(base + ["--output", str(tmp_path / "o2")])  # without the flag nothing changes
    assert not os.path.exists(tmp_path / "o2" / "fid_kid.csv")
    assert (tmp_path / "o2" / "metrics.csv").read_bytes() == (tmp_path / "o1" / "metrics.csv").read_bytes()
    assert "FID" not in capsys.readouterr().out


def test_run_ood_writes_fid_kid(gpu, tmp_path, inception_file, one_model):
    import run_ood
    from PIL import Image
    from rdeic_amd.synthetic import synth_image
    dirs = []
    for d, name in enumerate(("sketch", "xray")):
        os.makedirs(tmp_path / "in" / name)
        Image.fromarray(synth_image(128, 128, 40 + d)).save(tmp_path / "in" / name / "im0.png")
        dirs.append(str(tmp_path / "in" / name))
    base = ["--domains", ",".join(dirs), "--sampler", "ddim", "--steps", "2"]
    run_ood.main(base + ["--output_dir", str(tmp_path / "o1"), "--cache_dir", str(tmp_path / "c1"),
                         "--fid_inception", inception_file, "--fid_patch", "64"])
    header, rows = _fid_rows(tmp_path / "o1" / "fid_kid.csv")
    assert header == FID.CSV_COLUMNS and [r["set"] for r in rows] == ["sketch", "xray", "all"]
    assert [(r["n_images"], r["n_patches"]) for r in rows] == [("1", "5"), ("1", "5"), ("2", "10")]
    assert all(np.isfinite(float(r[k])) for r in rows for k in ("fid", "kid_mean", "kid_std"))
    run_ood.main(base + ["--output_dir", str(tmp_path / "o2"), "--cache_dir", str(tmp_path / "c2")])
    assert not os.path.exists(tmp_path / "o2" / "fid_kid.csv")
    for name in ("ood_results_all.csv", "ood_results_sketch.csv", "ood_results_xray.csv"):
        assert (tmp_path / "o2" / name).read_bytes() == (tmp_path / "o1" / name).read_bytes()
