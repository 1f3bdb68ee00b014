"""Host side of FID / KID (rdeic_amd/fid.py): the layer table, the BatchNorm fold, the loader, the patch protocol,
the two scores against the restatement (tests/fid_ref.py) and the CLI flags. No GPU."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rdeic_amd import fid as FID
from tests import fid_ref as R


# ------------------------------------------------------------------ the layer table
def test_layer_table_shapes_for_299():
    shapes = FID.layer_shapes(299)
    sizes = [h for _, h, w, _ in shapes if h == w]
    assert len(sizes) == len(shapes)  # square all the way
    dedup = [s for i, s in enumerate(sizes) if i == 0 or s != sizes[i - 1]]
    assert [299] + dedup == [299, 149, 147, 73, 71, 35, 17, 8, 1]
    assert [s for s in sizes[:7]] == [149, 147, 147, 73, 73, 71, 35]  # 299 -> 149 -> 147 -> 147 -> 73 -> 73 -> 71 -> 35
    assert shapes[-1] == ("avgpool", 1, 1, 2048)
    widths = [c for name, _, _, c in shapes if name.startswith("Mixed")]
    assert widths == [256, 288, 288, 768, 768, 768, 768, 768, 1280, 2048, 2048]
    convs = FID.conv_layers()
    assert len(convs) == 94 and convs[0][:4] == ("Conv2d_1a_3x3", 3, 32, (3, 3))
    assert len({c[0] for c in convs}) == 94
    by = {c[0]: c for c in convs}
    assert by["Mixed_5b.branch_pool"][1:3] == (192, 32) and by["Mixed_5c.branch_pool"][1:3] == (256, 64)
    assert by["Mixed_6b.branch7x7_2"][1:] == (128, 128, (1, 7), 1, (0, 3))
    assert by["Mixed_6c.branch7x7dbl_2"][1:] == (160, 160, (7, 1), 1, (3, 0))
    assert by["Mixed_6e.branch7x7_1"][1:3] == (768, 192)
    assert by["Mixed_7a.branch3x3_2"][1:] == (192, 320, (3, 3), 2, (0, 0))
    assert by["Mixed_7c.branch3x3dbl_3b"][1:] == (384, 384, (3, 1), 1, (1, 0)) and by["Mixed_7c.branch1x1"][1] == 2048
    # the pool branches: average in A, C and Mixed_7b, max in Mixed_7c (and the plain max pools of B, D)
    pools = {name: [op[1] for b in spec for op in b if op[0] == "pool"] for name, spec in FID.TABLE
             if isinstance(spec, list)}
    assert all(pools[n] == ["avg"] for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6b", "Mixed_6e", "Mixed_7b"))
    assert pools["Mixed_6a"] == pools["Mixed_7a"] == pools["Mixed_7c"] == ["max"]
    # the chunk is a function of the constant 299 alone: every activation of a chunk stays under 2^31 bytes
    assert FID.image_bytes() == 4 * 147 * 147 * 64
    assert FID.CHUNK * FID.image_bytes() < 2 ** 31 <= (FID.CHUNK + 1) * FID.image_bytes()


def test_split_counts_depend_on_the_layer_alone():
    """The k chains of the deep layers are cut by a rule in K = kh * kw * cin only, so no launch shape enters it."""
    assert [FID.conv_splits(k) for k in (1, 36, 864, 1024, 1025, 1200, 2048, 2592, 4032)] == [1, 1, 1, 1, 3, 3, 4, 6, 8]
    ks = [cin * kh * kw for _, cin, _, (kh, kw), _, _ in FID.conv_layers()]
    assert max(ks) == 4032 and sum(FID.conv_splits(k) > 1 for k in ks) == 44
    for k in ks:
        n = FID.conv_splits(k)
        assert k <= FID.SPLIT_MIN_K if n == 1 else -(-k // n) <= FID.SPLIT_CHAIN
    # what rdeic_conv2d_splitk asks of a layer it takes: every split layer has cout % 8 == 0
    assert all(cout % 8 == 0 for _, cin, cout, (kh, kw), _, _ in FID.conv_layers() if FID.conv_splits(cin * kh * kw) > 1)


def test_seeded_state_dict_is_deterministic_and_complete():
    a, b = FID.seeded_inception(3), FID.seeded_inception(3)
    assert len(a) == 94 * 5 and all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["Mixed_7c.branch_pool.conv.weight"], FID.seeded_inception(4)["Mixed_7c.branch_pool.conv.weight"])
    assert a["Mixed_6b.branch7x7_2.conv.weight"].shape == (128, 128, 1, 7)
    assert (a["Conv2d_1a_3x3.bn.running_var"] > 0.9).all()


# ------------------------------------------------------------------ the BatchNorm fold and the loader
def test_bn_fold_matches_the_unfolded_block():
    g = torch.Generator().manual_seed(0)
    w = torch.randn((6, 4, 1, 7), generator=g)
    gamma, beta = 1 + 0.3 * torch.randn(6, generator=g), 0.2 * torch.randn(6, generator=g)
    mean, var = 0.5 * torch.randn(6, generator=g), 0.5 + torch.rand(6, generator=g)
    x = torch.randn((2, 4, 5, 9), generator=g, dtype=torch.float64)
    sd = {"c.conv.weight": w, "c.bn.weight": gamma, "c.bn.bias": beta, "c.bn.running_mean": mean, "c.bn.running_var": var}
    want = R.conv_bn_relu(x, sd, "c", padding=(0, 3))
    wf, bf = FID.fold_bn(w, gamma, beta, mean, var)
    assert wf.dtype == bf.dtype == torch.float64
    got = F.relu(F.conv2d(x, wf, bf, 1, (0, 3)))
    assert (got - want).abs().max() < 1e-13 * max(1.0, want.abs().max())
    assert (want > 0).any() and (want == 0).any()


def test_loader_folds_and_names_what_is_wrong(tmp_path):
    sd = FID.seeded_inception(1)
    sd["fc.weight"], sd["AuxLogits.conv0.conv.weight"] = torch.zeros(3), torch.zeros(3)  # ignored
    folded = FID.load_inception(sd)
    assert len(folded) == 94 and list(folded)[0] == "Conv2d_1a_3x3"
    w, b = folded["Mixed_6a.branch3x3"]
    assert w.dtype == b.dtype == torch.float32 and w.shape == (384, 288, 3, 3) and b.shape == (384,)
    wf, bf = FID.fold_bn(*[sd[f"Mixed_6a.branch3x3.{k}"] for k in
                           ("conv.weight", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var")])
    assert torch.equal(w, wf.float()) and torch.equal(b, bf.float())
    small = {k: v for k, v in sd.items() if k.startswith("Conv2d_1a")}
    torch.save(small, tmp_path / "part.pth")
    np.savez(tmp_path / "part.npz", **{k: v.numpy() for k, v in small.items()})
    for src in (str(tmp_path / "part.pth"), str(tmp_path / "part.npz")):  # both file kinds reach the same check
        with pytest.raises(ValueError, match=r"no 'Conv2d_2a_3x3\.conv\.weight'"):
            FID.load_inception(src)
    missing = dict(sd)
    del missing["Mixed_7b.branch3x3_2a.bn.running_var"]
    with pytest.raises(ValueError, match=r"no 'Mixed_7b\.branch3x3_2a\.bn\.running_var'"):
        FID.load_inception(missing)
    bad = dict(sd)
    bad["Mixed_6b.branch7x7_2.conv.weight"] = torch.zeros(128, 128, 7, 1)  # torchvision's default graph order
    with pytest.raises(ValueError, match=r"'Mixed_6b\.branch7x7_2\.conv\.weight' has shape \(128, 128, 7, 1\), "
                                         r"expected \(128, 128, 1, 7\)"):
        FID.load_inception(bad)
    with pytest.raises(FileNotFoundError):
        FID.load_inception(str(tmp_path / "missing.pth"))
    with pytest.raises(ValueError, match="no weights ship"):
        FID.InceptionV3(None)


# ------------------------------------------------------------------ patches
def test_patch_grid_counts():
    g = torch.Generator().manual_seed(2)
    img = torch.randint(0, 256, (1, 512, 768, 3), generator=g, dtype=torch.uint8)
    p = FID.patches(img, 256)
    assert p.shape == (8, 256, 256, 3)  # 2 x 3 from the top-left, 1 x 2 shifted by 128
    assert torch.equal(p[0], img[0, :256, :256]) and torch.equal(p[5], img[0, 256:512, 512:768])
    assert torch.equal(p[6], img[0, 128:384, 128:384]) and torch.equal(p[7], img[0, 128:384, 384:640])
    assert FID.patches(img[0, :256, :256], 256).shape == (1, 256, 256, 3)  # [h, w, 3] too; no shifted tile fits
    assert FID.patches(img[:, :255, :300], 256).shape == (0, 256, 256, 3)
    two = torch.cat([img, img.flip(1)])
    assert FID.patches(two, 0) is two
    p2 = FID.patches(two, 256)  # image-major
    assert p2.shape == (16, 256, 256, 3) and torch.equal(p2[:8], p) and torch.equal(p2[8], two[1, :256, :256])
    with pytest.raises(ValueError):
        FID.patches(img, 255)


# ------------------------------------------------------------------ FID
def _sets(d, na, nb, seed):
    rs = np.random.RandomState(seed)
    a = rs.randn(na, d) * (0.2 + rs.rand(d)) + rs.randn(d)
    b = (rs.randn(nb, d) @ (np.eye(d) + 0.1 * rs.randn(d, d))) * (0.2 + rs.rand(d)) + 0.3 * rs.randn(d)
    return a, b


@pytest.mark.parametrize("d,na,nb", [(64, 200, 300), (64, 16, 24), (64, 2, 2), (256, 40, 50)])
def test_fid_against_the_second_route(d, na, nb):
    a, b = _sets(d, na, nb, d + na)
    (m1, s1), (m2, s2) = R.mean_cov(a), R.mean_cov(b)
    tol = 1e-6 * R.trace_sum(a, b)
    got, want = FID.fid_from_moments(m1, s1, m2, s2), R.fid(a, b)
    print(f"d {d}, {na}/{nb}: fid {got:.9g}, second route {want:.9g}, |diff| / trace sum "
          f"{abs(got - want) / R.trace_sum(a, b):.2e}")
    assert want > 0 and abs(got - want) <= tol
    for m, s in ((m1, s1), (m2, s2)):
        self_fid = FID.fid_from_moments(m, s, m, s)
        print(f"   self-FID / trace sum {self_fid / (2 * np.trace(s)):.2e}")
        assert abs(self_fid) <= 1e-6 * 2 * np.trace(s)


def test_fid_from_host_sums_and_too_few_samples():
    """The statistics' host half without the device: (outer - n mu mu^T) / (n - 1) is np.cov."""
    a, _ = _sets(16, 9, 9, 5)
    total, outer = R.moments(a)
    mu = total / 9
    assert np.allclose((outer - 9 * np.outer(mu, mu)) / 8, np.cov(a, rowvar=False), rtol=0, atol=1e-12)

    class Stub:
        def __init__(self, n):
            self.n = n
    with pytest.raises(ValueError, match="at least 2 samples"):
        FID.fid(Stub(1), Stub(5))
    with pytest.raises(ValueError, match="at least 2 samples"):
        FID.fid(Stub(5), Stub(1))


# ------------------------------------------------------------------ KID
def test_kid_against_the_brute_force():
    rs = np.random.RandomState(9)
    a, b = rs.randn(13, 24), rs.randn(11, 24) * 1.2 + 0.2
    got, want = FID.kid(a, b, subsets=4, subset_size=6, seed=3), R.kid(a, b, 4, 6, 3)
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-12 * abs(w)
    assert got[1] > 0
    assert FID.kid(a, b, subsets=4, subset_size=6, seed=3) == got  # deterministic in the seed
    assert FID.kid(a, b, subsets=4, subset_size=6, seed=4) != got
    assert FID.kid([torch.from_numpy(a[:5]).float(), torch.from_numpy(a[5:]).float()], torch.from_numpy(b).float(),
                   subsets=2, subset_size=6, seed=3) == FID.kid(a.astype(np.float32), b.astype(np.float32), 2, 6, 3)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        clamped = FID.kid(a, b, subsets=3, subset_size=1000, seed=0)
    assert len(caught) == 1 and "clamped" in str(caught[0].message) and "11" in str(caught[0].message)
    want = R.kid(a, b, 3, 11, 0)
    assert abs(clamped[0] - want[0]) <= 1e-12 * abs(want[0]) and abs(clamped[1] - want[1]) <= 1e-12 * abs(want[1])
    # a set against itself, one subset: the unbiased estimate drops the diagonal of k(x, x) and k(y, y) only, so it
    # is below zero, not zero
    same = FID.kid(a, a, subsets=1, subset_size=13, seed=0)
    assert same[0] < 0 and same[1] == 0.0 and abs(same[0] - R.kid(a, a, 1, 13, 0)[0]) <= 1e-12 * abs(same[0])
    with pytest.raises(ValueError):
        FID.kid(a[:1], b)


# ------------------------------------------------------------------ CLI flags
def test_cli_flags(tmp_path):
    import inference_partition as P
    import run_ood as O
    path = str(tmp_path / "inception.npz")
    np.savez(path, x=np.zeros(1))
    missing = str(tmp_path / "missing.pth")
    for mod, base in ((P, ["--input", "x"]), (O, ["--domains", "x"])):
        a = mod.parse_args(base)
        assert a.fid_inception == ""
        a = mod.parse_args(base + ["--fid_inception", path])
        assert (a.fid_inception, a.fid_patch, a.kid_subset_size) == (path, 256, 1000)
        a = mod.parse_args(base + ["--fid_inception", path, "--fid_patch", "64", "--kid_subset_size", "50"])
        assert (a.fid_patch, a.kid_subset_size) == (64, 50)
        assert mod.parse_args(base + ["--fid_inception", path, "--fid_patch", "0"]).fid_patch == 0
        for extra in (["--fid_patch", "256"], ["--kid_subset_size", "10"], ["--fid_inception", missing],
                      ["--fid_inception", path, "--fid_patch", "63"], ["--fid_inception", path, "--fid_patch", "-2"],
                      ["--fid_inception", path, "--kid_subset_size", "1"]):
            with pytest.raises(SystemExit):  # at parse time: no model has been loaded
                mod.parse_args(base + extra)
    assert FID.CSV_COLUMNS == ["set", "n_images", "n_patches", "fid", "kid_mean", "kid_std"]
    assert P.metrics_fieldnames() == ["image", "bpp", "scale", "psnr", "ssim", "ms_ssim", "lpips"]  # unchanged
    row = {"set": "all", "n_images": 2, "n_patches": 10, "fid": 1.25, "kid_mean": 0.5, "kid_std": 0.125}
    assert FID.summary_line(row) == "FID 1.2500 KID 0.500000 ± 0.125000 (10 patches)"
    FID.write_csv([row], str(tmp_path / "o" / "fid_kid.csv"))
    assert (tmp_path / "o" / "fid_kid.csv").read_text().splitlines() == ["set,n_images,n_patches,fid,kid_mean,kid_std",
                                                                       "all,2,10,1.25,0.5,0.125"]
