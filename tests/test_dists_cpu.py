"""DISTS without a device: the weight and backbone loaders, the size and chunk rules, the known answers of the
restatement's L2 pool (tests/dists_ref.py), the restatement's defining properties, and the CLI flags."""
import numpy as np
import pytest
import torch

from rdeic_amd import dists as D
from tests import dists_ref as R


# ------------------------------------------------------------------ loaders
def test_backbone_layouts_load_to_the_same_tensors(tmp_path):
    tv, pkg, stage = (R.seeded_backbone(5, layout) for layout in ("torchvision", "lpips", "stage"))
    assert not set(tv) & set(pkg) and not set(tv) & set(stage)
    stage.update(R.seeded_weights(1))  # the single file carries alpha / beta beside the convs
    a, b, c = D.load_backbone(tv), D.load_backbone(pkg), D.load_backbone(stage)
    assert len(a) == len(b) == len(c) == 13
    flat = [cv for st in R.STAGES for cv in st]
    for (wa, ba), (wb, bb), (wc, bc), (_, cin, cout) in zip(a, b, c, flat):
        assert tuple(wa.shape) == (cout, cin, 3, 3) and tuple(ba.shape) == (cout,)
        assert torch.equal(wa, wb) and torch.equal(ba, bb) and torch.equal(wa, wc) and torch.equal(ba, bc)
    path = str(tmp_path / "vgg16.pth")
    torch.save(tv, path)
    for (wa, ba), (wd, bd) in zip(a, D.load_backbone(path)):
        assert torch.equal(wa, wd) and torch.equal(ba, bd)
    from rdeic_amd.lpips import seeded_backbone  # the bench's stand-in is the same draw
    assert torch.equal(seeded_backbone("vgg", 5)["features.28.weight"], tv["features.28.weight"])


def test_unknown_backbone_layout_names_the_keys():
    sd = {k.replace("features.", "backbone."): v for k, v in R.seeded_backbone().items()}
    with pytest.raises(ValueError) as e:
        D.load_backbone(sd)
    msg = str(e.value)
    assert "features.0.weight" in msg and "net.slice1.0.weight" in msg and "stage1.0.weight" in msg
    with pytest.raises(ValueError) as e:  # weights alone, no backbone anywhere
        D.DISTS(R.seeded_weights(), backbone=None, device="cpu")
    assert "stage1.0.weight" in str(e.value)
    bad = R.seeded_backbone()
    bad["features.5.weight"] = bad["features.5.weight"][:, :32]
    with pytest.raises(ValueError) as e:
        D.load_backbone(bad)
    assert "features.5" in str(e.value)  # a shape error names the tensor


def test_alpha_beta_load_the_same_4d_flat_and_npz(tmp_path):
    w = R.seeded_weights(3)
    assert tuple(w["alpha"].shape) == (1, 1475, 1, 1) == tuple(D.seeded_weights(3)["alpha"].shape)
    assert torch.equal(D.seeded_weights(3)["beta"], w["beta"])
    assert 0.05 < float(w["alpha"].min()) and float(w["alpha"].max()) < 0.15  # N(0.1, 0.01)
    a4, b4 = D.load_weights(w)
    af, bf = D.load_weights({"alpha": w["alpha"].reshape(-1), "beta": w["beta"].reshape(-1).numpy()})
    npz, pth = str(tmp_path / "w.npz"), str(tmp_path / "w.pt")
    np.savez(npz, alpha=w["alpha"].numpy(), beta=w["beta"].numpy())
    torch.save(w, pth)
    for a, b in ((af, bf), D.load_weights(npz), D.load_weights(pth)):
        assert a.dtype == np.float64 and a.shape == (1475,) and np.array_equal(a, a4) and np.array_equal(b, b4)
    assert np.array_equal(a4, w["alpha"].reshape(-1).double().numpy())
    with pytest.raises(ValueError) as e:
        D.load_weights({"alpha": w["alpha"]})
    assert "beta" in str(e.value)
    with pytest.raises(ValueError) as e:
        D.load_weights({"alpha": w["alpha"], "beta": w["beta"][:, :1474]})
    assert "beta" in str(e.value) and "1474" in str(e.value) and "1475" in str(e.value)
    with pytest.raises(FileNotFoundError):
        D.load_weights(str(tmp_path / "missing.npz"))


# ------------------------------------------------------------------ size rules
def test_activation_shapes_pool_with_ceil():
    acts = D.activation_shapes(37, 51)
    sizes = []
    for h, w, _ in acts:
        if (h, w) not in sizes:
            sizes.append((h, w))
    assert sizes == [(37, 51), (19, 26), (10, 13), (5, 7), (3, 4)]
    assert [s[2] for s in D.tap_shapes(37, 51)] == [4, 64, 128, 256, 512, 512]
    assert [s[:2] for s in D.tap_shapes(37, 51)] == [(37, 51)] + sizes
    assert D.tap_shapes(16, 16)[-1] == (1, 1, 512) and D.tap_shapes(1, 1)[-1] == (1, 1, 512)
    # the table's shapes are the restatement's
    taps = R.taps(R.seeded_backbone(), np.zeros((1, 37, 51, 3), np.uint8))
    assert [(t.shape[2], t.shape[3]) for t in taps] == [s[:2] for s in D.tap_shapes(37, 51)]
    assert [t.shape[1] for t in taps] == list(D.CHANNELS) and sum(D.CHANNELS) == D.N_WEIGHTS == 1475


def test_chunk_rule_and_size_limits():
    assert D.chunk_pairs(1024, 1024) == 3 and not D.split_pair(1024, 1024)
    assert D.chunk_pairs(64, 64) == D.chunk_pairs(64, 64) >= 1
    for h, w in ((1024, 1024), (2048, 2048), (64, 64), (37, 51)):
        pairs = D.chunk_pairs(h, w)
        images = pairs if D.split_pair(h, w) else 2 * pairs
        assert all(images * a * b * c * 4 < 2 ** 31 for a, b, c in D.activation_shapes(h, w))
    assert D.split_pair(2048, 2048) and D.chunk_pairs(2048, 2048) == 1
    assert D.image_bytes(4096, 2048) == 2 ** 31  # the first stage's 64 channels
    with pytest.raises(ValueError):
        D.chunk_pairs(4096, 2048)
    assert D.chunk_pairs(4096, 2047) == 1
    for h, w in ((0, 8), (8, 0)):  # only the empty image is refused below that
        with pytest.raises(ValueError):
            D.chunk_pairs(h, w)
    assert D.chunk_pairs(1, 1) == D.MAX_PAIRS <= 65535  # the moment kernels' image limit per launch


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("a", [3.0, -0.25])
def test_l2_pool_known_answers_on_a_constant_map(a):
    """In-bounds weight sums: 16/16 inside, 12/16 where one padding line is read, 9/16 where two are, 4/16 for a
    1x1 map; all with the 1e-12 term."""
    def want(frac):
        return np.sqrt(frac * a * a + 1e-12)
    x = torch.full((1, 2, 6, 8), a, dtype=torch.float64)  # even: only the near padding is read
    y = R.l2_pool(x).numpy()
    assert y.shape == (1, 2, 3, 4)
    assert np.allclose(y[:, :, 1:, 1:], want(1.0), rtol=1e-14, atol=0) and abs(y[0, 0, 1, 1] - abs(a)) < 1e-11
    assert np.allclose(y[:, :, 0, 1:], want(0.75), rtol=1e-14, atol=0)
    assert np.allclose(y[:, :, 1:, 0], want(0.75), rtol=1e-14, atol=0)
    assert np.allclose(y[:, :, 0, 0], want(0.5625), rtol=1e-14, atol=0) and abs(y[0, 0, 0, 0] - 0.75 * abs(a)) < 1e-11
    x = torch.full((1, 1, 7, 5), a, dtype=torch.float64)  # odd: the far padding is read too
    y = R.l2_pool(x).numpy()
    assert y.shape == (1, 1, 4, 3)
    assert np.allclose(y[0, 0, 1:3, 1], want(1.0), rtol=1e-14, atol=0)
    assert np.allclose(y[0, 0, [0, 3], 1], want(0.75), rtol=1e-14, atol=0)
    assert np.allclose(y[0, 0, 1:3, [0, 2]], want(0.75), rtol=1e-14, atol=0)
    assert np.allclose(y[0, 0, [0, 0, 3, 3], [0, 2, 0, 2]], want(0.5625), rtol=1e-14, atol=0)
    y = R.l2_pool(torch.full((1, 3, 1, 1), a, dtype=torch.float64)).numpy()
    assert y.shape == (1, 3, 1, 1) and np.allclose(y, want(0.25), rtol=1e-14, atol=0)
    assert abs(y[0, 0, 0, 0] - 0.5 * abs(a)) < 1e-11
    assert float(R.l2_pool(torch.zeros((1, 1, 4, 4), dtype=torch.float64)).max()) == 1e-6  # sqrt(1e-12)


def test_restatement_properties():
    bb, w = R.seeded_backbone(), R.seeded_weights()
    pred, tgt = R.pairs(32, 48)
    d64 = R.dists(bb, w, pred, tgt)
    d32 = R.dists(bb, w, pred, tgt, torch.float32)
    print(f"fp64 {d64}, fp32 - fp64 {d32 - d64}")
    assert np.isfinite(d64).all() and (d64[:3] > 0).all() and d64[0] < d64[1]  # noise is closer than another image
    assert abs(d64[3]) < 1e-12  # black against black: identical
    assert np.abs(d32 - d64).max() < 1e-5  # the device tolerance (tests/test_dists_gpu.py); measured ~1e-7
    assert np.array_equal(R.dists(bb, w, tgt, pred), d64)  # symmetric
    assert np.abs(R.dists(bb, w, tgt, tgt)).max() < 1e-12
    one = R.dists(bb, w, pred[:1, :16, :16], tgt[:1, :16, :16])  # 16x16: the deepest tap is one pixel
    assert R.taps(bb, pred[:1, :16, :16])[-1].shape[2:] == (1, 1) and np.isfinite(one).all()


# ------------------------------------------------------------------ CLIs
def test_cli_flags_and_default_headers(tmp_path):
    import inference_partition as P
    import run_ood as O
    from rdeic_amd import ood
    wpath, bpath = str(tmp_path / "dists.npz"), str(tmp_path / "vgg16.pth")
    w = R.seeded_weights()
    np.savez(wpath, alpha=w["alpha"].numpy(), beta=w["beta"].numpy())
    torch.save(R.seeded_backbone(), bpath)
    missing = str(tmp_path / "missing.pt")
    for mod, base in ((P, ["--input", "x"]), (O, ["--domains", "x"])):
        a = mod.parse_args(base)
        assert (a.dists_weights, a.dists_backbone) == ("", "")
        a = mod.parse_args(base + ["--dists_weights", wpath, "--dists_backbone", bpath])
        assert (a.dists_weights, a.dists_backbone) == (wpath, bpath)
        for extra in (["--dists_weights", missing], ["--dists_weights", wpath, "--dists_backbone", missing],
                      ["--dists_backbone", bpath]):
            with pytest.raises(SystemExit):  # at parse time: no model has been loaded
                mod.parse_args(base + extra)
    assert P.metrics_fieldnames() == ["image", "bpp", "scale", "psnr", "ssim", "ms_ssim", "lpips"]
    assert P.metrics_fieldnames(False, True) == ["image", "bpp", "scale", "psnr", "ssim", "ms_ssim", "lpips", "caption"]
    assert P.metrics_fieldnames(True, True)[6:] == ["lpips", "dists", "caption"]
    assert ood.COLUMNS == ["domain", "image_id", "bpp", "psnr", "ssim", "ms_ssim", "lpips", "niqe", "brisque"]
    assert ood.columns() == ood.COLUMNS
    assert ood.columns(True) == ["domain", "image_id", "bpp", "psnr", "ssim", "ms_ssim", "lpips", "dists", "niqe",
                                 "brisque"]
    rec = {"domain": "d", "image_id": "a", "bpp": 0.1, "psnr": 30.0, "dists": 0.25}
    ood.write_csv([rec], str(tmp_path / "plain.csv"))
    ood.write_csv([rec], str(tmp_path / "with.csv"), with_dists=True)
    plain, with_d = (open(tmp_path / n).read().splitlines() for n in ("plain.csv", "with.csv"))
    assert plain[0] == "domain,image_id,bpp,psnr,ssim,ms_ssim,lpips,niqe,brisque"
    assert plain[1] == "d,a,0.1,30.0,nan,nan,nan,nan,nan"
    assert with_d[0] == "domain,image_id,bpp,psnr,ssim,ms_ssim,lpips,dists,niqe,brisque"
    assert with_d[1] == "d,a,0.1,30.0,nan,nan,nan,0.25,nan,nan"
