"""LPIPS without a device: the weight loaders, the size and chunk rules, the fp64 / fp32 restatement of the
reference's model/lpips.py forward (tests/lpips_ref.py) on its defining properties, and the CLI flags."""
import numpy as np
import pytest
import torch

from rdeic_amd import lpips as L
from tests import lpips_ref as R


@pytest.mark.parametrize("net", ["alex", "vgg"])
def test_backbone_layouts_load_to_the_same_tensors(net, tmp_path):
    tv = R.seeded_backbone(net, 5, "torchvision")
    pkg = R.seeded_backbone(net, 5, "lpips")
    assert not set(tv) & set(pkg)
    pkg["lin0.model.1.weight"] = torch.zeros(1, 64, 1, 1)  # the package's full state dict carries more
    pkg["scaling_layer.shift"] = torch.zeros(1, 3, 1, 1)
    a, b = L.load_backbone(net, tv), L.load_backbone(net, pkg)
    assert len(a) == len(b) == len(R.CONVS[net])
    for (wa, ba), (wb, bb), (_, _, cin, cout, k, _, _) in zip(a, b, R.CONVS[net]):
        assert tuple(wa.shape) == (cout, cin, k, k) and tuple(ba.shape) == (cout,)
        assert torch.equal(wa, wb) and torch.equal(ba, bb)
    path = str(tmp_path / "bb.pth")
    torch.save(tv, path)
    for (wa, ba), (wc, bc) in zip(a, L.load_backbone(net, path)):
        assert torch.equal(wa, wc) and torch.equal(ba, bc)


def test_unknown_backbone_layout_names_the_keys():
    sd = {k.replace("features.", "backbone."): v for k, v in R.seeded_backbone("alex").items()}
    with pytest.raises(ValueError) as e:
        L.load_backbone("alex", sd)
    assert "features.0.weight" in str(e.value) and "net.slice1.0.weight" in str(e.value)
    bad = R.seeded_backbone("alex")
    bad["features.3.weight"] = bad["features.3.weight"][:, :32]
    with pytest.raises(ValueError):
        L.load_backbone("alex", bad)
    with pytest.raises(ValueError):
        L.load_backbone("resnet", R.seeded_backbone("alex"))


@pytest.mark.parametrize("net", ["alex", "vgg"])
def test_lin_loads_the_same_from_pth_and_npz(net, tmp_path):
    heads = R.lin_heads(net)
    assert [h.numel() for h in heads] == list(L.CHANNELS[net])
    assert all(h.dtype == torch.float32 and float(h.min()) >= 0.0 for h in heads)  # the published heads are >= 0
    pth = str(tmp_path / f"{net}.pth")
    torch.save({f"lin{k}.model.1.weight": h.reshape(1, -1, 1, 1) for k, h in enumerate(heads)}, pth)
    npz = str(tmp_path / "heads.npz")
    np.savez(npz, **{f"lin{k}": h.numpy() for k, h in enumerate(heads)})
    for got in (L.load_lin(net, pth), L.load_lin(net, npz)):
        assert len(got) == 5 and all(torch.equal(g, h) for g, h in zip(got, heads))
    with pytest.raises(ValueError):
        L.load_lin(net, {"lin0": heads[0]})
    with pytest.raises(ValueError):
        L.load_lin(net, {f"lin{k}": h[:-1] for k, h in enumerate(heads)})


def test_tap_shapes_and_minimum_size():
    assert [s[:2] for s in L.tap_shapes("alex", 64, 64)] == [(15, 15), (7, 7), (3, 3), (3, 3), (3, 3)]
    assert [s[:2] for s in L.tap_shapes("alex", 96, 80)] == [(23, 19), (11, 9), (5, 4), (5, 4), (5, 4)]
    assert [s[:2] for s in L.tap_shapes("alex", 35, 47)] == [(8, 11), (3, 5), (1, 2), (1, 2), (1, 2)]
    assert [s[2] for s in L.tap_shapes("vgg", 32, 48)] == [64, 128, 256, 512, 512]
    assert L.tap_shapes("vgg", 32, 48)[-1][:2] == (2, 3)
    # the table's shapes are the restatement's
    for net, h, w in (("alex", 35, 47), ("vgg", 32, 48)):
        taps = R.taps(net, R.seeded_backbone(net), torch.zeros(1, 3, h, w))
        assert [(t.shape[2], t.shape[3], t.shape[1]) for t in taps] == L.tap_shapes(net, h, w)
    for net in ("alex", "vgg"):
        m = L.MIN_SIZE[net]
        assert L.tap_shapes(net, m, m)[-1][:2] == (1, 1)
        for h, w in ((m - 1, m), (m, m - 1)):
            with pytest.raises(ValueError):
                L.tap_shapes(net, h, w)
            with pytest.raises(ValueError):
                L.chunk_pairs(net, h, w)
    assert L.MIN_SIZE == {"alex": 31, "vgg": 16}


@pytest.mark.parametrize("net,h,w", [("vgg", 1024, 1024), ("alex", 2048, 2048), ("alex", 64, 64), ("vgg", 2048, 2048)])
def test_chunk_rule_keeps_activations_under_2gib(net, h, w):
    pairs = L.chunk_pairs(net, h, w)
    assert pairs >= 1 and pairs == L.chunk_pairs(net, h, w)
    images = pairs if L.split_pair(net, h, w) else 2 * pairs  # images per backbone launch
    assert images >= 1
    for a, b, c in L.activation_shapes(net, h, w):
        assert images * a * b * c * 4 < 2 ** 31
    if not L.split_pair(net, h, w):  # and it is the most that fits
        assert any(2 * (pairs + 1) * a * b * c * 4 >= 2 ** 31 for a, b, c in L.activation_shapes(net, h, w))
    else:
        assert pairs == 1


def test_restatement_properties():
    bb = R.seeded_backbone("alex")
    b, a = R.noisy_pair(64, 64, 1)
    other = R.noisy_pair(64, 64, 2)[1]
    pred, tgt = np.stack([b, a, other]), np.stack([a, a, a])
    d64 = R.lpips("alex", bb, pred, tgt)
    d32 = R.lpips("alex", bb, pred, tgt, torch.float32)
    assert d64[1] == 0.0 and d32[1] == 0.0  # identical images
    assert 1e-3 < d64[0] < 2e-2 < d64[2]  # sigma-12 noise is a small distance, an unrelated image a large one
    assert np.allclose(R.lpips("alex", bb, tgt, pred), d64, rtol=1e-12, atol=0)  # symmetric
    assert np.allclose(d32, d64, rtol=1e-4, atol=0)  # the device tolerance (tests/test_lpips_gpu.py); measured ~1e-6
    # all-zero feature vectors (post-ReLU) normalise to 0, not NaN
    z = torch.zeros(1, 64, 2, 2, dtype=torch.float64)
    assert float(R.layer_distance(z, z, R.lin_heads("alex")[0])[0]) == 0.0


def test_cli_flags(tmp_path):
    import inference_partition as P
    a = P.parse_args(["--input", "x"])
    assert (a.lpips_backbone, a.lpips_lin, a.lpips_net) == ("", "", "alex")
    bb, lin = str(tmp_path / "alexnet.pth"), str(tmp_path / "heads.npz")
    torch.save(R.seeded_backbone("alex"), bb)
    np.savez(lin, **{f"lin{k}": h.numpy() for k, h in enumerate(R.lin_heads("vgg"))})
    a = P.parse_args(["--input", "x", "--lpips_backbone", bb, "--lpips_lin", lin, "--lpips_net", "vgg"])
    assert (a.lpips_backbone, a.lpips_lin, a.lpips_net) == (bb, lin, "vgg")
    with pytest.raises(SystemExit):  # a backbone without the heads is refused at start-up
        P.parse_args(["--input", "x", "--lpips_backbone", bb, "--lpips_lin", str(tmp_path / "missing.pth")])
    with pytest.raises(SystemExit):
        P.parse_args(["--input", "x", "--lpips_backbone", str(tmp_path / "missing.pth"), "--lpips_lin", lin])
    with pytest.raises(SystemExit):
        P.parse_args(["--input", "x", "--lpips_net", "resnet"])


def test_cli_default_lin_location(tmp_path, monkeypatch):
    """--lpips_lin defaults to ./weight/lpips/<net>.pth, the reference's location."""
    import inference_partition as P
    bb = str(tmp_path / "alexnet.pth")
    torch.save(R.seeded_backbone("alex"), bb)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit):
        P.parse_args(["--input", "x", "--lpips_backbone", bb])
    (tmp_path / "weight" / "lpips").mkdir(parents=True)
    torch.save({f"lin{k}.model.1.weight": h.reshape(1, -1, 1, 1) for k, h in enumerate(R.lin_heads("alex"))},
               str(tmp_path / "weight" / "lpips" / "alex.pth"))
    a = P.parse_args(["--input", "x", "--lpips_backbone", bb])
    assert a.lpips_lin.replace("\\", "/").endswith("weight/lpips/alex.pth")
    assert all(torch.equal(g, h) for g, h in zip(L.load_lin("alex", a.lpips_lin), R.lin_heads("alex")))
