"""run_ood.py / rdeic_amd/ood.py (reference experiments/run_ood.py) on synthetic weights: domain folders in, the three
CSVs out with the reference's columns, bpp from the stream files, NIQE as metrics.niqe gives it on the saved
reconstruction, and the test-time augmentation: the kept candidate is the lowest LPIPS of the N, for any batching."""
import csv
import functools
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLUMNS = ["domain", "image_id", "bpp", "psnr", "ssim", "ms_ssim", "lpips", "niqe", "brisque"]


@pytest.fixture()
def one_model(monkeypatch):
    """Every run_ood.main of this module shares one synthetic model (the load dominates a run)."""
    import inference
    monkeypatch.setattr(inference, "load_model", _load_once(inference.load_model))


@functools.lru_cache(maxsize=None)
def _load_once(load):
    return functools.lru_cache(maxsize=None)(load)


def _write_domains(root, h, w, names=("sketch", "xray")):
    from PIL import Image
    from rdeic_amd.synthetic import synth_image
    dirs = []
    for d, name in enumerate(names):
        os.makedirs(root / name)
        for k in range(2):
            Image.fromarray(synth_image(h, w, 40 + 2 * d + k)).save(root / name / f"im{k}.png")
        dirs.append(str(root / name))
    return dirs


def _niqe_file(tmp_path):
    rng = np.random.default_rng(5)
    a = rng.standard_normal((36, 36))
    np.savez(tmp_path / "niqe.npz", mu_prisparam=rng.standard_normal(36), cov_prisparam=a @ a.T / 36 + np.eye(36))
    return str(tmp_path / "niqe.npz")


def _rows(path):
    with open(path) as f:
        r = csv.reader(f)
        header = next(r)
        return header, [dict(zip(header, row)) for row in r]


def test_run_ood_writes_the_tables(gpu, tmp_path, one_model):
    import run_ood
    from PIL import Image
    from rdeic_amd import metrics
    dirs = _write_domains(tmp_path / "in", 120, 184)  # pads to 128x192, cropped back
    niqe_file = _niqe_file(tmp_path)
    out, cache = tmp_path / "out", tmp_path / "cache"
    recs = run_ood.main(["--domains", ",".join(dirs), "--sampler", "ddim", "--steps", "2", "--output_dir", str(out),
                         "--cache_dir", str(cache), "--save_recon", "--batch_size", "2", "--niqe_model", niqe_file])
    assert len(recs) == 4
    header, rows = _rows(out / "ood_results_all.csv")
    assert header == COLUMNS and len(rows) == 4
    assert [(r["domain"], r["image_id"]) for r in rows] == [("sketch", "im0"), ("sketch", "im1"), ("xray", "im0"),
                                                            ("xray", "im1")]
    nm = metrics.NIQE(niqe_file)
    for name in ("sketch", "xray"):
        h2, per = _rows(out / f"ood_results_{name}.csv")
        assert h2 == COLUMNS and per == [r for r in rows if r["domain"] == name]
    for r in rows:
        nbytes = (cache / r["domain"] / r["image_id"]).stat().st_size
        assert abs(float(r["bpp"]) - 8.0 * nbytes / (128 * 192)) < 1e-12
        assert math.isfinite(float(r["psnr"])) and 5.0 < float(r["psnr"]) <= 100.0
        assert r["ssim"] == r["ms_ssim"] == r["lpips"] == r["brisque"] == "nan"  # under 176 px, no backbone / model
        recon = np.array(Image.open(out / r["domain"] / f"{r['image_id']}.png"))
        assert recon.shape == (120, 184, 3)
        want = metrics.niqe(torch.from_numpy(recon[None]).cuda(), nm)[0]  # one 96x96 block at this size: NaN
        assert np.array_equal(np.array([float(r["niqe"])]), np.array([want]), equal_nan=True)


def test_tta_keeps_the_lowest_lpips_for_any_batching(gpu, tmp_path, one_model):
    import inference
    import run_ood
    from PIL import Image
    from rdeic_amd import lpips as L, metrics, ood
    from rdeic_amd.synthetic import synth_context
    dirs = _write_domains(tmp_path / "in", 192, 208, names=("sat",))  # pads to 192x256; 2x2 NIQE blocks; 16 | H, W
    torch.save(L.seeded_backbone("alex"), tmp_path / "alex.pth")
    lin = os.path.join(ROOT, "tests", "golden", "lpips_lin.npz")
    niqe_file = _niqe_file(tmp_path)
    rng = np.random.default_rng(6)
    np.savez(tmp_path / "brisque.npz", sv=rng.uniform(-1, 1, (8, 36)), sv_coef=rng.standard_normal(8), rho=-20.0,
             gamma=0.05, scale_min=np.full(36, -0.5), scale_max=np.full(36, 3.0))
    base = ["--domains", dirs[0], "--sampler", "ddim", "--steps", "2", "--latent_noise_std", "0.3",
            "--num_noise_samples", "3", "--save_recon", "--seed", "80", "--lpips_backbone", str(tmp_path / "alex.pth"),
            "--lpips_lin", lin, "--niqe_model", niqe_file, "--brisque_model", str(tmp_path / "brisque.npz")]
    r2 = run_ood.main(base + ["--output_dir", str(tmp_path / "o2"), "--cache_dir", str(tmp_path / "c2"),
                              "--batch_size", "2"])
    r1 = run_ood.main(base + ["--output_dir", str(tmp_path / "o1"), "--cache_dir", str(tmp_path / "c1"),
                              "--batch_size", "1"])
    assert len(r2) == 2 and r1 == r2
    model = inference.load_model("", "fp32")
    lp = L.LPIPS("alex", backbone=str(tmp_path / "alex.pth"), lin=lin)
    nm, bm = metrics.NIQE(niqe_file), metrics.BRISQUE(str(tmp_path / "brisque.npz"))
    ctx = synth_context().to(model.device)
    picked = []
    for k, rec in enumerate(r2):
        stem = rec["image_id"]
        assert (tmp_path / "c1" / "sat" / stem).read_bytes() == (tmp_path / "c2" / "sat" / stem).read_bytes()
        recon = np.array(Image.open(tmp_path / "o2" / "sat" / f"{stem}.png"))
        assert np.array_equal(recon, np.array(Image.open(tmp_path / "o1" / "sat" / f"{stem}.png")))
        orig = np.array(Image.open(os.path.join(dirs[0], f"{stem}.png")).convert("RGB"))
        padded = torch.from_numpy(ood.pad64(orig)[None]).cuda()
        c_lat, hint = model.decompress_bodies([(tmp_path / "c2" / "sat" / stem).read_bytes()])
        draws = ood.image_draws((1, 4, 24, 32), 80 + k, 2, "ddim", 3, model.device)
        cands = [model.relay_decode_u8(c_lat + (d[0] * 0.3).to(c_lat.dtype), hint, ctx, d[1], 2, "ddim")
                 for d in draws]  # one at a time here; the harness decodes the three in one batch
        scores = [float(lp(c, padded)[0]) for c in cands]
        best = int(np.argmin(scores))
        picked.append(best)
        print(f"\n[ood tta] {stem}: candidate LPIPS {scores}, kept {best}")
        assert len(set(scores)) == 3
        assert np.array_equal(cands[best][0, :192, :208].cpu().numpy(), recon)
        crop = torch.from_numpy(recon[None]).cuda()
        assert rec["lpips"] == float(lp(crop, torch.from_numpy(orig[None]).cuda())[0])
        assert rec["niqe"] == float(metrics.niqe(crop, nm)[0]) and math.isfinite(rec["niqe"])
        assert rec["brisque"] == float(metrics.brisque(crop, bm)[0]) and math.isfinite(rec["brisque"])
        assert math.isfinite(rec["ssim"]) and math.isfinite(rec["ms_ssim"]) and math.isfinite(rec["psnr"])
    # with --seed 80 neither image's best candidate is the first (LPIPS 0.1988 / 0.1980 / 0.1928 and 0.2048 / 0.1934 /
    # 0.1978 on an MI355X): keeping the first one would not pass
    assert 0 not in picked
    header, rows = _rows(tmp_path / "o2" / "ood_results_sat.csv")
    assert header == COLUMNS and [float(r["niqe"]) for r in rows] == [r["niqe"] for r in r2]
