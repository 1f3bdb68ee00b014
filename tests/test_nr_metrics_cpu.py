"""Host side of the no-reference metrics (rdeic_amd/metrics.py NIQE / BRISQUE, rdeic_amd/ood.py, run_ood.py)
without a GPU: the half-size filter's taps, the AGGD moment fit, model-file loading, the CLI's flags and its CSV."""
import csv
import math

import numpy as np
import pytest

from tests import nr_metrics_ref as R


def test_half_size_taps_from_the_cubic():
    assert int(round(R.TAPS.sum() * 256)) == 256 and np.all(R.TAPS * 256 == np.rint(R.TAPS * 256))
    # a = -0.5 cubic at the distances 1.75, 1.25, 0.75, 0.25 (and mirrored), normalised to sum 1
    raw = np.array([R.cubic(d) for d in (1.75, 1.25, 0.75, 0.25, 0.25, 0.75, 1.25, 1.75)])
    assert np.allclose(raw / raw.sum(), R.TAPS, rtol=0, atol=1e-15)
    assert np.array_equal(R.half_size_taps(), raw / raw.sum())
    assert np.array_equal(np.rint(raw / raw.sum() * 256), [-3, -9, 29, 111, 111, 29, -9, -3])


def _aggd_samples(alpha, beta_l, beta_r, n, seed):
    """Asymmetric generalised Gaussian draws: |x| = beta_side * Gamma(1/alpha)^(1/alpha), left with probability
    beta_l / (beta_l + beta_r)."""
    rng = np.random.default_rng(seed)
    mag = rng.gamma(1.0 / alpha, 1.0, n) ** (1.0 / alpha)
    left = rng.random(n) < beta_l / (beta_l + beta_r)
    return np.where(left, -beta_l * mag, beta_r * mag)


@pytest.mark.parametrize("alpha", [0.8, 2.0, 3.5])
def test_aggd_fit_recovers_alpha(alpha):
    from rdeic_amd import metrics
    x = _aggd_samples(alpha, 1.5, 1.0, 200_000, 7)
    mom = R.six_moments(x)
    a, bl, br, mean, l, r = metrics.aggd_fit(mom, x.size)
    assert abs(float(a) - alpha) <= 0.05, float(a)
    assert float(bl) > float(br) and abs(float(bl) / float(br) - 1.5) < 0.05
    assert float(mean) < 0  # the heavier left side pulls the mean down
    ra = R.aggd(mom, float(x.size))  # the restatement agrees on every output
    assert float(a) == ra[0]
    assert np.allclose([float(bl), float(br), float(mean), float(l), float(r)], ra[1:], rtol=1e-12, atol=0)


def test_features_match_the_restatement_on_its_own_moments():
    """The product's vectorised fits against the spelled-out ones, on the restatement's float64 moments."""
    from rdeic_amd import metrics
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (96, 192, 3), dtype=np.uint8)
    _, m0, _, m1 = R.planes(img, crop=True)
    r0, r1 = R.region_moments(m0, 96, 96), R.region_moments(m1, 48, 48)
    got = np.concatenate([metrics.niqe_features(r0, 96 * 96), metrics.niqe_features(r1, 48 * 48)], axis=-1)
    assert np.allclose(got, R.niqe_block_features(img), rtol=1e-12, atol=0)
    w0, w1 = R.region_moments(m0, 0, 0), R.region_moments(m1, 0, 0)
    got = np.concatenate([metrics.brisque_features(w0[0], m0.size), metrics.brisque_features(w1[0], m1.size)])
    want = np.concatenate([R.brisque_features_scale(w0[0], float(m0.size)),
                           R.brisque_features_scale(w1[0], float(m1.size))])
    assert np.allclose(got, want, rtol=1e-12, atol=0)
    # degenerate moments (an all-zero map) end as NaN features, not as an exception
    assert np.isnan(metrics.niqe_features(np.zeros((1, 5, 6)), 9216)).all()


def test_grid_search_equals_the_full_scan():
    """metrics._grid_argmin bisects the monotone tables; the definition is the argmin over all 9801 grid points."""
    from rdeic_amd import metrics
    rng = np.random.default_rng(4)
    for table in (metrics._RHO, metrics._RHO_GGD):
        mids = (table[:-1] + table[1:]) / 2
        targets = np.concatenate([rng.uniform(table.min() * 0.5, table.max() * 1.5, 2000), table[::97], mids[::89],
                                  np.nextafter(mids[::101], 0), np.nextafter(mids[::101], 10), [1e-9, 1e9]])
        want = np.array([np.argmin((table - t) ** 2) for t in targets])
        assert np.array_equal(metrics._grid_argmin(table, targets), want)
    assert np.array_equal(metrics._grid_argmin(metrics._RHO, np.array([np.nan, np.inf, 0.5])),
                          [-1, -1, R.grid_argmin(R.RHO, 0.5)])
    # the product's tables (scipy gammaln) against the restatement's (math.lgamma)
    assert np.allclose(metrics._RHO, R.RHO, rtol=1e-13, atol=0)
    assert np.allclose(metrics._RHO_GGD, R.RHO_GGD, rtol=1e-13, atol=0)
    assert np.array_equal(metrics.ALPHA_GRID, R.GRID) and R.GRID.size == 9801


def _niqe_params(seed=0):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((36, 36))
    return rng.standard_normal(36), a @ a.T / 36 + np.eye(36)


def _svr(seed=0, n=8):
    rng = np.random.default_rng(seed)
    return {"sv": rng.uniform(-1, 1, (n, 36)), "sv_coef": rng.standard_normal(n), "rho": np.array(-20.0),
            "gamma": np.array(0.05), "scale_min": -np.ones(36) * 0.5, "scale_max": np.ones(36) * 3.0}


def test_niqe_model_files(tmp_path):
    from safetensors.numpy import save_file
    from scipy.io import savemat
    from rdeic_amd import metrics
    mu, cov = _niqe_params()
    np.savez(tmp_path / "n.npz", mu_prisparam=mu, cov_prisparam=cov)
    save_file({"mu_prisparam": mu, "cov_prisparam": cov}, str(tmp_path / "n.safetensors"))
    savemat(str(tmp_path / "n.mat"), {"mu_prisparam": mu[None, :], "cov_prisparam": cov})  # 1x36, as published
    for ext in ("npz", "safetensors", "mat"):
        m = metrics.NIQE(str(tmp_path / f"n.{ext}"))
        assert m.mu.shape == (36,) and np.array_equal(m.mu, mu) and np.array_equal(m.cov, cov), ext
    np.savez(tmp_path / "bad.npz", mu_prisparam=mu)
    with pytest.raises(KeyError, match="cov_prisparam"):
        metrics.NIQE(str(tmp_path / "bad.npz"))
    np.savez(tmp_path / "shape.npz", mu_prisparam=mu[:18], cov_prisparam=cov)
    with pytest.raises(ValueError, match="36"):
        metrics.NIQE(str(tmp_path / "shape.npz"))
    with pytest.raises(ValueError, match="npz"):
        metrics.NIQE(str(tmp_path / "n.txt"))


def test_brisque_model_files_and_score(tmp_path):
    from safetensors.numpy import save_file
    from rdeic_amd import metrics
    svr = _svr()
    np.savez(tmp_path / "b.npz", **svr)
    save_file({k: np.atleast_1d(v) for k, v in svr.items()}, str(tmp_path / "b.safetensors"))
    feat = np.random.default_rng(1).uniform(0, 2, (3, 36))
    for ext in ("npz", "safetensors"):
        m = metrics.BRISQUE(str(tmp_path / f"b.{ext}"))
        assert m.gamma == 0.05 and m.rho == -20.0
        got = m.score(feat)
        for i in range(3):
            x = -1.0 + 2.0 * (feat[i] - svr["scale_min"]) / (svr["scale_max"] - svr["scale_min"])
            want = sum(svr["sv_coef"][j] * math.exp(-0.05 * ((x - svr["sv"][j]) ** 2).sum()) for j in range(8)) + 20.0
            assert abs(got[i] - want) < 1e-12
    svr.pop("gamma")
    np.savez(tmp_path / "bad.npz", **svr)
    with pytest.raises(KeyError, match="gamma"):
        metrics.BRISQUE(str(tmp_path / "bad.npz"))


def test_niqe_score_needs_two_finite_blocks():
    from rdeic_amd import metrics

    class P:
        mu, cov = _niqe_params()
    feat = np.random.default_rng(2).standard_normal((4, 36))
    d = P.mu - feat.mean(0)
    want = math.sqrt(d @ np.linalg.pinv((P.cov + np.cov(feat, rowvar=False)) / 2) @ d)
    assert abs(metrics.niqe_score(feat, P) - want) < 1e-12
    feat[1:, 3] = np.nan
    assert math.isnan(metrics.niqe_score(feat, P))
    assert math.isnan(metrics.niqe_score(feat[:0], P))


def test_run_ood_flags(tmp_path, capsys):
    import run_ood
    a = run_ood.parse_args(["--domains", "x/a,x/b"])
    assert (a.sampler, a.steps, a.guidance_scale, a.latent_noise_std, a.num_noise_samples) == ("ddpm", 2, 1.0, 0.0, 1)
    assert (a.output_dir, a.cache_dir, a.save_recon, a.seed) == ("indicators/", "encodings/ood/", False, 231)
    assert (a.ckpt, a.dtype, a.batch_size, a.lpips_backbone, a.niqe_model, a.brisque_model) == \
        ("", "fp32", 1, "", "", "")
    np.savez(tmp_path / "n.npz", x=np.zeros(1))
    a = run_ood.parse_args(["--domains", "d", "--sampler", "ddim", "--steps", "3", "--latent_noise_std", "0.1",
                            "--num_noise_samples", "4", "--save_recon", "--seed", "5", "--batch_size", "2",
                            "--dtype", "bf16", "--niqe_model", str(tmp_path / "n.npz"),
                            "--brisque_model", str(tmp_path / "n.npz")])
    assert (a.sampler, a.steps, a.latent_noise_std, a.num_noise_samples, a.save_recon, a.seed, a.batch_size,
            a.dtype) == ("ddim", 3, 0.1, 4, True, 5, 2, "bf16")
    with pytest.raises(SystemExit):
        run_ood.parse_args([])  # --domains is required
    with pytest.raises(SystemExit):
        run_ood.parse_args(["--domains", "d", "--niqe_model", str(tmp_path / "missing.mat")])
    assert "is not a file" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        run_ood.parse_args(["--help"])
    assert e.value.code == 0 and "--num_noise_samples" in capsys.readouterr().out


def test_csv_columns_and_nan(tmp_path):
    from rdeic_amd import ood
    recs = [{"domain": "a", "image_id": "i0", "bpp": 0.25, "psnr": 20.0, "ssim": float("nan"),
             "ms_ssim": float("nan"), "lpips": float("nan"), "niqe": 5.5, "brisque": float("nan"), "extra": 1},
            {"domain": "a", "image_id": "i1", "bpp": 0.5, "psnr": 22.0}]
    ood.write_csv(recs, str(tmp_path / "out" / "ood_results_a.csv"))
    with open(tmp_path / "out" / "ood_results_a.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["domain", "image_id", "bpp", "psnr", "ssim", "ms_ssim", "lpips", "niqe", "brisque"]
    assert rows[1] == ["a", "i0", "0.25", "20.0", "nan", "nan", "nan", "5.5", "nan"]
    assert rows[2] == ["a", "i1", "0.5", "22.0", "nan", "nan", "nan", "nan", "nan"]
    s = ood.summary(recs)
    assert s["a"]["psnr"] == (21.0, math.sqrt(2.0)) and math.isnan(s["a"]["lpips"][0]) and s["a"]["niqe"][0] == 5.5
    assert ood.select_candidate(None) == 0 and ood.select_candidate(np.array([0.3, 0.1, 0.1])) == 1
    assert ood.pad64(np.zeros((120, 184, 3), np.uint8)).shape == (128, 192, 3)
