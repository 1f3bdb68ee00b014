"""NIQE / BRISQUE on the device (csrc/nr_metrics.hip, rdeic_amd/metrics.py) against the float64 restatement
tests/nr_metrics_ref.py: the luma / MSCN / half-size planes, the region moments, determinism, the scores end to end,
and degenerate inputs.

Inputs are seeded u8 images: Gaussian noise around mid-grey, and a smooth diagonal gradient with mild noise (plus a
noiseless gradient and a constant for the planes). Two conditions on the inputs, both asserted on the CPU:
  * no pixel's luma is an exact .5 tie before rounding ((299 r + 587 g + 114 b) mod 1000 == 500; the blue channel of
    such pixels is moved by one level): the rounding direction there depends on the last bit of the arithmetic;
  * for the end-to-end test, no fitted R of the reference lies within MARGIN (relative) of a decision midpoint between
    grid neighbours, so the discontinuous argmin cannot hide a sound device result. MARGIN is 1e-5, not 1e-4: the
    grid's cells are narrower than 2e-4 relative wherever alpha > 1.6 (rho(2.000) and rho(2.001) differ by 1.1e-4
    relative, asserted below), and the MSCN map of any noise-like image fits alpha near 2, so no input can keep 1e-4
    from both neighbours' midpoints. 1e-5 is what a seed search can still meet over 40 fits an image (the cells these
    inputs land in are 4e-5 to 1e-3 wide) and is above the moments' measured error (8e-6 relative at worst, below);
    the image seeds were searched on the CPU, with the reference alone, to satisfy it.

Tolerances: 4x the device's worst error against the float64 reference measured on an MI355X on these inputs
(the figures are printed before every assertion):
    half-size plane     worst abs 0, worst rel 0 on every input: integers times k/256, every partial sum representable
                        in fp32, so the plane is asserted exactly (4 x 0)
    MSCN planes         worst abs 4.97e-5 (96x96 gradient, scale 1; noise images 1e-6 to 3e-6), worst rel 3.6e-4 (noiseless
                        gradient, relative to max(|M|, 1e-2))                                  -> ATOL_M 2.0e-4
    moment sums         worst rel 7.56e-6 (100x100 gradient, scale 1; scale 0 and noise images 4e-8 to 3e-7), worst abs
                        1.6e-3; counts exact                                                     -> RTOL_MOM 3.0e-5
    NIQE / BRISQUE      worst rel 3.21e-8 / 4.5e-9, worst abs 2.6e-7 / 1.2e-7                    -> RTOL_SCORE 1.3e-7
"""
import functools
import math

import numpy as np
import pytest
import torch

from tests import nr_metrics_ref as R

pytestmark = pytest.mark.gpu

MARGIN = 1e-5
SIGN_GAP = 1e-4
ATOL_M = 2.0e-4       # MSCN planes, absolute (values of order 1)
RTOL_MOM = 3.0e-5     # the four sums of a region's moments, relative
RTOL_SCORE = 1.3e-7   # NIQE / BRISQUE scores, relative


def _fix_ties(img):
    t = R.luma_ties(img)
    b = img[..., 2].astype(int)
    img = img.copy()
    img[..., 2] = np.where(t, np.where(b < 255, b + 1, b - 1), b).astype(np.uint8)
    assert not R.luma_ties(img).any()
    return img


def noise_img(h, w, seed):
    rng = np.random.default_rng(seed)
    return _fix_ties(np.clip(np.rint(rng.normal(128.0, 45.0, (h, w, 3))), 0, 255).astype(np.uint8))


def grad_img(h, w, seed, noise=12.0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 40.0 + 150.0 * (0.5 * yy / h + 0.5 * xx / w)
    img = base[..., None] * np.array([1.0, 0.9, 1.1]) + rng.normal(0.0, noise, (h, w, 3))
    return _fix_ties(np.clip(np.rint(img), 0, 255).astype(np.uint8))


def const_img(h, w, value=(200, 90, 31)):
    return np.broadcast_to(np.array(value, dtype=np.uint8), (h, w, 3)).copy()


@functools.lru_cache(maxsize=None)
def _case(name):
    """(block, uint8 [N,H,W,3]) of a named input; built once."""
    return {
        "crop200x296": (96, np.stack([noise_img(200, 296, 21)])),
        "block96": (96, np.stack([grad_img(96, 96, 22)])),
        "plane100": (0, np.stack([noise_img(100, 100, 23)])),
        "smooth100": (0, np.stack([grad_img(100, 100, 24, noise=0.0)])),
        "batch192x288": (96, np.stack([noise_img(192, 288, 1000), grad_img(192, 288, 1000)])),
        "batch100": (0, np.stack([noise_img(100, 100, 1000), grad_img(100, 100, 1000)])),
        "niqe192": (96, np.stack([noise_img(192, 192, NIQE_SEEDS[0]), grad_img(192, 192, NIQE_SEEDS[1])])),
        "brisque100": (0, np.stack([noise_img(100, 100, BRISQUE_SEEDS[0]), grad_img(100, 100, BRISQUE_SEEDS[1])])),
    }[name]


NIQE_SEEDS = (1581, 2901)    # smallest decision margins 1.15e-5 / 1.30e-5 over 40 fits each; sign gaps 7.1e-4 / 4.9e-4
BRISQUE_SEEDS = (1008, 1000)  # 1.29e-5 / 2.24e-5 over 10 fits each; sign gaps 8.6e-4 / 3.3e-4


@functools.lru_cache(maxsize=None)
def _ref_planes(name):
    block, imgs = _case(name)
    return [R.planes(im, crop=block == 96) for im in imgs]


@functools.lru_cache(maxsize=None)
def _ref_moments(name):
    block, _ = _case(name)
    return [(R.region_moments(m0, block, block), R.region_moments(m1, block // 2, block // 2))
            for _, m0, _, m1 in _ref_planes(name)]


def _check_signs(name):
    """A condition on the inputs: no sign of M (so no count, and no side of a product map) hangs on fp32 rounding.
    |Y - mu| stays above 1e-4 at every pixel of both scales: the fp32 filter's error on mu is a few 1e-6 on these
    inputs (49 products of weights summing to 1 with |Y - shift| of order 50, unit roundoff 6e-8)."""
    for y0, _, y1, _ in _ref_planes(name):
        for y in (y0, y1):
            assert np.abs(y - R.mscn(y)[1]).min() > SIGN_GAP


def _device(name):
    from rdeic_amd import metrics
    block, imgs = _case(name)
    return metrics.nr_moments(torch.from_numpy(imgs).cuda(), block, planes=True)


def _worst(got, want, floor):
    d = np.abs(np.asarray(got, dtype=np.float64) - want)
    return float(d.max()), float((d / np.maximum(np.abs(want), floor)).max())


@pytest.mark.parametrize("name", ["crop200x296", "block96", "plane100", "smooth100"])
def test_planes_match_the_reference(gpu, name):
    _, _, v = _device(name)
    for i, (y0, m0, y1, m1) in enumerate(_ref_planes(name)):
        assert v["y0"].shape[1:] == y0.shape and v["y1"].shape[1:] == y1.shape
        assert np.array_equal(v["y0"][i].cpu().numpy(), y0)  # integers: exact
        ay, ry = _worst(v["y1"][i].cpu().numpy(), y1, 1.0)
        a0, r0 = _worst(v["m0"][i].cpu().numpy(), m0, 1e-2)
        a1, r1 = _worst(v["m1"][i].cpu().numpy(), m1, 1e-2)
        print(f"\n[nr planes] {name}[{i}]: y1 abs {ay:.3e} rel {ry:.3e} | m0 abs {a0:.3e} rel {r0:.3e} | "
              f"m1 abs {a1:.3e} rel {r1:.3e}")
        assert np.array_equal(v["y1"][i].cpu().numpy(), y1)  # measured error 0: see the table above
        assert a0 <= ATOL_M and a1 <= ATOL_M


@pytest.mark.parametrize("h,w,block", [(100, 100, 0), (200, 296, 96)])
def test_constant_image_is_exact(gpu, h, w, block):
    from rdeic_amd import metrics
    m0, m1, v = metrics.nr_moments(torch.from_numpy(const_img(h, w)[None]).cuda(), block, planes=True)
    y = float(R.luma(const_img(1, 1))[0, 0])
    assert torch.all(v["m0"] == 0) and torch.all(v["m1"] == 0)
    assert torch.all(v["y0"] == y) and torch.all(v["y1"] == y)
    assert np.all(m0 == 0) and np.all(m1 == 0)


@pytest.mark.parametrize("name", ["batch192x288", "batch100"])
def test_moments_match_the_reference(gpu, name):
    d0, d1, _ = _device(name)
    refs = _ref_moments(name)
    _check_signs(name)
    assert d0.shape == (len(refs),) + refs[0][0].shape and d1.shape == d0.shape
    if name == "batch192x288":
        assert d0.shape == (2, 6, 5, 6)
    worst, counts = 0.0, True
    for i, (r0, r1) in enumerate(refs):
        for s, (got, want) in enumerate(((d0[i], r0), (d1[i], r1))):
            a, r = _worst(got[..., 2:], want[..., 2:], 1e-300)
            same = np.array_equal(got[..., :2], want[..., :2])
            print(f"\n[nr moments] {name}[{i}] scale {s}: sums abs {a:.3e} rel {r:.3e}, counts equal {same}")
            worst, counts = max(worst, r), counts and same
    assert counts  # n_neg, n_pos: exact
    assert worst <= RTOL_MOM
    # the circular shift stays inside a region: the restatement with the neighbour block's column instead differs
    if name == "batch192x288":
        m0 = _ref_planes(name)[0][1]
        leak = (m0 * np.roll(m0, (0, 1), axis=(0, 1)))[:96, 96:192]
        assert abs((leak * leak).sum() - refs[0][0][1, 1, 5]) > 10 * RTOL_MOM * refs[0][0][1, 1, 5]


def test_moments_are_deterministic(gpu):
    from rdeic_amd import metrics
    for name in ("batch192x288", "batch100"):
        block, imgs = _case(name)
        x = torch.from_numpy(imgs).cuda()
        a = metrics.nr_moments(x, block)
        b = metrics.nr_moments(x, block)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        # an image's moments do not depend on its batch either
        c = metrics.nr_moments(x[1:], block)
        assert np.array_equal(a[0][1:], c[0]) and np.array_equal(a[1][1:], c[1])


def _niqe_params():
    rng = np.random.default_rng(100)
    a = rng.standard_normal((36, 36))
    return rng.standard_normal(36) + 1.0, a @ a.T / 36.0 + np.eye(36)


def _svr():
    rng = np.random.default_rng(101)
    return {"sv": rng.uniform(-1.0, 1.0, (8, 36)), "sv_coef": rng.standard_normal(8) * 10.0, "rho": np.array(-30.0),
            "gamma": np.array(0.05), "scale_min": np.full(36, -0.5), "scale_max": np.full(36, 3.0)}


ALPHA_COLS = [0, 2, 6, 10, 14, 18, 20, 24, 28, 32]


def _check_margins(fits):
    mids = (R.RHO[1799] + R.RHO[1800]) / 2  # the cell at alpha = 2: why MARGIN cannot be 1e-4
    assert abs(R.RHO[1801] - R.RHO[1800]) / mids < 2e-4
    worst = min(R.decision_margin(v, table) for v, table in fits)
    print(f"\n[nr e2e] {len(fits)} fits, smallest decision margin {worst:.3e}")
    assert worst > MARGIN


def test_niqe_end_to_end(gpu, tmp_path):
    from rdeic_amd import metrics
    _, imgs = _case("niqe192")
    mu_p, cov_p = _niqe_params()
    fits = []
    want = [R.niqe(im, mu_p, cov_p, fits) for im in imgs]
    _check_margins(fits)
    _check_signs("niqe192")
    np.savez(tmp_path / "niqe.npz", mu_prisparam=mu_p, cov_prisparam=cov_p)
    x = torch.from_numpy(imgs).cuda()
    m0, m1 = metrics.nr_moments(x, 96)
    feat = np.concatenate([metrics.niqe_features(m0, 96 * 96), metrics.niqe_features(m1, 48 * 48)], axis=-1)
    for i, im in enumerate(imgs):
        ref_feat = R.niqe_block_features(im)
        assert np.array_equal(feat[i][:, ALPHA_COLS], ref_feat[:, ALPHA_COLS])  # every alpha, on the grid
    got = metrics.niqe(x, metrics.NIQE(str(tmp_path / "niqe.npz")))
    a, r = _worst(got, np.array(want), 1e-300)
    print(f"\n[nr e2e] niqe {got} ref {want}: abs {a:.3e} rel {r:.3e}")
    assert got.dtype == np.float64 and got.shape == (2,) and r <= RTOL_SCORE


def test_brisque_end_to_end(gpu, tmp_path):
    from rdeic_amd import metrics
    _, imgs = _case("brisque100")
    svr = _svr()
    fits = []
    want = [R.brisque(im, svr, fits) for im in imgs]
    _check_margins(fits)
    _check_signs("brisque100")
    np.savez(tmp_path / "brisque.npz", **svr)
    x = torch.from_numpy(imgs).cuda()
    m0, m1 = metrics.nr_moments(x, 0)
    feat = np.concatenate([metrics.brisque_features(m0[:, 0], 100 * 100), metrics.brisque_features(m1[:, 0], 50 * 50)],
                          axis=-1)
    for i, im in enumerate(imgs):
        assert np.array_equal(feat[i][ALPHA_COLS], R.brisque_features(im)[ALPHA_COLS])
    got = metrics.brisque(x, metrics.BRISQUE(str(tmp_path / "brisque.npz")))
    a, r = _worst(got, np.array(want), 1e-300)
    print(f"\n[nr e2e] brisque {got} ref {want}: abs {a:.3e} rel {r:.3e}")
    assert got.dtype == np.float64 and got.shape == (2,) and r <= RTOL_SCORE


def test_degenerate_inputs_end_cleanly(gpu, tmp_path):
    from rdeic_amd import metrics
    mu_p, cov_p = _niqe_params()
    np.savez(tmp_path / "niqe.npz", mu_prisparam=mu_p, cov_prisparam=cov_p)
    np.savez(tmp_path / "brisque.npz", **_svr())
    nm, bm = metrics.NIQE(str(tmp_path / "niqe.npz")), metrics.BRISQUE(str(tmp_path / "brisque.npz"))
    cases = {"constant": const_img(192, 192), "one block": noise_img(96, 96, 1), "no block": noise_img(64, 64, 2)}
    for what, img in cases.items():
        got = metrics.niqe(torch.from_numpy(img[None]).cuda(), nm)
        assert got.shape == (1,) and math.isnan(got[0]), what
        assert math.isnan(R.niqe(img, mu_p, cov_p)), what
    assert math.isnan(metrics.brisque(torch.from_numpy(const_img(64, 64)[None]).cuda(), bm)[0])
    assert math.isfinite(metrics.brisque(torch.from_numpy(cases["no block"][None]).cuda(), bm)[0])
    with pytest.raises(ValueError, match="even"):
        metrics.brisque(torch.from_numpy(noise_img(65, 64, 3)[None]).cuda(), bm)
    torch.cuda.synchronize()
