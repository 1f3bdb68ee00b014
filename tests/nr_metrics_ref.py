"""Float64 numpy restatement of the no-reference metrics (NIQE: Mittal, Soundararajan, Bovik 2013; BRISQUE: Mittal,
Moorthy, Bovik 2012) with the conventions the project fixes for them, written from the specification and not from
rdeic_amd/metrics.py or csrc/nr_metrics.hip: one image at a time, no shared helpers, every step spelled out.

    luma        Y = rint(255 * (0.299 r + 0.587 g + 0.114 b)), r, g, b in [0, 1]
    crop        NIQE: top-left floor(H/96)*96 x floor(W/96)*96; BRISQUE: the whole image (even H, W)
    MSCN        mu = G * Y, sigma = sqrt(|G * Y^2 - mu^2|), M = (Y - mu) / (sigma + 1); G = 7x7 Gaussian, sigma 7/6,
                sum 1, separable, replicate border
    half size   8 taps [-3 -9 29 111 111 29 -9 -3] / 256 on inputs 2i-3 .. 2i+4, symmetric reflection, vertical then
                horizontal, from the un-normalised Y of scale 0
    moments     per region (96x96 / 48x48 blocks, or the whole plane) and map (M, M * roll(M, d), d = (0,1), (1,0),
                (1,1), (1,-1), torch.roll semantics within the region): n_neg, n_pos, S_neg, S_pos, S_abs, S_sq
    AGGD / GGD  moment matching on the grid alpha = 0.2, 0.201, ..., 10.0
"""
import math

import numpy as np

TAPS = np.array([-3.0, -9.0, 29.0, 111.0, 111.0, 29.0, -9.0, -3.0]) / 256.0
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))
GRID = np.arange(200, 10001) / 1000.0


def cubic(x: float, a: float = -0.5) -> float:
    """Keys' cubic convolution kernel."""
    x = abs(x)
    if x <= 1.0:
        return (a + 2.0) * x ** 3 - (a + 3.0) * x ** 2 + 1.0
    if x < 2.0:
        return a * x ** 3 - 5.0 * a * x ** 2 + 8.0 * a * x - 4.0 * a
    return 0.0


def half_size_taps() -> np.ndarray:
    """Antialiased bicubic resize by 1/2: output i sits at input coordinate 2i + 0.5, the kernel is stretched by 2,
    so input 2i-3+k is at distance |k - 3.5| / 2 in kernel units: 1.75, 1.25, 0.75, 0.25, 0.25, ... ; normalised."""
    w = np.array([cubic((k - 3.5) / 2.0) for k in range(8)])
    return w / w.sum()


def luma(img_u8: np.ndarray) -> np.ndarray:
    x = img_u8.astype(np.float64) / 255.0
    return np.rint(255.0 * (0.299 * x[..., 0] + 0.587 * x[..., 1] + 0.114 * x[..., 2]))


def luma_ties(img_u8: np.ndarray) -> np.ndarray:
    """Pixels whose luma is exactly k + 0.5 before rounding ((299 r + 587 g + 114 b) mod 1000 == 500): there the
    rounding direction depends on the last bit of the arithmetic, so test images avoid them."""
    v = img_u8.astype(np.int64)
    return (299 * v[..., 0] + 587 * v[..., 1] + 114 * v[..., 2]) % 1000 == 500


def niqe_crop(y: np.ndarray) -> np.ndarray:
    return y[:y.shape[0] // 96 * 96, :y.shape[1] // 96 * 96]


def gaussian7() -> np.ndarray:
    d = np.arange(7) - 3.0
    g = np.exp(-d * d / (2.0 * (7.0 / 6.0) ** 2))
    return g / g.sum()


def gauss_filter(x: np.ndarray) -> np.ndarray:
    g = gaussian7()
    p = np.pad(x, 3, mode="edge")
    h, w = x.shape
    rows = np.zeros((h + 6, w))
    for k in range(7):
        rows += g[k] * p[:, k:k + w]
    out = np.zeros((h, w))
    for k in range(7):
        out += g[k] * rows[k:k + h, :]
    return out


def mscn(y: np.ndarray):
    """(M, mu, sigma) of a luma plane."""
    mu = gauss_filter(y)
    sigma = np.sqrt(np.abs(gauss_filter(y * y) - mu * mu))
    return (y - mu) / (sigma + 1.0), mu, sigma


def half_size(y: np.ndarray) -> np.ndarray:
    h, w = y.shape
    assert h % 2 == 0 and w % 2 == 0
    p = np.pad(y, ((3, 4), (0, 0)), mode="symmetric")  # -1 -> 0, -2 -> 1, H -> H-1, ...
    v = np.zeros((h // 2, w))
    for k in range(8):
        v += TAPS[k] * p[k:k + h:2, :]
    p = np.pad(v, ((0, 0), (3, 4)), mode="symmetric")
    out = np.zeros((h // 2, w // 2))
    for k in range(8):
        out += TAPS[k] * p[:, k:k + w:2]
    return out


def six_moments(x: np.ndarray) -> np.ndarray:
    neg, pos = x[x < 0], x[x > 0]
    return np.array([neg.size, pos.size, (neg * neg).sum(), (pos * pos).sum(), np.abs(x).sum(), (x * x).sum()])


def region_moments(m: np.ndarray, bh: int, bw: int) -> np.ndarray:
    """[regions, 5, 6], regions row-major; bh = bw = 0: the whole plane."""
    if bh == 0:
        bh, bw = m.shape
    out = []
    for by in range(m.shape[0] // bh):
        for bx in range(m.shape[1] // bw):
            blk = m[by * bh:(by + 1) * bh, bx * bw:(bx + 1) * bw]
            maps = [blk] + [blk * np.roll(blk, d, axis=(0, 1)) for d in SHIFTS]
            out.append([six_moments(q) for q in maps])
    return np.array(out, dtype=np.float64).reshape(-1, 5, 6)


def rho_table() -> np.ndarray:
    return np.array([math.exp(2.0 * math.lgamma(2.0 / a) - math.lgamma(1.0 / a) - math.lgamma(3.0 / a)) for a in GRID])


RHO = rho_table()
RHO_GGD = 1.0 / RHO


def grid_argmin(table: np.ndarray, target: float) -> int:
    best, best_k = float("inf"), -1
    for k in range(table.size):
        d = (table[k] - target) ** 2
        if d < best:
            best, best_k = d, k
    return best_k


def nearest_on_grid(table: np.ndarray, target: float, fits=None) -> float:
    """alpha = grid[argmin (table - target)^2]; NaN for a non-finite target. fits (a list) collects
    (target, table) of every finite fit, for the decision-margin check of the tests."""
    if not np.isfinite(target):
        return float("nan")
    if fits is not None:
        fits.append((float(target), table))
    return float(GRID[grid_argmin(table, float(target))])


def decision_margin(target: float, table: np.ndarray) -> float:
    """Distance of a fitted value from the nearest decision midpoint between grid neighbours, relative to the value."""
    mids = (table[:-1] + table[1:]) / 2.0
    return float(np.min(np.abs(mids - target)) / abs(target))


def aggd(mom: np.ndarray, n: float, fits=None):
    """(alpha, beta_l, beta_r, mean, l, r) from the six moments of n samples."""
    with np.errstate(divide="ignore", invalid="ignore"):
        l = np.sqrt(mom[2] / mom[0])
        r = np.sqrt(mom[3] / mom[1])
        g = l / r
        rhat = (mom[4] / n) ** 2 / (mom[5] / n)
        big_r = rhat * (g ** 3 + 1.0) * (g + 1.0) / (g ** 2 + 1.0) ** 2
    alpha = nearest_on_grid(RHO, big_r, fits)
    if not np.isfinite(alpha):
        nan = float("nan")
        return nan, nan, nan, nan, float(l), float(r)
    c = math.sqrt(math.exp(math.lgamma(1.0 / alpha) - math.lgamma(3.0 / alpha)))
    beta_l, beta_r = l * c, r * c
    mean = (beta_r - beta_l) * math.exp(math.lgamma(2.0 / alpha) - math.lgamma(1.0 / alpha))
    return alpha, float(beta_l), float(beta_r), float(mean), float(l), float(r)


def niqe_features_scale(mom: np.ndarray, n: float, fits=None) -> np.ndarray:
    """18 features of one block at one scale from its [5, 6] moments."""
    a, bl, br, _, _, _ = aggd(mom[0], n, fits)
    f = [a, (bl + br) / 2.0]
    for k in range(1, 5):
        a, bl, br, mean, _, _ = aggd(mom[k], n, fits)
        f += [a, mean, bl, br]
    return np.array(f)


def brisque_features_scale(mom: np.ndarray, n: float, fits=None) -> np.ndarray:
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = (mom[0][5] / n) / (mom[0][4] / n) ** 2
    f = [nearest_on_grid(RHO_GGD, ratio, fits), mom[0][5] / n]
    for k in range(1, 5):
        a, _, _, mean, l, r = aggd(mom[k], n, fits)
        f += [a, mean, l * l, r * r]
    return np.array(f)


def planes(img_u8: np.ndarray, crop: bool):
    """(Y0, M0, Y1, M1) of one image."""
    y0 = luma(img_u8)
    if crop:
        y0 = niqe_crop(y0)
    y1 = half_size(y0)
    return y0, mscn(y0)[0], y1, mscn(y1)[0]


def niqe_block_features(img_u8: np.ndarray, fits=None) -> np.ndarray:
    """[blocks, 36]."""
    _, m0, _, m1 = planes(img_u8, crop=True)
    r0, r1 = region_moments(m0, 96, 96), region_moments(m1, 48, 48)
    return np.array([np.concatenate([niqe_features_scale(r0[b], 96.0 * 96.0, fits),
                                     niqe_features_scale(r1[b], 48.0 * 48.0, fits)]) for b in range(r0.shape[0])])


def niqe(img_u8: np.ndarray, mu_p: np.ndarray, cov_p: np.ndarray, fits=None) -> float:
    if img_u8.shape[0] < 96 or img_u8.shape[1] < 96:
        return float("nan")
    feat = niqe_block_features(img_u8, fits)
    kept = np.array([f for f in feat if np.all(np.isfinite(f))])
    if kept.shape[0] < 2:
        return float("nan")
    mu_d = kept.sum(axis=0) / kept.shape[0]
    dev = kept - mu_d
    cov_d = dev.T @ dev / (kept.shape[0] - 1)
    d = mu_p - mu_d
    return float(np.sqrt(d @ np.linalg.pinv((cov_p + cov_d) / 2.0) @ d))


def brisque_features(img_u8: np.ndarray, fits=None) -> np.ndarray:
    _, m0, _, m1 = planes(img_u8, crop=False)
    return np.concatenate([brisque_features_scale(region_moments(m0, 0, 0)[0], float(m0.size), fits),
                           brisque_features_scale(region_moments(m1, 0, 0)[0], float(m1.size), fits)])


def brisque(img_u8: np.ndarray, svr: dict, fits=None) -> float:
    """svr: sv [n,36], sv_coef [n], rho, gamma, scale_min [36], scale_max [36]."""
    x = brisque_features(img_u8, fits)
    x = -1.0 + 2.0 * (x - svr["scale_min"]) / (svr["scale_max"] - svr["scale_min"])
    total = 0.0
    for i in range(svr["sv"].shape[0]):
        total += float(svr["sv_coef"][i]) * math.exp(-float(svr["gamma"]) * float(((x - svr["sv"][i]) ** 2).sum()))
    return total - float(svr["rho"])
