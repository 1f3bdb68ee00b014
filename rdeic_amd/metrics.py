"""Full-reference image quality of reconstructions on the device (rdeic_image_ssim, image_mse):
PSNR, SSIM and MS-SSIM as the reference's evaluation scripts report them
(experiments/run_robustness.py:40-93, inference_partition.py:28-70 via pyiqa "psnr" / "ssim" /
"ms_ssim" with test_y_channel). pyiqa is not in this image: SSIM / MS-SSIM follow the published
definition (Wang et al. 2004; Wang, Simoncelli, Bovik 2003) with pyiqa's defaults — YIQ luma,
11x11 Gaussian sigma 1.5, 'valid' windows, relu'd contrast-structure term, 5 scales — and are
checked against the CPU restatement in oracle/metrics_ref.py; parity with pyiqa itself is unpinned.
LPIPS (pyiqa "lpips": AlexNet, v0.1, inputs in [0, 1]) runs on the device too (rdeic_amd/lpips.py) with a
backbone state dict the caller supplies; no backbone weights ship with the project."""
from __future__ import annotations

import os
from typing import Tuple

import numpy as np
import torch

from . import _lib, ops

MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def psnr(pred_u8: torch.Tensor, target_u8: torch.Tensor) -> np.ndarray:
    """Per-image PSNR in dB of uint8 [N,H,W,3] device tensors (10 log10(255^2 / MSE))."""
    n = pred_u8.shape[0]
    mse = torch.empty(n, dtype=torch.float32, device=pred_u8.device)
    ops.call("rdeic_image_mse", target_u8.contiguous().data_ptr(), pred_u8.contiguous().data_ptr(), n,
             pred_u8[0].numel(), mse.data_ptr(), ops.stream_ptr())
    m = mse.cpu().numpy().astype(np.float64)
    with np.errstate(divide="ignore"):
        return np.where(m > 0, 10.0 * np.log10(255.0 ** 2 / np.maximum(m, 1e-30)), 100.0)


def ssim_levels(pred_u8: torch.Tensor, target_u8: torch.Tensor, levels: int = 5) -> np.ndarray:
    """[N, levels, 2] (mean SSIM, mean cs) per scale, on the device."""
    if pred_u8.shape != target_u8.shape or pred_u8.dim() != 4 or pred_u8.shape[3] != 3:
        raise ValueError("expected matching uint8 [N, H, W, 3] images")
    n, h, w, _ = pred_u8.shape
    nf = int(_lib.load().rdeic_image_ssim_ws_floats(n, h, w, levels))
    ws = torch.empty(nf, dtype=torch.float32, device=pred_u8.device)
    out = torch.empty((n, levels, 2), dtype=torch.float32, device=pred_u8.device)
    ops.call("rdeic_image_ssim", pred_u8.contiguous().data_ptr(), target_u8.contiguous().data_ptr(), n, h, w, levels,
             ws.data_ptr(), nf, out.data_ptr(), ops.stream_ptr())
    return out.cpu().numpy().astype(np.float64)


def ssim_ms_ssim(pred_u8: torch.Tensor, target_u8: torch.Tensor) -> Tuple[np.ndarray, np.ndarray]:
    """(SSIM [N], MS-SSIM [N]) of uint8 [N,H,W,3] device images (H, W >= 176 for 5 scales)."""
    lv = ssim_levels(pred_u8, target_u8, len(MS_SSIM_WEIGHTS))
    w = np.asarray(MS_SSIM_WEIGHTS)
    ms = np.prod(lv[:, :-1, 1] ** w[:-1], axis=1) * lv[:, -1, 0] ** w[-1]
    return lv[:, 0, 0], ms


def lpips(pred_u8: torch.Tensor, target_u8: torch.Tensor, model) -> np.ndarray:
    """Per-image LPIPS [N] (float64) of uint8 [N,H,W,3] device tensors; model: an rdeic_amd.lpips.LPIPS."""
    return model(pred_u8, target_u8)


def dists(pred_u8: torch.Tensor, target_u8: torch.Tensor, model) -> np.ndarray:
    """Per-image DISTS [N] (float64) of uint8 [N,H,W,3] device tensors; model: an rdeic_amd.dists.DISTS."""
    return model(pred_u8, target_u8)


def fid_kid(pred_u8_batches, target_u8_batches, tower, patch: int = 256, **kw) -> dict:
    """FID and KID between reconstructions and originals (matching iterables of uint8 [n,H,W,3] batches) through
    the patch protocol; tower: an rdeic_amd.fid.InceptionV3. Keys: n_images, n_patches, fid, kid_mean, kid_std."""
    from . import fid as _fid
    return _fid.fid_kid(pred_u8_batches, target_u8_batches, tower, patch=patch, **kw)


# ------------------------------------------------------------------ no-reference metrics (NIQE, BRISQUE)
# The reference's experiments/run_ood.py:93-127 scores reconstructions with pyiqa "niqe" / "brisque". pyiqa and its
# model files are not in this image: the published algorithms (Mittal, Soundararajan, Bovik 2013; Mittal, Moorthy,
# Bovik 2012) are restated — the per-pixel passes and region moments on the device (csrc/nr_metrics.hip), the AGGD
# fits and the scores below in float64 — and checked against tests/nr_metrics_ref.py; parity with pyiqa itself is
# unpinned. The model parameters come from a file the caller names; none ships with the project.
NIQE_BLOCK = 96
ALPHA_GRID = np.arange(200, 10001) / 1000.0  # 0.2, 0.201, ..., 10.0


def _gamma_tables():
    from scipy.special import gammaln
    g1, g2, g3 = gammaln(1.0 / ALPHA_GRID), gammaln(2.0 / ALPHA_GRID), gammaln(3.0 / ALPHA_GRID)
    return g1, g2, g3, np.exp(2.0 * g2 - g1 - g3)  # rho(a) = Gamma(2/a)^2 / (Gamma(1/a) Gamma(3/a))


_LG1, _LG2, _LG3, _RHO = _gamma_tables()
_RHO_GGD = 1.0 / _RHO  # Gamma(1/a) Gamma(3/a) / Gamma(2/a)^2
assert np.all(np.diff(_RHO) > 0) and np.all(np.diff(_RHO_GGD) < 0)  # _grid_argmin bisects


def _grid_argmin(table: np.ndarray, target: np.ndarray) -> np.ndarray:
    """Index of the grid point whose table value is nearest to each target (first on ties); -1 where the
    target is not finite."""
    flat = np.asarray(target, dtype=np.float64).reshape(-1)
    idx = np.full(flat.shape, -1, dtype=np.int64)
    ok = np.isfinite(flat)
    # both tables are strictly monotone over the grid (asserted below), so the argmin over all 9801 points is one of
    # the two neighbours a bisection finds; squared distances compared as the full scan would, first index on ties
    down = table[0] > table[-1]
    asc = table[::-1] if down else table
    hi = np.clip(np.searchsorted(asc, flat[ok]), 1, asc.size - 1)
    lo = hi - 1
    if down:
        lo, hi = asc.size - 1 - hi, asc.size - 1 - lo
    idx[ok] = np.where((table[hi] - flat[ok]) ** 2 < (table[lo] - flat[ok]) ** 2, hi, lo)
    return idx.reshape(np.shape(target))


def aggd_fit(mom: np.ndarray, count: float):
    """Asymmetric generalised Gaussian fit from the six moments [..., 6] = (n_neg, n_pos, S_neg, S_pos, S_abs,
    S_sq) of `count` samples. Returns (alpha, beta_l, beta_r, mean, l, r), each [...]; NaN where a side is empty."""
    mom = np.asarray(mom, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        l = np.sqrt(mom[..., 2] / mom[..., 0])
        r = np.sqrt(mom[..., 3] / mom[..., 1])
        g = l / r
        rhat = (mom[..., 4] / count) ** 2 / (mom[..., 5] / count)
        R = rhat * (g ** 3 + 1) * (g + 1) / (g ** 2 + 1) ** 2
        idx = _grid_argmin(_RHO, R)
        bad = idx < 0
        k = np.where(bad, 0, idx)
        alpha = np.where(bad, np.nan, ALPHA_GRID[k])
        c = np.exp(0.5 * (_LG1[k] - _LG3[k]))  # sqrt(Gamma(1/alpha) / Gamma(3/alpha))
        beta_l, beta_r = l * c, r * c
        mean = (beta_r - beta_l) * np.exp(_LG2[k] - _LG1[k])
    return alpha, beta_l, beta_r, mean, l, r


def ggd_alpha(mom: np.ndarray, count: float) -> np.ndarray:
    """Generalised Gaussian shape from the moments of M: the grid point whose Gamma(1/a) Gamma(3/a) / Gamma(2/a)^2
    is nearest to (S_sq / n) / (S_abs / n)^2."""
    mom = np.asarray(mom, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = (mom[..., 5] / count) / (mom[..., 4] / count) ** 2
    idx = _grid_argmin(_RHO_GGD, ratio)
    return np.where(idx < 0, np.nan, ALPHA_GRID[np.where(idx < 0, 0, idx)])


def nr_moments(pred_u8: torch.Tensor, block: int, planes: bool = False):
    """Region moments of uint8 [N,H,W,3] device images: two float64 arrays [N, regions, 5, 6] (scale 0, scale 1).
    block = 96: the 96x96 / 48x48 blocks of the top-left crop to multiples of 96 (NIQE); block = 0: the whole plane
    (BRISQUE; H and W even). planes=True also returns {"y0", "m0", "y1", "m1"}: the luma and MSCN planes of the
    crop and of its half-size plane, float32 device tensors [N, h, w]."""
    if pred_u8.dim() != 4 or pred_u8.shape[3] != 3 or pred_u8.dtype != torch.uint8:
        raise ValueError("expected uint8 [N, H, W, 3] images")
    n, h, w, _ = pred_u8.shape
    if block == 0 and (h % 2 or w % 2):
        raise ValueError(f"whole-plane moments need even H and W for the half-size plane, got {h}x{w}")
    nf = int(_lib.load().rdeic_nr_moments_ws_floats(n, h, w, block))
    if nf == 0:
        raise ValueError(f"no region of block {block} in {n} images of {h}x{w}")
    hc, wc = ((h // block) * block, (w // block) * block) if block else (h, w)
    regions = (hc // block) * (wc // block) if block else 1
    ws = torch.empty(nf, dtype=torch.float32, device=pred_u8.device)
    out = torch.empty((2, n, regions, 5, 6), dtype=torch.float64, device=pred_u8.device)
    ops.call("rdeic_nr_moments", pred_u8.contiguous().data_ptr(), n, h, w, block, ws.data_ptr(), nf,
             out[0].data_ptr(), out[1].data_ptr(), ops.stream_ptr())
    res = out.cpu().numpy()
    if not planes:
        return res[0], res[1]
    p, q = n * hc * wc, n * (hc // 2) * (wc // 2)
    views = {"y0": ws[:p].view(n, hc, wc), "m0": ws[p:2 * p].view(n, hc, wc),
             "y1": ws[2 * p:2 * p + q].view(n, hc // 2, wc // 2),
             "m1": ws[2 * p + q:2 * p + 2 * q].view(n, hc // 2, wc // 2)}
    return res[0], res[1], views


def _load_arrays(path: str, keys) -> dict:
    """The named arrays of a .npz, .safetensors or .mat file, float64."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npz":
        with np.load(path) as z:
            have = {k: z[k] for k in z.files}
    elif ext == ".safetensors":
        from safetensors.numpy import load_file
        have = load_file(path)
    elif ext == ".mat":
        from scipy.io import loadmat
        have = {k: v for k, v in loadmat(path).items() if not k.startswith("__")}
    else:
        raise ValueError(f"{path}: expected a .npz, .safetensors or .mat file")
    missing = [k for k in keys if k not in have]
    if missing:
        raise KeyError(f"{path}: missing {', '.join(missing)} (has {', '.join(sorted(have)) or 'nothing'})")
    return {k: np.asarray(have[k], dtype=np.float64) for k in keys}


class NIQE:
    """The pristine multivariate Gaussian of NIQE: mu_prisparam (36) and cov_prisparam (36x36) from the published
    niqe_modelparameters.mat, or a .npz / .safetensors file with the same keys."""

    def __init__(self, model_path: str):
        a = _load_arrays(model_path, ("mu_prisparam", "cov_prisparam"))
        self.mu = a["mu_prisparam"].reshape(-1)
        self.cov = a["cov_prisparam"]
        if self.mu.shape != (36,) or self.cov.shape != (36, 36):
            raise ValueError(f"{model_path}: mu_prisparam {a['mu_prisparam'].shape} / cov_prisparam {self.cov.shape}, "
                             "expected 36 and 36x36")


class BRISQUE:
    """The epsilon-SVR (RBF kernel) of BRISQUE from a .npz / .safetensors file: sv [n,36], sv_coef [n], rho, gamma,
    and the per-dimension feature range scale_min / scale_max [36] mapped to [-1, 1]. No SVR numbers are built in."""

    def __init__(self, model_path: str):
        a = _load_arrays(model_path, ("sv", "sv_coef", "rho", "gamma", "scale_min", "scale_max"))
        self.sv, self.sv_coef = a["sv"], a["sv_coef"].reshape(-1)
        self.rho, self.gamma = float(a["rho"].reshape(-1)[0]), float(a["gamma"].reshape(-1)[0])
        self.scale_min, self.scale_max = a["scale_min"].reshape(-1), a["scale_max"].reshape(-1)
        if self.sv.ndim != 2 or self.sv.shape[1] != 36 or self.sv_coef.shape != (self.sv.shape[0],) or \
                self.scale_min.shape != (36,) or self.scale_max.shape != (36,):
            raise ValueError(f"{model_path}: sv {self.sv.shape}, sv_coef {self.sv_coef.shape}, scale_min "
                             f"{self.scale_min.shape}, scale_max {self.scale_max.shape}; expected [n,36], [n], 36, 36")

    def score(self, feat: np.ndarray) -> np.ndarray:
        x = -1.0 + 2.0 * (feat - self.scale_min) / (self.scale_max - self.scale_min)
        d2 = ((x[:, None, :] - self.sv[None, :, :]) ** 2).sum(-1)
        return (self.sv_coef[None, :] * np.exp(-self.gamma * d2)).sum(-1) - self.rho


def niqe_features(mom: np.ndarray, count: float) -> np.ndarray:
    """[..., 18] NIQE features of one scale from moments [..., 5, 6]: (alpha, (beta_l + beta_r) / 2) of M, then
    (alpha, mean, beta_l, beta_r) of each product map."""
    a, bl, br, mean, _, _ = aggd_fit(mom, count)
    cols = [a[..., 0], (bl[..., 0] + br[..., 0]) / 2]
    for k in range(1, 5):
        cols += [a[..., k], mean[..., k], bl[..., k], br[..., k]]
    return np.stack(cols, axis=-1)


def brisque_features(mom: np.ndarray, count: float) -> np.ndarray:
    """[..., 18] BRISQUE features of one scale from whole-plane moments [..., 5, 6]: (GGD alpha, S_sq / n) of M,
    then (alpha, mean, l^2, r^2) of each product map."""
    a, _, _, mean, l, r = aggd_fit(mom, count)
    cols = [ggd_alpha(mom[..., 0, :], count), mom[..., 0, 5] / count]
    for k in range(1, 5):
        cols += [a[..., k], mean[..., k], l[..., k] ** 2, r[..., k] ** 2]
    return np.stack(cols, axis=-1)


def niqe_score(feat: np.ndarray, model: NIQE) -> float:
    """NIQE distance of one image's block features [blocks, 36]; NaN with fewer than 2 finite blocks."""
    kept = feat[np.isfinite(feat).all(axis=1)]
    if kept.shape[0] < 2:
        return float("nan")
    mu_d = kept.mean(axis=0)
    cov_d = np.cov(kept, rowvar=False)  # unbiased
    d = model.mu - mu_d
    return float(np.sqrt(d @ np.linalg.pinv((model.cov + cov_d) / 2) @ d))


def niqe(pred_u8: torch.Tensor, model: NIQE) -> np.ndarray:
    """Per-image NIQE [N] (float64) of uint8 [N,H,W,3] device images (lower is better). Images with fewer than two
    96x96 blocks, or fewer than two blocks with finite features, score NaN."""
    n, h, w, _ = pred_u8.shape
    if h < NIQE_BLOCK or w < NIQE_BLOCK:
        return np.full(n, np.nan)
    m0, m1 = nr_moments(pred_u8, NIQE_BLOCK)
    feat = np.concatenate([niqe_features(m0, NIQE_BLOCK ** 2), niqe_features(m1, (NIQE_BLOCK // 2) ** 2)], axis=-1)
    return np.array([niqe_score(feat[i], model) for i in range(n)], dtype=np.float64)


def brisque(pred_u8: torch.Tensor, model: BRISQUE) -> np.ndarray:
    """Per-image BRISQUE [N] (float64) of uint8 [N,H,W,3] device images (lower is better); H and W even
    (ValueError otherwise: the half-size plane is defined for an exact factor of 2)."""
    n, h, w, _ = pred_u8.shape
    m0, m1 = nr_moments(pred_u8, 0)
    feat = np.concatenate([brisque_features(m0[:, 0], h * w), brisque_features(m1[:, 0], (h // 2) * (w // 2))],
                          axis=-1)
    with np.errstate(invalid="ignore"):
        return model.score(feat)
