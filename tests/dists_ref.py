"""CPU restatement of the DISTS forward (Ding et al. 2020, as restated in DESIGN.md §21) in plain torch, generic
in dtype and used in float64. It takes the backbone dict (torchvision keys, features.<i>.*) and the alpha / beta
the device class takes. Shared by tests/test_dists_cpu.py and tests/test_dists_gpu.py; no device code."""
from functools import lru_cache

import numpy as np
import torch
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
CHANNELS = (3, 64, 128, 256, 512, 512)
# the torchvision VGG16 `features` convs per stage, restated here independently of rdeic_amd's table:
# (features index, cin, cout); 3x3, stride 1, pad 1, ReLU after each; an L2 pool before stages 2..5
STAGES = (((0, 3, 64), (2, 64, 64)), ((5, 64, 128), (7, 128, 128)), ((10, 128, 256), (12, 256, 256), (14, 256, 256)),
          ((17, 256, 512), (19, 512, 512), (21, 512, 512)), ((24, 512, 512), (26, 512, 512), (28, 512, 512)))


def seeded_backbone(seed: int = 0, layout: str = "torchvision") -> dict:
    """He-scaled normal weights, small normal biases from a seeded generator (rdeic_amd.lpips.seeded_backbone's
    scheme), keyed features.<i>.* (torchvision), net.slice<k>.<i>.* (lpips) or stage<k>.<i>.* (single file)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, stage in enumerate(STAGES, 1):
        for i, cin, cout in stage:
            name = {"torchvision": f"features.{i}", "lpips": f"net.slice{k}.{i}", "stage": f"stage{k}.{i}"}[layout]
            sd[f"{name}.weight"] = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (cin * 9)) ** 0.5
            sd[f"{name}.bias"] = torch.randn((cout,), generator=g) * 0.05
    return sd


def seeded_weights(seed: int = 0) -> dict:
    """alpha, beta [1, 1475, 1, 1] from N(0.1, 0.01)."""
    g = torch.Generator().manual_seed(seed)
    n = sum(CHANNELS)
    return {"alpha": 0.1 + 0.01 * torch.randn((1, n, 1, 1), generator=g),
            "beta": 0.1 + 0.01 * torch.randn((1, n, 1, 1), generator=g)}


def l2_pool(x: torch.Tensor) -> torch.Tensor:
    """NCHW: sqrt(depthwise_conv(x * x, g, stride 2, padding 1) + 1e-12), g = hanning(5)[1:-1] outer, normalised."""
    a = torch.tensor(np.hanning(5)[1:-1], dtype=x.dtype)
    g = a[:, None] * a[None, :]
    g = (g / g.sum())[None, None].repeat(x.shape[1], 1, 1, 1)
    return torch.sqrt(F.conv2d(x * x, g, stride=2, padding=1, groups=x.shape[1]) + 1e-12)


def taps(backbone: dict, img_u8: np.ndarray, dtype=torch.float64):
    """The six taps (NCHW) of uint8 [N,H,W,3] images: the image in [0, 1] itself, then the five stage outputs."""
    x = torch.from_numpy(np.ascontiguousarray(img_u8)).to(dtype).permute(0, 3, 1, 2) / 255
    out = [x]
    mean = torch.tensor(MEAN, dtype=dtype)[None, :, None, None]
    std = torch.tensor(STD, dtype=dtype)[None, :, None, None]
    h = (x - mean) / std
    for k, stage in enumerate(STAGES):
        if k:
            h = l2_pool(h)
        for i, _, _ in stage:
            w, b = backbone[f"features.{i}.weight"], backbone[f"features.{i}.bias"]
            h = F.relu(F.conv2d(h, w.to(dtype), b.to(dtype), stride=1, padding=1))
        out.append(h)
    return out


def moments(x: torch.Tensor, y: torch.Tensor):
    """NCHW maps -> (mx, my, vx, vy, cxy), each [N, C], biased, over all pixels."""
    mx, my = x.mean([2, 3], keepdim=True), y.mean([2, 3], keepdim=True)
    vx, vy = ((x - mx) ** 2).mean([2, 3]), ((y - my) ** 2).mean([2, 3])
    cxy = (x * y).mean([2, 3]) - mx[:, :, 0, 0] * my[:, :, 0, 0]
    return mx[:, :, 0, 0], my[:, :, 0, 0], vx, vy, cxy


@torch.no_grad()
def dists(backbone: dict, weights: dict, pred_u8: np.ndarray, target_u8: np.ndarray, dtype=torch.float64) -> np.ndarray:
    """[N] scores of uint8 [N,H,W,3] arrays, computed in `dtype`."""
    c1 = c2 = 1e-6
    alpha = torch.as_tensor(weights["alpha"]).reshape(-1).to(dtype)
    beta = torch.as_tensor(weights["beta"]).reshape(-1).to(dtype)
    wsum = alpha.sum() + beta.sum()
    f0, f1 = taps(backbone, pred_u8, dtype), taps(backbone, target_u8, dtype)
    d1 = d2 = 0
    for a, b, al, be in zip(f0, f1, torch.split(alpha / wsum, CHANNELS), torch.split(beta / wsum, CHANNELS)):
        mx, my, vx, vy, cxy = moments(a, b)
        s1 = (2 * mx * my + c1) / (mx ** 2 + my ** 2 + c1)
        s2 = (2 * cxy + c2) / (vx + vy + c2)
        d1 = d1 + (al[None] * s1).sum(1)
        d2 = d2 + (be[None] * s2).sum(1)
    return (1 - (d1 + d2)).double().numpy()


@lru_cache(maxsize=None)
def pairs(h: int, w: int):
    """(pred [4], target [4]) uint8: a noisy copy, an unrelated image, a flat grey target, black against black."""
    from rdeic_amd.synthetic import synth_image
    a, other = synth_image(h, w, 11), synth_image(h, w, 12)
    rng = np.random.default_rng(11)
    noisy = np.clip(a.astype(np.float64) + rng.normal(0, 12.0, a.shape), 0, 255).astype(np.uint8)
    grey, black = np.full_like(a, 128), np.zeros_like(a)
    return np.stack([noisy, other, a, black]), np.stack([a, a, grey, black])
