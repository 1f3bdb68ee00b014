"""CPU restatement of the reference's LPIPS forward (model/lpips.py:75-89, 108-126, 142-232) with the backbone
passed in, runnable in fp32 and fp64, plus the seeded test backbone. Shared by tests/test_lpips_cpu.py and
tests/test_lpips_gpu.py; plain torch, no device code."""
import os
from functools import lru_cache

import numpy as np
import torch
import torch.nn.functional as F

from rdeic_amd import lpips as L

LIN_NPZ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lpips_lin.npz")
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)


# the torchvision feature stacks, restated here independently of rdeic_amd/lpips.py's table:
# (features index, lpips-package slice, cin, cout, kernel, stride, pad)
ALEX_CONVS = ((0, 1, 3, 64, 11, 4, 2), (3, 2, 64, 192, 5, 1, 2), (6, 3, 192, 384, 3, 1, 1), (8, 4, 384, 256, 3, 1, 1),
              (10, 5, 256, 256, 3, 1, 1))
VGG_CONVS = tuple((i, k, cin, cout, 3, 1, 1) for i, k, cin, cout in (
    (0, 1, 3, 64), (2, 1, 64, 64), (5, 2, 64, 128), (7, 2, 128, 128), (10, 3, 128, 256), (12, 3, 256, 256),
    (14, 3, 256, 256), (17, 4, 256, 512), (19, 4, 512, 512), (21, 4, 512, 512), (24, 5, 512, 512), (26, 5, 512, 512),
    (28, 5, 512, 512)))
CONVS = {"alex": ALEX_CONVS, "vgg": VGG_CONVS}
# features modules in order: c = conv + ReLU, t = tap, pK = max pool K / 2
PLAN = {"alex": "c t p3 c t p3 c t c t c t".split(),
        "vgg": "c c t p2 c c t p2 c c c t p2 c c c t p2 c c c t".split()}


def seeded_backbone(net: str, seed: int = 0, layout: str = "torchvision") -> dict:
    """He-scaled normal weights, small normal biases from a seeded generator, keyed as the torchvision
    state dict (features.<i>.*) or the lpips package's (net.slice<k>.<i>.*)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, k, cin, cout, ks, _, _ in CONVS[net]:
        name = f"features.{i}" if layout == "torchvision" else f"net.slice{k}.{i}"
        sd[f"{name}.weight"] = torch.randn((cout, cin, ks, ks), generator=g) * (2.0 / (cin * ks * ks)) ** 0.5
        sd[f"{name}.bias"] = torch.randn((cout,), generator=g) * 0.05
    return sd


@lru_cache(maxsize=None)
def lin_heads(net: str):
    return tuple(L.load_lin(net, LIN_NPZ))


def scaling_layer(img_u8: np.ndarray, dtype) -> torch.Tensor:
    """uint8 [N,H,W,3] -> NCHW ScalingLayer output for inputs in [0, 1] (mean 0.5, std 0.5: x * 2 - 1)."""
    x = torch.from_numpy(np.ascontiguousarray(img_u8)).to(dtype).permute(0, 3, 1, 2) / 255
    x = x * 2 - 1
    shift = torch.tensor(SHIFT, dtype=dtype)[None, :, None, None]
    scale = torch.tensor(SCALE, dtype=dtype)[None, :, None, None]
    return (x - shift) / scale


def taps(net: str, backbone: dict, x: torch.Tensor):
    """The five post-ReLU taps (NCHW) of the torchvision feature stack; backbone keyed features.<i>.*"""
    out, ci = [], 0
    for op in PLAN[net]:
        if op == "c":
            i, _, _, _, _, s, p = CONVS[net][ci]
            w, b = backbone[f"features.{i}.weight"], backbone[f"features.{i}.bias"]
            x = F.relu(F.conv2d(x, w.to(x.dtype), b.to(x.dtype), stride=s, padding=p))
            ci += 1
        elif op == "t":
            out.append(x)
        else:
            x = F.max_pool2d(x, kernel_size=int(op[1]), stride=2)
    return out


def normalize_tensor(x: torch.Tensor, eps: float = 1e-10) -> torch.Tensor:
    return x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + eps)


def layer_distance(f0: torch.Tensor, f1: torch.Tensor, lin: torch.Tensor) -> torch.Tensor:
    """NCHW taps -> [N]: spatial_average(lin(normalize(f0) - normalize(f1))^2)."""
    d = (normalize_tensor(f0) - normalize_tensor(f1)) ** 2
    return (d * lin.to(d.dtype)[None, :, None, None]).sum(1).mean([1, 2])


@torch.no_grad()
def lpips(net: str, backbone, pred_u8: np.ndarray, target_u8: np.ndarray, dtype=torch.float64) -> np.ndarray:
    """[N] scores of uint8 [N,H,W,3] arrays, computed in `dtype`."""
    f0 = taps(net, backbone, scaling_layer(pred_u8, dtype))
    f1 = taps(net, backbone, scaling_layer(target_u8, dtype))
    val = 0
    for a, b, lin in zip(f0, f1, lin_heads(net)):
        val = val + layer_distance(a, b, lin)
    return val.double().numpy()


def noisy_pair(h: int, w: int, seed: int, sigma: float = 12.0):
    """(prediction, target): synth_image plus N(0, sigma^2) noise, and the image itself."""
    from rdeic_amd.synthetic import synth_image
    a = synth_image(h, w, seed)
    rng = np.random.default_rng(seed)
    b = np.clip(a.astype(np.float64) + rng.normal(0, sigma, a.shape), 0, 255).astype(np.uint8)
    return b, a
