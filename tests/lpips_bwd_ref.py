"""CPU autograd reference of the LPIPS training loss (reference model/lpips.py:75-89 with inp_range (-1, 1)): the
restatement of tests/lpips_ref.py under torch autograd, in fp64 or fp32, and the image pairs and seeds the loss
tests use. Shared by tests/test_lpips_bwd_cpu.py and tests/test_lpips_bwd_gpu.py; plain torch, no device code.

The loss is piecewise smooth: a ReLU or max-pool decision that differs between fp32 and fp64 is a jump of the
gradient, not rounding. The cases below are seeds for which the fp32 CPU restatement's own gradient stays
within 1e-4 (relative L2) of fp64, i.e. for which no such flip carries weight (test_lpips_bwd_cpu.py)."""
from functools import lru_cache

import numpy as np
import torch

from tests import lpips_ref as R

# (net, N, H, W, seed)
CASES = {"alex": ("alex", 2, 64, 48, 0), "vgg": ("vgg", 1, 32, 48, 0)}
CPU_FP32_GRAD_BOUND = 1e-4


def float_pair(n: int, h: int, w: int, seed: int):
    """(prediction, target) fp32 [n, h, w, 3] in [-1, 1]: synthetic images, the prediction with N(0, 12/255) noise
    and off the uint8 grid."""
    ps, ts = [], []
    for i in range(n):
        p, t = R.noisy_pair(h, w, seed * 100 + i)
        ps.append(p)
        ts.append(t)
    g = torch.Generator().manual_seed(seed)
    pred = torch.from_numpy(np.stack(ps)).float() / 127.5 - 1.0
    pred = (pred + (torch.rand(pred.shape, generator=g) - 0.5) / 127.5).clamp(-1.0, 1.0)
    return pred.contiguous(), (torch.from_numpy(np.stack(ts)).float() / 127.5 - 1.0).contiguous()


def scaling_layer_float(x_nchw: torch.Tensor) -> torch.Tensor:
    dtype = x_nchw.dtype
    shift = torch.tensor(R.SHIFT, dtype=dtype)[None, :, None, None]
    scale = torch.tensor(R.SCALE, dtype=dtype)[None, :, None, None]
    return (x_nchw - shift) / scale


def loss_and_grad(net: str, backbone: dict, pred: torch.Tensor, target: torch.Tensor, dtype):
    """(loss, d loss / d pred [n, h, w, 3]) in `dtype` under CPU autograd; loss = mean_n sum_k score_k."""
    x = pred.to(dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    with torch.no_grad():
        f1 = R.taps(net, backbone, scaling_layer_float(target.to(dtype).permute(0, 3, 1, 2)))
    f0 = R.taps(net, backbone, scaling_layer_float(x))
    val = 0
    for a, b, lin in zip(f0, f1, R.lin_heads(net)):
        val = val + R.layer_distance(a, b, lin)
    loss = val.mean()
    loss.backward()
    return loss.detach(), x.grad.permute(0, 2, 3, 1).contiguous()


@lru_cache(maxsize=None)
def case(name: str):
    """(pred, target, fp64 loss, fp64 gradient, fp32 CPU loss, fp32 CPU gradient) of CASES[name]; computed once."""
    net, n, h, w, seed = CASES[name]
    pred, target = float_pair(n, h, w, seed)
    bb = R.seeded_backbone(net)
    l64, g64 = loss_and_grad(net, bb, pred, target, torch.float64)
    l32, g32 = loss_and_grad(net, bb, pred, target, torch.float32)
    return pred, target, l64, g64, l32, g32


def rel_l2(got: torch.Tensor, want: torch.Tensor) -> float:
    return float((got.double() - want.double()).norm() / want.double().norm())
