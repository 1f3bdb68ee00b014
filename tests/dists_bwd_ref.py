"""CPU autograd reference of the DISTS training loss: the float-input restatement of tests/dists_ref.py (DESIGN
§21) under torch autograd, generic in dtype, with the image pairs of tests/lpips_bwd_ref.float_pair. Shared by
tests/test_dists_bwd_cpu.py and tests/test_dists_bwd_gpu.py; plain torch, no device code.

The loss is piecewise smooth: a ReLU decision that differs between fp32 and fp64 is a jump of the gradient, not
rounding. The cases below are seeds for which the fp32 CPU restatement's own gradient stays within 5e-4 (relative
L2) of fp64, i.e. for which no such flip carries weight (test_dists_bwd_cpu.py)."""
from functools import lru_cache

import torch
import torch.nn.functional as F

from tests import dists_ref as R
from tests.lpips_bwd_ref import float_pair, rel_l2  # noqa: F401  (rel_l2 re-exported for the tests)

# (N, H, W, seed); the second has odd sides: the pools see 21 -> 11 -> 6 -> 3 -> 2 and 35 -> 18 -> 9 -> 5 -> 3
CASES = ((2, 32, 48, 0), (1, 21, 35, 0))
CPU_FP32_GRAD_BOUND = 5e-4
CPU_FP32_LOSS_BOUND = 1e-6
C1 = C2 = 1e-6


def prep_float(x_nchw: torch.Tensor):
    """[-1, 1] -> (raw, normalised): r = v * 0.5 + 0.5 (a multiply, then an add), then (r - mean_c) / std_c."""
    dtype = x_nchw.dtype
    mean = torch.tensor(R.MEAN, dtype=dtype)[None, :, None, None]
    std = torch.tensor(R.STD, dtype=dtype)[None, :, None, None]
    r = x_nchw * 0.5 + 0.5
    return r, (r - mean) / std


def taps_float(backbone: dict, x_nchw: torch.Tensor):
    """The six taps (NCHW) of float images in [-1, 1]: the image in [0, 1] itself, then the five stage outputs."""
    dtype = x_nchw.dtype
    r, h = prep_float(x_nchw)
    out = [r]
    for k, stage in enumerate(R.STAGES):
        if k:
            h = R.l2_pool(h)
        for i, _, _ in stage:
            w, b = backbone[f"features.{i}.weight"], backbone[f"features.{i}.bias"]
            h = F.relu(F.conv2d(h, w.to(dtype), b.to(dtype), stride=1, padding=1))
        out.append(h)
    return out


def tap_score(a: torch.Tensor, b: torch.Tensor, al: torch.Tensor, be: torch.Tensor) -> torch.Tensor:
    """[N]: sum_c al_c S1_c + be_c S2_c of two NCHW maps."""
    mx, my, vx, vy, cxy = R.moments(a, b)
    s1 = (2 * mx * my + C1) / (mx ** 2 + my ** 2 + C1)
    s2 = (2 * cxy + C2) / (vx + vy + C2)
    return (al[None] * s1 + be[None] * s2).sum(1)


def normalised(weights: dict, dtype):
    """(alpha, beta) per tap, normalised by the sum over all taps as the metric does."""
    alpha = torch.as_tensor(weights["alpha"]).reshape(-1).to(torch.float64)
    beta = torch.as_tensor(weights["beta"]).reshape(-1).to(torch.float64)
    wsum = alpha.sum() + beta.sum()
    return (torch.split((alpha / wsum).to(dtype), R.CHANNELS), torch.split((beta / wsum).to(dtype), R.CHANNELS))


def loss_and_grad(backbone: dict, weights: dict, pred: torch.Tensor, target: torch.Tensor, dtype):
    """(loss, d loss / d pred [n, h, w, 3]) in `dtype` under CPU autograd; loss = mean_n (1 - sum_k score_k)."""
    x = pred.to(dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    with torch.no_grad():
        f1 = taps_float(backbone, target.to(dtype).permute(0, 3, 1, 2))
    f0 = taps_float(backbone, x)
    als, bes = normalised(weights, dtype)
    val = 0
    for a, b, al, be in zip(f0, f1, als, bes):
        val = val + tap_score(a, b, al, be)
    loss = (1 - val).mean()
    loss.backward()
    return loss.detach(), x.grad.permute(0, 2, 3, 1).contiguous()


@lru_cache(maxsize=None)
def case(n: int, h: int, w: int, seed: int):
    """(pred, target, fp64 loss, fp64 gradient, fp32 CPU loss, fp32 CPU gradient) of one case; computed once."""
    pred, target = float_pair(n, h, w, seed)
    bb, wt = R.seeded_backbone(0), R.seeded_weights(0)
    l64, g64 = loss_and_grad(bb, wt, pred, target, torch.float64)
    l32, g32 = loss_and_grad(bb, wt, pred, target, torch.float32)
    return pred, target, l64, g64, l32, g32
