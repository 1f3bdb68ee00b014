"""DISTS (Ding, Ma, Wang, Simoncelli 2020) on the device: the metric, and the training loss DISTS.loss with its
backward (float images in [-1, 1], gradient to the prediction; the kernels' formulas are in DESIGN §25).

The network is the VGG16 feature stack LPIPS("vgg") runs (the library's fp32 convs, ReLU in the epilogue), with
an L2 Hanning pool where VGG has its max pools, the input image itself as a sixth (first) tap, and per tap and
channel two SSIM-like ratios of the global means, variances and covariance, weighted by the learned `alpha` and
`beta` (1475 values each). Four kernels of dists.hip sit around the convs: the prep (uint8 -> the raw v / 255
tap and the ImageNet-normalised conv input, both fp32 NHWC with a zero fourth channel), the L2 pool, the
two-pass channel moments in fp64 and the per-tap score.

No weights ship with the project: the caller passes `alpha` / `beta` (.pt / .pth / .npz, or a dict) and the
torchvision VGG16 state dict (``features.<i>.*``), the lpips package's, or a weights file that carries the convs
itself as ``stage<k>.<i>.*``. The computation is pinned against an fp64 restatement of the published algorithm
with a seeded backbone and seeded weights (tests/dists_ref.py); parity with pyiqa, DISTS_pytorch, the published
alpha / beta and torchvision's weights is unpinned, none of them is available offline.

Scores are batch-invariant bit for bit: split-K is pinned off for the backbone convs, every conv output element
is one fixed-order k sum, the pool is element-wise, and the moment kernels' partial grid depends on the tap shape
only. The batch is therefore chunked freely (chunk_pairs) to keep every activation tensor under 2^31 bytes.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib, lpips as _lpips, ops, tower

CHANNELS = (3, 64, 128, 256, 512, 512)  # per tap; the image itself first
N_WEIGHTS = sum(CHANNELS)  # 1475
MAX_TENSOR_BYTES = tower.MAX_TENSOR_BYTES
MAX_PAIRS = 32768  # per launch: rdeic_dists_moments takes at most 65535 images
_TABLE = _lpips.NETS["vgg"]  # ("conv", ...) / ("pool", 2, 2) / ("tap",): the pools become L2 pools here


def activation_shapes(h: int, w: int) -> List[Tuple[int, int, int]]:
    """(h, w, c) of every activation tensor of one image: the two 4-channel prep outputs (raw, normalised), then
    every conv and L2-pool output in forward order. The pools halve with ceil: (h + 2 - 3) // 2 + 1."""
    if h < 1 or w < 1:
        raise ValueError(f"DISTS needs a non-empty image, got {h}x{w}")
    shapes, c = [(h, w, 4), (h, w, 4)], 4
    for op in _TABLE:
        if op[0] == "conv":
            c = op[2]  # 3x3, stride 1, pad 1: the size stays
        elif op[0] == "pool":
            h, w = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
        else:
            continue
        shapes.append((h, w, c))
    return shapes


def tap_shapes(h: int, w: int) -> List[Tuple[int, int, int]]:
    """(h, w, c) of the six taps; tap 0 is the 4-channel raw image (3 channels used)."""
    acts, taps, i = activation_shapes(h, w), [], 1
    taps.append(acts[0])
    for op in _TABLE:
        if op[0] == "tap":
            taps.append(acts[i])
        else:
            i += 1
    return taps


def image_bytes(h: int, w: int) -> int:
    """fp32 bytes of the largest activation tensor of one image."""
    return max(4 * a * b * c for a, b, c in activation_shapes(h, w))


def chunk_pairs(h: int, w: int) -> int:
    """Image pairs per backbone launch, a function of (H, W) alone (tower.chunk_pairs), at most MAX_PAIRS (the
    moment kernels take the image from the grid's third dimension). An image whose own activations reach 2^31
    bytes is refused."""
    return tower.chunk_pairs(image_bytes(h, w), MAX_PAIRS, who=f"DISTS at {h}x{w}")


def split_pair(h: int, w: int) -> bool:
    """True where even one pair's activations would reach 2^31 bytes in one launch."""
    return tower.split_pair(image_bytes(h, w))


def load_weights(src: Union[str, Dict]) -> Tuple[np.ndarray, np.ndarray]:
    """(alpha, beta) as float64 [1475] from a path (.pt / .pth / .npz) or a dict holding `alpha` and `beta`,
    [1, 1475, 1, 1] or flat."""
    sd = tower.load_state(src, "DISTS")
    out = []
    for name in ("alpha", "beta"):
        if name not in sd:
            raise ValueError(f"DISTS weights: no '{name}' found; got {sorted(sd)[:6]}{' ...' if len(sd) > 6 else ''}")
        v = torch.as_tensor(sd[name]).detach().to("cpu", torch.float64).reshape(-1).numpy().copy()
        if v.size != N_WEIGHTS:
            raise ValueError(f"DISTS {name}: {v.size} weights, expected {N_WEIGHTS} (sum of {CHANNELS})")
        out.append(v)
    return out[0], out[1]


def load_backbone(src: Union[str, Dict[str, torch.Tensor]]) -> List[Tuple[torch.Tensor, torch.Tensor]]:
    """[(weight [cout,cin,3,3], bias [cout])] fp32 CPU tensors of the 13 convs, in order, from the torchvision
    VGG16 state dict (features.<i>.*), the lpips package's (net.slice<k>.<i>.*), or the single-file layout
    stage<k>.<i>.* (<i> the torchvision features index)."""
    sd = tower.load_state(src, "DISTS")
    layers = _lpips.conv_layers("vgg")
    stage = [f"stage{k}.{i}" for i, k, *_ in layers]
    if all(f"{n}.weight" in sd and f"{n}.bias" in sd for n in stage):
        sd = {f"features.{i}.{p}": sd[f"{n}.{p}"] for n, (i, *_) in zip(stage, layers) for p in ("weight", "bias")}
    try:
        return _lpips.load_backbone("vgg", sd)
    except ValueError as e:
        if "expected the torchvision keys" not in str(e):
            raise  # a shape error: it names its tensor
        raise ValueError(f"DISTS backbone: expected the torchvision keys features.0.weight/.bias ... "
                         f"features.28.weight/.bias, the lpips package's net.slice1.0.weight/.bias ... "
                         f"net.slice5.28.weight/.bias, or {stage[0]}.weight/.bias ... {stage[-1]}.weight/.bias; "
                         f"got {sorted(sd)[:6]}{' ...' if len(sd) > 6 else ''}") from None


def seeded_weights(seed: int = 0) -> Dict[str, torch.Tensor]:
    """Stand-in alpha / beta [1, 1475, 1, 1] from N(0.1, 0.01), the published implementation's initialisation, for
    tests and benchmarks (no trained weights ship)."""
    g = torch.Generator().manual_seed(seed)
    return {"alpha": 0.1 + 0.01 * torch.randn((1, N_WEIGHTS, 1, 1), generator=g),
            "beta": 0.1 + 0.01 * torch.randn((1, N_WEIGHTS, 1, 1), generator=g)}


def prep(img_u8: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """uint8 [n, h, w, 3] -> (raw, normalised), both fp32 [n, h, w, 4] with a zero fourth channel."""
    n, h, w, _ = img_u8.shape
    raw = torch.empty((n, h, w, 4), dtype=torch.float32, device=img_u8.device)
    norm = torch.empty((n, h, w, 4), dtype=torch.float32, device=img_u8.device)
    ops.call("rdeic_dists_prep", img_u8.contiguous().data_ptr(), n, h, w, raw.data_ptr(), norm.data_ptr(),
             ops.stream_ptr())
    return raw, norm


def l2_pool(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sqrt(depthwise 3x3 Hanning conv of x^2, stride 2, zero padding 1, + 1e-12) of an fp32 NHWC activation."""
    n, h, w, c = x.shape
    if x.dtype != torch.float32 or min(n, h, w, c) < 1:
        raise ValueError(f"l2_pool: non-empty fp32 [n, h, w, c] expected, got {tuple(x.shape)} {x.dtype}")
    ho, wo = (h + 1) // 2, (w + 1) // 2
    if out is None:
        out = torch.empty((n, ho, wo, c), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (n, ho, wo, c) or out.dtype != torch.float32:
        raise ValueError(f"l2_pool: out must be fp32 {(n, ho, wo, c)}")
    ops.call("rdeic_dists_l2pool", x.data_ptr(), n, h, w, c, ops.pix_ld(x), out.data_ptr(), ops.pix_ld(out),
             ops.stream_ptr())
    return out


def moments(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """fp64 [n, 5, c]: mx, my, vx, vy, cxy (biased) per image and channel of two fp32 NHWC maps of one shape."""
    if x.shape != y.shape or x.dim() != 4 or x.dtype != torch.float32 or y.dtype != torch.float32 or x.numel() == 0:
        raise ValueError("moments: two non-empty fp32 [n, h, w, c] maps of one shape expected")
    n, h, w, c = x.shape
    nd = int(_lib.load().rdeic_dists_moments_ws_doubles(n, h * w, c))
    ws = torch.empty(max(nd, 1), dtype=torch.float64, device=x.device)
    out = torch.empty((n, 5, c), dtype=torch.float64, device=x.device)
    ops.call("rdeic_dists_moments", x.data_ptr(), ops.pix_ld(x), y.data_ptr(), ops.pix_ld(y), n, h * w, c,
             ws.data_ptr(), nd, out.data_ptr(), ops.stream_ptr())
    return out


def tap_score(mom: torch.Tensor, alpha: torch.Tensor, beta: torch.Tensor, out: Optional[torch.Tensor] = None,
              accumulate: bool = False) -> torch.Tensor:
    """out[n] (+)= sum_c alpha_c S1_c + beta_c S2_c of the moments [n, 5, c] of one tap (fp64 throughout)."""
    n, _, c = mom.shape
    for v in (alpha, beta):
        if v.dtype != torch.float64 or v.numel() != c or not v.is_contiguous():
            raise ValueError(f"tap_score: alpha and beta must be {c} contiguous fp64 weights")
    if mom.dtype != torch.float64 or mom.shape[1] != 5 or not mom.is_contiguous():
        raise ValueError("tap_score: contiguous fp64 [n, 5, c] moments expected")
    if out is None:
        if accumulate:
            raise ValueError("tap_score: accumulate needs out")
        out = torch.empty(n, dtype=torch.float64, device=mom.device)
    elif out.dtype != torch.float64 or tuple(out.shape) != (n,) or not out.is_contiguous():
        raise ValueError(f"tap_score: out must be contiguous fp64 [{n}]")
    ops.call("rdeic_dists_score", mom.data_ptr(), alpha.data_ptr(), beta.data_ptr(), n, c, int(accumulate),
             out.data_ptr(), ops.stream_ptr())
    return out


def _pool(x: torch.Tensor, op) -> torch.Tensor:
    return l2_pool(x)


class DISTS(tower.Backbone):
    """DISTS(weights, backbone)(pred_u8, target_u8): uint8 [N, H, W, 3] device tensors -> float64 numpy [N].
    DISTS(weights, backbone).loss(pred, target): the training loss of float images in [-1, 1], differentiable in pred."""

    def __init__(self, weights=None, backbone=None, device="cuda"):
        if weights is None:
            raise ValueError("DISTS needs its alpha / beta weights and a VGG16 backbone; none ship with the project")
        wsd = tower.load_state(weights, "DISTS")
        alpha, beta = load_weights(wsd)
        self.table = _TABLE
        super().__init__(load_backbone(wsd if backbone is None else backbone), _lpips.conv_layers("vgg"), device)
        # normalised once in fp64; per tap, padded with zeros to the tap's stored channel count (4 at tap 0)
        total = alpha.sum() + beta.sum()
        self.alpha, self.beta, c0 = [], [], 0
        for c in CHANNELS:
            pad = (-c) % 4
            for dst, v in ((self.alpha, alpha), (self.beta, beta)):
                dst.append(torch.from_numpy(np.concatenate([v[c0:c0 + c] / total, np.zeros(pad)])).to(self.device))
            c0 += c

    def features(self, img_u8: torch.Tensor) -> List[torch.Tensor]:
        """The six taps [n, h_k, w_k, C_k] fp32 of uint8 [n, H, W, 3] images (tap 0: 4 channels, the last zero)."""
        acts = list(prep(img_u8))  # [raw, normalised]: the walk alone holds the normalised image
        raw = acts.pop(0)
        return [raw] + tower.forward(self.table, self.convs, _pool, acts, keep_all=False)

    def _score_tap(self, k: int, a: torch.Tensor, b: torch.Tensor, out: torch.Tensor) -> None:
        tap_score(moments(a, b), self.alpha[k], self.beta[k], out=out, accumulate=k > 0)

    def __call__(self, pred_u8: torch.Tensor, target_u8: torch.Tensor, chunk: Optional[int] = None) -> np.ndarray:
        """chunk: pairs per backbone launch (default chunk_pairs(H, W)); it never changes a score."""
        out = tower.score_pairs(pred_u8, target_u8, chunk, chunk_pairs, split_pair,  # this module's, looked up now
                                self.features, self._score_tap, torch.float64)
        return 1.0 - out.cpu().numpy()

    # ------------------------------------------------------------------ training loss
    def forward_acts(self, x: torch.Tensor):
        """Every activation of the normalised prep output x [n, h, w, 4], x first, and the index of each of the
        five backbone taps in that list."""
        return tower.forward(self.table, self.convs, _pool, [x], keep_all=True)

    def features_float(self, img: torch.Tensor) -> List[torch.Tensor]:
        """The six taps of float [n, H, W, 3] images in [-1, 1] (tap 0: (v + 1) / 2, 4 channels, the last zero)."""
        raw, x = prep_float(img)
        acts, taps = self.forward_acts(x)
        return [raw] + [acts[i] for i in taps]

    def loss(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """mean_n D_n, D_n = 1 - sum_k sum_c (alpha_c S1_c + beta_c S2_c), of float NHWC device images [N, H, W, 3]
        in [-1, 1] (not clamped), fp32 or bf16, as an fp32 device scalar. The gradient goes to pred only; the
        backbone runs in fp32 whatever the image dtype."""
        tower.check_float_pair(pred, target, "DISTS.loss")
        n, h, w, _ = pred.shape
        if n > 2 * MAX_PAIRS - 1 or n * image_bytes(h, w) >= MAX_TENSOR_BYTES:  # one backbone launch per side
            raise ValueError(f"DISTS.loss at {h}x{w}: {n} images' activations ({n * image_bytes(h, w)} bytes) reach "
                             f"2^31 bytes in one launch")
        return _LossFn.apply(pred, target.detach(), self)


class _LossFn(torch.autograd.Function):
    """DISTS.loss: forward and backward on the kernels of dists.hip and the fp32 convs; torch only sequences."""

    @staticmethod
    def forward(ctx, pred, target, model: "DISTS"):
        n = pred.shape[0]
        f1 = model.features_float(target)  # the target's other activations are dropped at once
        raw, x = prep_float(pred)
        acts, taps = model.forward_acts(x)
        out = torch.empty(n, dtype=torch.float64, device=pred.device)
        moms = []
        for k, a in enumerate([raw] + [acts[i] for i in taps]):
            moms.append(moments(a, f1[k]))
            tap_score(moms[-1], model.alpha[k], model.beta[k], out=out, accumulate=k > 0)
        ctx.save_for_backward(raw, *acts, *f1, *moms)  # kept until the graph is freed: backward may run again
        ctx.model, ctx.n_acts = model, len(acts)
        ctx.pred_meta = (tuple(pred.shape), pred.dtype)
        ctx.splitk = ops.splitk_state()  # the backward runs on autograd's thread: the dgrads split K as allowed here
        return (1.0 - out).mean().to(torch.float32)

    @staticmethod
    def backward(ctx, gout):
        model, saved = ctx.model, ctx.saved_tensors
        na = ctx.n_acts
        raw, acts, f1, moms = saved[0], saved[1:1 + na], saved[1 + na:7 + na], saved[7 + na:]
        (n, h, w, _), dtype = ctx.pred_meta
        gs = (-gout.to(torch.float64) / n).expand(n).contiguous()  # d loss / d score_n
        w0, packs = model._bwd_weights()

        def tap_grad(k, x, out=None):
            return tap_bwd(x, f1[k], moms[k], model.alpha[k], model.beta[k], gs, out=out)

        with ops.splitk_as(ctx.splitk):
            d = tower.backward(tower.backward_plan(model.table, 1), acts, packs, tap_grad,
                               lambda op, x, y, dy: l2_pool_bwd(x, y, dy))
            _, _, _, ks, s, p = model.table[0]  # conv 0: the gather dgrad with its ReLU mask, then the raw tap
            dnorm = _lpips.conv_dgrad_small(d, acts[1], w0, (h, w), 4, ks, s, p, prep_bwd=False)
            dpred = prep_bwd(dnorm, tap_grad(0, raw), dtype)
        return dpred, None, None


def prep_float(img: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Float NHWC [n, h, w, 3] in [-1, 1] (fp32 / bf16, any pixel stride) -> (raw, normalised), both fp32
    [n, h, w, 4] with a zero fourth channel: r = v * 0.5 + 0.5, then (r - mean_c) / std_c."""
    n, h, w, _ = img.shape
    raw = torch.empty((n, h, w, 4), dtype=torch.float32, device=img.device)
    norm = torch.empty((n, h, w, 4), dtype=torch.float32, device=img.device)
    try:
        ld = ops.pix_ld(img)
    except ValueError:
        img = img.contiguous()
        ld = 3
    ops.call("rdeic_dists_prep_float", img.data_ptr(), ld, ops.dt_code(img), n * h * w, raw.data_ptr(),
             norm.data_ptr(), ops.stream_ptr())
    return raw, norm


def prep_bwd(dnorm: torch.Tensor, draw: torch.Tensor, dtype=torch.float32,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The image gradient [n, h, w, 3] (fp32 / bf16) of prep_float from the fp32 4-channel gradients of its two
    outputs: 0.5 * (dnorm_c / std_c + draw_c)."""
    if dnorm.shape != draw.shape or dnorm.dim() != 4 or dnorm.shape[3] != 4 or dnorm.dtype != torch.float32 \
            or draw.dtype != torch.float32:
        raise ValueError("prep_bwd: two fp32 [n, h, w, 4] gradients of one shape expected")
    n, h, w, _ = dnorm.shape
    if out is None:
        out = torch.empty((n, h, w, 3), dtype=dtype, device=dnorm.device)
    elif tuple(out.shape) != (n, h, w, 3):
        raise ValueError(f"prep_bwd: out must be {(n, h, w, 3)}")
    ops.call("rdeic_dists_prep_bwd", dnorm.data_ptr(), ops.pix_ld(dnorm), draw.data_ptr(), ops.pix_ld(draw),
             n * h * w, out.data_ptr(), ops.pix_ld(out), ops.dt_code(out), ops.stream_ptr())
    return out


def l2_pool_bwd(x: torch.Tensor, y: torch.Tensor, dy: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Input gradient of y = l2_pool(x) (y the stored forward output): dx_j = x_j sum_o g_(o,j) dy_o / y_o."""
    n, h, w, c = x.shape
    so = (n, (h + 1) // 2, (w + 1) // 2, c)
    if min(n, h, w, c) < 1 or tuple(y.shape) != so or tuple(dy.shape) != so \
            or any(t.dtype != torch.float32 for t in (x, y, dy)):
        raise ValueError(f"l2_pool_bwd: fp32 x [n, h, w, c] and y, dy {so} expected")
    if out is None:
        out = torch.empty((n, h, w, c), dtype=torch.float32, device=x.device)
    elif out.shape != x.shape or out.dtype != torch.float32:
        raise ValueError(f"l2_pool_bwd: out must be fp32 {tuple(x.shape)}")
    ops.call("rdeic_dists_l2pool_bwd", x.data_ptr(), n, h, w, c, ops.pix_ld(x), y.data_ptr(), ops.pix_ld(y),
             dy.data_ptr(), ops.pix_ld(dy), out.data_ptr(), ops.pix_ld(out), ops.stream_ptr())
    return out


def tap_bwd(x: torch.Tensor, y: torch.Tensor, mom: torch.Tensor, alpha: torch.Tensor, beta: torch.Tensor,
            gs: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gs[n] * d tap_score(moments(x, y), alpha, beta)[n] / d x, written to a new tensor or added to out. gs: fp64
    [n] on the device. Two launches: the fp64 coefficients per (image, channel), then the element-wise apply."""
    if x.shape != y.shape or x.dim() != 4 or x.dtype != torch.float32 or y.dtype != torch.float32 or x.numel() == 0:
        raise ValueError("tap_bwd: two non-empty fp32 [n, h, w, c] maps of one shape expected")
    n, h, w, c = x.shape
    for v in (alpha, beta):
        if v.dtype != torch.float64 or v.numel() != c or not v.is_contiguous():
            raise ValueError(f"tap_bwd: alpha and beta must be {c} contiguous fp64 weights")
    if mom.dtype != torch.float64 or tuple(mom.shape) != (n, 5, c) or not mom.is_contiguous():
        raise ValueError(f"tap_bwd: contiguous fp64 moments {(n, 5, c)} expected")
    if gs.dtype != torch.float64 or tuple(gs.shape) != (n,) or not gs.is_contiguous():
        raise ValueError(f"tap_bwd: gs must be contiguous fp64 [{n}]")
    acc = out is not None
    if out is None:
        out = torch.empty((n, h, w, c), dtype=torch.float32, device=x.device)
    elif out.shape != x.shape or out.dtype != torch.float32:
        raise ValueError(f"tap_bwd: out must be fp32 {tuple(x.shape)}")
    coef = torch.empty((n, 5, c), dtype=torch.float64, device=x.device)
    ops.call("rdeic_dists_score_bwd", mom.data_ptr(), alpha.data_ptr(), beta.data_ptr(), gs.data_ptr(), n, h * w, c,
             coef.data_ptr(), ops.stream_ptr())
    ops.call("rdeic_dists_tap_bwd", x.data_ptr(), ops.pix_ld(x), y.data_ptr(), ops.pix_ld(y), coef.data_ptr(), n,
             h * w, c, int(acc), out.data_ptr(), ops.pix_ld(out), ops.stream_ptr())
    return out
