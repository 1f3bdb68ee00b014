"""LPIPS (Zhang et al. 2018, v0.1; reference model/lpips.py) on the device.

The reference's evaluation reports LPIPS through pyiqa's default metric: AlexNet, v0.1, inputs in [0, 1].
Here the metric is a table-driven feature extractor over the library's fp32 convs (rdeic_conv2d, ReLU in the
epilogue as leaky-ReLU with slope 0) plus three kernels of lpips.hip: the ScalingLayer prep (uint8 -> fp32
NHWC with a zero fourth channel), the max pool, and the per-tap distance (normalise, squared difference,
`lin` 1x1 conv and spatial mean in one pass).

No backbone weights ship with the project: the caller passes the torchvision AlexNet / VGG16 state dict
(``features.<i>.weight``) or the `lpips` package's full state dict (``net.slice<k>.<i>.weight``), and the five
learned `lin` heads in the reference's layout (``lin<k>.model.1.weight``, weight/lpips/<net>.pth) or as an
.npz. The computation is pinned against an fp64 restatement of model/lpips.py with a seeded random backbone
and the published heads (tests/lpips_ref.py); parity with pyiqa / the lpips package / torchvision weights is
unpinned, none of them is available offline.

Scores are batch-invariant bit for bit: split-K is pinned off for the backbone convs, every conv output
element is one fixed-order k sum, and the distance kernel's partial grid depends on the tap shape only. The
batch is therefore chunked freely (chunk_pairs) to keep every activation tensor under 2^31 bytes.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib, ops, tower

# (torchvision `features` index, cout, kernel, stride, pad) / ("pool", k, s) / ("tap",) in forward order.
# The lpips package's slice<k> holds the modules between tap k-1 and tap k under their features index.
_ALEX = (("conv", 0, 64, 11, 4, 2), ("tap",), ("pool", 3, 2), ("conv", 3, 192, 5, 1, 2), ("tap",), ("pool", 3, 2),
         ("conv", 6, 384, 3, 1, 1), ("tap",), ("conv", 8, 256, 3, 1, 1), ("tap",), ("conv", 10, 256, 3, 1, 1),
         ("tap",))
_VGG = (("conv", 0, 64, 3, 1, 1), ("conv", 2, 64, 3, 1, 1), ("tap",), ("pool", 2, 2),
        ("conv", 5, 128, 3, 1, 1), ("conv", 7, 128, 3, 1, 1), ("tap",), ("pool", 2, 2),
        ("conv", 10, 256, 3, 1, 1), ("conv", 12, 256, 3, 1, 1), ("conv", 14, 256, 3, 1, 1), ("tap",), ("pool", 2, 2),
        ("conv", 17, 512, 3, 1, 1), ("conv", 19, 512, 3, 1, 1), ("conv", 21, 512, 3, 1, 1), ("tap",), ("pool", 2, 2),
        ("conv", 24, 512, 3, 1, 1), ("conv", 26, 512, 3, 1, 1), ("conv", 28, 512, 3, 1, 1), ("tap",))
NETS = {"alex": _ALEX, "vgg": _VGG}
CHANNELS = {"alex": (64, 192, 384, 256, 256), "vgg": (64, 128, 256, 512, 512)}
MIN_SIZE = {"alex": 31, "vgg": 16}  # the smallest H, W at which every tap has at least one pixel
MAX_TENSOR_BYTES = tower.MAX_TENSOR_BYTES


def _table(net: str):
    if net not in NETS:
        raise ValueError(f"unknown LPIPS net {net!r} (alex | vgg)")
    return NETS[net]


def conv_layers(net: str) -> List[Tuple[int, int, int, int, int, int, int]]:
    """(features index, slice number, cin, cout, kernel, stride, pad) of every conv, in order."""
    out, cin, k = [], 3, 1
    for op in _table(net):
        if op[0] == "conv":
            out.append((op[1], k, cin, op[2], op[3], op[4], op[5]))
            cin = op[2]
        elif op[0] == "tap":
            k += 1
    return out


def activation_shapes(net: str, h: int, w: int) -> List[Tuple[int, int, int]]:
    """(h, w, c) of every activation tensor of one image, the 4-channel prep output first.
    Raises ValueError below the minimum size."""
    table = _table(net)
    if h < MIN_SIZE[net] or w < MIN_SIZE[net]:
        raise ValueError(f"LPIPS({net}) needs H, W >= {MIN_SIZE[net]}, got {h}x{w}")
    shapes, c = [(h, w, 4)], 4
    for op in table:
        if op[0] == "conv":
            _, _, c, k, s, p = op
            h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        elif op[0] == "pool":
            _, k, s = op
            h, w = (h - k) // s + 1, (w - k) // s + 1
        else:
            continue
        shapes.append((h, w, c))
    return shapes


def tap_shapes(net: str, h: int, w: int) -> List[Tuple[int, int, int]]:
    """(h, w, c) of the five taps."""
    acts, taps, i = activation_shapes(net, h, w), [], 0
    for op in _table(net):
        if op[0] == "tap":
            taps.append(acts[i])
        else:
            i += 1
    return taps


def image_bytes(net: str, h: int, w: int) -> int:
    """fp32 bytes of the largest activation tensor of one image."""
    return max(4 * a * b * c for a, b, c in activation_shapes(net, h, w))


def chunk_pairs(net: str, h: int, w: int) -> int:
    """Image pairs per backbone launch, a function of (net, H, W) alone (tower.chunk_pairs); an image whose own
    activations reach 2^31 bytes is refused."""
    return tower.chunk_pairs(image_bytes(net, h, w), who=f"LPIPS({net}) at {h}x{w}")


def split_pair(net: str, h: int, w: int) -> bool:
    """True where even one pair's activations would reach 2^31 bytes in one launch."""
    return tower.split_pair(image_bytes(net, h, w))


def load_backbone(net: str, src: Union[str, Dict[str, torch.Tensor]]) -> List[Tuple[torch.Tensor, torch.Tensor]]:
    """[(weight [cout,cin,k,k], bias [cout])] fp32 CPU tensors of every conv, in order, from the torchvision
    state dict (features.<i>.*) or the lpips package's (net.slice<k>.<i>.*)."""
    sd = tower.load_state(src, "LPIPS")
    layers = conv_layers(net)
    layouts = ([f"features.{i}" for i, *_ in layers], [f"net.slice{k}.{i}" for i, k, *_ in layers])
    for names in layouts:
        if all(f"{n}.weight" in sd and f"{n}.bias" in sd for n in names):
            break
    else:
        raise ValueError(f"LPIPS({net}) backbone: expected the torchvision keys {layouts[0][0]}.weight/.bias ... "
                         f"{layouts[0][-1]}.weight/.bias or the lpips package's {layouts[1][0]}.weight/.bias ... "
                         f"{layouts[1][-1]}.weight/.bias; got {sorted(sd)[:6]}{' ...' if len(sd) > 6 else ''}")
    out = []
    for name, (_, _, cin, cout, k, _, _) in zip(names, layers):
        wt = sd[f"{name}.weight"].detach().to("cpu", torch.float32)
        b = sd[f"{name}.bias"].detach().to("cpu", torch.float32)
        if tuple(wt.shape) != (cout, cin, k, k) or tuple(b.shape) != (cout,):
            raise ValueError(f"{name}: shapes {tuple(wt.shape)} / {tuple(b.shape)}, expected "
                             f"{(cout, cin, k, k)} / {(cout,)}")
        out.append((wt.contiguous(), b.contiguous()))
    return out


def load_lin(net: str, src: Union[str, Dict[str, torch.Tensor]]) -> List[torch.Tensor]:
    """The five head vectors [C_k] fp32 (CPU): the reference's .pth layout (lin<k>.model.1.weight [1,C,1,1]),
    or an .npz / dict with lin0..lin4 (or <net>_lin0..<net>_lin4, the layout of tests/golden/lpips_lin.npz)."""
    sd = tower.load_state(src, "LPIPS")
    out = []
    _table(net)
    for k, c in enumerate(CHANNELS[net]):
        names = (f"lin{k}.model.1.weight", f"{net}_lin{k}", f"lin{k}")
        v = next((sd[n] for n in names if n in sd), None)
        if v is None:
            raise ValueError(f"LPIPS({net}) heads: none of {names} found; got {sorted(sd)[:6]}")
        v = torch.as_tensor(v).detach().to("cpu", torch.float32).reshape(-1).contiguous()
        if v.numel() != c:
            raise ValueError(f"LPIPS({net}) lin{k}: {v.numel()} weights, expected {c}")
        out.append(v)
    return out


def seeded_backbone(net: str, seed: int = 0) -> Dict[str, torch.Tensor]:
    """A stand-in backbone for benchmarks (none ships): He-scaled normal weights and small normal biases from a
    seeded generator, keyed as the torchvision state dict (features.<i>.*)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, _, cin, cout, k, _, _ in conv_layers(net):
        sd[f"features.{i}.weight"] = torch.randn((cout, cin, k, k), generator=g) * (2.0 / (cin * k * k)) ** 0.5
        sd[f"features.{i}.bias"] = torch.randn((cout,), generator=g) * 0.05
    return sd


def _pool(x: torch.Tensor, op) -> torch.Tensor:
    return max_pool(x, op[1], op[2])


class LPIPS(tower.Backbone):
    """LPIPS(net)(pred_u8, target_u8): uint8 [N, H, W, 3] device tensors -> float64 numpy [N].
    LPIPS(net).loss(pred, target): the training loss of float images in [-1, 1], differentiable in pred."""

    def __init__(self, net: str = "alex", backbone=None, lin=None, device="cuda"):
        if backbone is None or lin is None:
            raise ValueError("LPIPS needs a backbone (torchvision / lpips state dict) and the lin heads; "
                             "no backbone weights ship with the project")
        self.net = net
        self.table = _table(net)
        super().__init__(load_backbone(net, backbone), conv_layers(net), device)
        self.lin = [v.to(self.device) for v in load_lin(net, lin)]

    # ------------------------------------------------------------------ pieces
    def prep(self, img_u8: torch.Tensor) -> torch.Tensor:
        n, h, w, _ = img_u8.shape
        x = torch.empty((n, h, w, 4), dtype=torch.float32, device=img_u8.device)
        ops.call("rdeic_lpips_prep", img_u8.contiguous().data_ptr(), n, h, w, x.data_ptr(), ops.stream_ptr())
        return x

    def features(self, img_u8: torch.Tensor) -> List[torch.Tensor]:
        """The five taps [n, h_k, w_k, C_k] fp32 of uint8 [n, H, W, 3] images."""
        return tower.forward(self.table, self.convs, _pool, [self.prep(img_u8)], keep_all=False)

    def _score_tap(self, k: int, a: torch.Tensor, b: torch.Tensor, out: torch.Tensor) -> None:
        layer_distance(a, b, self.lin[k], out=out, accumulate=k > 0)

    def __call__(self, pred_u8: torch.Tensor, target_u8: torch.Tensor, chunk: Optional[int] = None) -> np.ndarray:
        """chunk: pairs per backbone launch (default chunk_pairs(net, H, W)); it never changes a score."""
        out = tower.score_pairs(pred_u8, target_u8, chunk, lambda h, w: chunk_pairs(self.net, h, w),
                                lambda h, w: split_pair(self.net, h, w), self.features, self._score_tap, torch.float32)
        return out.cpu().numpy().astype(np.float64)

    # ------------------------------------------------------------------ training loss
    def forward_acts(self, x: torch.Tensor):
        """Every activation of the prep output x [n, h, w, 4], x first, and the index of each tap in that list."""
        return tower.forward(self.table, self.convs, _pool, [x], keep_all=True)

    def features_float(self, img: torch.Tensor) -> List[torch.Tensor]:
        """The five taps of float [n, H, W, 3] images in [-1, 1]."""
        acts, taps = self.forward_acts(prep_float(img))
        return [acts[i] for i in taps]

    def loss(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """mean_n sum_k score_k (reference model/lpips.py:85-89 with inp_range (-1, 1)) of float NHWC device images
        [N, H, W, 3] in [-1, 1], fp32 or bf16, as an fp32 device scalar. The gradient goes to pred only; the
        backbone runs in fp32 whatever the image dtype."""
        tower.check_float_pair(pred, target, "LPIPS.loss")
        n, h, w, _ = pred.shape
        if n * image_bytes(self.net, h, w) >= MAX_TENSOR_BYTES:  # validates the size; one backbone launch per side
            raise ValueError(f"LPIPS.loss({self.net}) at {h}x{w}: {n} images' activations reach 2^31 bytes")
        return _LossFn.apply(pred, target.detach(), self)


class _LossFn(torch.autograd.Function):
    """LPIPS.loss: forward and backward on the kernels of lpips.hip and the fp32 convs; torch only sequences."""

    @staticmethod
    def forward(ctx, pred, target, model: "LPIPS"):
        n = pred.shape[0]
        f1 = model.features_float(target)  # the target's other activations are dropped at once
        acts, taps = model.forward_acts(prep_float(pred))
        out = torch.empty(n, dtype=torch.float32, device=pred.device)
        for k, i in enumerate(taps):
            layer_distance(acts[i], f1[k], model.lin[k], out=out, accumulate=k > 0)
        ctx.save_for_backward(*acts, *f1)  # kept until the graph is freed: a retained graph can run backward again
        ctx.model, ctx.n_acts = model, len(acts)
        ctx.pred_meta = (tuple(pred.shape), pred.dtype)
        ctx.splitk = ops.splitk_state()  # the backward runs on autograd's thread: the dgrads split K as allowed here
        return out.mean()

    @staticmethod
    def backward(ctx, gout):
        model, saved = ctx.model, ctx.saved_tensors
        acts, f1 = saved[:ctx.n_acts], saved[ctx.n_acts:]
        (n, h, w, _), dtype = ctx.pred_meta
        gscore = (gout.to(torch.float32) / n).expand(n).contiguous()
        w0, packs = model._bwd_weights()
        with ops.splitk_as(ctx.splitk):
            d = tower.backward(tower.backward_plan(model.table, 0), acts, packs,
                               lambda k, x, out: layer_distance_bwd(x, f1[k], model.lin[k], gscore, out=out),
                               lambda op, x, y, dy: max_pool_bwd(x, dy, op[1], op[2]))
            _, _, _, ks, s, p = model.table[0]  # conv 0: the gather dgrad with its ReLU mask and the prep backward
            dpred = torch.empty((n, h, w, 3), dtype=dtype, device=d.device)
            conv_dgrad_small(d, acts[1], w0, (h, w), 4, ks, s, p, prep_bwd=True, out=dpred)
        return dpred, None, None


def pack_bwd_weights(raw, net: str, device):
    """tower.pack_bwd_weights of a backbone's raw [(weight, bias)] list: conv1 as [kh][kw][4][cout], and [None] +
    the other convs' flipped packs."""
    return tower.pack_bwd_weights(raw, conv_layers(net), device)


def prep_float(img: torch.Tensor) -> torch.Tensor:
    """The ScalingLayer for inputs in [-1, 1]: float NHWC [n, h, w, 3] (fp32 / bf16, any pixel stride) ->
    fp32 [n, h, w, 4], channels 0..2 (v - shift_c) / scale_c, channel 3 zero."""
    n, h, w, _ = img.shape
    x = torch.empty((n, h, w, 4), dtype=torch.float32, device=img.device)
    try:
        ld = ops.pix_ld(img)
    except ValueError:
        img = img.contiguous()
        ld = 3
    ops.call("rdeic_lpips_prep_float", img.data_ptr(), ld, ops.dt_code(img), n * h * w, x.data_ptr(),
             ops.stream_ptr())
    return x


def layer_distance_bwd(f0: torch.Tensor, f1: torch.Tensor, lin: torch.Tensor, gscore: torch.Tensor,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gscore[n] * d layer_distance(f0, f1, lin)[n] / d f0, written to a new tensor or added to out. An all-zero
    pixel of f0 gets exactly 0."""
    if f0.shape != f1.shape or f0.dtype != torch.float32 or f1.dtype != torch.float32:
        raise ValueError("layer_distance_bwd: two fp32 [n, h, w, c] taps of one shape expected")
    n, h, w, c = f0.shape
    if lin.dtype != torch.float32 or lin.numel() != c or not lin.is_contiguous():
        raise ValueError(f"layer_distance_bwd: lin must be {c} contiguous fp32 weights")
    if gscore.dtype != torch.float32 or tuple(gscore.shape) != (n,) or not gscore.is_contiguous():
        raise ValueError(f"layer_distance_bwd: gscore must be contiguous fp32 [{n}]")
    acc = out is not None
    if out is None:
        out = torch.empty((n, h, w, c), dtype=torch.float32, device=f0.device)
    elif out.shape != f0.shape or out.dtype != torch.float32:
        raise ValueError(f"layer_distance_bwd: out must be fp32 {tuple(f0.shape)}")
    ops.call("rdeic_lpips_layer_bwd", f0.data_ptr(), ops.pix_ld(f0), f1.data_ptr(), ops.pix_ld(f1), lin.data_ptr(),
             gscore.data_ptr(), n, h * w, c, int(acc), out.data_ptr(), ops.pix_ld(out), ops.stream_ptr())
    return out


def max_pool_bwd(x: torch.Tensor, dy: torch.Tensor, k: int, s: int) -> torch.Tensor:
    """Input gradient of max_pool(x, k, s): torch's rule (the first maximum of a window takes its gradient)."""
    n, h, w, c = x.shape
    ho, wo = (h - k) // s + 1, (w - k) // s + 1
    if x.dtype != torch.float32 or dy.dtype != torch.float32 or tuple(dy.shape) != (n, ho, wo, c):
        raise ValueError(f"max_pool_bwd: fp32 x and dy {(n, ho, wo, c)} expected, got {tuple(dy.shape)}")
    dx = torch.empty((n, h, w, c), dtype=torch.float32, device=x.device)
    ops.call("rdeic_maxpool2d_bwd", x.data_ptr(), n, h, w, c, ops.pix_ld(x), dy.data_ptr(), ops.pix_ld(dy), k, s,
             dx.data_ptr(), c, ops.stream_ptr())
    return dx


def conv_dgrad_small(dz: torch.Tensor, z: Optional[torch.Tensor], wt: torch.Tensor, in_hw, cin: int, k: int,
                     stride: int, pad: int, prep_bwd: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Input gradient of a conv with cin <= 4 (any kernel, stride, pad) from dz [n, ho, wo, cout] fp32.
    z: the conv's output after its ReLU (mask z > 0), or None. wt: the weight as [k][k][cin][cout] fp32.
    prep_bwd: also the backward of prep_float (3 channels, each / scale_c). out: [n, h, w, channels] fp32 / bf16."""
    n, ho, wo, cout = dz.shape
    h, w = in_hw
    if dz.dtype != torch.float32 or tuple(wt.shape) != (k, k, cin, cout) or wt.dtype != torch.float32 \
            or not wt.is_contiguous() or (ho, wo) != ((h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1):
        raise ValueError("conv_dgrad_small: dz fp32 [n, ho, wo, cout] and wt fp32 [k, k, cin, cout] expected")
    if z is not None and (z.shape != dz.shape or z.dtype != torch.float32):
        raise ValueError("conv_dgrad_small: z must match dz")
    co = min(cin, 3) if prep_bwd else cin
    if out is None:
        out = torch.empty((n, h, w, co), dtype=torch.float32, device=dz.device)
    elif tuple(out.shape) != (n, h, w, co):
        raise ValueError(f"conv_dgrad_small: out must be {(n, h, w, co)}")
    ops.call("rdeic_conv_dgrad_small", dz.data_ptr(), ops.pix_ld(dz), None if z is None else z.data_ptr(),
             0 if z is None else ops.pix_ld(z), wt.data_ptr(), n, h, w, cin, cout, k, k, stride, pad, int(prep_bwd),
             out.data_ptr(), ops.pix_ld(out), ops.dt_code(out), ops.stream_ptr())
    return out


def max_pool(x: torch.Tensor, k: int, s: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Max pool of an fp32 NHWC activation: window k, stride s, no padding, floor mode."""
    n, h, w, c = x.shape
    if x.dtype != torch.float32 or h < k or w < k:
        raise ValueError(f"max_pool: fp32 [n, h >= {k}, w >= {k}, c] expected, got {tuple(x.shape)} {x.dtype}")
    ho, wo = (h - k) // s + 1, (w - k) // s + 1
    if out is None:
        out = torch.empty((n, ho, wo, c), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (n, ho, wo, c) or out.dtype != torch.float32:
        raise ValueError(f"max_pool: out must be fp32 {(n, ho, wo, c)}")
    ops.call("rdeic_maxpool2d", x.data_ptr(), n, h, w, c, ops.pix_ld(x), k, s, out.data_ptr(), ops.pix_ld(out),
             ops.stream_ptr())
    return out


def layer_distance(f0: torch.Tensor, f1: torch.Tensor, lin: torch.Tensor, out: Optional[torch.Tensor] = None,
                   accumulate: bool = False) -> torch.Tensor:
    """out[n] (+)= mean_p sum_c lin_c (f0 / (|f0_p| + 1e-10) - f1 / (|f1_p| + 1e-10))^2 of fp32 NHWC taps."""
    if f0.shape != f1.shape or f0.dtype != torch.float32 or f1.dtype != torch.float32:
        raise ValueError("layer_distance: two fp32 [n, h, w, c] taps of one shape expected")
    n, h, w, c = f0.shape
    if lin.dtype != torch.float32 or lin.numel() != c or not lin.is_contiguous():
        raise ValueError(f"layer_distance: lin must be {c} contiguous fp32 weights")
    if out is None:
        if accumulate:
            raise ValueError("layer_distance: accumulate needs out")
        out = torch.empty(n, dtype=torch.float32, device=f0.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (n,) or not out.is_contiguous():
        raise ValueError(f"layer_distance: out must be contiguous fp32 [{n}]")
    nf = int(_lib.load().rdeic_lpips_layer_ws_floats(n, h * w, c))
    ws = torch.empty(max(nf, 1), dtype=torch.float32, device=f0.device)
    ops.call("rdeic_lpips_layer", f0.data_ptr(), ops.pix_ld(f0), f1.data_ptr(), ops.pix_ld(f1), lin.data_ptr(), n,
             h * w, c, int(accumulate), ws.data_ptr(), nf, out.data_ptr(), ops.stream_ptr())
    return out
