"""The sequential feature tower LPIPS and DISTS share: one table walk forward, one reversed walk backward, one
pair driver, the 2^31-byte size rules, the weight-file loader and the conv packing. A metric supplies its table
(("conv", features index, cout, kernel, stride, pad) / ("pool", ...) / ("tap",) in forward order), its prep, its
pool and per-tap kernels and what happens at conv 0; the walks launch nothing of their own but the library's fp32
convs and rdeic_act_bwd. FID takes the loader, the cap and the conv-0 padding only: Inception is no sequential
table.

The size rules and the float-image checks are plain functions: lpips.py and dists.py keep their own module-level
names as delegations and look them up there at call time, so nothing here captures one of them.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops

MAX_TENSOR_BYTES = 2 ** 31


# ---------------------------------------------------------------- weights
def load_state_file(path, what: str) -> Dict[str, torch.Tensor]:
    """The tensors of an .npz, or of a .pt / .pth (a `state_dict` nest is opened). what: the FileNotFoundError's
    first word ("LPIPS", "DISTS", "Inception")."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{what} weights not found: {path}")
    if str(path).endswith(".npz"):
        with np.load(path) as z:
            return {k: torch.from_numpy(np.array(z[k])) for k in z.files}
    sd = torch.load(path, map_location="cpu", weights_only=True)
    return sd.get("state_dict", sd) if isinstance(sd, dict) else sd


def load_state(src, what: str) -> Dict[str, torch.Tensor]:
    """A state dict as it is; a path through load_state_file."""
    return load_state_file(src, what) if isinstance(src, (str, os.PathLike)) else src


def pad_cin4(wt: torch.Tensor) -> torch.Tensor:
    """Conv 0's [cout, 3, kh, kw] weight with a zero fourth input channel (the prep kernels'): exact zero
    products, 16-byte gathers."""
    return torch.nn.functional.pad(wt, (0, 0, 0, 0, 0, 1))


def pack_convs(raw, layers) -> List[ops.ConvParams]:
    """The forward's fp32 packs of a backbone's raw [(weight, bias)] list; layers: (..., stride, pad) per conv."""
    return [ops.ConvParams.pack(pad_cin4(wt) if i == 0 else wt, b, stride=s, pad=p, dtype=torch.float32)
            for i, ((wt, b), (*_, s, p)) in enumerate(zip(raw, layers))]


def pack_bwd_weights(raw, layers, device):
    """The backward's device weights of a backbone's raw [(weight, bias)] list: conv 0 as [kh][kw][4][cout] for
    the gather dgrad, and [None] + the other convs packed for the input-gradient conv (autograd.conv_dgrad's form:
    flipped, [cin][kh kw cout], a stride-1 conv with pad k - 1 - p). layers: (..., cin, cout, k, stride, pad)."""
    packs = [None]
    for (w, _), (*_, cin, cout, k, _, p) in zip(raw[1:], layers[1:]):
        wd = w.to(device).contiguous()
        wld = -(-(k * k * cout) // 64) * 64
        packed = torch.empty((cin, wld), dtype=torch.float32, device=device)
        ops.call("rdeic_pack_conv_weight_dgrad", wd.data_ptr(), cout, cin, k, k, packed.data_ptr(), wld, 0,
                 ops.stream_ptr())
        packs.append(ops.ConvParams(packed, wld, None, cin, cout, k, k, 1, k - 1 - p))
    return pad_cin4(raw[0][0]).permute(2, 3, 1, 0).contiguous().to(device), packs


class Backbone:
    """What a metric holds of its conv stack: the forward packs, the CPU masters and the backward's device weights,
    packed on first use and owned by the instance (they go when it goes)."""

    def __init__(self, raw, layers, device):
        self.device = torch.device(device)
        self.convs = pack_convs(raw, layers)
        self._raw, self._layers, self._bwd = raw, layers, None

    def _bwd_weights(self):
        """(conv 0's weight for the gather dgrad, [None] + the dgrad packs of the other convs): pack_bwd_weights."""
        if self._bwd is None:
            self._bwd = pack_bwd_weights(self._raw, self._layers, self.device)
        return self._bwd


# ---------------------------------------------------------------- size rules
def chunk_pairs(per: int, max_pairs: Optional[int] = None, who: str = "tower") -> int:
    """Image pairs per backbone launch from `per`, the bytes of one image's largest activation: the most for which
    every activation of the 2 x pairs images stays under 2^31 bytes, at least 1 (the two images of that pair may
    still be too large together: split_pair) and at most max_pairs. An image whose own activations reach 2^31
    bytes is refused."""
    if per >= MAX_TENSOR_BYTES:
        raise ValueError(f"{who}: one image's activation reaches 2^31 bytes")
    pairs = max(1, ((MAX_TENSOR_BYTES - 1) // per) // 2)
    return pairs if max_pairs is None else min(max_pairs, pairs)


def split_pair(per: int) -> bool:
    """True where even one pair's activations would reach 2^31 bytes in one launch."""
    return 2 * per >= MAX_TENSOR_BYTES


# ---------------------------------------------------------------- the walks
def forward(table, convs, pool: Callable, acts: list, keep_all: bool):
    """The table walk on acts = [x], x the 4-channel prep output: conv (ReLU in the epilogue), pool(x, op), tap.
    keep_all=False: returns the taps; the one entry of acts is replaced as the walk goes, so an activation that
    is no tap goes as soon as its consumer has run (acts is a list for that: an argument of its own would live
    as long as the call). keep_all=True: every activation is appended to acts; returns (acts, the index of each
    tap in it). Split-K is pinned off: a k grouping that depended on the batch would break batch invariance."""
    taps, ci = [], 0
    with ops.splitk_as((False, False)):
        for op in table:
            if op[0] == "tap":
                taps.append(len(acts) - 1 if keep_all else acts[-1])
                continue
            if op[0] == "conv":
                y = ops.conv2d(acts[-1], convs[ci], act=ops.LEAKY, slope=0.0)
                ci += 1
            else:
                y = pool(acts[-1], op)
            if keep_all:
                acts.append(y)
            else:
                acts[-1] = y
    return (acts, taps) if keep_all else taps


def backward_plan(table, first_tap: int) -> List[Tuple[tuple, int, int]]:
    """The forward's records (op, index of its input in forward(keep_all=True)'s acts, conv or tap number) in
    reverse order (a pool carries the number of the convs before it; nothing reads it). first_tap: the number of the table's first tap (1 where the metric has a tap of its own before
    the table, DISTS's raw image)."""
    recs, i, ci, k = [], 0, 0, first_tap
    for op in table:
        if op[0] == "tap":
            recs.append((op, i, k))
            k += 1
        else:
            recs.append((op, i, ci))
            i += 1
            ci += op[0] == "conv"
    return recs[::-1]


def backward(plan, acts: Sequence[torch.Tensor], packs, tap_grad: Callable, pool_grad: Callable):
    """The reversed walk down to conv 0: returns the gradient at conv 0's output (before its ReLU mask), which the
    metric finishes itself. tap_grad(k, x, out): the gradient of tap k at x, a new tensor (out None) or added to
    out. pool_grad(op, x, y, dy): the input gradient of y = pool(x, op). A conv past the first takes the ReLU mask
    in place and the packed stride-1 dgrad. The caller sets the split-K state."""
    d = None
    for op, i, j in plan:
        if op[0] == "tap":
            d = tap_grad(j, acts[i], d)
        elif d is None:
            continue  # nothing after the last tap
        elif op[0] == "pool":
            d = pool_grad(op, acts[i], acts[i + 1], d)
        elif j > 0:
            cout, z = op[2], acts[i + 1]
            ops.call("rdeic_act_bwd", d.data_ptr(), ops.pix_ld(d), z.data_ptr(), ops.pix_ld(z), d.numel() // cout,
                     cout, ops.LEAKY, 0.0, d.data_ptr(), ops.pix_ld(d), 0, ops.stream_ptr())  # the ReLU mask, in place
            d = ops.conv2d(d, packs[j], out_hw=tuple(acts[i].shape[1:3]))  # stride 1 throughout
    return d


# ---------------------------------------------------------------- the pair driver
def score_pairs(pred_u8: torch.Tensor, target_u8: torch.Tensor, chunk: Optional[int], step_rule: Callable,
                split_rule: Callable, features: Callable, score_tap: Callable, out_dtype) -> torch.Tensor:
    """out[N] of uint8 [N, H, W, 3] pairs, chunked: step_rule(h, w) pairs per backbone launch at most (it validates
    the size), `chunk` fewer; one launch on the concatenated pair, or prediction and target one after the other
    where split_rule(h, w). score_tap(k, f0, f1, out) writes (k == 0) or adds tap k's score of a chunk."""
    if pred_u8.shape != target_u8.shape or pred_u8.dim() != 4 or pred_u8.shape[3] != 3 \
            or pred_u8.dtype != torch.uint8 or target_u8.dtype != torch.uint8:
        raise ValueError("expected matching uint8 [N, H, W, 3] images")
    n, h, w, _ = pred_u8.shape
    step = min(step_rule(h, w), int(chunk) if chunk else n) if n else 1
    out = torch.empty(n, dtype=out_dtype, device=pred_u8.device)

    def one_chunk(pred, tgt, out):  # a frame of its own: a chunk's features go before the next chunk's are made
        m = pred.shape[0]
        if split_rule(h, w):
            f0, f1 = features(pred), features(tgt)
        else:
            f = features(torch.cat([pred, tgt]))
            f0, f1 = [t[:m] for t in f], [t[m:] for t in f]
        for k, (a, b) in enumerate(zip(f0, f1)):
            score_tap(k, a, b, out)

    for s0 in range(0, n, max(1, step)):
        one_chunk(pred_u8[s0:s0 + step], target_u8[s0:s0 + step], out[s0:s0 + step])
    return out


def check_float_pair(pred: torch.Tensor, target: torch.Tensor, who: str) -> None:
    """The input checks of a loss: two float32 / bfloat16 [N, H, W, 3] device images of one non-empty shape."""
    for t in (pred, target):
        if t.dim() != 4 or t.shape[3] != 3 or t.dtype not in (torch.float32, torch.bfloat16) or not t.is_cuda:
            raise ValueError(f"{who}: float32 / bfloat16 [N, H, W, 3] device images expected")
    if pred.shape != target.shape or pred.numel() == 0:
        raise ValueError(f"{who}: prediction and target must share a non-empty shape")
