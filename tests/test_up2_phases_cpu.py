"""The nearest-x2 upsample 3x3 conv as four folded 2x2 phase convs (rdeic_amd.params.fold_up2_phases,
rdeic_conv2d_up2_phases): the fold identity in float64, the pack's phase / tap order, and the image-group
split that keeps every launch's input and output span below 2 GiB. No GPU needed."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from rdeic_amd import _lib
from rdeic_amd.params import fold_up2_phases


def _phase_conv(x, f, bias, cout, cin):
    """conv3x3(nearest_x2(x)) assembled from the four 2x2 phase convs of x (all float64, NCHW)."""
    n, _, h, w = x.shape
    out = torch.empty(n, cout, 2 * h, 2 * w, dtype=torch.float64)
    for a in (0, 1):
        for b in (0, 1):
            wab = f[2 * a + b].reshape(cout, 2, 2, cin).permute(0, 3, 1, 2)  # k = (dy, dx, ci) -> [co, ci, dy, dx]
            xp = F.pad(x, (1 - b, b, 1 - a, a))  # (left, right, top, bottom)
            out[:, :, a::2, b::2] = F.conv2d(xp, wab, bias)
    return out


@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (2, 5, 7), (3, 6, 10), (2, 8, 8)])
def test_fold_identity_float64(n, h, w):
    g = torch.Generator().manual_seed(h * 100 + w)
    cin, cout = 5, 3
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64)
    bias = torch.randn(cout, generator=g, dtype=torch.float64)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wt, bias, padding=1)
    got = _phase_conv(x, fold_up2_phases(wt, dtype=torch.float64), bias, cout, cin)
    err = (got - ref).abs().max().item()
    print(f"fold identity {n}x{h}x{w}: max abs diff {err:.3e}")
    assert err <= 1e-12


def test_pack_phase_and_tap_order():
    """One channel, W = [[1,2,3],[4,5,6],[7,8,9]]: phase 2a+b folds rows by R_a and columns by R_b
    (R_0 = [[1,0,0],[0,1,1]], R_1 = [[1,1,0],[0,0,1]]); taps row-major (dy, dx)."""
    wt = torch.arange(1, 10, dtype=torch.float32).reshape(1, 1, 3, 3)
    f = fold_up2_phases(wt)
    assert f.shape == (4, 1, 4) and f.dtype == torch.float32
    assert f[0, 0].tolist() == [1, 5, 11, 28]   # rows (w0, w1+w2), cols (c0, c1+c2)
    assert f[1, 0].tolist() == [3, 3, 24, 15]   # rows (w0, w1+w2), cols (c0+c1, c2)
    assert f[2, 0].tolist() == [5, 16, 7, 17]   # rows (w0+w1, w2), cols (c0, c1+c2)
    assert f[3, 0].tolist() == [12, 9, 15, 9]   # rows (w0+w1, w2), cols (c0+c1, c2)
    # two channels: k = tap * cin + channel
    w2 = torch.stack([wt[0, 0], 10 * wt[0, 0]])[None]
    f2 = fold_up2_phases(w2)
    assert f2[0, 0].tolist() == [1, 10, 5, 50, 11, 110, 28, 280]


def test_fold_rounds_once():
    """The bf16 pack is the float64 corner sum rounded (through fp32) once, not a sum of bf16-rounded weights."""
    wt = torch.zeros(1, 1, 3, 3)
    wt[0, 0, 0, 1] = 1.0 + 2.0 ** -8 - 2.0 ** -12   # bf16: 1.0 (just under half a step of 2^-7)
    wt[0, 0, 0, 2] = 0.5 + 2.0 ** -9 - 2.0 ** -13   # bf16: 0.5 (just under half a step of 2^-8)
    assert wt.to(torch.bfloat16)[0, 0, 0, 1:].tolist() == [1.0, 0.5]
    f = fold_up2_phases(wt).to(torch.bfloat16)
    # phase 0, tap (0, 1) = w01 + w02 = 1.5 + 0.00549: above half a step (2^-8) at 1.5, so it rounds up
    assert f[0, 0, 1].item() == 1.5 + 2.0 ** -7


@pytest.mark.parametrize("n,h,w,ld0,out_ld", [
    (15, 256, 256, 256, 256),   # 15/16 of 2 GiB of output: one group
    (16, 256, 256, 256, 256),   # exactly 2^31 output bytes: must split
    (17, 256, 256, 256, 256),
    (64, 256, 256, 256, 256),
    (16, 256, 256, 2048, 64),   # the input span is the larger one (2^32 bytes)
    (3, 512, 512, 512, 512),    # 2^30 output bytes per image: one image per group
    (16, 181, 181, 64, 520),    # odd sizes: 15 images fit, 16 do not
])
def test_image_group_split_below_2gib(n, h, w, ld0, out_ld):
    lib = _lib.load()
    d = _lib.ConvDesc()
    d.n, d.h, d.w, d.ld0, d.out_ld = n, h, w, ld0, out_ld
    g = lib.rdeic_conv2d_up2_group(C.byref(d))
    in_span, out_span = g * h * w * ld0 * 2, g * 4 * h * w * out_ld * 2
    print(f"n={n} {h}x{w} ld0={ld0} out_ld={out_ld}: {g} images per group, spans {in_span} / {out_span} bytes")
    assert 1 <= g <= n
    assert in_span < 2 ** 31 and out_span < 2 ** 31
    if n * 4 * h * w * out_ld * 2 < 2 ** 31 and n * h * w * ld0 * 2 < 2 ** 31:
        assert g == n  # no split where none is needed


def test_image_group_split_rejects_oversized_image():
    lib = _lib.load()
    d = _lib.ConvDesc()
    d.n, d.h, d.w, d.ld0, d.out_ld = 2, 1024, 1024, 256, 256  # one image's output is 2^31 bytes
    assert lib.rdeic_conv2d_up2_group(C.byref(d)) == 0
