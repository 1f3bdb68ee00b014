"""Row-band launches of the fast conv kernels (rdeic_conv2d_band_rows, ops.set_launch_limit): one image whose tensors
exceed the launch limit runs as several launches of the SAME kernel over bands of output rows.

* Forced limit, small shapes: the limit is lowered until a small image needs 3-5 bands (the last one shorter); the
  output and the fused GroupNorm partials must equal the one-launch result bit for bit, and the launch counters must
  show one fast-kernel launch per band (and per image).
* Real single images past the 2 GiB reach on the default limit: the fast-path counter must move, and the result must
  equal, bit for bit, the same kernel run as separate small launches on 72-row crops (top, bottom, around every band
  boundary the planner reports, around byte offset 2^31), with the same GroupNorm table.
* GroupNorm on such a tensor: apply against crops, and the affine from fused partials against the stand-alone pass."""
import contextlib
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@contextlib.contextmanager
def _limit(nbytes):
    from rdeic_amd import ops
    prev = ops.set_launch_limit(nbytes)
    try:
        yield
    finally:
        ops.set_launch_limit(prev)


@contextlib.contextmanager
def _option(key, value):
    from rdeic_amd import ops
    prev = ops.set_conv_option(key, value)
    try:
        yield
    finally:
        ops.set_conv_option(key, prev)


def _pack(cin, cout, seed, k=3, stride=1, pad=1):
    from rdeic_amd import ops
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    b = torch.randn(cout, generator=g) * 0.1
    return w, ops.ConvParams.pack(w.cuda(), b.cuda(), stride=stride, pad=pad)


def _phase_pack(w, p):
    from rdeic_amd import ops
    from rdeic_amd.params import fold_up2_phases
    f = fold_up2_phases(w).to(BF).contiguous().cuda()
    return ops.ConvParams(f, 4 * w.shape[1], p.bias, w.shape[0], w.shape[1], 2, 2, 1, 1)


def _ab(n, c, seed):
    """A GroupNorm affine table [n, c, 2] (a, b) without a pass over the tensor."""
    g = torch.Generator().manual_seed(seed)
    return torch.stack([0.8 + 0.2 * torch.rand(n, c, generator=g), 0.3 * torch.randn(n, c, generator=g)], -1).cuda()


def _plan(h, w, ld, ho, wo, out_ld, tile, *, k=3, stride=1, pad=1, up2=False, stats=False):
    """(rows per band, bands) of the library's planner under the current limit."""
    from rdeic_amd import _lib
    d = _lib.ConvDesc()
    d.n, d.h, d.w, d.c0, d.ld0, d.ho, d.wo, d.cout, d.out_ld = 1, h, w, ld, ld, ho, wo, out_ld, out_ld
    d.kh, d.kw, d.stride, d.pad_t, d.pad_l, d.up2, d.dtype = k, k, stride, pad, pad, int(up2), 1
    if stats:
        d.gn_part, d.gn_hw = 64, ho * wo
    rows = int(_lib.load().rdeic_conv2d_band_rows(C.byref(d), tile))
    return rows, (0 if rows <= 0 else -(-ho // rows))


def _part(y):
    info = getattr(y, "_rdeic_gn_part", None)
    return None if info is None else info[0]


def _compare_forced(run, kind, limit, plan, n_img=1):
    """run() once on the default limit and once on `limit`: bit-identical output and partials, one launch per band."""
    from rdeic_amd import ops
    c0 = ops.launch_count(kind)
    y0 = run()
    one = ops.launch_count(kind) - c0
    assert one == 1, f"the fast kernel did not take the launch on the default limit ({one} launches)"
    with _limit(limit):
        rows, nb = plan()
        assert 3 <= nb <= 5, (rows, nb)
        c1 = ops.launch_count(kind)
        y1 = run()
        got = ops.launch_count(kind) - c1
    torch.cuda.synchronize()
    print(f"limit {limit}: {nb} bands of {rows} rows, {got} launches")
    assert got == nb * n_img
    assert torch.equal(y0, y1)
    p0, p1 = _part(y0), _part(y1)
    assert (p0 is None) == (p1 is None)
    if p0 is not None:  # 16-byte header (the rows per partial in its first word, the rest unwritten), then the sums
        assert torch.equal(p0[:1], p1[:1]) and torch.equal(p0[4:], p1[4:])
    return y0


# ---------------------------------------------------------------- forced limit, small shapes

@pytest.mark.parametrize("halo8", [0, 1])
@pytest.mark.parametrize("n,res", [(1, False), (2, True)])
def test_halo_bands_forced(gpu, halo8, n, res):
    """GN + SiLU 128 -> 128 at 40 x 64: the 4-row kernel in bands of 12, 12, 12, 4 rows, the 8-row kernel in 16, 16, 8;
    with a batch of 2 each image is banded (groups and bands in one call)."""
    from rdeic_amd import ops
    h, w, c = 40, 64, 128
    torch.manual_seed(10 * n + halo8)
    x = torch.randn(n, h, w, c, dtype=BF, device="cuda")
    r = torch.randn(n, h, w, c, dtype=BF, device="cuda") if res else None
    _, p = _pack(c, c, seed=1)
    ab = _ab(n, c, seed=2)
    tile = 8 if halo8 else 4
    rows_in = (16 if halo8 else 12) + 2
    assert h % rows_in != 0
    with _option(9, halo8):
        _compare_forced(lambda: ops.conv2d(x, p, gn=ab, gn_silu=True, res=r, stats=True), ops.COUNT_HALO_CONV,
                        rows_in * w * c * 2, lambda: _plan(h, w, c, h, w, c, tile, stats=True), n_img=n)


def test_dma_3x3_stats_bands_forced(gpu):
    from rdeic_amd import ops
    h, w, cin, cout = 48, 64, 256, 128
    x = torch.randn(1, h, w, cin, dtype=BF, device="cuda")
    _, p = _pack(cin, cout, seed=3)
    _compare_forced(lambda: ops.conv2d(x, p, stats=True), ops.COUNT_DMA_CONV, 12 * w * cin * 2,  # 10 rows + 2
                    lambda: _plan(h, w, cin, h, w, cout, 1, stats=True))


def test_dma_1x1_bands_forced(gpu):
    from rdeic_amd import ops
    h, w, cin, cout = 48, 64, 256, 128
    x = torch.randn(1, h, w, cin, dtype=BF, device="cuda")
    _, p = _pack(cin, cout, seed=4, k=1, pad=0)
    _compare_forced(lambda: ops.conv2d(x, p), ops.COUNT_DMA_CONV, 10 * w * cin * 2,
                    lambda: _plan(h, w, cin, h, w, cout, 1, k=1, pad=0))


def test_dma_stride2_asymmetric_pad_bands_forced(gpu):
    """The VAE Downsample: 3x3, stride 2, zero pad on the bottom / right only. Bands of 7 output rows = 15 input
    rows; an interior band starts at an input row with no padding above it."""
    from rdeic_amd import ops
    h, w, c = 64, 64, 128
    x = torch.randn(1, h, w, c, dtype=BF, device="cuda")
    _, p = _pack(c, c, seed=5, stride=2, pad=0)
    _compare_forced(lambda: ops.conv2d(x, p, pad_t=0, pad_l=0, out_hw=(h // 2, w // 2)), ops.COUNT_DMA_CONV,
                    15 * w * c * 2, lambda: _plan(h, w, c, h // 2, w // 2, c, 1, stride=2, pad=0))


def test_dma_concat_emb_residual_bands_forced(gpu):
    """Two-input concat 64 + 64 -> 128 with a per-image embedding and a residual: the output rows are the wider
    span (bands of 7 rows)."""
    from rdeic_amd import ops
    h, w, c, cout = 32, 64, 64, 128
    x = torch.randn(1, h, w, c, dtype=BF, device="cuda")
    x2 = torch.randn(1, h, w, c, dtype=BF, device="cuda")
    r = torch.randn(1, h, w, cout, dtype=BF, device="cuda")
    emb = torch.randn(1, cout, device="cuda")
    _, p = _pack(2 * c, cout, seed=6)
    _compare_forced(lambda: ops.conv2d(x, p, x2=x2, emb=emb, res=r), ops.COUNT_DMA_CONV, 7 * w * cout * 2,
                    lambda: _plan(h, w, c, h, w, cout, 1))


def test_up2_phase_bands_forced(gpu):
    """Nearest-x2 + 3x3 as four folded phase convs, 128 -> 128 from 24 x 32: bands of 20, 20, 8 output rows (whole
    source rows, whole 64-row statistic blocks of every phase)."""
    from rdeic_amd import ops
    h, w, c = 24, 32, 128
    x = torch.randn(1, h, w, c, dtype=BF, device="cuda")
    wt, p = _pack(c, c, seed=7)
    ph = _phase_pack(wt, p)
    _compare_forced(lambda: ops.conv2d(x, p, up2=True, stats=True, phases=ph), ops.COUNT_DMA_CONV, 20 * 2 * w * c * 2,
                    lambda: _plan(h, w, c, 2 * h, 2 * w, c, 1, up2=True, stats=True))


def test_narrow_bands_and_groups_forced(gpu):
    """norm -> SiLU -> conv 128 -> 3 (fp32 out): 40 x 64 in bands of 16, 16, 8 rows; 3 x 16 x 64 in image groups only."""
    from rdeic_amd import ops
    c = 128
    _, p = _pack(c, 3, seed=8)
    x = torch.randn(1, 40, 64, c, dtype=BF, device="cuda")
    ab = _ab(1, c, seed=9)
    _compare_forced(lambda: ops.conv2d(x, p, gn=ab, gn_silu=True, out_f32=True), ops.COUNT_EDGE, 18 * 64 * c * 2,
                    lambda: _plan(40, 64, c, 40, 64, 3, 8))
    x3 = torch.randn(3, 16, 64, c, dtype=BF, device="cuda")
    ab3 = _ab(3, c, seed=10)
    y0 = ops.conv2d(x3, p, gn=ab3, gn_silu=True, out_f32=True)
    with _limit(16 * 64 * c * 2 + 4096):  # one image per launch, no bands
        assert _plan(16, 64, c, 16, 64, 3, 8)[0] == 16
        c0 = ops.launch_count(ops.COUNT_EDGE)
        y1 = ops.conv2d(x3, p, gn=ab3, gn_silu=True, out_f32=True)
        assert ops.launch_count(ops.COUNT_EDGE) - c0 == 3
    assert torch.equal(y0, y1)


# ---------------------------------------------------------------- real single images past the 2 GiB reach

def _crop_starts(h, rows_per_band, row_bytes, crop=72):
    """First rows of the 72-row crops: top, bottom, around every band boundary, around byte offset 2^31."""
    marks = list(range(rows_per_band, h, rows_per_band)) + [2 ** 31 // row_bytes]
    starts = {0, h - crop}
    for m in marks:
        if 0 < m < h:
            starts.add(min(max(m - crop // 2, 0), h - crop) // 8 * 8)
    return sorted(starts)


def _check_crops(y, run_crop, starts, h, crop=72, scale=1):
    """run_crop(a) = the same kernel on input rows [a, a + crop) as an image of its own. Its border rows see zero
    padding where the large image has neighbours, so interior rows are compared, plus the image's own top / bottom."""
    for a in starts:
        yc = run_crop(a)
        lo = 0 if a == 0 else scale
        hi = scale * crop if a + crop == h else scale * (crop - 1)
        assert torch.equal(y[:, scale * a + lo:scale * a + hi], yc[:, lo:hi]), f"crop at row {a}"
        del yc


def test_halo8_single_image_past_2gib(gpu):
    from rdeic_amd import ops
    h, w, c = 4160, 2048, 128   # 2.18 GB in and out
    x = torch.randn(1, h, w, c, dtype=BF, device="cuda")
    _, p = _pack(c, c, seed=11)
    ab = _ab(1, c, seed=12)
    rows, nb = _plan(h, w, c, h, w, c, 8, stats=True)
    assert nb >= 2 and rows % 8 == 0
    c0 = ops.launch_count(ops.COUNT_HALO_CONV)
    y = ops.conv2d(x, p, gn=ab, gn_silu=True, stats=True)
    assert ops.launch_count(ops.COUNT_HALO_CONV) - c0 == nb
    _check_crops(y, lambda a: ops.conv2d(x[:, a:a + 72], p, gn=ab, gn_silu=True), _crop_starts(h, rows, w * c * 2), h)
    # the fused partials of the banded launches: the affine they give against the stand-alone statistics pass
    g = torch.Generator().manual_seed(13)
    gamma, beta = (1 + 0.1 * torch.randn(c, generator=g)).cuda(), (0.1 * torch.randn(c, generator=g)).cuda()
    assert _part(y) is not None
    ab_f = ops.group_norm_ab(y, gamma, beta, 32, 1e-6)
    yv = y.view(y.shape)  # a view carries no partials: the stand-alone pass reads the tensor
    ab_s = ops.group_norm_ab(yv, gamma, beta, 32, 1e-6)
    torch.testing.assert_close(ab_f, ab_s, rtol=2e-4, atol=2e-5)
    # GroupNorm apply on the > 2 GiB tensor against crops, bit for bit
    z = ops.group_norm_apply(y, ab_f, True)
    for a in _crop_starts(h, rows, w * c * 2):
        assert torch.equal(z[:, a:a + 72], ops.group_norm_apply(y[:, a:a + 72], ab_f, True)), f"apply crop at {a}"
    del x, y, z
    torch.cuda.empty_cache()


def test_narrow_single_image_4gib(gpu):
    """128 -> 3 at 4096 x 4096: the input is exactly 4 GiB. Without bands the kernel's 32-bit record count wraps to
    zero, every load reads as out of range and the output is the bias alone."""
    from rdeic_amd import ops
    h, w, c = 4096, 4096, 128
    x = torch.randn(1, h, w, c, dtype=BF, device="cuda")
    _, p = _pack(c, 3, seed=14)
    ab = _ab(1, c, seed=15)
    rows, nb = _plan(h, w, c, h, w, 3, 8)
    assert nb >= 3 and rows % 8 == 0
    c0 = ops.launch_count(ops.COUNT_EDGE)
    y = ops.conv2d(x, p, gn=ab, gn_silu=True, out_f32=True)
    assert ops.launch_count(ops.COUNT_EDGE) - c0 == nb
    assert (y[0, 100, 100] - p.bias).abs().max().item() > 1e-3  # not bias-only
    _check_crops(y, lambda a: ops.conv2d(x[:, a:a + 72], p, gn=ab, gn_silu=True, out_f32=True),
                 _crop_starts(h, rows, w * c * 2), h)
    del x, y
    torch.cuda.empty_cache()


def test_dma_single_image_past_2gib(gpu):
    from rdeic_amd import ops
    h, w, cin, cout = 2112, 2048, 256, 128   # 2.2 GB in
    x = torch.randn(1, h, w, cin, dtype=BF, device="cuda")
    _, p = _pack(cin, cout, seed=16)
    rows, nb = _plan(h, w, cin, h, w, cout, 1, stats=True)
    assert nb >= 2
    c0 = ops.launch_count(ops.COUNT_DMA_CONV)
    y = ops.conv2d(x, p, stats=True)
    assert ops.launch_count(ops.COUNT_DMA_CONV) - c0 == nb
    _check_crops(y, lambda a: ops.conv2d(x[:, a:a + 72], p), _crop_starts(h, rows, w * cin * 2), h)
    del x, y
    torch.cuda.empty_cache()


def test_up2_phases_single_image_past_2gib(gpu):
    from rdeic_amd import ops
    h, w, c = 1088, 1024, 256   # 2.28 GB out
    x = torch.randn(1, h, w, c, dtype=BF, device="cuda")
    wt, p = _pack(c, c, seed=17)
    ph = _phase_pack(wt, p)
    rows, nb = _plan(h, w, c, 2 * h, 2 * w, c, 1, up2=True, stats=True)
    assert nb >= 2 and rows % 2 == 0
    c0 = ops.launch_count(ops.COUNT_DMA_CONV)
    y = ops.conv2d(x, p, up2=True, stats=True, phases=ph)
    assert ops.launch_count(ops.COUNT_DMA_CONV) - c0 == nb
    # crops in source rows; band boundaries and the 2^31 offset are output rows
    starts = _crop_starts(h, rows // 2, 2 * (2 * w) * c * 2)
    _check_crops(y, lambda a: ops.conv2d(x[:, a:a + 72], p, up2=True, phases=ph), starts, h, scale=2)
    del x, y
    torch.cuda.empty_cache()
