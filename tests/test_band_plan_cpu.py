"""The row-band planner of the fast conv kernels (rdeic_conv2d_band_rows, rdeic_set_conv_option key 12): host
arithmetic only, no GPU. One image whose tensors exceed the launch limit (the 2 GiB reach of a 32-bit byte offset)
runs as bands of output rows; every band's input, output and residual spans must stay inside the limit, bands must
tile the output rows exactly once, and their heights must respect the kernel's row tile and the 64-row statistic
blocks."""
import ctypes as C
import math

import pytest

from rdeic_amd import _lib

DEFAULT = 2 ** 31 - 1
MIB = 1 << 20


def _desc(n, h, w, cin, cout, *, k=3, stride=1, pad=1, up2=False, ho=None, wo=None, stats=False, res=False):
    d = _lib.ConvDesc()
    d.n, d.h, d.w, d.c0, d.ld0 = n, h, w, cin, cin
    d.cout, d.out_ld, d.kh, d.kw, d.stride, d.pad_t, d.pad_l = cout, cout, k, k, stride, pad, pad
    d.up2 = int(up2)
    hi, wi = (2 * h, 2 * w) if up2 else (h, w)
    d.ho = ho if ho is not None else (hi + 2 * pad - k) // stride + 1
    d.wo = wo if wo is not None else (wi + 2 * pad - k) // stride + 1
    d.dtype = 1
    if stats:
        d.gn_part, d.gn_hw = 64, d.ho * d.wo  # any non-null address: the planner never reads through it
    if res:
        d.res, d.res_ld = 64, cout
    return d


def _in_rows(d, r0, rows):
    """Stored input rows [lo, hi) a band of output rows [r0, r0 + rows) reads (exact, from the conv geometry)."""
    if d.up2:  # 3x3 / pad 1 on the nearest-x2 image: upsampled rows r0 - 1 .. r0 + rows, halved
        lo, hi = (r0 - 1) // 2, (r0 + rows) // 2 + 1
    else:
        lo, hi = r0 * d.stride - d.pad_t, (r0 + rows - 1) * d.stride - d.pad_t + d.kh
    return max(lo, 0), min(hi, d.h)


def _check_plan(d, rows, tile, limit):
    assert 0 < rows <= d.ho
    starts = list(range(0, d.ho, rows))
    covered = 0
    for r0 in starts:
        rb = min(rows, d.ho - r0)
        lo, hi = _in_rows(d, r0, rb)
        in_span = (hi - lo) * d.w * d.ld0 * 2
        out_span = rb * d.wo * max(d.out_ld, d.res_ld if d.res else 0) * 2
        assert in_span <= limit and out_span <= limit, (r0, rb, in_span, out_span, limit)
        if rows < d.ho:
            assert rb % max(tile, 1) == 0, (r0, rb, tile)
            if d.up2:
                assert rb % 2 == 0
            if d.gn_part:  # whole 64-row statistic blocks (up2: of each phase's rb/2 x wo/2 source pixels)
                assert (rb * d.wo) % (256 if d.up2 else 64) == 0, (r0, rb)
        covered += rb
    assert covered == d.ho  # consecutive bands from 0: [0, ho) exactly once
    return len(starts)


@pytest.fixture
def lib():
    lib = _lib.load()
    prev = lib.rdeic_set_conv_option(12, DEFAULT)
    yield lib
    lib.rdeic_set_conv_option(12, prev)


CASES = {
    "4096x4096x128": dict(n=1, h=4096, w=4096, cin=128, cout=128),
    "2048x2112x256": dict(n=1, h=2048, w=2112, cin=256, cout=128),
    "1024x1088x256_up2": dict(n=1, h=1024, w=1088, cin=256, cout=256, up2=True),
    "3x1024x1024x128": dict(n=3, h=1024, w=1024, cin=128, cout=128),
}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("tile", [1, 4, 8])
@pytest.mark.parametrize("stats", [False, True])
def test_default_limit_plans(lib, name, tile, stats):
    d = _desc(**CASES[name], stats=stats, res=(tile > 1))
    rows = lib.rdeic_conv2d_band_rows(C.byref(d), tile)
    span = max(d.h * d.w * d.ld0 * 2, d.ho * d.wo * d.out_ld * 2)
    print(f"{name} tile {tile} stats {stats}: image span {span} bytes, {rows} rows per band of {d.ho}")
    if span <= DEFAULT:
        assert rows == d.ho  # a descriptor that fits is not banded
    else:
        assert rows < d.ho
        assert _check_plan(d, rows, tile, DEFAULT) >= 2


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("tile", [1, 4, 8])
def test_one_mib_limit(lib, name, tile):
    """At 1 MiB a 4096- or 2112-pixel row of 128 / 256 channels does not leave room for the three input rows of one
    output row: no plan. The 1024-pixel rows (256 KiB) fit two output rows for the tile-free LDS-DMA path only."""
    assert lib.rdeic_set_conv_option(12, MIB) == DEFAULT
    d = _desc(**CASES[name], stats=True)
    rows = lib.rdeic_conv2d_band_rows(C.byref(d), tile)
    print(f"{name} tile {tile}: {rows} rows per band at 1 MiB")
    if name == "3x1024x1024x128" and tile == 1:
        assert rows == 2
        assert _check_plan(d, rows, tile, MIB) == 512
    else:
        assert rows == 0


@pytest.mark.parametrize("limit", [3 * MIB, 16 * MIB, 100 * MIB + 12345, 1 << 30])
@pytest.mark.parametrize("tile", [1, 4, 8])
def test_lowered_limits(lib, limit, tile):
    lib.rdeic_set_conv_option(12, limit)
    shapes = [_desc(1, 1024, 1024, 128, 128, stats=True, res=True),
              _desc(1, 1024, 1088, 256, 128, stats=True),
              _desc(1, 512, 576, 256, 256, up2=True, stats=True),
              _desc(1, 1024, 1024, 128, 128, k=1, pad=0),
              _desc(1, 1024, 1024, 128, 128, stride=2, pad=0, ho=512, wo=512, stats=True),
              _desc(1, 1000, 200, 64, 320, stats=True)]  # 200-pixel rows: 8 rows per whole statistic block
    for d in shapes:
        rows = lib.rdeic_conv2d_band_rows(C.byref(d), tile)
        span = max(d.h * d.w * d.ld0 * 2, d.ho * d.wo * d.out_ld * 2)
        if span <= limit:
            assert rows == d.ho
        elif rows:
            nb = _check_plan(d, rows, tile, limit)
            print(f"limit {limit} tile {tile} {d.h}x{d.w}x{d.c0}->{d.cout}: {nb} bands of {rows}")
        else:  # no plan: an interior band of the smallest height (tile, statistic blocks) does not fit
            q = (256 if d.up2 else 64) if d.gn_part else 1
            step = math.lcm(max(tile, 1), 2 if d.up2 else 1, q // math.gcd(d.wo, q))
            lo, hi = _in_rows(d, step, step)
            need = max((hi - lo) * d.w * d.ld0 * 2, step * d.wo * d.out_ld * 2)
            assert need > limit, (step, need, limit)


def test_option_clamps_and_returns_previous(lib):
    assert lib.rdeic_set_conv_option(12, 12345) == DEFAULT
    assert lib.rdeic_set_conv_option(12, 0) == 12345       # non-positive: the default
    assert lib.rdeic_set_conv_option(12, DEFAULT) == DEFAULT


def test_up2_group_still_rejects_oversized_image(lib):
    """rdeic_conv2d_up2_group keeps its meaning (0 = one image is too large) while the planner bands that image."""
    d = _desc(2, 1024, 1024, 256, 256, up2=True)
    assert lib.rdeic_conv2d_up2_group(C.byref(d)) == 0
    rows = lib.rdeic_conv2d_band_rows(C.byref(d), 1)
    assert 0 < rows < d.ho
    _check_plan(d, rows, 1, DEFAULT)
