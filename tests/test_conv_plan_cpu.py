"""The conv planner (rdeic_conv2d_plan, rdeic_amd/csrc/conv_route.cpp): host arithmetic only, no launches, no GPU.
Which kernel family a descriptor runs on, how a launch past the launch limit is cut into image groups / row bands,
and which descriptors are rejected."""
import ctypes as C
import json
import os

import pytest

from rdeic_amd import _lib
from rdeic_amd._lib import (ROUTE_DIRECT, ROUTE_DMA, ROUTE_EDGE_IN8, ROUTE_EDGE_NARROW, ROUTE_HALO, ROUTE_MATERIALIZE,
                            ROUTE_SMALLC, ROUTE_TILE)

DEFAULT = 2 ** 31 - 1
MIB = 1 << 20
A = 0x10000000  # a 16-byte-aligned address; the planner never reads through a pointer
NAMES = {ROUTE_EDGE_IN8: "EDGE_IN8", ROUTE_EDGE_NARROW: "EDGE_NARROW", ROUTE_HALO: "HALO", ROUTE_SMALLC: "SMALLC",
         ROUTE_DMA: "DMA", ROUTE_TILE: "TILE", ROUTE_DIRECT: "DIRECT", ROUTE_MATERIALIZE: "MATERIALIZE"}
OPTION_DEFAULTS = {0: 1, 5: 1, 6: 1, 9: 1, 10: 1, 12: DEFAULT}


def _desc(n, h, w, c, cout, *, k=3, stride=1, pad=None, c1=0, up2=False, gn=False, emb=False, res=False, out_ld=None,
          out_f32=False, dtype=1, out_mode=0, batch=1, in_off=0, stats=False):
    """A valid descriptor: c input channels (the last c1 of them a second concat segment), packed weights."""
    d = _lib.ConvDesc()
    pad = k // 2 if pad is None else pad
    c0 = c - c1
    d.in0, d.c0, d.ld0 = A + in_off, c0, c0
    if c1:
        d.in1, d.c1, d.ld1 = 2 * A, c1, c1
    d.n, d.h, d.w, d.up2 = n, h, w, int(up2)
    d.weight, d.wld = 3 * A, (k * k * c + 63) // 64 * 64
    d.cout, d.kh, d.kw, d.stride, d.pad_t, d.pad_l = cout, k, k, stride, pad, pad
    hi, wi = (2 * h, 2 * w) if up2 else (h, w)
    d.ho, d.wo = (hi + 2 * pad - k) // stride + 1, (wi + 2 * pad - k) // stride + 1
    if gn:
        d.gn_ab, d.gn_silu = 4 * A, 1
    if emb:
        d.emb, d.emb_ld = 5 * A, cout
    ow = cout // 2 if out_mode == 2 else cout // 4 if out_mode == 1 else cout
    d.out, d.out_ld, d.out_mode = 6 * A, out_ld or ow, out_mode
    if res:
        d.res, d.res_ld = 7 * A, ow
    d.dtype, d.out_f32, d.batch = dtype, int(out_f32), batch
    if batch > 1:
        d.in_bs, d.w_bs, d.out_bs = n * h * w * c0, cout * d.wld, n * d.ho * d.wo * cout
    if stats:
        d.gn_part, d.gn_hw = 8 * A, d.ho * d.wo
    return d


def _plan(lib, d, tile=-2):
    p = _lib.ConvPlan()
    rc = lib.rdeic_conv2d_plan(C.byref(d), tile, C.byref(p))
    return rc, p


@pytest.fixture
def lib():
    """The library with every switch the routes read at its default, restored afterwards."""
    lib = _lib.load()
    prev = {k: lib.rdeic_set_conv_option(k, v) for k, v in OPTION_DEFAULTS.items()}
    prev_path = lib.rdeic_set_conv_path(2)
    yield lib
    for k, v in prev.items():
        lib.rdeic_set_conv_option(k, v)
    lib.rdeic_set_conv_path(prev_path)


# ---- 1. GroupNorm-input convs: the routes the parent's Python mirrors implied ----
TABLE = json.load(open(os.path.join(os.path.dirname(__file__), "conv_routes_parent.json")))


def _table_desc(k, c, cout, n, h, w, bits):
    f = {name for i, name in enumerate(TABLE["flag_bits"]) if bits >> i & 1}
    return _desc(n, h, w, c, cout, k=k, c1=c // 2 if "concat" in f else 0, up2="up2" in f, gn=True, emb="emb" in f,
                 res="res" in f, out_ld=2 * cout if "sliced" in f else None, out_f32="out_f32" in f)


def _smallc_rung(d):
    """The small-cout rung of the parent's ladder (conv2d_run: bf16, 3x3 / stride 1 / pad 1 to <= 4 channels from
    one 32-channel-aligned input). It takes GroupNorm inputs (the kernel applies the affine while staging), so where
    the three mirrors all said no, the parent ran this kernel and not the direct one: the route is SMALLC there."""
    return d.cout <= 4 and d.kh == 3 and d.kw == 3 and d.c0 % 32 == 0 and not d.c1 and not d.up2


def test_groupnorm_routes_match_parent_mirrors(lib):
    bad = []
    for k, c, cout, n, h, w, bits, limit, halo, narrow, mat in TABLE["rows"]:
        lib.rdeic_set_conv_option(12, limit or DEFAULT)
        d = _table_desc(k, c, cout, n, h, w, bits)
        want = ROUTE_EDGE_NARROW if narrow else ROUTE_HALO if halo else ROUTE_MATERIALIZE if mat else \
            ROUTE_SMALLC if _smallc_rung(d) else ROUTE_DIRECT
        rc, p = _plan(lib, d)
        if rc != 0 or p.route != want:
            bad.append(((k, c, cout, n, h, w, bits, limit), NAMES[want], rc, NAMES.get(p.route)))
    assert len(TABLE["rows"]) > 6000
    assert not bad, bad[:20]


def test_groupnorm_routes_where_the_mirror_disagreed(lib):
    """At a 1 MiB launch limit the parent's _halo_eligible asked the band planner for 8-row bands of a bf16 output
    without a residual; the library bands the kernel form it runs (4-row tiles with emb / an fp32 output) on the
    real output, and finds a plan. The mirror said materialise, the library took the halo conv: its answer stands."""
    assert len(TABLE["mirror_disagrees"]) == 13
    for k, c, cout, n, h, w, bits, limit, halo, narrow, mat, library in TABLE["mirror_disagrees"]:
        assert (halo, narrow, mat) == (0, 0, 1) and library == "HALO"
        lib.rdeic_set_conv_option(12, limit)
        rc, p = _plan(lib, _table_desc(k, c, cout, n, h, w, bits))
        assert rc == 0 and p.route == ROUTE_HALO and p.launches > 1


# ---- 2. everything else: routes read off the parent's two ladders (conv2d_run, conv2d_tile_run) ----
ALIGNED = dict(n=2, h=16, w=16, c=128, cout=128)      # both concat segments multiples of 64 channels
UNALIGNED = dict(n=2, h=16, w=16, c=40, cout=64)      # 16-byte gathers, but no 64-channel blocks
HALO_SHAPE = dict(n=1, h=8, w=64, c=128, cout=128)    # tiles as 8 x 64 pixels x 128 channels
ROUTES = [
    # (name, descriptor, tile, {option: value}, conv path, route)
    ("conv_in", dict(n=1, h=64, w=64, c=8, cout=128), -2, {}, 2, ROUTE_EDGE_IN8),
    ("conv_in_tile", dict(n=1, h=64, w=64, c=8, cout=128), 3, {}, 2, ROUTE_EDGE_IN8),
    ("conv_in_edge_off", dict(n=1, h=64, w=64, c=8, cout=128), -2, {10: 0}, 2, ROUTE_TILE),
    ("geglu", dict(n=1, h=4096, w=1, c=320, cout=2560, k=1, out_mode=2), -2, {}, 2, ROUTE_DMA),
    ("geglu_dma_off", dict(n=1, h=4096, w=1, c=320, cout=2560, k=1, out_mode=2), -1, {5: 0}, 2, ROUTE_DMA),
    ("fp32", dict(**ALIGNED, dtype=0), -2, {}, 2, ROUTE_DIRECT),
    ("cout16", dict(n=2, h=16, w=16, c=64, cout=16), -2, {}, 2, ROUTE_DIRECT),
    ("cout32", dict(n=2, h=16, w=16, c=64, cout=32), 25, {}, 2, ROUTE_DIRECT),
    ("cout3_3x3", dict(n=1, h=16, w=16, c=128, cout=3), -2, {}, 2, ROUTE_SMALLC),
    ("cout3_1x1", dict(n=1, h=16, w=16, c=128, cout=3, k=1), -2, {}, 2, ROUTE_DIRECT),
    ("aligned", ALIGNED, -2, {}, 2, ROUTE_DMA),
    ("aligned_tile-1", ALIGNED, -1, {}, 2, ROUTE_TILE),
    ("aligned_tile3", ALIGNED, 3, {}, 2, ROUTE_TILE),
    ("aligned_tile25", ALIGNED, 25, {}, 2, ROUTE_DMA),
    ("unaligned", UNALIGNED, -2, {}, 2, ROUTE_TILE),
    ("unaligned_tile-1", UNALIGNED, -1, {}, 2, ROUTE_TILE),
    ("unaligned_tile3", UNALIGNED, 3, {}, 2, ROUTE_TILE),
    ("unaligned_tile25", UNALIGNED, 25, {}, 2, ROUTE_TILE),
    ("dma_off", ALIGNED, -2, {5: 0}, 2, ROUTE_TILE),
    ("dma_off_tile-1", ALIGNED, -1, {5: 0}, 2, ROUTE_TILE),
    ("dma_off_tile25", ALIGNED, 25, {5: 0}, 2, ROUTE_DMA),   # an explicit LDS-DMA tile is not gated by option 5
    ("halo0", HALO_SHAPE, -2, {6: 0}, 2, ROUTE_DMA),
    ("halo1", HALO_SHAPE, -2, {6: 1}, 2, ROUTE_DMA),
    ("halo2", HALO_SHAPE, -2, {6: 2}, 2, ROUTE_HALO),
    ("halo2_tile25", HALO_SHAPE, 25, {6: 2}, 2, ROUTE_DMA),  # conv2d_tile_run had no halo rung on the big-tile path
    ("halo0_gn", dict(**HALO_SHAPE, gn=True), -2, {6: 0}, 2, ROUTE_MATERIALIZE),
    ("narrow_edge_off", dict(n=2, h=16, w=64, c=128, cout=3, gn=True), -2, {10: 0}, 2, ROUTE_SMALLC),
    ("path0", ALIGNED, -2, {}, 0, ROUTE_DIRECT),
    ("path0_cout3", dict(n=1, h=16, w=16, c=128, cout=3), -2, {}, 0, ROUTE_DIRECT),
    ("batched_gemm", dict(n=1, h=256, w=1, c=64, cout=128, k=1, batch=8), -2, {}, 2, ROUTE_DMA),
    ("concat64+64", dict(**ALIGNED, c1=64), -2, {}, 2, ROUTE_DMA),
    ("concat88+40", dict(n=2, h=16, w=16, c=128, cout=128, c1=40), -2, {}, 2, ROUTE_TILE),
    ("stride2", dict(**ALIGNED, stride=2), -2, {}, 2, ROUTE_DMA),
    ("up2", dict(**ALIGNED, up2=True), -2, {}, 2, ROUTE_DMA),
    ("misaligned_input", dict(**ALIGNED, in_off=8), -2, {}, 2, ROUTE_DIRECT),
    # one image past the limit (its output), no band plan (one output row is 2 MiB), inputs inside the limit: the
    # whole launch still runs (dma_ok bounds the input spans only)
    ("no_band_plan", dict(n=1, h=8, w=1024, c=64, cout=1024, k=1), -2, {12: MIB}, 2, ROUTE_DMA),
]


@pytest.mark.parametrize("name,desc,tile,options,path,route", ROUTES, ids=[r[0] for r in ROUTES])
def test_routes(lib, name, desc, tile, options, path, route):
    for k, v in options.items():
        lib.rdeic_set_conv_option(k, v)
    lib.rdeic_set_conv_path(path)
    d = _desc(**desc)
    rc, p = _plan(lib, d, tile)
    assert rc == 0 and NAMES[p.route] == NAMES[route]
    if name == "no_band_plan":
        assert lib.rdeic_conv2d_band_rows(C.byref(d), 1) == 0
        assert (p.images, p.rows, p.launches) == (1, d.ho, 1)


# ---- 3. slices ----
def _in_rows(d, r0, rows):
    """Stored input rows [lo, hi) that output rows [r0, r0 + rows) read."""
    lo, hi = r0 * d.stride - d.pad_t, (r0 + rows - 1) * d.stride - d.pad_t + d.kh
    return max(lo, 0), min(hi, d.h)


SLICED = [
    # (name, descriptor, limit, route, row tile of rdeic_conv2d_band_rows)
    ("dma_groups", dict(n=7, h=64, w=64, c=128, cout=128, res=True), 3 * MIB, ROUTE_DMA, 1),
    ("dma_bands", dict(n=2, h=256, w=256, c=128, cout=256, res=True), 3 * MIB, ROUTE_DMA, 1),
    ("dma_bands_1x1_stats", dict(n=1, h=1000, w=200, c=64, cout=320, k=1, stats=True), 3 * MIB, ROUTE_DMA, 1),
    ("halo8_bands", dict(n=2, h=256, w=256, c=128, cout=128, gn=True, res=True), 3 * MIB, ROUTE_HALO, 8),
    ("halo4_bands", dict(n=1, h=252, w=256, c=128, cout=128, gn=True, stats=True), 3 * MIB, ROUTE_HALO, 4),
    ("halo_groups", dict(n=7, h=64, w=64, c=128, cout=128, gn=True), 3 * MIB, ROUTE_HALO, 8),
    ("narrow_bands", dict(n=2, h=256, w=256, c=128, cout=3, gn=True, out_f32=True), 3 * MIB, ROUTE_EDGE_NARROW, 8),
    ("narrow_groups", dict(n=7, h=64, w=64, c=128, cout=3, gn=True), 3 * MIB, ROUTE_EDGE_NARROW, 8),
]


@pytest.mark.parametrize("name,desc,limit,route,tile", SLICED, ids=[s[0] for s in SLICED])
def test_slices(lib, name, desc, limit, route, tile):
    lib.rdeic_set_conv_option(12, limit)
    d = _desc(**desc)
    rc, p = _plan(lib, d)
    assert rc == 0 and NAMES[p.route] == NAMES[route]
    assert p.launches >= 3 and 0 < p.images <= d.n and 0 < p.rows <= d.ho
    assert p.images == 1 or p.rows == d.ho  # image groups, or row bands of each image
    es, osz = 2, 4 if d.out_f32 else 2
    covered = set()
    count = 0
    for i0 in range(0, d.n, p.images):
        ni = min(p.images, d.n - i0)
        for r0 in range(0, d.ho, p.rows):
            rb = min(p.rows, d.ho - r0)
            lo, hi = (0, d.h) if p.rows == d.ho else _in_rows(d, r0, rb)
            in_span = (ni - 1) * d.h * d.w * d.ld0 * es + (hi - lo) * d.w * d.ld0 * es
            out_span = ((ni - 1) * d.ho + rb) * d.wo * d.out_ld * osz
            res_span = ((ni - 1) * d.ho + rb) * d.wo * d.res_ld * osz if d.res else 0
            assert max(in_span, out_span, res_span) <= limit, (i0, r0, in_span, out_span, res_span)
            if p.rows < d.ho:
                assert rb % tile == 0
                if d.gn_part:
                    assert (rb * d.wo) % 64 == 0  # whole 64-row statistic blocks
            cells = {(i, r) for i in range(i0, i0 + ni) for r in range(r0, r0 + rb)}
            assert not (cells & covered)
            covered |= cells
            count += 1
    assert len(covered) == d.n * d.ho  # [0, n) x [0, ho) exactly once
    assert count == p.launches
    if p.rows < d.ho:
        assert lib.rdeic_conv2d_band_rows(C.byref(d), tile) == p.rows


# ---- 4. rejections ----
def test_rejections(lib):
    d = _desc(**ALIGNED)
    assert _plan(lib, d)[0] == 0
    d.wld = 9 * 128 - 64  # wld < ktot
    assert _plan(lib, d)[0] == _lib.EINVAL
    d = _desc(**ALIGNED)
    d.out_mode = 3
    assert _plan(lib, d)[0] == _lib.EINVAL
    d = _desc(n=1, h=256, w=1, c=64, cout=128, k=1)
    d.ln_rows = 9 * A  # without ln_colsum
    assert _plan(lib, d)[0] == _lib.EINVAL
    d = _desc(n=1, h=256, w=1, c=64, cout=128, k=1, out_mode=2, res=True)  # GEGLU with a residual
    assert _plan(lib, d)[0] == _lib.EINVAL
    d = _desc(n=1, h=256, w=1, c=40, cout=128, k=1, out_mode=2)  # GEGLU outside the LDS-DMA kernel's shapes
    assert _plan(lib, d)[0] == _lib.EINVAL
    assert lib.rdeic_conv2d_plan(None, -2, C.byref(_lib.ConvPlan())) == _lib.EINVAL
