"""What runs is what the plan says (rdeic_conv2d_plan): for the smallest shape of every conv route, the library's
launch counters move by the plan's route and number of launches, on the default launch limit and on a lowered one,
and the output does not depend on the limit (bit for bit).

The lowered limit forces at least three slices wherever the route can be sliced. Three cases cannot be, as stated:
the 4-row halo shape is one row tile high (a single image of it has no smaller band: it is run as three images, one
image per launch), and conv_in, the register tiles and the direct kernel are never sliced (conv_in past the limit
leaves its route; the plan says so and the counters must agree)."""
import contextlib
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
KIB = 1024


@contextlib.contextmanager
def _limit(nbytes):
    from rdeic_amd import ops
    prev = ops.set_launch_limit(nbytes)
    try:
        yield
    finally:
        ops.set_launch_limit(prev)


def _pack(cin, cout, k, seed):
    from rdeic_amd import ops
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    return ops.ConvParams.pack(w.cuda(), (torch.randn(cout, generator=g) * 0.1).cuda(), pad=k // 2)


def _ab(n, c, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([0.8 + 0.2 * torch.rand(n, c, generator=g), 0.3 * torch.randn(n, c, generator=g)], -1).cuda()


def _counted(run, monkeypatch):
    """run() with every descriptor ops.conv2d plans captured: (output, counter deltas, the plans of rdeic_conv2d)."""
    from rdeic_amd import _lib, ops
    kinds = (ops.COUNT_HALO_CONV, ops.COUNT_EDGE, ops.COUNT_DMA_CONV, ops.COUNT_GN_APPLY, ops.COUNT_GN_PARTS_APPLY)
    descs = []
    real = ops._conv_plan

    def spy(d, tile=-1):
        descs.append(_lib.ConvDesc.from_buffer_copy(d))
        return real(d, tile)

    monkeypatch.setattr(ops, "_conv_plan", spy)
    monkeypatch.setattr(ops, "TILE_TABLE", {})  # no table tile: every conv below goes through rdeic_conv2d
    c0 = [ops.launch_count(k) for k in kinds]
    y = run()
    torch.cuda.synchronize()
    delta = dict(zip(kinds, (ops.launch_count(k) - c for k, c in zip(kinds, c0))))
    monkeypatch.setattr(ops, "_conv_plan", real)
    plans = []
    for d in descs:
        p = _lib.ConvPlan()
        assert _lib.load().rdeic_conv2d_plan(C.byref(d), -2, C.byref(p)) == 0
        plans.append(p)
    return y, delta, plans


def _expected(plans, deferred=False):
    """Counter deltas the plans imply: the materialise step (one GroupNorm apply launch), then the conv's slices."""
    from rdeic_amd import _lib, ops
    want = {ops.COUNT_HALO_CONV: 0, ops.COUNT_EDGE: 0, ops.COUNT_DMA_CONV: 0, ops.COUNT_GN_APPLY: 0,
            ops.COUNT_GN_PARTS_APPLY: 0}
    by_route = {_lib.ROUTE_HALO: ops.COUNT_HALO_CONV, _lib.ROUTE_EDGE_IN8: ops.COUNT_EDGE,
                _lib.ROUTE_EDGE_NARROW: ops.COUNT_EDGE, _lib.ROUTE_DMA: ops.COUNT_DMA_CONV}
    for p in plans:
        if p.route == _lib.ROUTE_MATERIALIZE:
            want[ops.COUNT_GN_PARTS_APPLY if deferred else ops.COUNT_GN_APPLY] += 1
        elif p.route in by_route:
            want[by_route[p.route]] += p.launches
    return want


def _check(run, monkeypatch, routes, lowered, sliced, deferred=False, routes_lowered=None):
    """routes: the plan routes of one run() on the default limit (routes_lowered: on the lowered one, default the
    same). sliced: the last plan has at least three launches on the lowered limit."""
    y0, d0, p0 = _counted(run, monkeypatch)
    assert [p.route for p in p0] == routes and p0[-1].launches == 1
    assert d0 == _expected(p0, deferred), (d0, [(p.route, p.launches) for p in p0])
    with _limit(lowered):
        y1, d1, p1 = _counted(run, monkeypatch)
    print(f"lowered limit {lowered}: " + ", ".join(f"route {p.route} x {p.launches} ({p.images} images, {p.rows} rows)"
                                                   for p in p1), d1)
    assert [p.route for p in p1] == (routes_lowered or routes)
    assert (p1[-1].launches >= 3) == sliced
    assert d1 == _expected(p1, deferred), (d1, [(p.route, p.launches) for p in p1])
    assert torch.equal(y0, y1)


def _gn_conv(n, h, w, c, cout, res=False, seed=0):
    from rdeic_amd import ops
    torch.manual_seed(seed)
    x = torch.randn(n, h, w, c, dtype=BF, device="cuda")
    r = torch.randn(n, h, w, cout, dtype=BF, device="cuda") if res else None
    p, ab = _pack(c, cout, 3, seed + 1), _ab(n, c, seed + 2)
    return lambda: ops.conv2d(x, p, gn=ab, gn_silu=True, res=r)


def test_halo_4row(gpu, monkeypatch):
    from rdeic_amd import _lib
    # 1 x 4 x 64 x 32 -> 128 with a residual: one tile row, one launch
    _, d, plans = _counted(_gn_conv(1, 4, 64, 32, 128, res=True), monkeypatch)
    assert [(p.route, p.launches) for p in plans] == [(_lib.ROUTE_HALO, 1)] and d == _expected(plans)
    # three such images, one image (64 KiB of output) per launch on the lowered limit
    _check(_gn_conv(3, 4, 64, 32, 128, res=True), monkeypatch, [_lib.ROUTE_HALO], 64 * KIB, True)


def test_halo_8row(gpu, monkeypatch):
    from rdeic_amd import _lib
    # 16 KiB per output row: bands of 8 rows of each of the 2 images
    _check(_gn_conv(2, 16, 64, 32, 128), monkeypatch, [_lib.ROUTE_HALO], 128 * KIB, True)


def test_narrow(gpu, monkeypatch):
    from rdeic_amd import _lib
    # 4 KiB per input row: 8 output rows read 10
    _check(_gn_conv(2, 16, 64, 32, 3), monkeypatch, [_lib.ROUTE_EDGE_NARROW], 40 * KIB, True)


def test_conv_in(gpu, monkeypatch):
    from rdeic_amd import _lib, ops
    x = torch.randn(1, 8, 64, 8, dtype=BF, device="cuda")
    p = _pack(8, 32, 3, 5)
    # never sliced: an 8 KiB input past the limit leaves the route for the direct kernel (same k order)
    _check(lambda: ops.conv2d(x, p), monkeypatch, [_lib.ROUTE_EDGE_IN8], 4 * KIB, False,
           routes_lowered=[_lib.ROUTE_DIRECT])


@pytest.mark.parametrize("k", [3, 1])
def test_dma(gpu, monkeypatch, k):
    from rdeic_amd import _lib, ops
    x = torch.randn(2, 16, 16, 64, dtype=BF, device="cuda")
    p = _pack(64, 64, k, 6 + k)
    # 2 KiB per row: 4-row bands (6 input rows) of the 3x3 conv, 6-row bands of the 1x1
    _check(lambda: ops.conv2d(x, p), monkeypatch, [_lib.ROUTE_DMA], 12 * KIB, True)


def test_register_tile(gpu, monkeypatch):
    from rdeic_amd import _lib, ops
    x = torch.randn(1, 16, 16, 40, dtype=BF, device="cuda")
    p = _pack(40, 64, 3, 8)
    _check(lambda: ops.conv2d(x, p), monkeypatch, [_lib.ROUTE_TILE], 4 * KIB, False)


def test_direct(gpu, monkeypatch):
    from rdeic_amd import _lib, ops
    x = torch.randn(1, 16, 16, 32, dtype=BF, device="cuda")
    p = _pack(32, 16, 3, 9)
    _check(lambda: ops.conv2d(x, p), monkeypatch, [_lib.ROUTE_DIRECT], 4 * KIB, False)


@pytest.mark.parametrize("deferred", [False, True])
def test_materialize(gpu, monkeypatch, deferred):
    """1 x 16 x 16 x 64 -> 64 with a GroupNorm input (w % 64 != 0: no halo): the apply launch, then the LDS-DMA conv.
    deferred: the affine's finalize is pending (group_norm_ab(defer=True) after a conv with fused statistics) and
    runs inside the apply launch (rdeic_groupnorm_parts_apply)."""
    from rdeic_amd import _lib, ops
    c = 64
    x0 = torch.randn(1, 16, 16, c, dtype=BF, device="cuda")
    p0, p = _pack(c, c, 1, 10), _pack(c, c, 3, 11)
    x = ops.conv2d(x0, p0, stats=True)
    g = torch.Generator().manual_seed(12)
    gamma, beta = (1 + 0.2 * torch.randn(c, generator=g)).cuda(), (0.2 * torch.randn(c, generator=g)).cuda()

    def run():
        ab = ops.group_norm_ab(x, gamma, beta, 32, 1e-6, defer=deferred)
        assert hasattr(ab, "_rdeic_pending") == deferred
        return ops.conv2d(x, p, gn=ab, gn_silu=True)

    _check(run, monkeypatch, [_lib.ROUTE_MATERIALIZE, _lib.ROUTE_DMA], 12 * KIB, True, deferred=deferred)
