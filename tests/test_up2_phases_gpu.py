"""rdeic_conv2d_up2_phases: the nearest-x2 upsample 3x3 conv run as four folded 2x2 phase convs in one
LDS-DMA launch (4/9 of the MACs), against float64 truth and against the fused-gather path it replaces.

Shapes (the smallest that reach each mechanism): n=2 8x8 64->128 (one M tile, every border); n=1 6x10 128->64
(ragged M below a tile, h*w % 64 != 0: the statistics fall back to the pass over the output); n=3 16x16 64->320
(fused statistics, a partial N tile, several images). Each with and without bias.

(a) the phase path's max-abs and rms error against float64 truth (fp32 master weights, bf16 inputs) is at
    most 2x the fused-gather path's: the worst case of rounding a four-weight corner sum once against four
    independently rounded weights of one sign;
(b) the fused statistics, finalized by rdeic_groupnorm_parts_ab, equal rdeic_groupnorm_stats of the produced
    tensor within tests/test_gn_fused_gpu.py's tolerance;
(c) two runs are bit-equal and a launch plan's replay is bit-equal to eager;
(d) with the switch off (in Python, or in the library alone) the output is bit-identical to the fused gather's.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(2, 8, 8, 64, 128), (1, 6, 10, 128, 64), (3, 16, 16, 64, 320)]
CASES = [s + (b,) for s in SHAPES for b in (True, False)]
_CACHE: dict = {}


def _case(case):
    """Inputs, both packs, float64 truth and both paths' outputs of a case, computed once."""
    if case in _CACHE:
        return _CACHE[case]
    from rdeic_amd import ops
    from rdeic_amd.params import ParamStore
    n, h, w, cin, cout, bias = case
    g = torch.Generator().manual_seed(1000 * h + cin + int(bias))
    wt = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)
    bs = torch.randn(cout, generator=g) * 0.1 if bias else None
    x = (torch.randn(n, h, w, cin, generator=g) * 1.5 + 0.25).to(torch.bfloat16)
    store = ParamStore()
    store.declare_conv("up", cout, cin, 3, bias=bias)
    store.t["up.weight"] = wt.cuda()
    if bias:
        store.t["up.bias"] = bs.cuda()
    p, ph = store.conv("up"), store.conv_up2_phases("up")
    assert ph is not None and tuple(ph.weight.shape) == (4, cout, 4 * cin) and ph.weight.dtype == torch.bfloat16
    truth = F.conv2d(F.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2, mode="nearest"), wt.double(),
                     None if bs is None else bs.double(), padding=1).permute(0, 2, 3, 1).contiguous()
    xg = x.cuda()
    assert ops.UP2_PHASES
    y_ph = ops.conv2d(xg, p, up2=True, stats=True, phases=ph)
    y_old = ops.conv2d(xg, p, up2=True, stats=True)
    torch.cuda.synchronize()
    _CACHE[case] = dict(x=xg, p=p, ph=ph, truth=truth, y_ph=y_ph, y_old=y_old)
    return _CACHE[case]


@pytest.mark.parametrize("case", CASES)
def test_error_against_float64_truth(gpu, case):
    c = _case(case)
    assert not torch.equal(c["y_ph"], c["y_old"])  # the phase launch ran (its weights round differently)
    e_ph = c["y_ph"].double().cpu() - c["truth"]
    e_old = c["y_old"].double().cpu() - c["truth"]
    mx_ph, mx_old = e_ph.abs().max().item(), e_old.abs().max().item()
    rms_ph, rms_old = e_ph.pow(2).mean().sqrt().item(), e_old.pow(2).mean().sqrt().item()
    print(f"{case}: max abs {mx_ph:.4e} vs {mx_old:.4e} (ratio {mx_ph / mx_old:.3f}), "
          f"rms {rms_ph:.4e} vs {rms_old:.4e} (ratio {rms_ph / rms_old:.3f})")
    # the yardstick itself is sane: |y| < 8 rounds to bf16 within 2^-6, the bf16 weights add ~2e-3 rms
    assert mx_old < 0.1
    assert mx_ph <= 2 * mx_old
    assert rms_ph <= 2 * rms_old


@pytest.mark.parametrize("case", CASES)
def test_statistics_match_standalone(gpu, case):
    from rdeic_amd import ops
    c = _case(case)
    n, h, w, cin, cout, _ = case
    y = c["y_ph"]
    fused = getattr(y, "_rdeic_gn_part", None) is not None
    assert fused == ((4 * h * w) % 64 == 0)  # 6x10: no partial buffer, the GroupNorm reads the tensor
    g = torch.Generator().manual_seed(7)
    gamma = (1 + 0.1 * torch.randn(cout, generator=g)).cuda()
    beta = (0.1 * torch.randn(cout, generator=g)).cuda()
    ab_f = ops.group_norm_ab(y, gamma, beta, 32, 1e-5)
    ab_s = ops.group_norm_ab(y.clone(), gamma, beta, 32, 1e-5)  # a fresh tensor: the stand-alone pass
    torch.testing.assert_close(ab_f, ab_s, rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize("case", CASES)
def test_deterministic_and_plan_replay(gpu, case):
    from rdeic_amd import ops
    from rdeic_amd.plan import LaunchPlan
    c = _case(case)
    y2 = ops.conv2d(c["x"], c["p"], up2=True, stats=True, phases=c["ph"])
    assert torch.equal(y2, c["y_ph"])
    plan = LaunchPlan()
    xs = c["x"].clone()
    out = plan.record(lambda t: ops.conv2d(t, c["p"], up2=True, stats=True, phases=c["ph"]), xs)
    assert [name for name, *_ in plan.calls] == ["rdeic_conv2d_up2_phases"]
    assert torch.equal(out, c["y_ph"])
    out.zero_()
    torch.cuda.synchronize()
    assert torch.equal(plan.replay(), c["y_ph"])


@pytest.mark.parametrize("case", CASES)
def test_switch_off_is_the_fused_gather(gpu, case):
    from rdeic_amd import ops
    c = _case(case)
    prev = ops.set_up2_phases(False)
    try:
        y_off = ops.conv2d(c["x"], c["p"], up2=True, stats=True, phases=c["ph"])
    finally:
        ops.set_up2_phases(prev)
    assert torch.equal(y_off, c["y_old"])
    lib_prev = ops.set_conv_option(11, 0)  # the library's switch alone (bench.py --conv-option 11=0)
    try:
        y_lib = ops.conv2d(c["x"], c["p"], up2=True, stats=True, phases=c["ph"])
    finally:
        ops.set_conv_option(11, lib_prev)
    assert torch.equal(y_lib, c["y_old"])
    assert torch.equal(ops.conv2d(c["x"], c["p"], up2=True, stats=True, phases=c["ph"]), c["y_ph"])


def test_every_phase_tile_is_bit_identical(gpu):
    """The tiles built for the phase launch give the same bits (same k order), the heuristic included."""
    from rdeic_amd import ops
    c = _case(CASES[4])
    for t in (25, 26, 30, 32, 33, 36):
        ops.FORCE_TILE = t
        try:
            y = ops.conv2d(c["x"], c["p"], up2=True, stats=True, phases=c["ph"])
        finally:
            ops.FORCE_TILE = None
        assert torch.equal(y, c["y_ph"]), t
