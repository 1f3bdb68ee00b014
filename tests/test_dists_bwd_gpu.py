"""The DISTS training loss on the device (DISTS.loss): each new kernel of dists.hip against fp64 autograd
of the restatement (tests/dists_ref.py, tests/dists_bwd_ref.py), the whole loss and its gradient on the two CPU cases
with the fp32 CPU restatement as the yardstick, and the contract of the public entry point."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dists_bwd_ref as B
from tests import dists_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def D(gpu):
    from rdeic_amd import dists
    return dists


@pytest.fixture(scope="module")
def model(D):
    return D.DISTS(R.seeded_weights(), backbone=R.seeded_backbone())


def _strided(t: torch.Tensor, ld: int) -> torch.Tensor:
    """A device copy of NHWC t whose pixel stride is ld >= c."""
    n, h, w, c = t.shape
    buf = torch.zeros((n, h, w, ld), dtype=t.dtype, device="cuda")
    buf[..., :c] = t.cuda()
    return buf[..., :c]


# ------------------------------------------------------------------ 1. prep_float
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("ld", [3, 4])
def test_prep_float_is_the_restated_arithmetic(D, dtype, ld):
    g = torch.Generator().manual_seed(3)
    img = (torch.rand((2, 5, 7, 3), generator=g) * 2.2 - 1.1).to(dtype)  # not clamped: a little past [-1, 1]
    raw, norm = D.prep_float(_strided(img, ld))
    r, v = B.prep_float(img.float().permute(0, 3, 1, 2))  # fp32: a multiply, an add, a subtract, a divide
    for got, want in ((raw, r), (norm, v)):
        got = got.cpu()
        assert torch.equal(got[..., :3], want.permute(0, 2, 3, 1)) and float(got[..., 3].abs().max()) == 0.0


# ------------------------------------------------------------------ 2. L2-pool backward
def _l2pool_case(D, n, h, w, c, ld_extra, zero_block, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, h, w, c), generator=g)
    if zero_block:
        x[:, 2:6, 1:5] = 0.0
    ho, wo = (h + 1) // 2, (w + 1) // 2
    dy = torch.randn((n, ho, wo, c), generator=g)
    xd, dyd = _strided(x, c + ld_extra), _strided(dy, c + ld_extra)
    yd = D.l2_pool(xd, out=_strided(torch.zeros((n, ho, wo, c)), c + ld_extra))
    out = _strided(torch.zeros_like(x), c + ld_extra) if ld_extra else None
    got = D.l2_pool_bwd(xd, yd, dyd, out=out).cpu().double()
    # fp64 autograd of the restated pool, and the bound's sum_o g_(o,j) |dy_o| / y_o by autograd of the same conv
    x64 = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y64 = R.l2_pool(x64)
    y64.backward(dy.double().permute(0, 3, 1, 2))
    a = torch.tensor(np.hanning(5)[1:-1], dtype=torch.float64)
    k = (a[:, None] * a[None, :] / (a.sum() ** 2))[None, None].repeat(c, 1, 1, 1)
    u = torch.zeros_like(x64).requires_grad_(True)
    (F.conv2d(u, k, stride=2, padding=1, groups=c) * (dy.double().permute(0, 3, 1, 2).abs() / y64.detach())).sum().backward()
    want = x64.grad.permute(0, 2, 3, 1)
    bound = 2e-6 * x.double().abs() * u.grad.permute(0, 2, 3, 1)
    return x, got, want, bound


@pytest.mark.parametrize("shape,ld_extra", [((2, 5, 7, 8), 0), ((1, 6, 6, 6), 0), ((1, 1, 1, 4), 0), ((1, 1, 9, 4), 0),
                                            ((1, 8, 8, 64), 8)], ids=str)
def test_l2pool_backward(D, shape, ld_extra):
    zero_block = shape == (1, 8, 8, 64)
    x, got, want, bound = _l2pool_case(D, *shape, ld_extra, zero_block)
    err = (got - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"l2pool_bwd {shape}: worst error / bound {worst:.3f}, gradient norm {float(want.norm()):.3e}")
    assert float(want.norm()) > 0 and bool((err <= bound).all())
    if zero_block:
        assert float(got[:, 2:6, 1:5].abs().max()) == 0.0 and float(got.abs().max()) > 0


# ------------------------------------------------------------------ 3. tap-score backward
def _tap_case(D, n, h, w, c, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(0.5 + torch.randn((n, h, w, c), generator=g))
    y = torch.relu(0.5 + torch.randn((n, h, w, c), generator=g))
    al = 0.1 + 0.01 * torch.randn(c, generator=g, dtype=torch.float64)
    be = 0.1 + 0.01 * torch.randn(c, generator=g, dtype=torch.float64)
    tot = al.sum() + be.sum()
    al, be = al / tot, be / tot
    gs = -torch.linspace(1.0, 0.6, n, dtype=torch.float64) / n
    x64 = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    (B.tap_score(x64, y.double().permute(0, 3, 1, 2), al, be) * gs).sum().backward()
    return x, y, al, be, gs, x64.grad.permute(0, 2, 3, 1)


@pytest.mark.parametrize("shape", [(2, 5, 7, 4), (1, 9, 9, 64), (2, 3, 3, 512), (1, 1, 1, 4)], ids=str)
def test_tap_score_backward(D, shape):
    x, y, al, be, gs, want = _tap_case(D, *shape)
    xd, yd, ald, bed, gsd = x.cuda(), y.cuda(), al.cuda(), be.cuda(), gs.cuda()
    mom = D.moments(xd, yd)
    got = D.tap_bwd(xd, yd, mom, ald, bed, gsd)
    err = B.rel_l2(got.cpu(), want)
    print(f"tap_bwd {shape}: relative L2 error {err:.3e}, gradient norm {float(want.norm()):.3e}")
    assert float(want.norm()) > 0 and err <= 1e-4
    base = torch.randn(shape, generator=torch.Generator().manual_seed(5)).cuda()
    added = D.tap_bwd(xd, yd, mom, ald, bed, gsd, out=base.clone())
    assert torch.equal(added, base + got)  # add mode: one fp32 add of the rounded value
    assert B.rel_l2((added - base).cpu(), want) <= 1e-4 + 1e-6 * float(base.norm() / want.norm())
    if shape[1] * shape[2] == 1:  # hw = 1: both variances and the covariance are zero, only A survives
        assert float(mom[:, 2:].abs().max()) == 0.0


def test_tap_score_backward_of_identical_maps_is_exactly_zero(D):
    x, _, al, be, gs, _ = _tap_case(D, 2, 9, 7, 64, seed=1)
    xd = x.cuda()
    mom = D.moments(xd, xd.clone())
    assert torch.equal(mom[:, 2], mom[:, 3]) and torch.equal(mom[:, 2], mom[:, 4])
    got = D.tap_bwd(xd, xd.clone(), mom, al.cuda(), be.cuda(), gs.cuda())
    assert float(got.abs().max()) == 0.0


# ------------------------------------------------------------------ 4. the whole loss
def _loss_and_grad(model, pred, target):
    p = pred.cuda().requires_grad_(True)
    t = target.cuda().requires_grad_(True)
    loss = model.loss(p, t)
    loss.backward()
    return loss.detach(), p.grad, t.grad


@pytest.mark.parametrize("case", B.CASES, ids=lambda c: "x".join(map(str, c)))
def test_loss_and_gradient_against_fp64(model, case):
    pred, target, l64, g64, l32, g32 = B.case(*case)
    loss, grad, tgrad = _loss_and_grad(model, pred, target)
    cpu_err, dev_err = B.rel_l2(g32, g64), B.rel_l2(grad.cpu(), g64)
    dl = abs(float(loss) - float(l64))
    print(f"DISTS.loss {case}: loss {float(loss):.6e} (fp64 {float(l64):.6e}, abs {dl:.1e}); gradient rel L2 "
          f"device {dev_err:.3e}, fp32 CPU {cpu_err:.3e}")
    assert loss.dtype == torch.float32 and loss.dim() == 0 and grad.dtype == torch.float32 and tgrad is None
    assert dl <= 1e-5
    assert dev_err <= 4 * cpu_err  # the yardstick rule of DESIGN §23
    assert dev_err <= 2e-3


def test_identical_images_give_zero_loss_and_an_exactly_zero_gradient(model):
    pred, _ = B.float_pair(2, 21, 35, 1)
    p = pred.cuda().requires_grad_(True)
    loss = model.loss(p, pred.cuda())
    loss.backward()
    assert abs(float(loss.detach())) <= 1e-12 and float(p.grad.abs().max()) == 0.0


# ------------------------------------------------------------------ 5. contract
def test_repeats_bit_for_bit_and_backward_twice(model):
    pred, target = B.case(*B.CASES[0])[:2]
    l0, g0, _ = _loss_and_grad(model, pred, target)
    p = pred.cuda().requires_grad_(True)
    loss = model.loss(p, target.cuda())
    (ga,) = torch.autograd.grad(loss, p, retain_graph=True)
    (gb,) = torch.autograd.grad(loss, p)
    assert torch.equal(loss, l0) and torch.equal(ga, g0) and torch.equal(gb, g0) and float(g0.abs().max()) > 0


def test_bf16_prediction_with_pixel_stride_4(model):
    pred, target = B.case(*B.CASES[1])[:2]
    pb = _strided(pred.bfloat16(), 4).requires_grad_(True)
    loss_b = model.loss(pb, target.cuda())
    (gb,) = torch.autograd.grad(loss_b, pb)
    pf = pred.bfloat16().float().cuda().requires_grad_(True)  # the same values in fp32
    loss_f = model.loss(pf, target.cuda())
    (gf,) = torch.autograd.grad(loss_f, pf)
    assert gb.dtype == torch.bfloat16 and gb.shape == pred.shape and torch.equal(loss_b, loss_f)
    assert bool(((gb.float() - gf).abs() <= 2.0 ** -8 * gf.abs()).all())  # one bf16 rounding of the fp32 gradient
    assert float(gf.abs().max()) > 0


def test_value_on_the_uint8_grid_is_the_metrics_mean(model):
    pred_u8, tgt_u8 = (torch.from_numpy(a).cuda() for a in R.pairs(32, 48))
    want = model(pred_u8, tgt_u8).mean()
    got = model.loss(pred_u8.float() / 127.5 - 1.0, tgt_u8.float() / 127.5 - 1.0)
    print(f"uint8 grid: loss {float(got):.8f}, metric mean {want:.8f}")
    assert abs(float(got) - want) <= 1e-6


def test_packs_are_made_once_and_owned_by_the_instance(D):
    from rdeic_amd import autograd as AG
    m = D.DISTS(R.seeded_weights(), backbone=R.seeded_backbone())
    assert m._bwd is None
    before = len(AG.STEP_PACKS.entries)
    pred, target = B.float_pair(1, 16, 16, 2)
    _loss_and_grad(m, pred, target)
    first = m._bwd
    assert first is not None and len(first[1]) == 13 and first[1][0] is None
    _loss_and_grad(m, pred, target)
    assert m._bwd is first
    assert len(AG.STEP_PACKS.entries) == before


def test_oversize_batch_and_input_checks(D, model, monkeypatch):
    pred, target = (t.cuda() for t in B.float_pair(2, 16, 16, 0))
    monkeypatch.setattr(D, "MAX_TENSOR_BYTES", 2 * D.image_bytes(16, 16))

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")
    monkeypatch.setattr(D, "prep_float", no_launch)
    with pytest.raises(ValueError, match=str(2 * D.image_bytes(16, 16))):
        model.loss(pred, target)
    monkeypatch.undo()
    assert torch.isfinite(model.loss(pred, target))
    with pytest.raises(ValueError):
        model.loss(pred, target[:, :8])
    with pytest.raises(ValueError):
        model.loss(pred.half(), target.half())
    with pytest.raises(ValueError):
        model.loss(pred[:0], target[:0])
