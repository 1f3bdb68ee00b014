"""The backward of the LPIPS training loss on the device (rdeic_amd/lpips.py LPIPS.loss, csrc/lpips.hip): each
kernel against torch's CPU autograd, the whole loss against the fp64 autograd restatement of the reference's
model/lpips.py (tests/lpips_bwd_ref.py), and bit-for-bit repeatability.

Tolerances.
* Layer backward, relative L2 1e-4 to fp64 autograd on the same fp32 inputs: the forward's worst-case figure
  (tests/test_lpips_gpu.py: quotients within (c/2 + 3) u, u = 2^-24, a factor 3 for the difference of the two
  normalised maps, doubled by the second product: 9.3e-5 at c = 512); the typical figure is two decades lower.
* Max pool backward: bit-exact to torch fp32. An element is a sum of at most 4 window gradients, added from 0
  in output row-major order, which is torch's scatter order.
* Small-cin dgrad, per element (K + 3) u A: an element is a sum of K <= 9 taps x cout products (gamma_K of the
  sum of their magnitudes A, computed in fp64), one rounding each for the product, the mask-free accumulate
  and the division by scale_c. A bf16 output adds its own rounding, 2^-8 relative.
* Whole loss: value 1e-4 relative (the metric's bound, tests/test_lpips_gpu.py), gradient relative L2 2e-3
  (the fine-tune step's gradient bar, tests/test_finetune_gpu.py TOL) against fp64.
  Measured on an MI355X: see DESIGN.md section 16."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import lpips_bwd_ref as B
from tests import lpips_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
VALUE_RTOL = 1e-4   # tests/test_lpips_gpu.py RTOL
GRAD_TOL = 2e-3     # tests/test_finetune_gpu.py TOL


def _model(net):
    from rdeic_amd.lpips import LPIPS
    return LPIPS(net, backbone=R.seeded_backbone(net), lin=R.LIN_NPZ)


# ------------------------------------------------------------------ 1. float prep
@pytest.mark.parametrize("dtype,ld", [(torch.float32, 3), (torch.float32, 5), (torch.bfloat16, 3), (torch.bfloat16, 4)])
def test_prep_float_is_bit_exact(gpu, dtype, ld):
    from rdeic_amd.lpips import prep_float
    g = torch.Generator().manual_seed(3)
    buf = (torch.rand((2, 9, 7, ld), generator=g) * 2 - 1).to(dtype)
    img = buf[..., :3]
    want = B.scaling_layer_float(img.float().permute(0, 3, 1, 2)).permute(0, 2, 3, 1).contiguous()
    got = prep_float(buf.cuda()[..., :3]).cpu()
    assert got.shape == (2, 9, 7, 4) and got.dtype == torch.float32
    assert torch.equal(got[..., :3].contiguous().view(torch.int32), want.view(torch.int32))
    assert (got[..., 3].view(torch.int32) == 0).all()


# ------------------------------------------------------------------ 2. layer-distance backward
def _layer_case(n, h, w, c):
    g = torch.Generator().manual_seed(c * 1000 + h * 31 + w)
    f0 = F.relu(torch.rand((n, h, w, c), generator=g) - 0.3)
    f1 = F.relu(torch.rand((n, h, w, c), generator=g) - 0.3)
    lin = torch.rand(c, generator=g) * 0.1
    gs = torch.rand(n, generator=g) + 0.5
    return f0, f1, lin, gs


def _layer_ref(f0, f1, lin, gs):
    a = f0.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    d = R.layer_distance(a, f1.double().permute(0, 3, 1, 2), lin.double())
    (d * gs.double()).sum().backward()
    return a.grad.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("n,h,w,c", [(2, 7, 5, 64), (1, 3, 3, 192), (1, 2, 2, 512)])
def test_layer_backward(gpu, n, h, w, c):
    from rdeic_amd.lpips import layer_distance_bwd
    f0, f1, lin, gs = _layer_case(n, h, w, c)
    want = _layer_ref(f0, f1, lin, gs)
    a, b, l, g = f0.cuda(), f1.cuda(), lin.cuda(), gs.cuda()
    got = layer_distance_bwd(a, b, l, g)
    err = B.rel_l2(got.cpu(), want)
    print(f"layer backward n={n} hw={h}x{w} c={c}: relative L2 error {err:.3e}")
    assert torch.isfinite(got).all() and float(want.norm()) > 0
    assert err <= 1e-4
    assert torch.equal(layer_distance_bwd(a, b, l, g), got)  # repeatable bit for bit
    acc = got.clone()  # a second call adds
    layer_distance_bwd(a, b, l, g, out=acc)
    assert torch.equal(acc, got + got)
    # an image alone gets the gradient it gets in the batch
    assert torch.equal(layer_distance_bwd(a[:1], b[:1], l, g[:1]), got[:1])


@pytest.mark.parametrize("n,h,w,c", [(2, 7, 5, 64), (1, 3, 3, 192), (1, 2, 2, 512)])
def test_layer_backward_zero_pixel(gpu, n, h, w, c):
    """One pixel of f0 all zero: its gradient is exactly 0, everything is finite, and the other pixels still
    match (torch's own autograd has 0 / 0 at that pixel, so it is left out of the comparison)."""
    from rdeic_amd.lpips import layer_distance_bwd
    f0, f1, lin, gs = _layer_case(n, h, w, c)
    f0[n - 1, h // 2, w // 2] = 0
    want = _layer_ref(f0, f1, lin, gs)
    got = layer_distance_bwd(f0.cuda(), f1.cuda(), lin.cuda(), gs.cuda()).cpu()
    assert torch.isfinite(got).all()
    assert (got[n - 1, h // 2, w // 2].view(torch.int32) << 1 == 0).all()  # +0 or -0
    keep = torch.ones((n, h, w), dtype=torch.bool)
    keep[n - 1, h // 2, w // 2] = False
    assert torch.isfinite(want[keep]).all()
    assert B.rel_l2(got[keep], want[keep]) <= 1e-4


@pytest.mark.parametrize("n,h,w,c", [(2, 7, 5, 64), (1, 2, 2, 512)])
def test_layer_backward_identical_maps(gpu, n, h, w, c):
    from rdeic_amd.lpips import layer_distance_bwd
    f0, _, lin, gs = _layer_case(n, h, w, c)
    f0[0, 0, 0] = 0
    a = f0.cuda()
    got = layer_distance_bwd(a, a.clone(), lin.cuda(), gs.cuda())
    assert float(got.abs().max()) == 0.0


# ------------------------------------------------------------------ 3. max pool backward
@pytest.mark.parametrize("shape,k", [((2, 15, 13, 64), 3), ((2, 9, 7, 64), 2), ((1, 8, 11, 192), 3), ((1, 7, 7, 3), 3)])
def test_max_pool_backward_is_bit_exact(gpu, shape, k):
    from rdeic_amd.lpips import max_pool_bwd
    n, h, w, c = shape
    g = torch.Generator().manual_seed(h * 100 + w + k)
    x = torch.randn(shape, generator=g)  # continuous values: ties have measure zero
    ho, wo = (h - k) // 2 + 1, (w - k) // 2 + 1
    dy = torch.randn((n, ho, wo, c), generator=g)
    xr = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    F.max_pool2d(xr, kernel_size=k, stride=2).backward(dy.permute(0, 3, 1, 2).contiguous())
    want = xr.grad.permute(0, 2, 3, 1).contiguous()
    got = max_pool_bwd(x.cuda(), dy.cuda(), k, 2).cpu()
    assert got.shape == want.shape
    assert torch.equal(got, want)
    if k == 2 and h % 2:  # floor mode: no window covers the last row and column
        assert (got[:, h - 1] == 0).all() and (got[:, :, w - 1] == 0).all()
    assert torch.equal(max_pool_bwd(x.cuda(), dy.cuda(), k, 2).cpu(), got)


# ------------------------------------------------------------------ 4. strided small-cin dgrad
def _dgrad_case(n, h, w, cin, cout, k, s, p, relu, prep):
    g = torch.Generator().manual_seed(k * 100 + s)
    wt = torch.randn((cout, cin, k, k), generator=g) * (2.0 / (cin * k * k)) ** 0.5
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    dz = torch.randn((n, ho, wo, cout), generator=g)
    z = F.relu(torch.randn((n, ho, wo, cout), generator=g)) if relu else None
    x = torch.zeros((n, cin, h, w), dtype=torch.float64, requires_grad=True)
    up = dz.double() * (z > 0).double() if relu else dz.double()
    F.conv2d(x, wt.double(), stride=s, padding=p).backward(up.permute(0, 3, 1, 2).contiguous())
    want = x.grad.permute(0, 2, 3, 1).contiguous()
    xa = torch.zeros((n, cin, h, w), dtype=torch.float64, requires_grad=True)  # sum of the terms' magnitudes
    F.conv2d(xa, wt.double().abs(), stride=s, padding=p).backward(up.abs().permute(0, 3, 1, 2).contiguous())
    mag = xa.grad.permute(0, 2, 3, 1).contiguous()
    if prep:
        scale = torch.tensor(R.SCALE, dtype=torch.float64)
        want, mag = want[..., :3] / scale, mag[..., :3] / scale
    return wt, dz, z, want, mag


@pytest.mark.parametrize("relu,prep,dtype", [(False, False, torch.float32), (True, False, torch.float32),
                                             (False, True, torch.float32), (True, True, torch.float32),
                                             (True, True, torch.bfloat16)])
@pytest.mark.parametrize("geom", [(2, 38, 50, 4, 64, 11, 4, 2), (1, 9, 7, 4, 64, 3, 1, 1), (1, 6, 5, 3, 128, 3, 1, 1)])
def test_conv_dgrad_small(gpu, geom, relu, prep, dtype):
    from rdeic_amd.lpips import conv_dgrad_small
    n, h, w, cin, cout, k, s, p = geom
    wt, dz, z, want, mag = _dgrad_case(n, h, w, cin, cout, k, s, p, relu, prep)
    wdev = wt.permute(2, 3, 1, 0).contiguous().cuda()
    out = torch.full((n, h, w, want.shape[3] + 2), -7.0, dtype=dtype, device="cuda")  # a wider pixel stride
    got = conv_dgrad_small(dz.cuda(), None if z is None else z.cuda(), wdev, (h, w), cin, k, s, p, prep_bwd=prep,
                           out=out[..., :want.shape[3]])
    assert (out[..., want.shape[3]:] == -7.0).all()  # nothing written past the channels
    got = got.cpu().double()
    taps = (-(-k // s)) ** 2  # at most ceil(k / s)^2 taps reach an input pixel
    bound = (taps * cout + 3) * U * mag
    if dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * want.abs()
    err = (got - want).abs()
    print(f"dgrad {geom} relu={relu} prep={prep} {dtype}: max error {float(err.max()):.3e}, "
          f"max bound {float(bound.max()):.3e}, max |want| {float(want.abs().max()):.3e}")
    assert float(want.abs().max()) > 0
    assert (err <= bound).all()
    if s == 4:  # row 37 and column 49 are covered by no window
        assert float(mag[:, 37].abs().max()) == 0 and float(mag[:, :, 49].abs().max()) == 0
        assert (got[:, 37] == 0).all() and (got[:, :, 49] == 0).all()
    again = torch.empty_like(out)
    conv_dgrad_small(dz.cuda(), None if z is None else z.cuda(), wdev, (h, w), cin, k, s, p, prep_bwd=prep,
                     out=again[..., :want.shape[3]])
    assert torch.equal(again[..., :want.shape[3]], out[..., :want.shape[3]])


# ------------------------------------------------------------------ 5. the whole loss
@pytest.mark.parametrize("name", ["alex", "vgg"])
def test_loss_value_and_gradient(gpu, name):
    pred, target, l64, g64, l32, g32 = B.case(name)
    cpu_v, cpu_g = abs(float(l32) - float(l64)) / float(l64), B.rel_l2(g32, g64)
    assert cpu_g <= B.CPU_FP32_GRAD_BOUND  # the case has no fp32 / fp64 mask flip (tests/test_lpips_bwd_cpu.py)
    m = _model(B.CASES[name][0])
    p = pred.cuda().requires_grad_(True)
    loss = m.loss(p, target.cuda())
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda
    loss.backward()
    loss = loss.detach()
    rel_v = abs(float(loss) - float(l64)) / float(l64)
    rel_g = B.rel_l2(p.grad.cpu(), g64)
    print(f"LPIPS.loss {name}: loss {float(loss):.6e} (fp64 {float(l64):.6e}); value error device {rel_v:.2e}, "
          f"CPU fp32 {cpu_v:.2e}; gradient relative L2 error device {rel_g:.2e}, CPU fp32 {cpu_g:.2e}")
    assert p.grad.shape == pred.shape and torch.isfinite(p.grad).all()
    assert rel_v <= VALUE_RTOL
    assert rel_g <= GRAD_TOL


def test_loss_is_deterministic_and_target_gets_no_gradient(gpu):
    pred, target, *_ = B.case("alex")
    m = _model("alex")
    grads, vals = [], []
    for _ in range(2):
        p, t = pred.cuda().requires_grad_(True), target.cuda().requires_grad_(True)
        loss = m.loss(p, t)
        loss.backward()
        assert t.grad is None
        grads.append(p.grad)
        vals.append(loss.detach())
    assert torch.equal(vals[0], vals[1])
    assert torch.equal(grads[0].view(torch.int32), grads[1].view(torch.int32))


def test_loss_matches_the_metric_kernels_and_takes_bf16(gpu):
    """The loss is the mean of the scores the forward kernels give on the float prep; bf16 images give a bf16
    gradient close to the fp32 one (the backbone stays fp32; the inputs' own rounding is 2^-9 relative)."""
    from rdeic_amd.lpips import layer_distance
    pred, target, *_ = B.case("alex")
    m = _model("alex")
    p, t = pred.cuda(), target.cuda()
    f0, f1 = m.features_float(p), m.features_float(t)
    out = torch.empty(p.shape[0], device="cuda")
    for k in range(5):
        layer_distance(f0[k], f1[k], m.lin[k], out=out, accumulate=k > 0)
    assert torch.equal(m.loss(p, t), out.mean())
    pf = p.clone().requires_grad_(True)
    m.loss(pf, t).backward()
    pb = p.bfloat16().requires_grad_(True)
    lb = m.loss(pb, t.bfloat16())
    lb.backward()
    assert pb.grad.dtype == torch.bfloat16 and torch.isfinite(pb.grad).all() and bool(torch.isfinite(lb))
    # same images after rounding to bf16, evaluated in fp32: only the gradient's own bf16 rounding differs
    pr = p.bfloat16().float().requires_grad_(True)
    m.loss(pr, t.bfloat16().float()).backward()
    assert B.rel_l2(pb.grad.float().cpu(), pr.grad.cpu()) <= 2.0 ** -8
    assert np.isfinite(float(lb))


def test_loss_backward_twice_on_a_retained_graph_and_owns_its_packs(gpu):
    """The activations stay with the graph: a second backward on a retained graph gives the same bits. The
    backward's packed weights belong to the LPIPS instance, not to the fine-tune step's process-wide cache."""
    from rdeic_amd import autograd as A
    pred, target, *_ = B.case("alex")
    m = _model("alex")
    before = (len(A.PACKS.fwd), len(A.PACKS.dgrad))
    p = pred.cuda().requires_grad_(True)
    loss = m.loss(p, target.cuda())
    (g1,) = torch.autograd.grad(loss, p, retain_graph=True)
    (g2,) = torch.autograd.grad(loss, p)
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32)) and float(g1.abs().max()) > 0
    assert (len(A.PACKS.fwd), len(A.PACKS.dgrad)) == before
    with pytest.raises(RuntimeError):  # the graph is freed now: torch's own message
        torch.autograd.grad(loss, p)
