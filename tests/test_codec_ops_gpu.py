"""Every small kernel of the inference path on its own, on the MI355X, against tests/codec_ops_ref.py: the
checkerboard entropy-model kernels and the VQ search (csrc/entropy.hip), the sampler / layout / image / cast / pack
kernels (csrc/elementwise.hip), rdeic_softmax_rows and rdeic_transpose (csrc/attention.hip). The inputs are fixed
and seeded (built in tests/codec_ops_ref.py; tests/test_codec_ops_ref_cpu.py shows that they tell a subtly wrong
op from the right one). Every output buffer starts as a sentinel and is compared in full, so what a kernel must
leave alone (pad channels, the other checkerboard colour, rows past `rows`, the tail) is asserted with the rest.

Bit-exact ops (torch.equal, on the bit patterns where a sign of zero or a bf16 value is at stake): ckbd_encode,
ckbd_indexes, ckbd_dequant, vq_argmin, gather_rows, axpby, ddim_step, spaced_step, cfg_combine, nchw_to_nhwc,
nhwc_to_nchw, image_u8_to_nhwc, nhwc_to_image_u8, image_mse, cast, pack_conv_weight, transpose.

row_sqnorm has a derived bound: a lane adds ceil(dim/64) rounded squares, then 6 shuffle adds follow, so
|err| <= (ceil(dim/64) + 7) * 2^-24 * sum(v^2) against the float64 sum.

Ops with a transcendental: worst absolute error against the float64 reference over all cases of the op below,
measured once on an MI355X on these inputs (fp32 output); the assertion is 4 x that, rounded up to one significant
digit, and stays below the fp32 tolerance of tests/test_kernels_gpu.py (2e-5 of the output's largest magnitude).
The inputs are seeded, so the margin covers compiler and math-library changes only.

    op                    cases                                              measured     asserted    2e-5 * max|out|
    timestep_embedding    t in {0, 1, 299, 999}, dim in {2, 320}             4.997e-08    2e-07       2e-5
    silu_f32              x in [-100, 100] with 0, +-88; 4 element counts    1.176e-06    5e-06       2e-3
    softmax_rows          5 rows, 8 widths, scaled scores over [-80, 80]     4.298e-07    2e-06       2e-5

softmax_rows in bf16: the reference is rounded to bf16 first and one bf16 ulp of it is allowed on top of the
fp32 bound. Every fp32 softmax row also sums to 1 within cols * 2^-23 (a bf16 row cannot: each of its elements
carries a relative rounding of 2^-9)."""
import math

import numpy as np
import pytest
import torch

from oracle import coders_ref as cr
from oracle import model_ref as mr
from tests import codec_ops_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
TIMESTEP_BOUND = 2e-7
SILU_BOUND = 5e-6
SOFTMAX_BOUND = 2e-6
FP32_TOL = 2e-5  # tests/test_kernels_gpu.py, relative to the output's largest magnitude
SENT = -12345.0  # exact in bf16 (-12352 is what the fill leaves there; the comparison is of bit patterns)


def _bits(t):
    """Bit patterns, so that -0.0 != +0.0 and NaN == NaN."""
    t = t.cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and torch.equal(_bits(got), _bits(want))


def _dt(dtype):
    return 1 if dtype == torch.bfloat16 else 0


def _sent(shape, dtype=torch.float32, value=SENT):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), value, dtype=dtype)


# ------------------------------------------------------------------------------------------ checkerboard
def _embed(x_nchw, width, off, dtype, fill):
    """NCHW values as channels off.. of a [n][h][w][width] buffer filled with `fill` elsewhere."""
    n, c, h, w = x_nchw.shape
    buf = torch.full((n, h, w, width), fill, dtype=dtype)
    buf[..., off:off + c] = x_nchw.permute(0, 2, 3, 1).to(dtype)
    return buf


def _run_checkerboard(shape, dtype, phase):
    """Encoder, then the decoder's two kernels, through the strided views compression.py passes."""
    from rdeic_amd import ops
    n, hy, wy, c = shape
    y, params, table = R.ckbd_case(n, hy, wy, c, dtype)
    sym_r, idx_r, half_r, anchor_r = R.ckbd_encode_ref(y, params, phase, table, dtype)
    n_stage = c * hy * (wy // 2)
    img_stride, off = n_stage + 13, 5
    yw, yo, pld, yhw, yho, ald = c + 16, 8, 2 * c + 16, c + 7, 3, 2 * c
    dt, sp = _dt(dtype), ops.stream_ptr()
    tab = table.cuda()
    bound = float(cr.SCALE_BOUND)

    ybuf = _embed(y, yw, yo, dtype, 1e4).cuda()  # a y slice of a wider latent
    pbuf = _embed(params, pld, 0, dtype, 1e4).cuda()  # padded params
    yh0 = _sent((n, hy, wy, yhw), dtype)
    an0 = _sent((n, hy, wy, ald), dtype)
    si0 = _sent((n, img_stride), torch.int32, -77)
    yhbuf, anbuf, sym, idx = yh0.cuda(), an0.cuda(), si0.cuda(), si0.cuda()
    ops.call("rdeic_ckbd_encode", ybuf[..., yo:].data_ptr(), yw, pbuf.data_ptr(), pld, n, hy, wy, c, phase,
             tab.data_ptr(), tab.numel(), bound, sym.data_ptr(), idx.data_ptr(), img_stride, off,
             yhbuf[..., yho:].data_ptr(), yhw, anbuf.data_ptr(), ald, dt, sp)
    # the decoder: indexes from the same params into its own dense per-image buffer, dequant of the encoder's symbols
    idx_d = _sent((n, n_stage), torch.int32, -77).cuda()
    ops.call("rdeic_ckbd_indexes", pbuf.data_ptr(), pld, n, hy, wy, c, phase, tab.data_ptr(), tab.numel(), bound,
             idx_d.data_ptr(), n_stage, 0, dt, sp)
    sym_d = sym[:, off:off + n_stage].contiguous()
    yhbuf_d, anbuf_d = yh0.cuda(), an0.cuda()
    ops.call("rdeic_ckbd_dequant", sym_d.data_ptr(), pbuf.data_ptr(), pld, n, hy, wy, c, phase, n_stage, 0,
             yhbuf_d[..., yho:].data_ptr(), yhw, anbuf_d.data_ptr(), ald, dt, sp)
    torch.cuda.synchronize()

    # expected buffers: the sentinel everywhere but where the stage writes
    own = mr._anchor_mask(hy, wy, phase)  # [hy][wy], this phase's colour
    want_yh = yh0.clone()
    want_yh[:, own, yho:yho + c] = half_r.permute(0, 2, 3, 1)[:, own]  # other colour and pad channels untouched
    want_an = an0.clone()
    want_an[..., :c] = anchor_r.permute(0, 2, 3, 1)  # the other colour exactly +0.0
    assert not anchor_r.permute(0, 2, 3, 1)[:, ~own].view(torch.int16 if dt else torch.int32).any()
    want_si = si0.clone()
    want_si[:, off:off + n_stage] = sym_r
    want_idx = si0.clone()
    want_idx[:, off:off + n_stage] = idx_r
    assert _same(sym, want_si), "sym"
    assert _same(idx, want_idx), "idx"
    assert _same(yhbuf, want_yh), "yhat"
    assert _same(anbuf, want_an), "anchor_out"
    # decoder agreement, bit for bit
    assert torch.equal(idx_d, idx[:, off:off + n_stage]) and torch.equal(idx_d.cpu(), idx_r), "decoder idx"
    assert _same(yhbuf_d, yhbuf.cpu()) and _same(anbuf_d, anbuf.cpu()), "decoder yhat / anchor_out"


@pytest.mark.parametrize("phase", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", R.CKBD_SHAPES)
def test_checkerboard(gpu, shape, dtype, phase):
    _run_checkerboard(shape, dtype, phase)


def test_checkerboard_past_grid_cap(gpu):
    n, hy, wy, c = R.CKBD_LARGE
    assert n * c * hy * (wy // 2) > R.GRID_CAP
    _run_checkerboard(R.CKBD_LARGE, torch.bfloat16, 1)


def _call(name, *args):
    """ops.call on the current stream with every tensor argument on the device, kept alive until the kernel is done."""
    from rdeic_amd import ops
    held = [a.cuda() if isinstance(a, torch.Tensor) else a for a in args]
    ops.call(name, *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in held], ops.stream_ptr())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- VQ
def _vq_argmin(dot, zn, en):
    rows, ncode = dot.shape
    idx = _sent(rows + 3, torch.int32, -77).cuda()
    _call("rdeic_vq_argmin", dot, zn, en, rows, ncode, idx)
    idx = idx.cpu()
    assert (idx[rows:] == -77).all()
    return idx[:rows].long()


@pytest.mark.parametrize("rows", R.VQ_ROWS)
@pytest.mark.parametrize("ncode", list(R.VQ_NCODES) + [R.vq_codebook_size()])
def test_vq_argmin(gpu, ncode, rows):
    dot, zn, en = R.vq_case(rows, ncode)
    got = _vq_argmin(dot, zn, en)
    assert torch.equal(got, R.vq_argmin_ref(dot, zn, en))
    for r, (a, b) in R.vq_ties(rows, ncode).items():
        assert got[r] == a  # the first of the two tied codes


@pytest.mark.parametrize("ncode", [1, 7, 1000, R.vq_codebook_size()])
def test_vq_argmin_non_finite(gpu, ncode):
    """torch.argmin's rule: NaN counts as the minimum and the first one wins; a row of +inf gives 0. Only the
    index buffer is read here: no index of this test is handed to rdeic_gather_rows."""
    nan, inf = float("nan"), float("inf")
    dot, zn, en = R.vq_case(5, ncode)
    dot[0, :] = -inf  # every distance +inf
    dot[1, :] = nan  # every distance NaN
    want = {0: 0, 1: 0}
    if ncode > 300:
        dot[2, 5] = dot[2, 300] = nan
        dot[3, 7], dot[3, 9], dot[3, 600] = inf, nan, nan  # -inf before the first NaN: the NaN still wins
        want.update({2: 5, 3: 9})
    got = _vq_argmin(dot, zn, en)
    print(f"\nvq_argmin non-finite ncode={ncode}: indexes {[hex(v) for v in got.tolist()]}")
    assert ((got >= 0) & (got < ncode)).all()
    for r, v in want.items():
        assert got[r] == v, (r, got.tolist())
    assert torch.equal(got, R.vq_argmin_ref(dot, zn, en))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", [4, 33])
def test_gather_rows(gpu, dim, dtype):
    g = torch.Generator().manual_seed(dim)
    K, rows, ldt, ldo = 50, 37, dim + 2, dim + 3
    table = torch.randn(K, ldt, generator=g)
    idx = torch.randint(0, K, (rows,), generator=g, dtype=torch.int32)
    idx[0], idx[1] = 0, K - 1
    out0 = _sent((rows + 1, ldo), dtype)
    out = out0.cuda()
    _call("rdeic_gather_rows", table, ldt, idx, rows, dim, out, ldo, _dt(dtype))
    want = out0.clone()
    want[:rows, :dim] = R.gather_rows_ref(table[:, :dim], idx, dtype)
    assert _same(out, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", [1, 63, 64, 65, 512])
@pytest.mark.parametrize("rows", [1, 5, 1023])
def test_row_sqnorm(gpu, rows, dim, dtype):
    g = torch.Generator().manual_seed(rows * 1000 + dim)
    ld = dim + 3
    x = (torch.randn(rows, ld, generator=g) * 2).to(dtype)
    out = _sent(rows + 4).cuda()
    _call("rdeic_row_sqnorm", x, rows, dim, ld, out, _dt(dtype))
    out = out.cpu()
    assert (out[rows:] == SENT).all()
    ref = R.row_sqnorm_ref(x[:, :dim].float())
    err = (out[:rows].double() - ref).abs()
    bound = (math.ceil(dim / 64) + 7) * 2.0 ** -24 * ref
    assert (err <= bound).all(), (float((err / ref).max()), float((bound / ref).max()))


# -------------------------------------------------------------------------------------- sampler, bit-exact
def _dev_out(count):
    return _sent(count + 3).cuda()


def _check_out(buf, want):
    buf = buf.cpu()
    assert (buf[want.numel():] == SENT).all(), "tail written"
    assert torch.equal(buf[:want.numel()], want.reshape(-1))


@pytest.mark.parametrize("n_img,per_img", [(1, c) for c in R.COUNTS] + [(3, 1001)])
def test_axpby(gpu, n_img, per_img):
    x, z = R.pair_case(n_img * per_img, 2)
    a = torch.tensor([0.9713, 0.5121, 0.1234][:n_img])
    b = torch.tensor([0.2379, 0.8589, 0.9924][:n_img])
    out = _dev_out(x.numel())
    _call("rdeic_axpby", x, z, n_img, per_img, a, b, out)
    _check_out(out, R.axpby_ref(x.view(n_img, per_img), z.view(n_img, per_img), a, b))


@pytest.mark.parametrize("with_x0", [True, False])
@pytest.mark.parametrize("count", R.COUNTS)
def test_ddim_step(gpu, count, with_x0):
    x, e = R.pair_case(count, 1)
    xp, x0 = _dev_out(count), _dev_out(count)
    _call("rdeic_ddim_step", x, e, count, *R.DDIM_COEF, xp, x0 if with_x0 else None)
    want_xp, want_x0 = R.ddim_step_ref(x, e, *R.DDIM_COEF)
    _check_out(xp, want_xp)
    if with_x0:
        _check_out(x0, want_x0)
    else:
        assert (x0.cpu() == SENT).all()


SPACED_COEF = (1.2793, 0.7979, 0.3127, 0.6871)  # A, B, C1, C2


@pytest.mark.parametrize("variant", ["noise", "no_noise", "no_x0"])
@pytest.mark.parametrize("count", R.COUNTS)
def test_spaced_step(gpu, count, variant):
    x, e = R.pair_case(count, 3)
    noise = None if variant == "no_noise" else R.pair_case(count, 4)[0]
    S = 0.0 if noise is None else 0.3711
    xp, x0 = _dev_out(count), _dev_out(count)
    _call("rdeic_spaced_step", x, e, noise, count, *SPACED_COEF, S, xp, None if variant == "no_x0" else x0)
    want_xp, want_x0 = R.spaced_step_ref(x, e, noise, *SPACED_COEF, S)
    _check_out(xp, want_xp)
    if variant == "no_x0":
        assert (x0.cpu() == SENT).all()
    else:
        _check_out(x0, want_x0)


@pytest.mark.parametrize("count", R.COUNTS)
def test_cfg_combine(gpu, count):
    from rdeic_amd import ops
    ec, eu = R.pair_case(count, 5)
    out = _dev_out(count)
    _call("rdeic_cfg_combine", ec, eu, count, 2.5, out)
    _check_out(out, R.cfg_combine_ref(ec, eu, 2.5))
    assert torch.equal(ops.cfg_combine(ec.cuda(), eu.cuda(), 7.3).cpu(), R.cfg_combine_ref(ec, eu, 7.3))


# ---------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mul,add", R.LAYOUT_MULADD)
@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("shape", R.LAYOUT_SHAPES)
def test_nchw_nhwc(gpu, shape, pad, mul, add, dtype):
    """Both directions through the ops wrappers (they derive ld from the view they are given)."""
    from rdeic_amd import ops
    n, c, h, w = shape
    ld = 16 if pad else c
    x = R.layout_case(*shape)
    buf0 = _sent((n, h, w, ld), dtype)
    buf = buf0.cuda()
    ops.nchw_to_nhwc(x.cuda(), dtype, mul, add, out=buf[..., :c])
    torch.cuda.synchronize()
    want = buf0.clone()
    want[..., :c] = R.nchw_to_nhwc_ref(x, mul, add, dtype)
    assert _same(buf, want)  # pad channels untouched
    src = want.cuda()  # NHWC of dtype with sentinel pads
    back = ops.nhwc_to_nchw(src[..., :c], mul, add)
    torch.cuda.synchronize()
    assert _same(back, R.nhwc_to_nchw_ref(want[..., :c], mul, add))


# ---------------------------------------------------------------------------------------------- images
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ld", [3, 8, 16, 20])
def test_image_u8_to_nhwc(gpu, ld, dtype):
    n, h, w = 1, 16, 16
    u8 = (np.arange(n * h * w * 3) % 256).astype(np.uint8)  # every byte value, in every channel
    assert all(set(u8[ch::3].tolist()) == set(range(256)) for ch in range(3))
    out0 = _sent((n * h * w + 1, ld), dtype)
    out = out0.cuda()
    _call("rdeic_image_u8_to_nhwc", torch.from_numpy(u8), n, h, w, out, ld, _dt(dtype))
    want = out0.clone()
    want[:-1, :3] = R.u8_to_x_ref(u8, dtype).view(-1, 3)
    if ld <= 16:
        want[:-1, 3:] = 0.0  # a zero-padded conv input; wider pixels keep their other channels
    assert _same(out, want)


def _run_nhwc_to_image(x, ld, dtype):
    pix = x.shape[0]
    xb = torch.full((pix, ld), 1e9, dtype=dtype)  # pad channels the kernel must not read
    xb[:, :3] = x.to(dtype)
    img = _sent(pix * 3 + 5, torch.uint8, 77).cuda()
    _call("rdeic_nhwc_to_image_u8", xb, 1, 1, pix, ld, img, _dt(dtype))
    img = img.cpu()
    assert (img[pix * 3:] == 77).all()
    got, src = img[:pix * 3], xb[:, :3].float().reshape(-1)
    assert torch.equal(got, R.x_to_u8_ref(src))
    return got, src


@pytest.mark.parametrize("dtype", DTYPES)
def test_nhwc_to_image_u8(gpu, dtype):
    got, src = _run_nhwc_to_image(R.x_to_u8_case(17 * 19), 5, dtype)
    # NaN: the kernel clamps with fmaxf(v, 0), which returns the non-NaN argument, so a NaN pixel decodes to 0
    assert int(torch.isnan(src).sum()) == 1 and (got[torch.isnan(src)] == 0).all()
    assert (got[src == math.inf] == 255).all() and (got[src == -math.inf] == 0).all()


def test_nhwc_to_image_u8_past_grid_cap(gpu):
    pix = R.GRID_CAP // 3 + 100
    assert pix * 3 > R.GRID_CAP
    _run_nhwc_to_image(R.x_to_u8_case(pix), 4, torch.float32)


@pytest.mark.parametrize("off_a,off_b", [(0, 0), (1, 1), (0, 1)])
@pytest.mark.parametrize("per_img", [3 * 64 * 64, 3 * 5 * 7, 16, 15])
def test_image_mse(gpu, per_img, off_a, off_b):
    """16-byte path (both images 16-byte aligned) and scalar path: with an odd per_img images 1 and 2 start
    unaligned, with a base offset of one byte all do."""
    n = 3
    g = torch.Generator().manual_seed(per_img)
    a = torch.randint(0, 256, (n * per_img,), generator=g, dtype=torch.uint8)
    b = torch.randint(0, 256, (n * per_img,), generator=g, dtype=torch.uint8)
    a[per_img:2 * per_img], b[per_img:2 * per_img] = 0, 255  # image 1: differs by 255 everywhere
    ad, bd = (torch.zeros(n * per_img + 1, dtype=torch.uint8).cuda() for _ in range(2))
    ad[off_a:off_a + n * per_img] = a.cuda()
    bd[off_b:off_b + n * per_img] = b.cuda()
    assert ad.data_ptr() % 16 == 0 and bd.data_ptr() % 16 == 0
    out = _sent(n + 2).cuda()
    _call("rdeic_image_mse", ad.data_ptr() + off_a, bd.data_ptr() + off_b, n, per_img, out)
    out = out.cpu()
    assert (out[n:] == SENT).all()
    want = R.image_mse_ref(a, b, per_img)
    assert want[1] == 65025.0
    assert torch.equal(out[:n], want)


# ------------------------------------------------------------------------------------- cast, pack, transpose
@pytest.mark.parametrize("dst", DTYPES)
@pytest.mark.parametrize("src", DTYPES)
@pytest.mark.parametrize("count", R.COUNTS)
def test_cast(gpu, count, src, dst):
    from rdeic_amd import ops
    x = (R.pair_case(count, 6)[0] * 100).to(src)
    assert _same(ops.cast(x.cuda(), dst), R.cast_ref(x, dst))


@pytest.mark.parametrize("dst", DTYPES)
@pytest.mark.parametrize("src", DTYPES)
def test_cast_special_values(gpu, src, dst):
    from rdeic_amd import ops
    inf, nan = math.inf, math.nan
    vals = [0.0, -0.0, inf, -inf, nan, 1e-40, -1e-45, 1.17549435e-38, 9.2e-41,  # zeros, non-finite, denormals
            1.00390625, 1.01171875, -1.00390625, -1.01171875,  # bf16 ties: 1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1.015625
            1.0039063692092896, 1.0039061307907104,  # one fp32 ulp either side of a tie
            3.3895313892515355e38, 3.3961775292304601e38, 3.4e38, -3.4e38, 3.4028234663852886e38]  # up to inf
    x = torch.tensor(vals, dtype=torch.float32).to(src)
    got, want = ops.cast(x.cuda(), dst).cpu(), R.cast_ref(x, dst)
    if src == torch.float32 and dst == torch.bfloat16:
        assert want[9] == 1.0 and want[10] == 1.015625 and want[13] == 1.0078125 and want[14] == 1.0
        assert want[15] == 3.3895313892515355e38 and torch.isinf(want[16:]).all()
    nanmask = torch.isnan(want)
    assert int(nanmask.sum()) == 1 and torch.equal(torch.isnan(got), nanmask)  # a NaN stays a NaN
    assert torch.equal(_bits(got)[~nanmask], _bits(want)[~nanmask])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cout,cin,k", [(5, 3, 3), (16, 8, 1)])
def test_pack_conv_weight(gpu, cout, cin, k, dtype):
    g = torch.Generator().manual_seed(cout * 100 + cin)
    w = torch.randn(cout, cin, k, k, generator=g)
    wld = k * k * cin + 5
    out0 = _sent(cout * wld + 3, dtype)
    out = out0.cuda()
    _call("rdeic_pack_conv_weight", w, cout, cin, k, k, out, wld, _dt(dtype))
    want = out0.clone()
    want[:cout * wld] = R.pack_conv_weight_ref(w, wld, dtype).reshape(-1)
    assert not _bits(want[:cout * wld].view(cout, wld)[:, k * k * cin:]).any()  # the tail is +0.0
    assert _same(out, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols", R.TRANSPOSE_SHAPES)
def test_transpose(gpu, rows, cols, dtype):
    src, ldin, ldout, in_bs, out_bs = R.transpose_case(rows, cols, dtype)
    out0 = _sent(R.TRANSPOSE_BATCH * out_bs, dtype)
    out = out0.cuda()
    _call("rdeic_transpose", src, rows, cols, ldin, out, ldout, R.TRANSPOSE_BATCH, in_bs, out_bs, _dt(dtype))
    assert _same(out, R.transpose_ref(src, rows, cols, ldin, out0, ldout, R.TRANSPOSE_BATCH, in_bs, out_bs))


# ---------------------------------------------------------------------------- ops with a transcendental
def _report(op, case, err, bound, scale):
    print(f"\n[measured] {op} {case}: max abs err {err:.3e} (asserted {bound:.0e}, 2e-5 * max|out| = "
          f"{FP32_TOL * scale:.1e})")
    assert bound <= FP32_TOL * scale


@pytest.mark.parametrize("dim", [2, 320])
def test_timestep_embedding(gpu, dim):
    t = torch.tensor([0, 1, 299, 999], dtype=torch.int64)
    freqs = R.timestep_freqs(dim)
    out = _sent(t.numel() * dim + 3).cuda()
    _call("rdeic_timestep_embedding", t, freqs, t.numel(), dim, out)
    out = out.cpu()
    assert (out[t.numel() * dim:] == SENT).all()
    ref = R.timestep_embedding_ref(t, freqs)
    err = float((out[:t.numel() * dim].view(t.numel(), dim).double() - ref).abs().max())
    _report("timestep_embedding", f"dim={dim}", err, TIMESTEP_BOUND, 1.0)
    assert err <= TIMESTEP_BOUND


@pytest.mark.parametrize("count", R.COUNTS)
def test_silu_f32(gpu, count):
    from rdeic_amd import ops
    x = R.silu_case()
    x = x[:count] if count <= x.numel() else x.repeat(count // x.numel() + 1)[:count]
    out = ops.silu_f32(x.cuda())
    torch.cuda.synchronize()
    ref = R.silu_ref(x)
    err = float((out.cpu().double() - ref).abs().max())
    _report("silu_f32", f"count={count}", err, SILU_BOUND, 100.0)
    assert err <= SILU_BOUND
    if count >= 3:
        assert out[0] == 0.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols", R.SOFTMAX_COLS)
def test_softmax_rows(gpu, cols, dtype):
    """cols 1024 / 2048 / 4096 take the register-resident kernels, every other width the generic one."""
    rows = R.SOFTMAX_ROWS
    s = R.softmax_case(cols)
    out0 = _sent((rows + 1) * cols, dtype)
    out = out0.cuda()
    _call("rdeic_softmax_rows", s, rows, cols, R.SOFTMAX_SCALE, out, _dt(dtype))
    out = out.cpu()
    assert _same(out[rows * cols:], out0[rows * cols:])  # rows past `rows` untouched
    got = out[:rows * cols].view(rows, cols)
    ref = R.softmax_rows_ref(s, R.SOFTMAX_SCALE)
    if dtype == torch.float32:
        err = float((got.double() - ref).abs().max())
        _report("softmax_rows", f"cols={cols}", err, SOFTMAX_BOUND, 1.0)
        assert err <= SOFTMAX_BOUND
        assert ((got.double().sum(1) - 1).abs() <= cols * 2.0 ** -23).all()
    else:
        rb = ref.to(torch.bfloat16).float()
        ulp = torch.where(rb == 0, torch.zeros_like(rb), torch.ldexp(torch.ones_like(rb), torch.frexp(rb).exponent - 8))
        assert ((got.float() - rb).abs() <= SOFTMAX_BOUND + ulp).all()
