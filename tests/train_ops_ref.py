"""TEST INFRASTRUCTURE: float64 references, the error metric and the bf16 yardstick of the per-op
training tests (tests/test_train_ops_gpu.py, checked for power by tests/test_train_ops_ref_cpu.py).
Plain torch, importable without a GPU, never imported by the product.

Every reference below is ONE function used twice:
  * reference: float64 tensors, `r` = identity. Torch autograd differentiates it.
  * bf16 yardstick: float32 tensors, `r` = round_bf16 (RoundBF16: rounds to bf16 in the forward AND in
    the backward), applied at exactly the tensors the HIP op materialises in bf16 (conv z / out / dz /
    dx, the norms' y / dx, ...). Parameter gradients stay fp32. The rounding is integer arithmetic on
    the fp32 bit pattern, so the yardstick uses no torch bf16 kernel and no MIOpen bf16 path.

Inputs are rounded to the compute dtype by the caller (to_compute), in bf16 mode the conv / linear
weights too (they are packed in bf16), so reference, yardstick and kernel see the same values.

Metric: mixed_err(got, ref) = max_i |got_i - ref_i| / (|ref_i| + rms(ref)) in float64: a small element
is held to the tensor's rms, not to its largest entry. rms(ref) == 0 demands exact zeros.

Bounds (bound()): fp32 mode FP32_BOUND[op]; bf16 mode BF16_FACTOR * err_Y + sum_noise(N) for the same
tensor and case, err_Y = mixed_err(yardstick, reference). sum_noise(N) = sqrt(N) * 2^-24, N the longest
sum behind one output element of the case (pixels of a weight gradient, k of a GEMM, ...): where the
yardstick rounds nothing to bf16 (parameter gradients, an fp32 GEMM output of bf16 operands) err_Y is
itself only the noise of ONE fp32 summation order, the host's, and can be exactly 0 when every partial
sum happens to be exact. An fp32 sum of N terms in another order differs by a random walk of N roundings
of relative size 2^-24 on partial sums no larger than ~sqrt(N) terms, i.e. by ~sqrt(N) * 2^-24 of the
result's rms, which is the unit mixed_err measures in. That is 1e-6 at N = 300 and 3e-6 at N = 2500,
three orders below the bf16 yardstick (2e-3 .. 8e-3), so it changes nothing for tensors that carry a
bf16 rounding and holds the others at summation-noise scale, far below the fp32-mode tolerance.

Layouts: activations NCHW, token tensors [rows, c]; the GPU tests convert to the kernels' NHWC."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from oracle import train_ref

NONE, LEAKY, GELU, SILU = 0, 1, 2, 3

FP32_BOUND = {"conv": 1e-5, "linear": 1e-5, "gemm": 1e-5, "act": 1e-5, "geglu": 1e-5,
              "group_norm": 1e-4, "layer_norm": 1e-4, "ckbd": 1e-4, "vq": 1e-4}
# our kernels differ from the yardstick in summation order and in at most one extra rounded intermediate;
# independent roundings add in quadrature and the maximum over ~1e5 elements needs head-room. A wrong
# term or index moves a result by the tensor's own scale, several hundred times the bf16 yardstick.
BF16_FACTOR = 4.0


# ------------------------------------------------------------------------------------ metric / rounding
def mixed_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    got = got.detach().to("cpu", torch.float64)
    ref = ref.detach().to("cpu", torch.float64)
    if got.shape != ref.shape:
        raise ValueError(f"shape mismatch {tuple(got.shape)} vs {tuple(ref.shape)}")
    if ref.numel() == 0:
        raise ValueError("empty reference")
    if not bool(torch.isfinite(got).all()):
        return math.inf
    rms = float(ref.pow(2).mean().sqrt())
    diff = (got - ref).abs()
    if rms == 0.0:
        return 0.0 if float(diff.max()) == 0.0 else math.inf
    return float((diff / (ref.abs() + rms)).max())


def bf16_round_(t32: torch.Tensor) -> torch.Tensor:
    """Round-to-nearest-even of fp32 values to bf16 precision, kept as fp32 (integer arithmetic)."""
    bits = t32.contiguous().view(torch.int32)
    bits = (bits + (0x7FFF + ((bits >> 16) & 1))) & -65536
    return bits.view(torch.float32)


class RoundBF16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, fwd: bool = True, bwd: bool = True):
        ctx.bwd = bwd
        return bf16_round_(x.to(torch.float32)).to(x.dtype) if fwd else x.clone()

    @staticmethod
    def backward(ctx, g):
        return (bf16_round_(g.to(torch.float32)).to(g.dtype) if ctx.bwd else g), None, None


def ident(t, fwd: bool = True, bwd: bool = True):
    return t


def round_bf16(t, fwd: bool = True, bwd: bool = True):
    return RoundBF16.apply(t, fwd, bwd)


def to_compute(t: torch.Tensor, bf16: bool) -> torch.Tensor:
    """fp32 values representable in the compute dtype (what the kernel is handed)."""
    t = t.detach().to(torch.float32)
    return bf16_round_(t).clone() if bf16 else t.clone()


def leaves(ts, dtype):
    return [None if t is None else t.detach().to(dtype).clone().requires_grad_(True) for t in ts]


def sum_noise(n_sum: int) -> float:
    """fp32 summation-order noise of an n_sum-term sum, in units of the result's rms (module docstring)."""
    return math.sqrt(max(int(n_sum), 1)) * 2.0 ** -24


def bound(op: str, bf16: bool, err_y: float = 0.0, n_sum: int = 1) -> float:
    return BF16_FACTOR * err_y + sum_noise(n_sum) if bf16 else FP32_BOUND[op]


# --------------------------------------------------------------------------------------- activations
def act_ref(z, kind: int, slope: float = 0.0):
    if kind == LEAKY:
        return torch.where(z > 0, z, z * slope)
    if kind == GELU:
        return 0.5 * z * (1.0 + torch.erf(z * 0.7071067811865476))
    if kind == SILU:
        return z * torch.sigmoid(z)
    return z


def act_op(z, kind: int, slope: float = 0.0, r=ident):
    """AG.act: out = act(z); materialises out and dz."""
    return r(act_ref(r(z), kind, slope))


def geglu_op(x, r=ident):
    """AG.geglu: x = [a | gate] -> a * gelu(gate); materialises out and dx."""
    a, g = r(x).chunk(2, dim=-1)
    return r(a * act_ref(g, GELU))


# -------------------------------------------------------------------------------------------- norms
def group_norm_core(x, gamma, beta, groups: int, eps: float, silu: bool):
    n, c = x.shape[0], x.shape[1]
    xg = x.reshape(n, groups, -1)
    mean = xg.mean(2, keepdim=True)
    var = xg.var(2, unbiased=False, keepdim=True)
    xh = ((xg - mean) / torch.sqrt(var + eps)).reshape(x.shape)
    shp = (1, c) + (1,) * (x.dim() - 2)
    y = xh * gamma.view(shp) + beta.view(shp)
    return y * torch.sigmoid(y) if silu else y


def group_norm_op(x, gamma, beta, groups: int, eps: float, silu: bool, r=ident, passthrough: bool = False,
                  core=group_norm_core):
    """AG.group_norm over NCHW x. Materialises y and dx; with passthrough the alias's gradient is added to the
    rounded dx and the sum rounded again (autograd's add of two compute-dtype tensors)."""
    xin = r(x)
    y = r(core(r(xin) if passthrough else xin, gamma, beta, groups, eps, silu))
    return (y, xin) if passthrough else y


def layer_norm_core(x, gamma, beta, eps: float):
    mean = x.mean(1, keepdim=True)
    var = x.var(1, unbiased=False, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma + beta


def layer_norm_op(x, gamma, beta, eps: float = 1e-5, r=ident, passthrough: bool = False, core=layer_norm_core):
    xin = r(x)
    y = r(core(r(xin) if passthrough else xin, gamma, beta, eps))
    return (y, xin) if passthrough else y


# ------------------------------------------------------------------------------------ conv / linear
def conv_op(x, W, b, emb, res, *, stride=1, pad=0, up2=False, pixel_shuffle=False, act=NONE, slope=0.0,
            out_f32=False, r=ident):
    """AG.conv2d: out = act(PixelShuffle?(conv(up2?(x)) + b + emb[img])) + res over NCHW.
    Materialised in the compute dtype: dx (and the full-size gradient before the 2x2 sum of an up2 conv),
    the conv output (z when an activation follows, else out with the residual fused into the same
    rounding), out, dz. out_f32: the conv's output stays fp32, only its gradient dz is rounded."""
    xin = r(x)
    xi = r(F.interpolate(xin, scale_factor=2.0, mode="nearest"), False, True) if up2 else xin
    z = F.conv2d(xi, W, b, stride=stride, padding=pad)
    if emb is not None:
        z = z + emb[:, :, None, None]
    if pixel_shuffle:
        z = F.pixel_shuffle(z, 2)
    if act == NONE:
        if res is not None:
            z = z + r(res, True, False)
        return r(z, not out_f32, True)
    z = r(z, not out_f32, True)
    out = act_ref(z, act, slope)
    if res is not None:
        out = out + r(res, True, False)
    return r(out, not out_f32, True)


def linear_op(x, W, b, res, r=ident, out_f32=False):
    """AG.linear: x W^T + b (+ res) over [rows, cin] tokens (the 1x1 conv kernels)."""
    z = r(x) @ W.t()
    if b is not None:
        z = z + b
    if res is not None:
        z = z + r(res, True, False)
    return r(z, not out_f32, True)


# layout ops (exact data movement), NCHW
def im2col_ref(x, kh, kw, stride, pad, ho, wo, up2):
    """[n*ho*wo, (ky*kw + kx)*c + ci] patches (zero outside; up2: of the nearest-upsampled input)."""
    if up2:
        x = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
    n, c, h, w = x.shape
    xp = torch.zeros((n, c, h + 2 * pad + stride, w + 2 * pad + stride), dtype=x.dtype)
    xp[:, :, pad:pad + h, pad:pad + w] = x
    cols = []
    for ky in range(kh):
        for kx in range(kw):
            cols.append(xp[:, :, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride])
    out = torch.stack(cols, 1)                      # n, taps, c, ho, wo
    return out.permute(0, 3, 4, 1, 2).reshape(n * ho * wo, kh * kw * c)


def zero_insert2_ref(x, odd: bool = False):
    n, c, h, w = x.shape
    out = torch.zeros((n, c, 2 * h, 2 * w), dtype=x.dtype)
    o = 1 if odd else 0
    out[:, :, o::2, o::2] = x
    return out


def sum_pool2_ref(x, pixels: int = 4):
    parts = [x[:, :, 0::2, 0::2], x[:, :, 1::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 1::2]]
    return sum(parts[:pixels])


def pixel_unshuffle2_ref(x, swapped: bool = False):
    """[n, 4c, h, w] with channel 4*cc + 2*i + j = x[n, cc, 2y + i, 2x + j] (swapped: the wrong 2*j + i)."""
    n, c, h2, w2 = x.shape
    t = x.reshape(n, c, h2 // 2, 2, w2 // 2, 2)     # n c y i x j
    t = t.permute(0, 1, 5, 3, 2, 4) if swapped else t.permute(0, 1, 3, 5, 2, 4)
    return t.reshape(n, 4 * c, h2 // 2, w2 // 2)


def ckbd_mask_ref(x, which: int, flipped: bool = False):
    h, w = x.shape[2], x.shape[3]
    m = anchor_mask(h, w, x.dtype, flipped)
    return x * (m if which else 1 - m)


# -------------------------------------------------------------------------------------- checkerboard
def anchor_mask(h, w, dtype, flipped: bool = False):
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    m = ((yy + xx) % 2 == (0 if flipped else 1)).to(dtype)
    return m[None, None]


def ckbd_op(y, pa, pn, noise, r=ident, flipped: bool = False, lower_bound=train_ref.lower_bound):
    """One slice of the checkerboard entropy model through oracle/train_ref.py (CkbdAnchorFn + CkbdLikFn):
    (anchor_hat, S = sum ln lik, nonanchor_hat). y feeds both Functions, so its gradient is autograd's sum of
    their two compute-dtype gradients. pa / pn: [n, 2c, h, w] = (scales | means)."""
    h, w = y.shape[2], y.shape[3]
    ma, mn = anchor_mask(h, w, y.dtype, flipped), 1 - anchor_mask(h, w, y.dtype, flipped)
    yin = r(y)
    y1, y2 = r(yin), r(yin)
    pa, pn = r(pa), r(pn)
    sa, mua = pa.chunk(2, 1)
    sn, mun = pn.chunk(2, 1)
    mua_d = mua.detach()
    anchor = r(train_ref.quantize_ste(y1 * ma - mua_d * ma) + mua_d * ma)
    scales = sa * ma + sn * mn
    means = mua * ma + mun * mn
    outputs = y2 + noise
    values = torch.abs(outputs - means)
    s = lower_bound(scales, train_ref.SCALE_BOUND)
    lik = (train_ref.standardized_cumulative((0.5 - values) / s)
           - train_ref.standardized_cumulative((-0.5 - values) / s))
    lik = lower_bound(lik, train_ref.LIKELIHOOD_BOUND)
    S = torch.log(lik).sum()
    mun_d = mun.detach()
    non = r(train_ref.quantize_ste(y2 * mn - mun_d * mn) + mun_d * mn)
    return anchor, S, non


def plain_bound(x, b):
    """LowerBound without its backward rule (the gradient of a plain max): a mutant."""
    return torch.clamp_min(x, b)


def quant_fracs(y, mu):
    """frac(y - mu) in [0, 1): distance pattern of the quantisation inputs from a rounding tie (0.5)."""
    d = y.double() - mu.double()
    return d - torch.floor(d)


# ------------------------------------------------------------------------------------------------ VQ
def vq_distances(z, E):
    """d[p][e] = -|z_p|^2 - |E_e|^2 + 2 z_p . E_e (larger = closer)."""
    return -(z ** 2).sum(1, keepdim=True) - (E ** 2).sum(1) + 2.0 * z @ E.t()


def vq_train_ref(z, E, embed_prob, beta: float, decay: float, temp: float, npos_fixed=None):
    """VectorQuantiser training forward (anchor 'closest', contrastive loss) as rdeic_vq_train states it.
    z [P, D] and E [K, D] float64 leaves. Returns (z_q straight-through, loss, E_new, embed_prob_new, idx).
      idx_p = argmax_e d[p][e]; z_q = E[idx]; loss = beta mean((z_q.detach - z)^2) + mean((z_q - z.detach)^2)
      embed_prob <- embed_prob * decay + usage * (1 - decay)
      E_e <- E_e (1 - a_e) + z[argmax_p d[p][e]] a_e, a = exp(-embed_prob K 10 / (1 - decay) - 1e-3)
      contrastive: per code, pos = mean of the max(1, P // K) largest d[:, e], neg = the P // 2 smallest,
      CE(target 0) over [pos, neg] / temp, mean over codes.
    The codebook is re-initialised in place before the backward, so the gradient of the -|E|^2 term of d is taken
    at the NEW row (what autograd does after the reference's .data update); z is detached inside d."""
    P, K = z.shape[0], E.shape[0]
    zd = z.detach()
    d = vq_distances(zd, E.detach())
    idx = d.argmax(1)
    zq = E[idx]
    loss = beta * ((zq.detach() - z) ** 2).mean() + ((zq - zd) ** 2).mean()
    zq_st = z + (zq - z).detach()
    usage = torch.bincount(idx, minlength=K).to(z.dtype) / P
    ep = embed_prob * decay + usage * (1.0 - decay)
    a = torch.exp(-(ep * K * 10.0) / (1.0 - decay) - 1e-3)[:, None]
    E_new = E.detach() * (1 - a) + zd[d.argmax(0)] * a
    # value of |E|^2 at the old rows, gradient 2 * E_new
    esq = (E.detach() ** 2).sum(1) + (2.0 * E_new * (E - E.detach())).sum(1)
    dg = -(zd ** 2).sum(1, keepdim=True) - esq + 2.0 * zd @ E.t()
    sd = dg.sort(dim=0).values
    npos = max(1, P // K) if npos_fixed is None else npos_fixed
    dis = torch.cat([sd[P - npos:].mean(0, keepdim=True), sd[:P // 2]], 0).t() / temp
    loss = loss + F.cross_entropy(dis, torch.zeros(K, dtype=torch.long))
    return zq_st, loss, E_new, ep, idx


def vq_gaps(z, E):
    """(per row: relative gap between the nearest and second nearest code, per code: relative gap between the
    closest and second closest point) of the float64 distances."""
    d = vq_distances(z.double(), E.double())
    t1 = d.topk(2, dim=1).values
    t0 = d.topk(2, dim=0).values
    return ((t1[:, 0] - t1[:, 1]) / t1[:, 0].abs()).min().item(), ((t0[0] - t0[1]) / t0[0].abs()).min().item()


# ------------------------------------------------------------------- running a reference / yardstick
def run_op(fn, inputs: dict, gouts, names, dtype, r):
    """Forward fn(**leaves, r=r) and backward of sum_i <out_i, gout_i>. Returns {output name: value,
    'd' + input name: gradient} (detached, on the CPU). gouts entries: a tensor, a float (scalar outputs) or
    None (no gradient reaches that output)."""
    lv = {k: (None if v is None else v.detach().to(dtype).clone().requires_grad_(True)) for k, v in inputs.items()}
    outs = fn(**lv, r=r)
    outs = outs if isinstance(outs, tuple) else (outs,)
    total = None
    for o, g in zip(outs, gouts):
        if g is None:
            continue
        term = (o * (g.to(dtype) if torch.is_tensor(g) else g)).sum()
        total = term if total is None else total + term
    total.backward()
    res = {nm: o.detach() for nm, o in zip(names, outs)}
    for k, v in lv.items():
        if v is not None and v.grad is not None:
            res["d" + k] = v.grad.detach()
    return res


def reference_and_yardstick(fn, inputs, gouts, names, bf16: bool):
    """(float64 reference, fp32 + RoundBF16 yardstick or None in fp32 mode) of one case."""
    ref = run_op(fn, inputs, gouts, names, torch.float64, ident)
    yard = run_op(fn, inputs, gouts, names, torch.float32, round_bf16) if bf16 else None
    return ref, yard


def case_bounds(op: str, ref: dict, yard, bf16: bool, n_sum: int = 1) -> dict:
    """{tensor: (bound, err_Y)} for every tensor of a case (n_sum: the case's longest sum, see bound())."""
    out = {}
    for k, v in ref.items():
        ey = mixed_err(yard[k], v) if bf16 else 0.0
        out[k] = (bound(op, bf16, ey, n_sum), ey)
    return out


def gn_n_sum(case) -> int:
    n, c, groups, h, w = case
    return max(n * h * w, h * w * (c // groups))      # dgamma / dbeta over pixels, statistics over a group


def ln_n_sum(case) -> int:
    return max(case)                                  # dgamma / dbeta over rows, statistics over c


def conv_n_sum(case, n, h, w) -> int:
    cin, cout, k = case[:3]
    o = conv_out_shape(case, n, h, w)
    return max(o[0] * o[2] * o[3], cin * k * k, cout * k * k)   # dW / db over pixels, out over cin taps, dx over cout taps


# ------------------------------------------------------------------ cases and seeded inputs (shared)
GN_CASES = [  # n, c, groups, h, w
    (2, 32, 32, 3, 11),     # cpg = 1, hw = 33: one full 32-pixel chunk plus 1
    (1, 320, 32, 8, 8),     # second 256-channel block
    (3, 640, 32, 5, 7),     # n > 2, three channel blocks
    (1, 2560, 32, 4, 4),    # concat width, hw < chunk
    (1, 1024, 2, 2, 17),    # cpg = 512 > 256
    (1, 576, 2, 1, 2),      # cpg = 288 > 256 with a group of only 576 elements: small enough for a 1/N error to show
]
LN_CASES = [(1, 64), (5, 72), (1025, 320), (2500, 64), (7, 2048)]  # rows, c

# cin, cout, k, stride, pad, up2, pixel_shuffle, act, slope, emb, res (tests/test_train_kernels_gpu.py's, 12x10)
CONV_CASES_SMALL = [
    (16, 24, 3, 1, 1, False, False, 0, 0.0, True, True),
    (24, 16, 3, 2, 1, False, False, 1, 0.01, False, False),
    (16, 32, 1, 2, 0, False, False, 0, 0.0, False, False),
    (8, 16, 5, 1, 2, False, False, 2, 0.0, False, False),
    (32, 32, 3, 1, 1, True, False, 0, 0.0, False, False),
    (16, 64, 1, 1, 0, False, True, 1, 0.01, False, True),
    (64, 40, 3, 1, 1, False, False, 1, 0.1, False, True),
]
# the same tuple + out_f32, at 8x8 with n = 2: the 64-channel-aligned routes of the real layers
CONV_CASES_ALIGNED = [
    (64, 128, 3, 1, 1, False, False, 0, 0.0, False, True, False),
    (128, 64, 3, 2, 1, False, False, 0, 0.0, False, False, False),
    (64, 64, 3, 1, 1, True, False, 0, 0.0, False, False, False),
    (64, 256, 1, 1, 0, False, True, 1, 0.01, False, True, False),
    (192, 64, 1, 1, 0, False, False, 0, 0.0, False, False, False),
    (64, 128, 3, 1, 1, False, False, 0, 0.0, False, False, True),
]
CONV_CASE_EVEN_K = (16, 16, 4, 2, 1, False, False, 0, 0.0, False, False, False)   # even kernel, stride 2, 8x8, n = 2
CONV_CASE_EMB3 = (16, 24, 3, 1, 1, False, False, 0, 0.0, True, False, False)      # n = 3: col_sum groups = 3


def conv_case_list():
    """[(id, case tuple with out_f32, n, h, w)] of every conv case of the GPU test."""
    out = [(f"small{i}", c + (False,), 2, 12, 10) for i, c in enumerate(CONV_CASES_SMALL)]
    out += [(f"aligned{i}", c, 2, 8, 8) for i, c in enumerate(CONV_CASES_ALIGNED)]
    out += [("even_k", CONV_CASE_EVEN_K, 2, 8, 8), ("emb_n3", CONV_CASE_EMB3, 3, 6, 10)]
    return out


def _gen(seed: int):
    return torch.Generator().manual_seed(seed)


def gn_inputs(case, seed: int, bf16: bool, mean: float = 0.5, spread: float = 2.0):
    n, c, groups, h, w = case
    g = _gen(seed)
    x = to_compute(torch.randn((n, c, h, w), generator=g) * spread + mean, bf16)
    gamma = torch.rand(c, generator=g) + 0.5
    beta = torch.randn(c, generator=g) * 0.1
    # upstream gradient correlated with x and with a DC part: with a purely random one the mean(g) and
    # xhat * mean(g * xhat) terms of dx shrink as 1 / sqrt(group size) and a kernel without them would pass
    gy = to_compute(torch.randn((n, c, h, w), generator=g) + 0.6 * (x - mean) / spread + 0.3, bf16)
    gres = to_compute(torch.randn((n, c, h, w), generator=g), bf16)
    return dict(x=x, gamma=gamma, beta=beta), gy, gres


def ln_inputs(case, seed: int, bf16: bool):
    rows, c = case
    g = _gen(seed)
    x = to_compute(torch.randn((rows, c), generator=g) * 1.5 + 0.3, bf16)
    gamma = torch.rand(c, generator=g) + 0.5
    beta = torch.randn(c, generator=g) * 0.1
    gy = to_compute(torch.randn((rows, c), generator=g) + 0.6 * (x - 0.3) / 1.5 + 0.3, bf16)  # as gn_inputs
    gres = to_compute(torch.randn((rows, c), generator=g), bf16)
    return dict(x=x, gamma=gamma, beta=beta), gy, gres


def conv_out_shape(case, n, h, w):
    cin, cout, k, stride, pad, up2, ps = case[:7]
    hi, wi = (2 * h, 2 * w) if up2 else (h, w)
    ho, wo = (hi + 2 * pad - k) // stride + 1, (wi + 2 * pad - k) // stride + 1
    return (n, cout // 4, 2 * ho, 2 * wo) if ps else (n, cout, ho, wo)


def conv_inputs(case, n, h, w, seed: int, bf16: bool):
    cin, cout, k, stride, pad, up2, ps, act, slope, use_emb, use_res, out_f32 = case
    g = _gen(seed)
    x = to_compute(torch.randn((n, cin, h, w), generator=g), bf16)
    W = to_compute(torch.randn((cout, cin, k, k), generator=g) / math.sqrt(cin * k * k), bf16)
    b = torch.randn(cout, generator=g) * 0.1
    emb = torch.randn((n, cout), generator=g) if use_emb else None
    oshape = conv_out_shape(case, n, h, w)
    res = to_compute(torch.randn(oshape, generator=g), bf16 and not out_f32) if use_res else None
    gout = to_compute(torch.randn(oshape, generator=g), bf16 and not out_f32)
    return dict(x=x, W=W, b=b, emb=emb, res=res), gout


def conv_fn(case):
    cin, cout, k, stride, pad, up2, ps, act, slope, use_emb, use_res, out_f32 = case

    def fn(x, W, b, emb, res, r):
        return conv_op(x, W, b, emb, res, stride=stride, pad=pad, up2=up2, pixel_shuffle=ps, act=act, slope=slope,
                       out_f32=out_f32, r=r)
    return fn


def conv_dz(case, inputs, gout):
    """float64 dz = gradient of the conv's own output [n, cout, ho, wo] (after the act backward and the
    PixelShuffle backward), for the hand-written dgrad / wgrad formulas of the mutants."""
    cin, cout, k, stride, pad, up2, ps, act, slope = case[:9]
    x, W, b, emb = (None if inputs[q] is None else inputs[q].double() for q in ("x", "W", "b", "emb"))
    xi = F.interpolate(x, scale_factor=2.0, mode="nearest") if up2 else x
    z = F.conv2d(xi, W, b, stride=stride, padding=pad)
    if emb is not None:
        z = z + emb[:, :, None, None]
    z = z.detach().requires_grad_(True)
    zz = F.pixel_shuffle(z, 2) if ps else z
    (act_ref(zz, act, slope) * gout.double()).sum().backward()
    return z.grad


def conv_dgrad_manual(dz, W, case, in_hw, flip: bool = True, odd: bool = False, pool_pixels: int = 4):
    """dx as autograd.py computes it: conv(dz zero-inserted for stride 2, W flipped and transposed, pad k-1-p),
    then the 2x2 sum for an up2 conv. flip / odd / pool_pixels select the mutants."""
    cin, cout, k, stride, pad, up2 = case[:6]
    h, w = in_hw
    hi, wi = (2 * h, 2 * w) if up2 else (h, w)
    src = zero_insert2_ref(dz, odd) if stride == 2 else dz
    Wt = W.transpose(0, 1)
    Wt = Wt.flip(2, 3) if flip else Wt
    top = k - 1 - pad
    bot_h, bot_w = hi + k - 1 - src.shape[2] - top, wi + k - 1 - src.shape[3] - top
    d_in = F.conv2d(F.pad(src, (top, bot_w, top, bot_h)), Wt)
    return sum_pool2_ref(d_in, pool_pixels) if up2 else d_in


def ckbd_inputs(seed: int, bf16: bool, n=3, c=5, h=5, w=6):
    """Slice inputs with scales on both sides of 0.11, |y - mu| up to ~25 scale units (the 1e-9 likelihood floor)
    and quantisation inputs away from rounding ties: frac(y - mu) drawn from [0.1, 0.4] u [0.6, 0.9] before the
    rounding to the compute dtype (the CPU test asserts [0.05, 0.45] u [0.55, 0.95] after it)."""
    g = _gen(seed)

    def params():
        scale = torch.rand((n, c, h, w), generator=g) * 0.5 + 0.01
        scale[:, :, ::2] *= 0.3
        mu = torch.randn((n, c, h, w), generator=g)
        return to_compute(torch.cat([scale, mu], 1), bf16)
    pa, pn = params(), params()
    ma = anchor_mask(h, w, torch.float32)
    mu = pa[:, c:] * ma + pn[:, c:] * (1 - ma)
    k = torch.randint(-3, 4, (n, c, h, w), generator=g).float()
    frac = torch.rand((n, c, h, w), generator=g) * 0.3 + 0.1
    frac = torch.where(torch.rand((n, c, h, w), generator=g) < 0.5, frac, frac + 0.5)
    y = to_compute(mu + k + frac, bf16)
    noise = torch.rand((n, c, h, w), generator=g) - 0.5
    gA = to_compute(torch.randn((n, c, h, w), generator=g), bf16)
    gN = to_compute(torch.randn((n, c, h, w), generator=g), bf16)
    return dict(y=y, pa=pa, pn=pn), noise, gA, gN


VQ_CASES = [(96, 40, 24), (192, 16, 8), (64, 300, 512)]  # P, K, D
VQ_SEEDS = {(96, 40, 24): 10, (192, 16, 8): 9, (64, 300, 512): 11}  # chosen so that the tie conditions hold


def vq_inputs(case, seed: int):
    """Scales chosen so that the distances spread over a few units of temp = 0.07 (as the real hyper-latents do):
    with larger inputs the contrastive cross entropy saturates at 0 and tests nothing. At D = 512 the first 6
    dimensions carry the geometry and the rest 2% of it: in 512 isotropic dimensions all distances concentrate
    and no seed keeps every nearest-code / closest-point gap above 1e-3."""
    P, K, D = case
    g = _gen(seed)
    scale = torch.full((D,), 0.15 if D <= 8 else 0.1)
    if D > 64:
        scale = torch.cat([torch.full((6,), 0.15), torch.full((D - 6,), 0.003)])
    z = torch.randn((P, D), generator=g) * scale
    E = torch.randn((K, D), generator=g) * scale
    # usage EMA around the re-initialisation threshold: a = exp(-ep K 1000) from ~1 down to ~0
    ep = 10.0 ** (torch.rand(K, generator=g) * 4 - 6) / K * 16
    gz = torch.randn((P, D), generator=g)
    return z, E, ep, gz


def vq_reference(case, seed: int, npos_fixed=None, gloss: float = 1.3):
    z, E, ep, gz = vq_inputs(case, seed)
    zl, El = leaves((z, E), torch.float64)
    zq, loss, E_new, ep_new, idx = vq_train_ref(zl, El, ep.double(), 0.25, 0.99, 0.07, npos_fixed)
    (loss * gloss + (zq * gz.double()).sum()).backward()
    return dict(zq=zq.detach(), loss=loss.detach().view(1), E_new=E_new, embed_prob=ep_new, dz=zl.grad, dE=El.grad), idx
