"""Plain CPU references, and the fixed inputs, for the per-op tests of the codec's small inference kernels
(csrc/entropy.hip, csrc/elementwise.hip, rdeic_softmax_rows / rdeic_transpose of csrc/attention.hip).

One function per op, dense tensors in the reference's layout (NCHW images, [rows][cols] matrices). The checkerboard
pieces are the oracle's own (oracle.model_ref.squeeze / unsqueeze, oracle.coders_ref.build_indexes /
quantize_symbols). The bit-exact ops are restated as one fp32 torch op per rounded device op, in the kernel's
documented order, every coefficient an fp32 tensor (so a division stays a division); the ops with a transcendental
are computed in float64.

`mutant=` names a deliberate defect of the REFERENCE. Only tests/test_codec_ops_ref_cpu.py passes it, to show that
the inputs built here (the very ones tests/test_codec_ops_gpu.py feeds the kernels) tell the defect from the
correct op. No GPU import in this file."""
import math

import numpy as np
import torch

from oracle import coders_ref as cr
from oracle import model_ref as mr

GRID_CAP = 16384 * 256  # threads of the largest grid the elementwise kernels launch; they stride beyond it
COUNTS = (1, 255, 257, GRID_CAP + 257)


def f32(v):
    return torch.tensor(v, dtype=torch.float32)


# ------------------------------------------------------------------------------------------ checkerboard
def _build_indexes(scales, table, mutant):
    if mutant not in ("lt", "no_bound"):
        return cr.build_indexes(scales, table)
    if mutant != "no_bound":
        scales = torch.max(scales, f32([cr.SCALE_BOUND]))
    indexes = scales.new_full(scales.size(), len(table) - 1).int()
    for s in table[:-1]:
        indexes -= ((scales < s) if mutant == "lt" else (scales <= s)).int()
    return indexes


def ckbd_encode_ref(y, params, phase, table, dtype=torch.float32, mutant=""):
    """y [n][c][hy][wy], params [n][2c][hy][wy] (scales, then means) -> (sym, idx, yhat_half, anchor_full):
    sym / idx int32 [n][c*hy*wy/2] in the stage order [c][hy][wy/2]; yhat_half = sym + mean scattered back to the
    full grid, zero at the other colour; anchor_full the same tensor (what the kernel leaves in anchor_out)."""
    if mutant == "phase":
        phase = 1 - phase
    y, params = y.to(dtype).float(), params.to(dtype).float()
    scales, means = params.chunk(2, 1)
    s_sq, m_sq = mr.squeeze(scales, phase), mr.squeeze(means, phase)
    idx = _build_indexes(s_sq, table, mutant)
    y_sq = mr.squeeze(y, phase)
    if mutant == "half_away":
        d = y_sq - m_sq
        sym = (torch.sign(d) * torch.floor(d.abs() + 0.5)).int()
    else:
        sym = cr.quantize_symbols(y_sq, m_sq)
    yhat_half = mr.unsqueeze((sym.float() + m_sq).to(dtype).float(), phase).to(dtype)
    n = y.shape[0]
    return sym.reshape(n, -1), idx.reshape(n, -1), yhat_half, yhat_half.clone()


def ckbd_dequant_ref(sym, params, phase, dtype=torch.float32):
    """sym int32 [n][c*hy*wy/2] (stage order), params as above -> (yhat_half, anchor_full)."""
    params = params.to(dtype).float()
    m_sq = mr.squeeze(params.chunk(2, 1)[1], phase)
    yhat_half = mr.unsqueeze((sym.reshape(m_sq.shape).float() + m_sq).to(dtype).float(), phase).to(dtype)
    return yhat_half, yhat_half.clone()


CKBD_SHAPES = ((3, 6, 10, 8), (2, 5, 4, 5), (1, 4, 2, 64))  # (n, hy, wy, c)
CKBD_LARGE = (4, 128, 260, 64)  # n*c*hy*wy/2 = 4259840 > GRID_CAP


def ckbd_table(dtype):
    """64 levels. fp32: the codec's table stretched down to 0.05, so that entries lie below the 0.11 scale bound and
    the bound decides indexes (the codec's own table starts exactly at float32(0.11), where clamping changes no
    index). bf16: the codec's table rounded to bf16 (entry 0 = 0.10986 < 0.11), so a bf16 scale can equal an entry."""
    if dtype == torch.float32:
        return cr.get_scale_table(min_=0.05)
    return cr.get_scale_table().to(dtype).float()


def ckbd_case(n, hy, wy, c, dtype):
    """(y, params, table), seeded by the shape, every value representable in dtype. Planted: y - mean exactly a
    half-integer (eighths, exact in bf16 too), scales exactly at table entries, scales below the bound."""
    g = torch.Generator().manual_seed(((n * 131 + hy) * 131 + wy) * 131 + c)
    table = ckbd_table(dtype)
    numel = n * c * hy * wy
    scale = torch.exp(torch.rand(numel, generator=g) * 8 - 3)
    mean = torch.randn(numel, generator=g) * 2
    y = mean + torch.randn(numel, generator=g) * 3
    # planted at random positions: a stride would put every plant on one colour of a narrow grid
    pos = torch.randperm(numel, generator=g)
    a, b, d = numel // 5, numel // 3, numel // 2
    scale[pos[:a]] = table[torch.randint(0, table.numel() - 1, (a,), generator=g)]
    scale[pos[a:b]] = 0.01
    scale[pos[b:d]] = 0.07
    pos = torch.randperm(numel, generator=g)[:numel // 3]
    mean[pos] = torch.randint(-16, 17, (pos.numel(),), generator=g).float() / 8
    y[pos] = mean[pos] + torch.randint(-6, 6, (pos.numel(),), generator=g).float() + 0.5
    shape = (n, c, hy, wy)
    params = torch.cat([scale.view(shape), mean.view(shape)], 1)
    return y.view(shape).to(dtype).float(), params.to(dtype).float(), table


# ---------------------------------------------------------------------------------------------------- VQ
def vq_argmin_ref(dot, zn, en, mutant=""):
    d = (zn[:, None] + en[None]) - 2 * dot
    if mutant == "last_min":
        return d.shape[1] - 1 - torch.argmin(d.flip(1), 1)
    return torch.argmin(d, 1)


def gather_rows_ref(table, idx, dtype=torch.float32):
    return table[idx.long()].to(dtype)


def row_sqnorm_ref(x):
    return (x.double() ** 2).sum(1)


VQ_NCODES = (1, 7, 255, 256, 257, 1000)  # and the checkpoint's codebook size (vq_codebook_size)
VQ_ROWS = (1, 5)
# (a, b), a < b. Thread of code j = j % 256; the block reduction first folds threads 128..255 onto 0..127.
#   (3, 259)   one thread, two trips of its loop        (130, 700)  threads 130 / 188, both above the split
#   (5, 200)   threads 5 / 200, across the split        (300, 513)  threads 44 / 1: the smaller index in the higher
VQ_TIES = ((3, 259), (130, 700), (5, 200), (300, 513))
VQ_TIE_SMALL = (2, 5)  # for the codebooks too small for any of the above


def vq_codebook_size():
    return mr.param_shapes()[mr.P + "quantize.embedding.weight"][0]


def vq_ties(rows, ncode):
    """{row: (a, b)}: the planted tie of each row that has one."""
    fit = [t for t in VQ_TIES if t[1] < ncode] or [t for t in (VQ_TIE_SMALL,) if t[1] < ncode]
    return {r: fit[r % len(fit)] for r in range(rows)} if fit else {}


def vq_case(rows, ncode):
    """(dot, zn, en) with, in every row, an exact two-way tie for the minimum at vq_ties(rows, ncode)[row]:
    en[b] = en[a] and dot[r][a] = dot[r][b] = 16 (every other distance is far larger)."""
    g = torch.Generator().manual_seed(rows * 100003 + ncode)
    dot = torch.randn(rows, ncode, generator=g)
    zn = torch.rand(rows, generator=g) * 4 + 1
    en = torch.rand(ncode, generator=g) * 4 + 1
    ties = vq_ties(rows, ncode)
    for a, b in set(ties.values()):
        en[b] = en[a]
    for r, (a, b) in ties.items():
        dot[r, a] = dot[r, b] = 16.0
    return dot, zn, en


# ------------------------------------------------------------------------------------ sampler and layout
def axpby_ref(x, z, a, b):
    """x, z [n_img][per_img], a, b [n_img]."""
    return a[:, None] * x + b[:, None] * z


DDIM_COEF = (0.62341, 0.78192, 0.93127, 0.36433)  # sqrt(1-a_t), sqrt(a_t), sqrt(a_prev), sqrt(1-a_prev-sigma^2)


def ddim_step_ref(x, e, c_sq1m, c_sqa, c_sqap, c_dir, mutant=""):
    p = (x - f32(c_sq1m) * e) / f32(c_sqa)
    xp = f32(c_sqap) * p + f32(c_dir) * (x if mutant == "dir_on_x" else e)
    return xp, p


def spaced_step_ref(x, e, noise, A, B, C1, C2, S):
    p = f32(A) * x - f32(B) * e
    mean = f32(C1) * p + f32(C2) * x
    return (mean if noise is None else mean + f32(S) * noise), p


def cfg_combine_ref(e_cond, e_uncond, scale):
    return mr.cfg(e_cond, e_uncond, f32(scale))


def pair_case(count, seed):
    g = torch.Generator().manual_seed(seed * 7919 + count % 7919)
    return torch.randn(count, generator=g), torch.randn(count, generator=g)


LAYOUT_SHAPES = ((2, 3, 5, 7), (1, 4, 8, 8))  # (n, c, h, w)
LAYOUT_MULADD = ((1.0, 0.0), (2.0, -1.0), (0.18215, 0.0))


def layout_case(n, c, h, w):
    g = torch.Generator().manual_seed(n * 1000 + c * 100 + h * 10 + w)
    return torch.randn(n, c, h, w, generator=g) * 3


def nchw_to_nhwc_ref(x, mul, add, dtype=torch.float32, mutant=""):
    v = (x + f32(add)) * f32(mul) if mutant == "add_first" else x * f32(mul) + f32(add)
    return v.permute(0, 2, 3, 1).contiguous().to(dtype)


def nhwc_to_nchw_ref(x, mul, add):
    return (x.float() * f32(mul) + f32(add)).permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------------------------ images
def u8_to_x_ref(u8, dtype=torch.float32, mutant=""):
    """uint8 array (any shape) -> x = fp32(u8 / 255.0 in fp64) * 2 - 1, rounded once to dtype."""
    v = (u8.astype(np.float64) / (256.0 if mutant == "div256" else 255.0)).astype(np.float32)
    v = v * np.float32(2) - np.float32(1)
    return torch.from_numpy(v).to(dtype)


def x_to_u8_ref(x, mutant=""):
    """((x + 1) / 2).clamp(0, 1) * 255, truncated. A NaN pixel becomes 0: the kernel clamps with fmaxf, which
    returns its non-NaN argument (torch.clamp would keep the NaN, whose conversion to uint8 is undefined)."""
    v = ((x.float() + 1) / 2).clamp(0, 1) * 255
    v = torch.nan_to_num(v, nan=0.0)
    if mutant == "round":
        v = torch.round(v)
    return v.to(torch.int32).to(torch.uint8)


def u8_boundary_values():
    """Every 2k/255 - 1 (fp32) with its two fp32 neighbours: the truncation boundaries of x -> u8."""
    k = np.arange(256, dtype=np.float64)
    b = (2.0 * k / 255.0 - 1.0).astype(np.float32)
    return torch.from_numpy(np.concatenate([b, np.nextafter(b, np.float32(-2)), np.nextafter(b, np.float32(2))]))


def x_to_u8_case(pix):
    """[pix][3] fp32: random in [-1.5, 1.5], then the boundaries, +-inf and NaN from the front."""
    g = torch.Generator().manual_seed(pix)
    x = (torch.rand(pix * 3, generator=g) * 3 - 1.5)
    special = torch.cat([u8_boundary_values(), torch.tensor([math.inf, -math.inf, math.nan])])
    k = min(special.numel(), x.numel())
    x[:k] = special[:k]
    return x.view(pix, 3)


def image_mse_ref(a, b, per_img):
    """a, b uint8 [n*per_img] -> fp32 [n]: exact int64 sum of squared differences / per_img in fp64, then fp32."""
    d = a.view(-1, per_img).to(torch.int64) - b.view(-1, per_img).to(torch.int64)
    return ((d * d).sum(1).double() / float(per_img)).float()


# ------------------------------------------------------------------------------------------------- other
def cast_ref(x, dtype):
    return x.to(dtype)


def pack_conv_weight_ref(w, wld, dtype=torch.float32):
    """torch conv weight [cout][cin][kh][kw] -> [cout][wld], k = (ky*kw + kx)*cin + ci, zero tail."""
    cout = w.shape[0]
    out = torch.zeros(cout, wld)
    out[:, :w[0].numel()] = w.permute(0, 2, 3, 1).reshape(cout, -1)
    return out.to(dtype)


TRANSPOSE_SHAPES = ((1, 1), (31, 33), (77, 64), (100, 513))  # (rows, cols)
TRANSPOSE_BATCH = 3


def transpose_case(rows, cols, dtype):
    """(flat input, ldin, ldout, in_bs, out_bs): batch TRANSPOSE_BATCH, leading dims and batch strides past the
    extents."""
    ldin, ldout = cols + 3, rows + 5
    in_bs, out_bs = rows * ldin + 7, cols * ldout + 11
    g = torch.Generator().manual_seed(rows * 1000 + cols)
    return torch.randn(TRANSPOSE_BATCH * in_bs, generator=g).to(dtype), ldin, ldout, in_bs, out_bs


def transpose_ref(src, rows, cols, ldin, out, ldout, batch, in_bs, out_bs, mutant=""):
    """out (flat, pre-filled) with out[b*out_bs + c*ldout + r] = src[b*in_bs + r*ldin + c]; the rest as it was."""
    b, r, c = np.meshgrid(np.arange(batch), np.arange(rows), np.arange(cols), indexing="ij")
    ldo = cols if mutant == "ldout_cols" else ldout
    dst, frm = (b * out_bs + c * ldo + r).reshape(-1), (b * in_bs + r * ldin + c).reshape(-1)
    keep = dst < out.numel()  # all of them, but for the mutant (whose stray writes past the buffer are dropped)
    res = out.clone()
    res[torch.from_numpy(dst[keep])] = src[torch.from_numpy(frm[keep])]
    return res


# ------------------------------------------------------------------- ops with a transcendental (float64)
def timestep_freqs(dim):
    half = dim // 2
    return torch.exp(-math.log(10000) * torch.arange(start=0, end=half, dtype=torch.float32) / half)


def timestep_embedding_ref(t, freqs):
    """float64 cos / sin of the fp32 product float32(t) * freqs[j] -> [n][2*half]."""
    arg = (t.float()[:, None] * freqs[None]).double()
    return torch.cat([torch.cos(arg), torch.sin(arg)], 1)


def silu_ref(x):
    xd = x.double()
    return xd / (1.0 + torch.exp(-xd))


def softmax_rows_ref(s, scale):
    return torch.softmax((s.float() * f32(scale)).double(), 1)


SOFTMAX_COLS = (1, 63, 65, 77, 1000, 1024, 2048, 4096)
SOFTMAX_ROWS = 5
SOFTMAX_SCALE = 512 ** -0.5  # the VAE attention block's; no power of two, so the fp32 product rounds


def softmax_case(cols):
    """fp32 scores whose scaled values spread over [-80, 80] (the extremes planted in every row)."""
    g = torch.Generator().manual_seed(cols)
    s = (torch.rand(SOFTMAX_ROWS, cols, generator=g) * 160 - 80) / SOFTMAX_SCALE
    s[:, 0] = 80 / SOFTMAX_SCALE
    if cols > 1:
        s[:, cols // 2] = -80 / SOFTMAX_SCALE
        s[1:, 0] = 79.0 / SOFTMAX_SCALE  # rows 1..: a crowd near the top, so that the sum is not one term
        s[1:, 1::2] = s[1:, 1::2] * 0.02 + 78 / SOFTMAX_SCALE
    return s


def silu_case():
    g = torch.Generator().manual_seed(5)
    x = torch.rand(4099, generator=g) * 200 - 100
    x[:3] = torch.tensor([0.0, 88.0, -88.0])
    return x
