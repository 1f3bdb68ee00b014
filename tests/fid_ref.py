"""A restatement of FID / KID on the CPU in torch / numpy, written from the published architecture (Szegedy et al.
2016 as pytorch-fid's FID variant lays it out: FIDInceptionA / C / E_1 / E_2 around torchvision's B / D blocks) and
from the published formulas (Heusel et al. 2017; Binkowski et al. 2018), not from rdeic_amd/fid.py. Activations
are NCHW, convs are F.conv2d followed by an unfolded BatchNorm(eps 1e-3) and ReLU. dtype float64 is the reference;
the same code in float32 is the yardstick for what fp32 arithmetic costs.

The bilinear source index and weight are part of the definition and are computed in float32, as torch does for a
float32 image (s = max((d + 0.5) * (in / out) - 0.5, 0)); the blend is done in `dtype`.
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-3


# ---------------------------------------------------------------- prep and pools
def _axis(n_in, n_out):
    scale = np.float32(n_in) / np.float32(n_out)
    d = np.arange(n_out, dtype=np.float32)
    s = np.maximum((d + np.float32(0.5)) * scale - np.float32(0.5), np.float32(0)).astype(np.float32)
    i0 = np.floor(s).astype(np.int64)
    i1 = np.minimum(i0 + 1, n_in - 1)
    t = (s - i0.astype(np.float32)).astype(np.float32)
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(t)


def prep(img_u8, size=(299, 299), dtype=torch.float64):
    """uint8 [n, h, w, 3] -> [n, 3, oh, ow]: bilinear resize of v / 255 (align_corners=False), then 2 v - 1."""
    oh, ow = (size, size) if isinstance(size, int) else size
    x = torch.as_tensor(img_u8).permute(0, 3, 1, 2).to(dtype) / 255
    y0, y1, ty = _axis(x.shape[2], oh)
    x0, x1, tx = _axis(x.shape[3], ow)
    ty, tx = ty.to(dtype)[None, None, :, None], tx.to(dtype)[None, None, None, :]
    top = x[:, :, y0][:, :, :, x0] * (1 - tx) + x[:, :, y0][:, :, :, x1] * tx
    bot = x[:, :, y1][:, :, :, x0] * (1 - tx) + x[:, :, y1][:, :, :, x1] * tx
    return (top * (1 - ty) + bot * ty) * 2 - 1


def max_pool(x, k, s, p=0):
    return F.max_pool2d(x, k, s, p)


def avg_pool(x, k=3, s=1, p=1):
    return F.avg_pool2d(x, k, s, p, count_include_pad=False)


# ---------------------------------------------------------------- the network
def conv_bn_relu(x, sd, name, stride=1, padding=0):
    dt = x.dtype
    y = F.conv2d(x, sd[name + ".conv.weight"].to(dt), None, stride, padding)
    y = F.batch_norm(y, sd[name + ".bn.running_mean"].to(dt), sd[name + ".bn.running_var"].to(dt),
                     sd[name + ".bn.weight"].to(dt), sd[name + ".bn.bias"].to(dt), False, 0.0, EPS)
    return F.relu(y)


def inception_a(x, sd, n):
    b1 = conv_bn_relu(x, sd, n + ".branch1x1")
    b5 = conv_bn_relu(conv_bn_relu(x, sd, n + ".branch5x5_1"), sd, n + ".branch5x5_2", padding=2)
    b3 = conv_bn_relu(x, sd, n + ".branch3x3dbl_1")
    b3 = conv_bn_relu(b3, sd, n + ".branch3x3dbl_2", padding=1)
    b3 = conv_bn_relu(b3, sd, n + ".branch3x3dbl_3", padding=1)
    bp = conv_bn_relu(avg_pool(x), sd, n + ".branch_pool")
    return torch.cat([b1, b5, b3, bp], 1)


def inception_b(x, sd, n):
    b3 = conv_bn_relu(x, sd, n + ".branch3x3", stride=2)
    bd = conv_bn_relu(x, sd, n + ".branch3x3dbl_1")
    bd = conv_bn_relu(bd, sd, n + ".branch3x3dbl_2", padding=1)
    bd = conv_bn_relu(bd, sd, n + ".branch3x3dbl_3", stride=2)
    return torch.cat([b3, bd, max_pool(x, 3, 2)], 1)


def inception_c(x, sd, n):
    b1 = conv_bn_relu(x, sd, n + ".branch1x1")
    b7 = conv_bn_relu(x, sd, n + ".branch7x7_1")
    b7 = conv_bn_relu(b7, sd, n + ".branch7x7_2", padding=(0, 3))
    b7 = conv_bn_relu(b7, sd, n + ".branch7x7_3", padding=(3, 0))
    bd = conv_bn_relu(x, sd, n + ".branch7x7dbl_1")
    bd = conv_bn_relu(bd, sd, n + ".branch7x7dbl_2", padding=(3, 0))
    bd = conv_bn_relu(bd, sd, n + ".branch7x7dbl_3", padding=(0, 3))
    bd = conv_bn_relu(bd, sd, n + ".branch7x7dbl_4", padding=(3, 0))
    bd = conv_bn_relu(bd, sd, n + ".branch7x7dbl_5", padding=(0, 3))
    bp = conv_bn_relu(avg_pool(x), sd, n + ".branch_pool")
    return torch.cat([b1, b7, bd, bp], 1)


def inception_d(x, sd, n):
    b3 = conv_bn_relu(conv_bn_relu(x, sd, n + ".branch3x3_1"), sd, n + ".branch3x3_2", stride=2)
    b7 = conv_bn_relu(x, sd, n + ".branch7x7x3_1")
    b7 = conv_bn_relu(b7, sd, n + ".branch7x7x3_2", padding=(0, 3))
    b7 = conv_bn_relu(b7, sd, n + ".branch7x7x3_3", padding=(3, 0))
    b7 = conv_bn_relu(b7, sd, n + ".branch7x7x3_4", stride=2)
    return torch.cat([b3, b7, max_pool(x, 3, 2)], 1)


def inception_e(x, sd, n, pool):
    b1 = conv_bn_relu(x, sd, n + ".branch1x1")
    b3 = conv_bn_relu(x, sd, n + ".branch3x3_1")
    b3 = torch.cat([conv_bn_relu(b3, sd, n + ".branch3x3_2a", padding=(0, 1)),
                    conv_bn_relu(b3, sd, n + ".branch3x3_2b", padding=(1, 0))], 1)
    bd = conv_bn_relu(x, sd, n + ".branch3x3dbl_1")
    bd = conv_bn_relu(bd, sd, n + ".branch3x3dbl_2", padding=1)
    bd = torch.cat([conv_bn_relu(bd, sd, n + ".branch3x3dbl_3a", padding=(0, 1)),
                    conv_bn_relu(bd, sd, n + ".branch3x3dbl_3b", padding=(1, 0))], 1)
    pooled = avg_pool(x) if pool == "avg" else max_pool(x, 3, 1, 1)
    bp = conv_bn_relu(pooled, sd, n + ".branch_pool")
    return torch.cat([b1, b3, bd, bp], 1)


BLOCKS = {
    "Mixed_5b": inception_a, "Mixed_5c": inception_a, "Mixed_5d": inception_a,
    "Mixed_6a": inception_b,
    "Mixed_6b": inception_c, "Mixed_6c": inception_c, "Mixed_6d": inception_c, "Mixed_6e": inception_c,
    "Mixed_7a": inception_d,
    "Mixed_7b": lambda x, sd, n: inception_e(x, sd, n, "avg"),
    "Mixed_7c": lambda x, sd, n: inception_e(x, sd, n, "max"),
}


def block(name, x, sd):
    """One Mixed block on an NCHW activation."""
    return BLOCKS[name](x, sd, name)


def tower(img_u8, sd, dtype=torch.float64):
    """uint8 [n, h, w, 3] -> [n, 2048] pool3 features."""
    x = prep(img_u8, 299, dtype)
    x = conv_bn_relu(x, sd, "Conv2d_1a_3x3", stride=2)
    x = conv_bn_relu(x, sd, "Conv2d_2a_3x3")
    x = conv_bn_relu(x, sd, "Conv2d_2b_3x3", padding=1)
    x = max_pool(x, 3, 2)
    x = conv_bn_relu(x, sd, "Conv2d_3b_1x1")
    x = conv_bn_relu(x, sd, "Conv2d_4a_3x3")
    x = max_pool(x, 3, 2)
    for name in BLOCKS:
        x = block(name, x, sd)
    return x.mean((2, 3))


# ---------------------------------------------------------------- set statistics and scores
def moments(x):
    """(sum [c], outer [c, c]) of [rows, c] features, float64."""
    x = np.asarray(x, np.float64)
    return x.sum(0), x.T @ x


def mean_cov(x):
    x = np.asarray(x, np.float64)
    return x.mean(0), np.cov(x, rowvar=False)


def fid(x1, x2):
    """The Frechet distance of two feature sets [rows, c] by the second route: tr (S1 S2)^(1/2) as the sum of
    the square roots of the (real, non-negative up to rounding) eigenvalues of the product S1 S2."""
    mu1, s1 = mean_cov(x1)
    mu2, s2 = mean_cov(x2)
    lam = np.linalg.eigvals(s1 @ s2).real
    d = mu1 - mu2
    return float(d @ d + np.trace(s1) + np.trace(s2) - 2.0 * np.sqrt(np.maximum(lam, 0.0)).sum())


def trace_sum(x1, x2):
    return float(np.trace(mean_cov(x1)[1]) + np.trace(mean_cov(x2)[1]))


def mmd2_brute(x, y):
    """Unbiased MMD^2 with k(a, b) = (a.b / d + 1)^3 as the plain double sums."""
    m, d = len(x), x.shape[1]
    k = lambda a, b: (float(np.dot(a, b)) / d + 1.0) ** 3  # noqa: E731
    sxx = sum(k(x[i], x[j]) for i in range(m) for j in range(m) if i != j)
    syy = sum(k(y[i], y[j]) for i in range(m) for j in range(m) if i != j)
    sxy = sum(k(x[i], y[j]) for i in range(m) for j in range(m))
    return sxx / (m * (m - 1)) + syy / (m * (m - 1)) - 2.0 * sxy / (m * m)


def kid(x1, x2, subsets, subset_size, seed):
    """(mean, std) of the brute-force MMD^2 over subsets drawn without replacement by np.random.RandomState(seed),
    set 1 first; subset_size clamped to the smaller set."""
    x1, x2 = np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    m = min(subset_size, len(x1), len(x2))
    rs = np.random.RandomState(seed)
    vals = []
    for _ in range(subsets):
        a = x1[rs.choice(len(x1), m, replace=False)]
        b = x2[rs.choice(len(x2), m, replace=False)]
        vals.append(mmd2_brute(a, b))
    return float(np.mean(vals)), float(np.std(vals))
