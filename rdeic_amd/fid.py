"""FID (Heusel et al. 2017) and KID (Binkowski et al. 2018) on the device: the InceptionV3 feature tower and the
set statistics; the two scores themselves are float64 numpy on the host.

The network is the FID variant of InceptionV3 (the pytorch-fid / pyiqa `pt_inception` graph, not torchvision's
default): 94 bias-free convs, each followed by BatchNorm(eps 1e-3) and ReLU; the pool branches of the A and C
blocks and of Mixed_7b average with count_include_pad=False, Mixed_7c's pool branch is a max pool. The BatchNorms
are folded into the convs in float64 at load time; the convs run on the library's fp32 route with the ReLU in the
epilogue, every branch writing straight into its channel slice of the block's concat buffer. Four kernels of
fid.hip sit around them: the prep (uint8 -> bilinear 299 x 299 -> 2 v - 1, a zero fourth channel), the padded
max / average pool, the global average pool and the fp64 feature moments (sum and sum of outer products).

No weights ship with the project: the caller passes the torchvision-named state dict (.pt / .pth / .npz, or a
dict). The computation is pinned against a float64 restatement of the published architecture and formulas on
seeded weights (tests/fid_ref.py); parity with pytorch-fid, pyiqa and the published `pt_inception` weights is
unpinned, none of them is available offline.

Features are batch-invariant bit for bit: the library's own split-K rule (it looks at the launch) is pinned off
for the tower's convs and every conv output element is one fixed-order k sum, the pools are element-wise and the
global pool's order depends on (hw, c) only. The batch is therefore chunked freely (CHUNK) to keep every
activation tensor under 2^31 bytes.

The fp32 conv route adds an output's K products as one chain in k order. For the deep layers (K up to 4032) that
chain's rounding is several times that of a blocked sum, so a conv with more than SPLIT_MIN_K products runs as
split-K with a count fixed by K alone (conv_splits): chains of at most SPLIT_CHAIN products, the partial sums added
in split order. The count depends on the layer only, so the invariance above holds.
"""
from __future__ import annotations

import os
import warnings
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops, tower

SIZE = 299
FEATURES = 2048
BN_EPS = 1e-3
POOL_MAX, POOL_AVG = 0, 1
SPLIT_MIN_K, SPLIT_CHAIN = 1024, 512


def conv_splits(k: int) -> int:
    """Split-K count of a conv with k = kh * kw * cin products per output: a function of the layer alone. 1 up to
    SPLIT_MIN_K products, else the fewest splits whose chains hold at most SPLIT_CHAIN."""
    return 1 if k <= SPLIT_MIN_K else -(-k // SPLIT_CHAIN)


# ---------------------------------------------------------------- the layer table
def _pair(v) -> Tuple[int, int]:
    return (v, v) if isinstance(v, int) else (int(v[0]), int(v[1]))


def _c(name: str, cout: int, k=1, stride: int = 1, pad=0):
    """("conv", name, cout, (kh, kw), stride, (pad_h, pad_w))"""
    return ("conv", name, cout, _pair(k), stride, _pair(pad))


def _p(mode: str, k: int, s: int, p: int):
    return ("pool", mode, k, s, p)


def _fork(a, b):
    """Two convs on one input, concatenated in order (the 1x3 / 3x1 pairs of InceptionE)."""
    return ("fork", a, b)


def _inception_a(pool_features: int):
    return [[_c("branch1x1", 64)],
            [_c("branch5x5_1", 48), _c("branch5x5_2", 64, 5, pad=2)],
            [_c("branch3x3dbl_1", 64), _c("branch3x3dbl_2", 96, 3, pad=1), _c("branch3x3dbl_3", 96, 3, pad=1)],
            [_p("avg", 3, 1, 1), _c("branch_pool", pool_features)]]


def _inception_b():
    return [[_c("branch3x3", 384, 3, stride=2)],
            [_c("branch3x3dbl_1", 64), _c("branch3x3dbl_2", 96, 3, pad=1), _c("branch3x3dbl_3", 96, 3, stride=2)],
            [_p("max", 3, 2, 0)]]


def _inception_c(c7: int):
    return [[_c("branch1x1", 192)],
            [_c("branch7x7_1", c7), _c("branch7x7_2", c7, (1, 7), pad=(0, 3)), _c("branch7x7_3", 192, (7, 1), pad=(3, 0))],
            [_c("branch7x7dbl_1", c7), _c("branch7x7dbl_2", c7, (7, 1), pad=(3, 0)),
             _c("branch7x7dbl_3", c7, (1, 7), pad=(0, 3)), _c("branch7x7dbl_4", c7, (7, 1), pad=(3, 0)),
             _c("branch7x7dbl_5", 192, (1, 7), pad=(0, 3))],
            [_p("avg", 3, 1, 1), _c("branch_pool", 192)]]


def _inception_d():
    return [[_c("branch3x3_1", 192), _c("branch3x3_2", 320, 3, stride=2)],
            [_c("branch7x7x3_1", 192), _c("branch7x7x3_2", 192, (1, 7), pad=(0, 3)),
             _c("branch7x7x3_3", 192, (7, 1), pad=(3, 0)), _c("branch7x7x3_4", 192, 3, stride=2)],
            [_p("max", 3, 2, 0)]]


def _inception_e(pool: str):
    return [[_c("branch1x1", 320)],
            [_c("branch3x3_1", 384),
             _fork(_c("branch3x3_2a", 384, (1, 3), pad=(0, 1)), _c("branch3x3_2b", 384, (3, 1), pad=(1, 0)))],
            [_c("branch3x3dbl_1", 448), _c("branch3x3dbl_2", 384, 3, pad=1),
             _fork(_c("branch3x3dbl_3a", 384, (1, 3), pad=(0, 1)), _c("branch3x3dbl_3b", 384, (3, 1), pad=(1, 0)))],
            [_p(pool, 3, 1, 1), _c("branch_pool", 192)]]


# (name, spec): a conv / pool tuple for the stem, a list of branches for a Mixed block
TABLE = [
    ("Conv2d_1a_3x3", _c("Conv2d_1a_3x3", 32, 3, stride=2)),
    ("Conv2d_2a_3x3", _c("Conv2d_2a_3x3", 32, 3)),
    ("Conv2d_2b_3x3", _c("Conv2d_2b_3x3", 64, 3, pad=1)),
    ("maxpool1", _p("max", 3, 2, 0)),
    ("Conv2d_3b_1x1", _c("Conv2d_3b_1x1", 80)),
    ("Conv2d_4a_3x3", _c("Conv2d_4a_3x3", 192, 3)),
    ("maxpool2", _p("max", 3, 2, 0)),
    ("Mixed_5b", _inception_a(32)), ("Mixed_5c", _inception_a(64)), ("Mixed_5d", _inception_a(64)),
    ("Mixed_6a", _inception_b()),
    ("Mixed_6b", _inception_c(128)), ("Mixed_6c", _inception_c(160)), ("Mixed_6d", _inception_c(160)),
    ("Mixed_6e", _inception_c(192)),
    ("Mixed_7a", _inception_d()),
    ("Mixed_7b", _inception_e("avg")), ("Mixed_7c", _inception_e("max")),
]
BLOCKS = dict(TABLE)


def _out_hw(op, h: int, w: int) -> Tuple[int, int]:
    if op[0] == "conv":
        (kh, kw), s, (ph, pw) = op[3], op[4], op[5]
        return (h + 2 * ph - kh) // s + 1, (w + 2 * pw - kw) // s + 1
    _, _, k, s, p = op
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


def _branch_shape(branch, cin: int, h: int, w: int, prefix: str, convs: Optional[list]) -> Tuple[int, int, int]:
    c = cin
    for op in branch:
        if op[0] == "fork":
            for sub in op[1:]:
                if convs is not None:
                    convs.append((prefix + sub[1], c) + sub[2:])
            c = op[1][2] + op[2][2]  # both keep the size
            continue
        if min(_out_hw(op, h, w)) < 1:
            raise ValueError(f"{prefix}{op[1]}: a {h}x{w} map is too small")
        if op[0] == "conv":
            if convs is not None:
                convs.append((prefix + op[1], c) + op[2:])
            c = op[2]
        h, w = _out_hw(op, h, w)
    return h, w, c


def block_shape(name: str, cin: int, h: int, w: int, convs: Optional[list] = None) -> Tuple[int, int, int]:
    """(h, w, c) of a table entry's output on a cin-channel h x w map; convs (optional) collects
    (state-dict prefix, cin, cout, (kh, kw), stride, (pad_h, pad_w)) of its convs in order."""
    spec = BLOCKS[name]
    if isinstance(spec, tuple):
        return _branch_shape([spec], cin, h, w, "", convs)
    outs = [_branch_shape(b, cin, h, w, name + ".", convs) for b in spec]
    if len({o[:2] for o in outs}) != 1:
        raise ValueError(f"{name}: branch sizes differ on a {h}x{w} map")
    return outs[0][0], outs[0][1], sum(o[2] for o in outs)


def layer_shapes(size: int = SIZE) -> List[Tuple[str, int, int, int]]:
    """(name, h, w, c) after every table entry for a size x size input, then ("avgpool", 1, 1, 2048)."""
    h, w, c, out = size, size, 3, []
    for name, _ in TABLE:
        h, w, c = block_shape(name, c, h, w)
        out.append((name, h, w, c))
    out.append(("avgpool", 1, 1, c))
    return out


def conv_layers() -> List[tuple]:
    """(state-dict prefix, cin, cout, (kh, kw), stride, (pad_h, pad_w)) of the 94 convs in forward order."""
    convs: list = []
    h, w, c = SIZE, SIZE, 3
    for name, _ in TABLE:
        h, w, c = block_shape(name, c, h, w, convs)
    return convs


def image_bytes() -> int:
    """fp32 bytes of the largest activation tensor of one 299 x 299 image (channels stored in fours)."""
    return max(4 * h * w * ((c + 3) // 4 * 4) for _, h, w, c in [("prep", SIZE, SIZE, 3)] + layer_shapes())


# images per tower launch: a function of the constant 299 alone (and under the global pool's 65535)
CHUNK = min(32768, (tower.MAX_TENSOR_BYTES - 1) // image_bytes())


# ---------------------------------------------------------------- weights
def fold_bn(weight, gamma, beta, mean, var, eps: float = BN_EPS) -> Tuple[torch.Tensor, torch.Tensor]:
    """(weight', bias') float64 with BatchNorm(conv(x, weight)) == conv(x, weight') + bias' (inference mode)."""
    w, g, b, m, v = (torch.as_tensor(t).detach().to("cpu", torch.float64) for t in (weight, gamma, beta, mean, var))
    scale = g / torch.sqrt(v + eps)
    return w * scale[:, None, None, None], b - m * scale


def load_inception(src: Union[str, Dict]) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """{prefix: (weight [cout, cin, kh, kw], bias [cout])} fp32 CPU tensors with the BatchNorms folded in (in
    float64), from the torchvision-named state dict (<prefix>.conv.weight, <prefix>.bn.weight / .bias /
    .running_mean / .running_var); fc.* and AuxLogits.* are ignored. A path (.pt / .pth / .npz) or a dict."""
    sd = tower.load_state(src, "Inception")
    out = {}
    for prefix, cin, cout, (kh, kw), _, _ in conv_layers():
        want = {"conv.weight": (cout, cin, kh, kw), "bn.weight": (cout,), "bn.bias": (cout,),
                "bn.running_mean": (cout,), "bn.running_var": (cout,)}
        t = {}
        for key, shape in want.items():
            name = f"{prefix}.{key}"
            if name not in sd:
                raise ValueError(f"Inception weights: no '{name}' found; expected the torchvision names "
                                 f"Conv2d_1a_3x3.conv.weight ... Mixed_7c.branch_pool.bn.running_var, got "
                                 f"{sorted(sd)[:4]}{' ...' if len(sd) > 4 else ''}")
            t[key] = torch.as_tensor(sd[name])
            if tuple(t[key].shape) != shape:
                raise ValueError(f"Inception weights: '{name}' has shape {tuple(t[key].shape)}, expected {shape}")
        w, b = fold_bn(t["conv.weight"], t["bn.weight"], t["bn.bias"], t["bn.running_mean"], t["bn.running_var"])
        out[prefix] = (w.to(torch.float32), b.to(torch.float32))
    return out


def seeded_inception(seed: int = 0) -> Dict[str, torch.Tensor]:
    """A stand-in state dict for tests and benchmarks (no trained weights ship): He-scaled conv weights
    N(0, 2 / fan_in), BatchNorm gamma 1 +- 0.05, beta 0.05 +- 0.05, running mean 0 +- 0.05, running var 1 +- 0.05
    (uniform), so activations neither die nor blow up through the 94 convs."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for prefix, cin, cout, (kh, kw), _, _ in conv_layers():
        std = (2.0 / (cin * kh * kw)) ** 0.5
        sd[f"{prefix}.conv.weight"] = torch.randn((cout, cin, kh, kw), generator=g) * std
        u = lambda: torch.rand(cout, generator=g) * 0.1 - 0.05  # noqa: E731
        sd[f"{prefix}.bn.weight"] = 1.0 + u()
        sd[f"{prefix}.bn.bias"] = 0.05 + u()
        sd[f"{prefix}.bn.running_mean"] = u()
        sd[f"{prefix}.bn.running_var"] = 1.0 + u()
    return sd


# ---------------------------------------------------------------- kernels
def prep(img_u8: torch.Tensor, size: Union[int, Tuple[int, int]] = SIZE) -> torch.Tensor:
    """uint8 [n, h, w, 3] -> fp32 [n, oh, ow, 4]: bilinear resize of v / 255 (align_corners=False, no antialias),
    then 2 v - 1; a zero fourth channel."""
    if img_u8.dim() != 4 or img_u8.shape[3] != 3 or img_u8.dtype != torch.uint8 or img_u8.numel() == 0:
        raise ValueError("prep: non-empty uint8 [n, h, w, 3] images expected")
    n, h, w, _ = img_u8.shape
    oh, ow = _pair(size)
    out = torch.empty((n, oh, ow, 4), dtype=torch.float32, device=img_u8.device)
    ops.call("rdeic_fid_prep", img_u8.contiguous().data_ptr(), n, h, w, oh, ow, out.data_ptr(), ops.stream_ptr())
    return out


def pool2d(x: torch.Tensor, k: int, s: int, p: int, mode: str, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Max (padding counts as -inf) or average (count_include_pad=False) pool of an fp32 NHWC activation,
    floor mode."""
    n, h, w, c = x.shape
    if x.dtype != torch.float32 or min(n, h, w, c) < 1 or mode not in ("max", "avg"):
        raise ValueError(f"pool2d: non-empty fp32 [n, h, w, c] and mode max / avg expected, got {tuple(x.shape)} "
                         f"{x.dtype} {mode}")
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    if out is None:
        out = torch.empty((n, ho, wo, c), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (n, ho, wo, c) or out.dtype != torch.float32:
        raise ValueError(f"pool2d: out must be fp32 {(n, ho, wo, c)}")
    ops.call("rdeic_pool2d", x.data_ptr(), n, h, w, c, ops.pix_ld(x), k, s, p, POOL_MAX if mode == "max" else POOL_AVG,
             out.data_ptr(), ops.pix_ld(out), ops.stream_ptr())
    return out


def global_avgpool(x: torch.Tensor) -> torch.Tensor:
    """fp32 [n, h, w, c] -> [n, c]: the mean over the pixels, a fixed-order fp64 sum rounded once."""
    n, h, w, c = x.shape
    if x.dtype != torch.float32 or min(n, h, w, c) < 1:
        raise ValueError(f"global_avgpool: non-empty fp32 [n, h, w, c] expected, got {tuple(x.shape)} {x.dtype}")
    out = torch.empty((n, c), dtype=torch.float32, device=x.device)
    for i0 in range(0, n, 65535):
        xs = x[i0:i0 + 65535]
        ops.call("rdeic_global_avgpool", xs.data_ptr(), ops.pix_ld(x), xs.shape[0], h * w, c, out[i0:].data_ptr(),
                 ops.stream_ptr())
    return out


def feat_moments(x: torch.Tensor, total: torch.Tensor, outer: torch.Tensor, accumulate: bool = False) -> None:
    """total[c] and outer[c, c] (fp64, contiguous) (+)= sum_k x_k and sum_k x_k x_k^T of fp32 [rows, c] features."""
    if x.dim() != 2 or x.dtype != torch.float32 or x.shape[0] < 1 or x.stride(1) != 1:
        raise ValueError("feat_moments: non-empty fp32 [rows, c] features with contiguous channels expected")
    rows, c = x.shape
    for t, shape in ((total, (c,)), (outer, (c, c))):
        if t.dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != x.device:
            raise ValueError(f"feat_moments: contiguous fp64 {shape} accumulators on the features' device expected")
    ld = x.stride(0) if rows > 1 else c
    ops.call("rdeic_feat_moments", x.data_ptr(), rows, c, ld, int(accumulate), total.data_ptr(), outer.data_ptr(),
             ops.stream_ptr())


# ---------------------------------------------------------------- the tower
class InceptionV3:
    """InceptionV3(weights).features(img_u8): uint8 [n, h, w, 3] device tensor -> fp32 [n, 2048]."""

    def __init__(self, weights=None, device="cuda"):
        if weights is None:
            raise ValueError("the FID tower needs the InceptionV3 state dict; no weights ship with the project")
        self.device = torch.device(device)
        self.convs: Dict[str, ops.ConvParams] = {}
        folded = load_inception(weights)
        for i, (prefix, _, _, _, stride, _) in enumerate(conv_layers()):
            w, b = folded[prefix]
            if i == 0:
                w = tower.pad_cin4(w)
            # the paddings differ per axis: every call passes pad_t / pad_l / out_hw itself
            self.convs[prefix] = ops.ConvParams.pack(w, b, stride=stride, dtype=torch.float32)

    def _conv(self, x: torch.Tensor, op, prefix: str, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        _, name, _, _, _, (ph, pw) = op
        p = self.convs[prefix + name]
        _, h, w, _ = x.shape
        return ops.conv2d(x, p, pad_t=ph, pad_l=pw, out_hw=_out_hw(op, h, w), act=ops.LEAKY, slope=0.0, out=out,
                          splits=conv_splits(p.kh * p.kw * p.cin))

    def _op(self, x: torch.Tensor, op, prefix: str, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        if op[0] == "conv":
            return self._conv(x, op, prefix, out)
        _, mode, k, s, p = op
        return pool2d(x, k, s, p, mode, out=out)

    def block(self, name: str, x: torch.Tensor) -> torch.Tensor:
        """One table entry on an fp32 NHWC activation (the caller pins split-K, as features does)."""
        spec = BLOCKS[name]
        if isinstance(spec, tuple):
            return self._op(x, spec, "")
        n, h, w, cin = x.shape
        ho, wo, cout = block_shape(name, cin, h, w)
        cat = torch.empty((n, ho, wo, cout), dtype=torch.float32, device=x.device)
        prefix, c0 = name + ".", 0
        for branch in spec:
            y = x
            for i, op in enumerate(branch):
                last = i == len(branch) - 1
                if op[0] == "fork":  # (only ever last) both halves straight into the concat buffer
                    for sub in op[1:]:
                        self._conv(y, sub, prefix, out=cat[..., c0:c0 + sub[2]])
                        c0 += sub[2]
                elif last:
                    c = op[2] if op[0] == "conv" else y.shape[3]
                    self._op(y, op, prefix, out=cat[..., c0:c0 + c])
                    c0 += c
                else:
                    y = self._op(y, op, prefix)
        return cat

    def _tower(self, img_u8: torch.Tensor) -> torch.Tensor:
        x = prep(img_u8, SIZE)
        with ops.splitk_as((False, False)):  # the library's rule looks at the launch; conv_splits at the layer
            for name, _ in TABLE:
                x = self.block(name, x)
        return global_avgpool(x)

    def features(self, img_u8: torch.Tensor, chunk: Optional[int] = None) -> torch.Tensor:
        """chunk: images per tower launch (default CHUNK); it never changes a feature."""
        if img_u8.dim() != 4 or img_u8.shape[3] != 3 or img_u8.dtype != torch.uint8:
            raise ValueError("expected uint8 [N, H, W, 3] images")
        n = img_u8.shape[0]
        step = max(1, min(CHUNK, int(chunk) if chunk else CHUNK))
        out = torch.empty((n, FEATURES), dtype=torch.float32, device=img_u8.device)
        for s0 in range(0, n, step):
            out[s0:s0 + step] = self._tower(img_u8[s0:s0 + step])
        return out


# ---------------------------------------------------------------- set statistics and scores
class FeatureStats:
    """Running fp64 sum and sum of outer products of a feature set on the device; memory is constant in the
    number of samples."""

    def __init__(self, c: int = FEATURES, device="cuda"):
        self.c, self.n = int(c), 0
        self.total = torch.zeros(self.c, dtype=torch.float64, device=device)
        self.outer = torch.zeros((self.c, self.c), dtype=torch.float64, device=device)

    def update(self, feats: torch.Tensor) -> None:
        if feats.dim() != 2 or feats.shape[1] != self.c:
            raise ValueError(f"FeatureStats.update: [rows, {self.c}] features expected, got {tuple(feats.shape)}")
        if feats.shape[0] == 0:
            return
        feat_moments(feats, self.total, self.outer, accumulate=True)
        self.n += int(feats.shape[0])

    def merge(self, other: "FeatureStats") -> None:
        """Adds another accumulator's sums (what a cross-rank reduction would do), in float64 on the host."""
        if other.c != self.c:
            raise ValueError("FeatureStats.merge: feature widths differ")
        for mine, theirs in ((self.total, other.total), (self.outer, other.outer)):
            mine.copy_(torch.from_numpy(mine.cpu().numpy() + theirs.cpu().numpy()))
        self.n += other.n

    def mean(self) -> np.ndarray:
        if self.n < 1:
            raise ValueError("FeatureStats.mean: no samples")
        return self.total.cpu().numpy() / self.n

    def cov(self) -> np.ndarray:
        """The unbiased covariance (outer - n mu mu^T) / (n - 1), float64 on the host."""
        if self.n < 2:
            raise ValueError(f"FeatureStats.cov needs at least 2 samples, has {self.n}")
        mu = self.mean()
        return (self.outer.cpu().numpy() - self.n * np.outer(mu, mu)) / (self.n - 1)


def _psd_sqrt(s: np.ndarray) -> np.ndarray:
    lam, v = np.linalg.eigh((s + s.T) * 0.5)
    return (v * np.sqrt(np.maximum(lam, 0.0))) @ v.T


def fid_from_moments(mu1, s1, mu2, s2) -> float:
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 sum_i sqrt(max(lambda_i, 0)), lambda the eigenvalues of
    S1^(1/2) S2 S1^(1/2) (symmetric PSD, so defined for singular covariances): two eigh calls, float64."""
    mu1, mu2 = np.asarray(mu1, np.float64), np.asarray(mu2, np.float64)
    s1, s2 = np.asarray(s1, np.float64), np.asarray(s2, np.float64)
    r = _psd_sqrt(s1)
    m = r @ s2 @ r
    lam = np.linalg.eigvalsh((m + m.T) * 0.5)
    d = mu1 - mu2
    return float(d @ d + np.trace(s1) + np.trace(s2) - 2.0 * np.sqrt(np.maximum(lam, 0.0)).sum())


def fid(stats_a: FeatureStats, stats_b: FeatureStats) -> float:
    for s in (stats_a, stats_b):
        if s.n < 2:
            raise ValueError(f"fid needs at least 2 samples on each side, got {stats_a.n} and {stats_b.n}")
    return fid_from_moments(stats_a.mean(), stats_a.cov(), stats_b.mean(), stats_b.cov())


def _host(f) -> np.ndarray:
    if isinstance(f, (list, tuple)):
        f = np.concatenate([_host(t) for t in f]) if len(f) else np.zeros((0, 0))
    elif isinstance(f, torch.Tensor):
        f = f.detach().cpu().numpy()
    return np.asarray(f, np.float64)


def kid(feats_a, feats_b, subsets: int = 100, subset_size: int = 1000, seed: int = 0) -> Tuple[float, float]:
    """(mean, std) over `subsets` subsets of the unbiased MMD^2 with the polynomial kernel (x.y / d + 1)^3, float64
    on the host. Each subset draws subset_size samples of each set without replacement from
    np.random.RandomState(seed) (set a first, then set b); subset_size is clamped to the smaller set."""
    a, b = _host(feats_a), _host(feats_b)
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1]:
        raise ValueError("kid: two [rows, d] feature sets of one width expected")
    m, d = int(subset_size), a.shape[1]
    if m > min(len(a), len(b)):
        m = min(len(a), len(b))
        warnings.warn(f"kid: subset_size {subset_size} clamped to the smaller set ({m})")
    if m < 2 or subsets < 1:
        raise ValueError("kid needs at least 2 samples on each side and at least 1 subset")
    rs = np.random.RandomState(seed)
    vals = np.empty(subsets)
    for i in range(subsets):
        x = a[rs.choice(len(a), m, replace=False)]
        y = b[rs.choice(len(b), m, replace=False)]
        kxx, kyy, kxy = (x @ x.T / d + 1.0) ** 3, (y @ y.T / d + 1.0) ** 3, (x @ y.T / d + 1.0) ** 3
        vals[i] = ((kxx.sum() - np.trace(kxx)) + (kyy.sum() - np.trace(kyy))) / (m * (m - 1.0)) \
            - 2.0 * kxy.sum() / (m * float(m))
    return float(vals.mean()), float(vals.std())


# ---------------------------------------------------------------- the patch protocol and the running pair
def patches(img_u8: torch.Tensor, size: int = 256) -> torch.Tensor:
    """The patch protocol of the generative-codec papers: the non-overlapping size x size tiles from the top-left
    plus the same grid shifted by size / 2 in both axes; partial tiles are dropped. uint8 [n, h, w, 3] (or
    [h, w, 3]) -> [k, size, size, 3]; size 0 passes whole images. Slicing only."""
    if img_u8.dim() == 3:
        img_u8 = img_u8[None]
    if img_u8.dim() != 4 or img_u8.shape[3] != 3:
        raise ValueError("patches: [n, h, w, 3] images expected")
    if size == 0:
        return img_u8
    if size < 0 or size % 2:
        raise ValueError("patches: size must be 0 or a positive even number")
    n, h, w, _ = img_u8.shape
    tiles = []
    for off in (0, size // 2):
        for y in range(off, h - size + 1, size):
            for x in range(off, w - size + 1, size):
                tiles.append(img_u8[:, y:y + size, x:x + size])
    if not tiles:
        return img_u8.new_empty((0, size, size, 3))
    return torch.stack(tiles, 1).reshape(-1, size, size, 3)  # image-major, the grids in order


class FidKid:
    """The running state of one FID / KID evaluation: every (reconstruction, original) pair goes through patches ->
    features -> two FeatureStats (FID) and two host feature lists (KID, 8 KB per sample)."""

    def __init__(self, tower: InceptionV3, patch: int = 256, batch: int = 64):
        self.tower, self.patch, self.batch = tower, int(patch), int(batch)
        self.stats = (FeatureStats(FEATURES, tower.device), FeatureStats(FEATURES, tower.device))
        self.feats: Tuple[List[np.ndarray], List[np.ndarray]] = ([], [])
        self.n_images = 0

    def add(self, pred_u8: torch.Tensor, target_u8: torch.Tensor) -> None:
        if pred_u8.dim() == 3:
            pred_u8, target_u8 = pred_u8[None], target_u8[None]
        if pred_u8.shape != target_u8.shape:
            raise ValueError("FidKid.add: a reconstruction and its original must share a shape")
        self.n_images += int(pred_u8.shape[0])
        for side, img in enumerate((pred_u8, target_u8)):
            tiles = patches(img.to(self.tower.device), self.patch)
            for s0 in range(0, tiles.shape[0], self.batch):
                f = self.tower.features(tiles[s0:s0 + self.batch])
                self.stats[side].update(f)
                self.feats[side].append(f.cpu().numpy())

    def merge(self, other: "FidKid") -> None:
        """Adds another run's sums and features (the `all` row over per-domain runs)."""
        for side in (0, 1):
            self.stats[side].merge(other.stats[side])
            self.feats[side].extend(other.feats[side])
        self.n_images += other.n_images

    @property
    def n_patches(self) -> int:
        return self.stats[0].n

    def result(self, kid_subsets: int = 100, kid_subset_size: int = 1000, seed: int = 0) -> Dict[str, float]:
        k_mean, k_std = kid(list(self.feats[0]), list(self.feats[1]), kid_subsets, kid_subset_size, seed)
        return {"n_images": self.n_images, "n_patches": self.n_patches, "fid": fid(self.stats[0], self.stats[1]),
                "kid_mean": k_mean, "kid_std": k_std}


CSV_COLUMNS = ["set", "n_images", "n_patches", "fid", "kid_mean", "kid_std"]


def write_csv(rows: Sequence[Dict], path: str) -> None:
    """fid_kid.csv: one row per set, columns CSV_COLUMNS."""
    import csv
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=CSV_COLUMNS)
        w.writeheader()
        for r in rows:
            w.writerow({k: r[k] for k in CSV_COLUMNS})


def add_cli_flags(p) -> None:
    """--fid_inception / --fid_patch / --kid_subset_size on an argparse parser (inference_partition.py, run_ood.py)."""
    p.add_argument("--fid_inception", type=str, default="",
                   help="InceptionV3 state dict, torchvision names (.pt / .pth / .npz): FID and KID between the "
                        "reconstructions and the originals, written to fid_kid.csv. Empty = not computed")
    p.add_argument("--fid_patch", type=int, default=None,
                   help="patch size of the FID / KID patch protocol (default 256; 0 = whole images)")
    p.add_argument("--kid_subset_size", type=int, default=None, help="KID subset size (default 1000)")


def check_cli_flags(p, args) -> None:
    """Refused at start-up, before any model loads: the patch / subset flags without --fid_inception, a path that
    is not a file, sizes out of range. Fills the defaults."""
    if not args.fid_inception:
        for flag in ("fid_patch", "kid_subset_size"):
            if getattr(args, flag) is not None:
                p.error(f"--{flag} needs --fid_inception")
    elif not os.path.isfile(args.fid_inception):
        p.error(f"--fid_inception {args.fid_inception} is not a file")
    args.fid_patch = 256 if args.fid_patch is None else args.fid_patch
    args.kid_subset_size = 1000 if args.kid_subset_size is None else args.kid_subset_size
    if args.fid_patch < 0 or args.fid_patch % 2 or args.kid_subset_size < 2:
        p.error("--fid_patch must be 0 or a positive even number and --kid_subset_size at least 2")


def summary_line(r: Dict) -> str:
    return f"FID {r['fid']:.4f} KID {r['kid_mean']:.6f} ± {r['kid_std']:.6f} ({r['n_patches']} patches)"


def fid_kid(pred_u8_batches: Iterable[torch.Tensor], target_u8_batches: Iterable[torch.Tensor], tower: InceptionV3,
            patch: int = 256, kid_subsets: int = 100, kid_subset_size: int = 1000, seed: int = 0) -> Dict[str, float]:
    """FID and KID between reconstructions and originals given as matching iterables of uint8 [n, h, w, 3] batches."""
    run = FidKid(tower, patch)
    for p, t in zip(pred_u8_batches, target_u8_batches):
        run.add(p, t)
    return run.result(kid_subsets, kid_subset_size, seed)
