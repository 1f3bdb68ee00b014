"""Time the no-reference metrics (rdeic_amd/metrics.py niqe / brisque, csrc/nr_metrics.hip) against the same
algorithm written with plain torch ops (conv2d, roll, masked sums) on the same GPU, in one process.

    python tools/nr_metrics_bench.py [--images 16] [--size 512] [--reps 30] [--warmup 5] [--out profiles/nr_metrics.jsonl]

Both forms go from a uint8 [N,H,W,3] device tensor to float64 scores on the host and share the host-side AGGD fits
(the moments are the only thing the device hands over), so the difference is the device work. Per variant one JSON
line: the median / min wall ms of `reps` calls after `warmup` (each call ends with the device-to-host copy of the
moments, i.e. a synchronise), the device-only ms of the moments pass by HIP events, and for the HIP path the achieved
bytes/s of that pass next to its plane traffic as built: per pixel 3 (RGB read) + 4 (Y written) + 8 (MSCN: Y read, M
written) + 5 (half-size: Y read, quarter plane written) + 2 (MSCN of the quarter plane) + 5 (both moment passes; the
shifted neighbours are cache hits) = 27 bytes; a single fused pass would need the 3 bytes of the RGB read alone.
The scores of the two forms are compared (relative difference printed) before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TAPS = [-3.0, -9.0, 29.0, 111.0, 111.0, 29.0, -9.0, -3.0]
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))


def _gauss(dev):
    d = torch.arange(7, dtype=torch.float64) - 3.0
    g = torch.exp(-d * d / (2.0 * (7.0 / 6.0) ** 2))
    return (g / g.sum()).float().to(dev)


def _filter(x, g):
    """Separable 7x7 Gaussian with a replicate border; x [N,1,H,W]."""
    x = F.conv2d(F.pad(x, (3, 3, 0, 0), mode="replicate"), g.view(1, 1, 1, 7))
    return F.conv2d(F.pad(x, (0, 0, 3, 3), mode="replicate"), g.view(1, 1, 7, 1))


def _mscn(y, g):
    mu = _filter(y, g)
    sigma = torch.sqrt(torch.abs(_filter(y * y, g) - mu * mu))
    return (y - mu) / (sigma + 1.0)


def _sym_pad(x, dim):
    lo = x.narrow(dim, 0, 3).flip(dim)
    hi = x.narrow(dim, x.shape[dim] - 4, 4).flip(dim)
    return torch.cat([lo, x, hi], dim=dim)


def _half(y, dev):
    t = torch.tensor(TAPS, dtype=torch.float32, device=dev) / 256.0
    v = F.conv2d(_sym_pad(y, 2), t.view(1, 1, 8, 1), stride=(2, 1))
    return F.conv2d(_sym_pad(v, 3), t.view(1, 1, 1, 8), stride=(1, 2))


def _moments(m, bh, bw):
    """[N, regions, 5, 6] float64 from m [N,1,H,W], regions of bh x bw (row-major)."""
    n, _, h, w = m.shape
    r = m.view(n, h // bh, bh, w // bw, bw).permute(0, 1, 3, 2, 4).reshape(n, -1, bh, bw)
    maps = torch.stack([r] + [r * torch.roll(r, d, dims=(2, 3)) for d in SHIFTS], dim=2)  # [N, R, 5, bh, bw]
    neg, pos, sq = maps < 0, maps > 0, maps * maps
    out = torch.stack([neg.sum((3, 4)).double(), pos.sum((3, 4)).double(), (sq * neg).sum((3, 4)).double(),
                       (sq * pos).sum((3, 4)).double(), maps.abs().sum((3, 4)).double(), sq.sum((3, 4)).double()],
                      dim=-1)
    return out


def torch_moments(x_u8, block):
    dev = x_u8.device
    g = _gauss(dev)
    n, h, w, _ = x_u8.shape
    if block:
        x_u8 = x_u8[:, :h // block * block, :w // block * block]
    v = x_u8.float() / 255.0
    y = torch.round(255.0 * (0.299 * v[..., 0] + 0.587 * v[..., 1] + 0.114 * v[..., 2])).unsqueeze(1)
    y1 = _half(y, dev)
    bh, bw = (block, block) if block else y.shape[2:]
    m0 = _moments(_mscn(y, g), bh, bw)
    m1 = _moments(_mscn(y1, g), bh // 2, bw // 2)
    return m0.cpu().numpy(), m1.cpu().numpy()


def scores(kind, x_u8, model, moments_fn):
    from rdeic_amd import metrics
    n, h, w, _ = x_u8.shape
    if kind == "niqe":
        m0, m1 = moments_fn(x_u8, 96)
        feat = np.concatenate([metrics.niqe_features(m0, 96 * 96), metrics.niqe_features(m1, 48 * 48)], axis=-1)
        return np.array([metrics.niqe_score(feat[i], model) for i in range(n)])
    m0, m1 = moments_fn(x_u8, 0)
    feat = np.concatenate([metrics.brisque_features(m0[:, 0], h * w),
                           metrics.brisque_features(m1[:, 0], (h // 2) * (w // 2))], axis=-1)
    return model.score(feat)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(wall)), float(np.min(wall))


def device_ms(fn, reps):
    """Median device ms of fn's launches by events (fn ends in a copy to the host, which the stop event precedes only
    in stream order: the events bracket the kernels and that copy)."""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "nr_metrics.jsonl"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("nr_metrics_bench needs a GPU: there is no CPU fallback to time")
    from rdeic_amd import metrics
    rng = np.random.default_rng(0)
    n, s = args.images, args.size
    base = rng.normal(128.0, 45.0, (n, s, s, 3))
    x = torch.from_numpy(np.clip(np.rint(base), 0, 255).astype(np.uint8)).cuda()

    class Niqe:
        a = rng.standard_normal((36, 36))
        mu, cov = rng.standard_normal(36) + 1.0, a @ a.T / 36.0 + np.eye(36)

    class Brisque:
        sv, sv_coef = rng.uniform(-1, 1, (8, 36)), rng.standard_normal(8)
        rho, gamma, scale_min, scale_max = -20.0, 0.05, np.full(36, -0.5), np.full(36, 3.0)
        score = metrics.BRISQUE.score

    models = {"niqe": Niqe, "brisque": Brisque()}
    hip = lambda t, block: metrics.nr_moments(t, block)  # noqa: E731
    lines = []
    for kind in ("niqe", "brisque"):
        block = 96 if kind == "niqe" else 0
        a, b = scores(kind, x, models[kind], hip), scores(kind, x, models[kind], torch_moments)
        rel = float(np.max(np.abs(a - b) / np.abs(b)))
        print(f"{kind}: hip vs torch-op scores, worst relative difference {rel:.3e}", file=sys.stderr)
        hc = s // 96 * 96 if block else s
        traffic = 27.0 * n * hc * hc
        res = {}
        for variant, fn in (("hip", hip), ("torch_ops", torch_moments)):
            med, best = timed(lambda: scores(kind, x, models[kind], fn), args.reps, args.warmup)
            dev = device_ms(lambda: fn(x, block), args.reps)
            res[variant] = med
            line = {"tool": "nr_metrics_bench", "metric": kind, "variant": variant, "images": n, "size": s,
                    "reps": args.reps, "warmup": args.warmup, "wall_ms_median": round(med, 4),
                    "wall_ms_min": round(best, 4), "moments_device_ms_median": round(dev, 4),
                    "score_rel_diff_vs_other": rel, "device": torch.cuda.get_device_name(0)}
            if variant == "hip":
                line.update(plane_traffic_bytes=traffic, fused_minimum_bytes=3.0 * n * hc * hc,
                            achieved_bytes_per_s=traffic / (dev * 1e-3))
            lines.append(line)
        for line in lines[-2:]:
            line["torch_ops_over_hip_wall"] = round(res["torch_ops"] / res["hip"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
