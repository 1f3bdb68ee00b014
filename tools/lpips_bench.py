"""Time the LPIPS metric (rdeic_amd/lpips.py) on the device: the whole call, and its split between the fp32
backbone convs and the three lpips.hip kernels, with each kernel's achieved bytes/s (the bytes the algorithm
needs, from shapes, over the event-timed launch). Seeded random backbone, random heads, synthetic images.

    python tools/lpips_bench.py [--net alex] [--pairs 16] [--size 512] [--reps 20] [--out FILE.json]
    python tools/lpips_bench.py --loss [--pairs 1] ...   the training loss LPIPS.loss, forward + backward
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12  # bytes/s, float4 copy on this part


def timed(fn, reps):
    """Median milliseconds of fn() by device events, after 3 warm-up calls."""
    for _ in range(3):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def bench_loss(a, m):
    """LPIPS.loss forward + backward on float images: the whole call (host clock, synchronised), the peak of
    device memory over it, and the backward's own kernels by device events."""
    from rdeic_amd import lpips as L
    from rdeic_amd.synthetic import synth_image
    n, s = a.pairs, a.size
    tgt = torch.from_numpy(np.stack([synth_image(s, s, 100 + i) for i in range(n)])).float() / 127.5 - 1.0
    g = torch.Generator().manual_seed(0)
    pred = (tgt + torch.randn(tgt.shape, generator=g) * (12.0 / 127.5)).clamp(-1, 1)
    p, t = pred.cuda().requires_grad_(True), tgt.cuda()

    def step():
        p.grad = None
        m.loss(p, t).backward()

    def fwd():
        with torch.no_grad():
            m.loss(p, t)

    def wall(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms), min(ms)

    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step_ms, step_min = wall(step)
    peak = torch.cuda.max_memory_allocated() - base
    fwd_ms, _ = wall(fwd)
    res = {"mode": "loss", "net": a.net, "pairs": n, "size": s, "fwd_bwd_ms": step_ms, "fwd_bwd_ms_min": step_min,
           "fwd_ms": fwd_ms, "peak_bytes_over_inputs": peak, "ops": []}

    def add(name, ms, nbytes):
        res["ops"].append({"name": name, "ms": ms, "bytes": nbytes, "TBps": nbytes / (ms * 1e-3) / 1e12})

    acts, taps = m.forward_acts(L.prep_float(p.detach()))
    f1 = m.features_float(t)
    gs = torch.full((n,), 1.0 / n, device="cuda")
    add(f"prep_float {n}x{s}x{s}", timed(lambda: L.prep_float(t), a.reps), n * s * s * (12 + 16))
    for k, i in enumerate(taps):
        f0, lv, fb = acts[i], m.lin[k], f1[k]
        add(f"layer_bwd{k} {tuple(f0.shape)}", timed(lambda: L.layer_distance_bwd(f0, fb, lv, gs), a.reps),
            4 * 3 * f0.numel())
    i = 0
    for op in m.table:
        if op[0] == "pool":
            xin = acts[i]
            dy = torch.randn_like(acts[i + 1])
            add(f"pool_bwd{op[1]}/{op[2]} {tuple(xin.shape)}", timed(lambda: L.max_pool_bwd(xin, dy, op[1], op[2]), a.reps),
                4 * (2 * xin.numel() + dy.numel()))
        i += op[0] != "tap"
    w0, _ = m._bwd_weights()
    _, _, _, ks, st, pd = m.table[0]
    dz, dx = torch.randn_like(acts[1]), torch.empty((n, s, s, 3), device="cuda")
    add(f"conv1 dgrad (gather, k{ks}/{st}) {tuple(dz.shape)}",
        timed(lambda: L.conv_dgrad_small(dz, acts[1], w0, (s, s), 4, ks, st, pd, prep_bwd=True, out=dx), a.reps),
        4 * (2 * dz.numel() + dx.numel()))
    for r in res["ops"]:
        print(f"{r['name']:64s} {r['ms']:8.4f} ms  {r['TBps']:.3f} TB/s")
    print(json.dumps({k_: v for k_, v in res.items() if k_ != "ops"}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loss", action="store_true", help="time LPIPS.loss forward + backward instead of the metric")
    ap.add_argument("--net", default="alex", choices=["alex", "vgg"])
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lpips_bench needs the GPU")
    from rdeic_amd import lpips as L, ops
    from rdeic_amd.synthetic import synth_image
    g = torch.Generator().manual_seed(1)
    lin = {f"lin{k}": torch.rand(c, generator=g) * 0.1 for k, c in enumerate(L.CHANNELS[a.net])}
    m = L.LPIPS(a.net, backbone=L.seeded_backbone(a.net), lin=lin)
    if a.loss:
        return bench_loss(a, m)
    n, s = a.pairs, a.size
    tgt = np.stack([synth_image(s, s, 100 + i) for i in range(n)])
    rng = np.random.default_rng(0)
    pred = np.clip(tgt + rng.normal(0, 12.0, tgt.shape), 0, 255).astype(np.uint8)
    p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(tgt).cuda()

    # the whole call, host clock around work that ends in a device-to-host copy
    for _ in range(3):
        m(p, t)
    torch.cuda.synchronize()
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        m(p, t)
        wall.append((time.perf_counter() - t0) * 1e3)
    res = {"net": a.net, "pairs": n, "size": s, "chunk_pairs": L.chunk_pairs(a.net, s, s),
           "call_ms": statistics.median(wall), "call_ms_min": min(wall), "ops": []}

    # launch by launch, on one chunk-sized batch as __call__ runs it
    cp = min(n, L.chunk_pairs(a.net, s, s))
    both = torch.cat([p[:cp], t[:cp]])
    nb = both.shape[0]
    groups = {"prep": 0.0, "conv": 0.0, "pool": 0.0, "layer": 0.0}

    def add(kind, name, ms, nbytes, flops=0.0):
        groups[kind] += ms
        rec = {"kind": kind, "name": name, "ms": ms, "bytes": nbytes, "TBps": nbytes / (ms * 1e-3) / 1e12,
               "of_hbm": nbytes / (ms * 1e-3) / HBM_ACHIEVABLE}
        if flops:
            rec["TFLOPs"] = flops / (ms * 1e-3) / 1e12
        res["ops"].append(rec)

    x = m.prep(both)
    add("prep", f"prep {nb}x{s}x{s}", timed(lambda: m.prep(both), a.reps), nb * s * s * (3 + 16))
    ci, k = 0, 0
    with ops.splitk_as((False, False)):
        for op in m.table:
            if op[0] == "conv":
                cv, xin = m.convs[ci], x
                y = ops.conv2d(xin, cv, act=ops.LEAKY, slope=0.0)
                fl = 2.0 * y.numel() * cv.kh * cv.kw * cv.cin
                add("conv", f"conv{ci} {tuple(xin.shape)}->{tuple(y.shape)} k{cv.kh}",
                    timed(lambda: ops.conv2d(xin, cv, act=ops.LEAKY, slope=0.0), a.reps),
                    4 * (xin.numel() + y.numel() + cv.weight.numel()), fl)
                x, ci = y, ci + 1
            elif op[0] == "pool":
                xin = x
                y = L.max_pool(xin, op[1], op[2])
                add("pool", f"pool{op[1]}/{op[2]} {tuple(xin.shape)}",
                    timed(lambda: L.max_pool(xin, op[1], op[2]), a.reps), 4 * (xin.numel() + y.numel()))
                x = y
            else:
                f0, f1, lv = x[:cp], x[cp:], m.lin[k]
                out = torch.empty(cp, dtype=torch.float32, device="cuda")
                add("layer", f"layer{k} {tuple(f0.shape)}",
                    timed(lambda: L.layer_distance(f0, f1, lv, out=out), a.reps), 4 * (2 * f0.numel() + lv.numel()))
                k += 1
    res["chunk_images"] = nb
    res["chunk_ms"] = {kind: v for kind, v in groups.items()}
    res["chunk_ms"]["sum"] = sum(groups.values())
    for r in res["ops"]:
        extra = f"  {r['TFLOPs']:.1f} TF" if "TFLOPs" in r else ""
        print(f"{r['kind']:5s} {r['name']:60s} {r['ms']:8.4f} ms  {r['TBps']:.3f} TB/s ({100 * r['of_hbm']:.0f}% of "
              f"achievable HBM){extra}")
    print(json.dumps({k_: v for k_, v in res.items() if k_ != "ops"}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
