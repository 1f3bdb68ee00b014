"""Time the LPIPS metric (rdeic_amd/lpips.py) on the device: the whole call, and its split between the fp32
backbone convs and the three lpips.hip kernels, with each kernel's achieved bytes/s (the bytes the algorithm
needs, from shapes, over the event-timed launch). Seeded random backbone, random heads, synthetic images.

    python tools/lpips_bench.py [--net alex] [--pairs 16] [--size 512] [--reps 20] [--out FILE.json]
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


def seeded_backbone(net, seed=0):
    from rdeic_amd import lpips as L
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, _, cin, cout, k, _, _ in L.conv_layers(net):
        sd[f"features.{i}.weight"] = torch.randn((cout, cin, k, k), generator=g) * (2.0 / (cin * k * k)) ** 0.5
        sd[f"features.{i}.bias"] = torch.randn((cout,), generator=g) * 0.05
    return sd


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


def main():
    ap = argparse.ArgumentParser()
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
    m = L.LPIPS(a.net, backbone=seeded_backbone(a.net), lin=lin)
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
