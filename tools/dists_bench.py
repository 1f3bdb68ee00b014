"""Time the DISTS metric (rdeic_amd/dists.py) on the device: the whole call, its split between the fp32 backbone
convs, the prep, the four L2 pools and the six moment reductions with their finalizes, each dists.hip kernel's
achieved bytes/s (the bytes the algorithm needs, from shapes, over the event-timed launch), and LPIPS("vgg") on
the same pairs in the same process as the yardstick for the shared backbone. Seeded backbone, seeded weights,
synthetic images.

    python tools/dists_bench.py [--pairs 16] [--size 512] [--reps 20] [--out profiles/FILE.jsonl]
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


def wall(fn, reps):
    """(median, min) milliseconds of fn() on the host clock; fn ends in a device-to-host copy."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dists_bench needs the GPU")
    from rdeic_amd import dists as D, lpips as L, ops
    from rdeic_amd.synthetic import synth_image
    backbone = L.seeded_backbone("vgg")
    m = D.DISTS(D.seeded_weights(), backbone=backbone)
    g = torch.Generator().manual_seed(1)
    lp = L.LPIPS("vgg", backbone=backbone,
                 lin={f"lin{k}": torch.rand(c, generator=g) * 0.1 for k, c in enumerate(L.CHANNELS["vgg"])})
    n, s = a.pairs, a.size
    tgt = np.stack([synth_image(s, s, 100 + i) for i in range(n)])
    rng = np.random.default_rng(0)
    pred = np.clip(tgt + rng.normal(0, 12.0, tgt.shape), 0, 255).astype(np.uint8)
    p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(tgt).cuda()

    # the whole calls, host clock around work that ends in a device-to-host copy
    d_ms, d_min = wall(lambda: m(p, t), a.reps)
    l_ms, l_min = wall(lambda: lp(p, t), a.reps)
    head = {"pairs": n, "size": s, "chunk_pairs": D.chunk_pairs(s, s), "dists_call_ms": d_ms,
            "dists_call_ms_min": d_min, "lpips_vgg_call_ms": l_ms, "lpips_vgg_call_ms_min": l_min,
            "dists_over_lpips_vgg": d_ms / l_ms}
    lines = []

    # launch by launch, on one chunk-sized batch as __call__ runs it
    cp = min(n, D.chunk_pairs(s, s))
    both = torch.cat([p[:cp], t[:cp]])
    nb = both.shape[0]
    groups = {"prep": 0.0, "conv": 0.0, "l2pool": 0.0, "moments": 0.0, "score": 0.0}

    def add(kind, name, ms, nbytes, flops=0.0):
        groups[kind] += ms
        rec = {"kind": kind, "name": name, "ms": ms, "bytes": nbytes, "TBps": nbytes / (ms * 1e-3) / 1e12,
               "of_hbm": nbytes / (ms * 1e-3) / HBM_ACHIEVABLE}
        if flops:
            rec["TFLOPs"] = flops / (ms * 1e-3) / 1e12
        lines.append(rec)

    def add_tap(k, f):
        f0, f1 = f[:cp], f[cp:]
        mom = D.moments(f0, f1)
        out = torch.empty(cp, dtype=torch.float64, device="cuda")
        # two passes over both maps; the fp64 partials are 5 / (8 * rows per block) of that and are left out
        add("moments", f"moments{k} {tuple(f0.shape)} (2 passes + 2 finalizes)",
            timed(lambda: D.moments(f0, f1), a.reps), 4 * 2 * 2 * f0.numel())
        add("score", f"score{k} [{cp}, 5, {f0.shape[3]}]",
            timed(lambda: D.tap_score(mom, m.alpha[k], m.beta[k], out=out), a.reps),
            8 * (mom.numel() + 2 * f0.shape[3]))

    raw, x = D.prep(both)
    add("prep", f"prep {nb}x{s}x{s}", timed(lambda: D.prep(both), a.reps), nb * s * s * (3 + 32))
    add_tap(0, raw)
    ci, k = 0, 1
    with ops.splitk_as((False, False)):
        for op in L.NETS["vgg"]:
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
                y = D.l2_pool(xin)
                add("l2pool", f"l2pool {tuple(xin.shape)}", timed(lambda: D.l2_pool(xin), a.reps),
                    4 * (xin.numel() + y.numel()))
                x = y
            else:
                add_tap(k, x)
                k += 1
    head["chunk_images"] = nb
    head["chunk_ms"] = dict(groups)
    head["chunk_ms"]["sum"] = sum(groups.values())
    for r in lines:
        extra = f"  {r['TFLOPs']:.1f} TF" if "TFLOPs" in r else ""
        print(f"{r['kind']:7s} {r['name']:62s} {r['ms']:8.4f} ms  {r['TBps']:.3f} TB/s ({100 * r['of_hbm']:.0f}% of "
              f"achievable HBM){extra}")
    print(json.dumps(head))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(head) + "\n")
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
