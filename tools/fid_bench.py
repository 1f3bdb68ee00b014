"""Time the FID / KID feature tower (rdeic_amd/fid.py) on the device: milliseconds per 299 x 299 image at batch
1 / 16 / 128 (uint8 in, [n, 2048] features out; prep, the 94 fp32 convs, the pools and the global pool), the
fid.hip kernels on their largest tower shapes at batch 16, and rdeic_feat_moments on [128, 2048] features. Seeded
weights, synthetic images. The run is one GPU step: give it a time limit of its own,

    timeout -k 10 600 python tools/fid_bench.py [--batches 1,16,128] [--reps 10] [--out profiles/FILE.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, reps):
    """Median milliseconds of fn() by device events, after 2 warm-up calls."""
    for _ in range(2):
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


def tower_flops(F):
    """MACs x 2 of the 94 convs for one 299 x 299 image, from the layer table."""
    total = 0.0
    h, w, c = F.SIZE, F.SIZE, 3
    for name, spec in F.TABLE:
        branches = [[spec]] if isinstance(spec, tuple) else spec
        for b in branches:
            bh, bw, bc = h, w, c
            for op in b:
                subs = op[1:] if op[0] == "fork" else [op]
                width = 0
                for sub in subs:
                    oh, ow = F._out_hw(sub, bh, bw)
                    if sub[0] == "conv":
                        total += 2.0 * oh * ow * sub[2] * sub[3][0] * sub[3][1] * bc
                        width += sub[2]
                bh, bw = F._out_hw(subs[0], bh, bw)
                bc = width or bc
        h, w, c = F.block_shape(name, c, h, w)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,128")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fid_bench needs the GPU")
    from rdeic_amd import _lib, fid as F
    from rdeic_amd.synthetic import synth_image
    tower = F.InceptionV3(F.seeded_inception(0))
    flops = tower_flops(F)
    lines = []
    for n in [int(v) for v in a.batches.split(",") if v]:
        img = torch.from_numpy(np.stack([synth_image(299, 299, 300 + i) for i in range(n)])).cuda()
        ms = timed(lambda: tower.features(img), a.reps)
        lines.append({"kind": "tower", "batch": n, "ms": ms, "ms_per_image": ms / n,
                      "conv_TFLOPs": flops * n / (ms * 1e-3) / 1e12})
        print(f"tower  batch {n:4d}: {ms:9.3f} ms, {ms / n:8.3f} ms / image, {lines[-1]['conv_TFLOPs']:.2f} TFLOP/s "
              f"over the convs' {flops / 1e9:.2f} GFLOP / image")
    # the fid.hip kernels on their largest tower shapes (the rest of a tower pass is the 94 convs)
    n = 16
    x = torch.rand((n, 147, 147, 64), device="cuda")
    lines.append({"kind": "pool", "name": f"max 3/2/0 {tuple(x.shape)}", "ms": timed(lambda: F.pool2d(x, 3, 2, 0, "max"), a.reps)})
    y = torch.rand((n, 35, 35, 288), device="cuda")
    lines.append({"kind": "pool", "name": f"avg 3/1/1 {tuple(y.shape)}", "ms": timed(lambda: F.pool2d(y, 3, 1, 1, "avg"), a.reps)})
    z = torch.rand((n, 8, 8, 2048), device="cuda")
    lines.append({"kind": "gap", "name": f"global avg {tuple(z.shape)}", "ms": timed(lambda: F.global_avgpool(z), a.reps)})
    u8 = torch.randint(0, 256, (n, 256, 256, 3), dtype=torch.uint8, device="cuda")
    lines.append({"kind": "prep", "name": f"prep {tuple(u8.shape)} -> 299", "ms": timed(lambda: F.prep(u8), a.reps)})
    f = torch.rand((128, 2048), device="cuda")
    total = torch.zeros(2048, dtype=torch.float64, device="cuda")
    outer = torch.zeros((2048, 2048), dtype=torch.float64, device="cuda")
    ms = timed(lambda: F.feat_moments(f, total, outer, accumulate=True), a.reps)
    lines.append({"kind": "moments", "name": "feat_moments [128, 2048] accumulate", "ms": ms,
                  "fp64_TFLOPs": 2.0 * 128 * (2048 * 2049 / 2) / (ms * 1e-3) / 1e12,
                  "TBps": 3 * 8 * 2048 * 2048 / (ms * 1e-3) / 1e12})
    for r in lines[-5:]:
        print(f"{r['kind']:8s} {r['name']:44s} {r['ms']:8.4f} ms" +
              (f"  {r['fp64_TFLOPs']:.2f} fp64 TFLOP/s, {r['TBps']:.2f} TB/s of accumulator traffic" if "TBps" in r else ""))
    head = {"chunk": F.CHUNK, "conv_gflop_per_image": flops / 1e9, "abi": int(_lib.load().rdeic_abi_count())}
    print(json.dumps({**head, "lines": lines}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(head) + "\n")
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
