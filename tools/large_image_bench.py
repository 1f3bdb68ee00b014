"""Time the VAE encoder and decoder on ONE large image (bf16, synthetic weights): the sizes whose full-resolution
tensors are past the 2 GiB reach of one conv launch and run as row bands.

usage: python tools/large_image_bench.py [--sizes 2048x2112,2176x3840,4096x4096] [--reps 3] [--skip-decode HxW,...]
                                         [--label NAME] >> profiles/NAME.jsonl

Prints one JSON line per (stage, size): wall ms per call (median of --reps after one warm-up, HIP events), the conv
launches' executed FLOPs and event-timed ms from the library's launch profiler (a separate pass), the peak device
memory of the call, and the fast-kernel launch counters (halo, phase, edge, LDS-DMA; 0 where the library does not have
the counter). A build without row bands runs the same script: time it only where it is correct (--skip-decode
4096x4096: its conv_out wraps there)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rdeic_amd import ops  # noqa: E402
from rdeic_amd.rdeic import RDEIC  # noqa: E402


def _counts():
    out = {}
    for name, kind in (("halo", 0), ("edge", 6), ("dma", 8), ("phases", 9)):
        try:
            out[name] = ops.launch_count(kind)
        except Exception:
            out[name] = 0
    return out


def _time(fn, reps):
    fn()  # warm-up (weight packing, allocator)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    c0 = _counts()
    ops.prof_start()
    fn()
    prof = ops.prof_read()
    ops.prof_stop()
    c1 = _counts()
    peak = torch.cuda.max_memory_allocated()
    conv = prof.get("conv", (0, 0.0, 0.0))
    return {"ms": statistics.median(ms), "ms_all": [round(m, 3) for m in ms], "conv_launches": conv[0],
            "conv_tflop": conv[1] / 1e12, "conv_ms": conv[2],
            "conv_tflops": (conv[1] / 1e12) / (conv[2] / 1e3) if conv[2] else 0.0,
            "peak_gib": peak / 2 ** 30, "launches": {k: c1[k] - c0[k] for k in c0}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048x2112,2176x3840,4096x4096")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-decode", default="")
    ap.add_argument("--label", default="head")
    a = ap.parse_args()
    skip = set(a.skip_decode.split(",")) if a.skip_decode else set()
    model = RDEIC(compute_dtype=torch.bfloat16).init_synthetic()
    model.use_plans = False
    for size in a.sizes.split(","):
        h, w = (int(v) for v in size.split("x"))
        g = torch.Generator(device="cuda").manual_seed(h + w)
        img = torch.randint(0, 256, (1, h, w, 3), dtype=torch.uint8, device="cuda", generator=g)
        z = torch.randn(1, h // 8, w // 8, 4, device="cuda", generator=g)
        stages = [("encode", lambda: model.encode_images_nhwc(img))]
        if size not in skip:
            stages.append(("decode", lambda: model.decode_nhwc(z, out_f32=True)))
        for name, fn in stages:
            with torch.no_grad():
                rec = _time(fn, a.reps)
            rec.update({"label": a.label, "stage": name, "size": size, "dtype": "bf16"})
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
