"""Text tower timings on one MI355X: one JSON line per measurement.

  tower:     OpenCLIPTextEncoder.encode_tokens at the full ViT-H/14 text shape (24 layers, 23 run for "penultimate"),
             seeded weights, B = 1 and 16, bf16 and fp32: median of `--calls` calls, each a host clock around the call
             ended by a device synchronise (the caller's view: token check, upload, ~210 launches), and the same calls'
             device-event time.
  attention: rdeic_attention_causal at l = 77, 16 heads of 64, B = 1 and 16, against rdeic_attention (non-causal,
             lq = lk = 77) on the same buffers; samples of `--reps` back-to-back launches between two events, the two
             kernels alternating, median / min / max per launch over `--calls` samples.

    python tools/text_bench.py [--calls 30] [--reps 50] [--only tower|attention] [--dtype bf16|fp32] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rdeic_amd import ops  # noqa: E402
from rdeic_amd.text import OpenCLIPTextEncoder, TextConfig  # noqa: E402


def emit(rec, fh):
    line = json.dumps(rec)
    print(line, flush=True)
    if fh:
        fh.write(line + "\n")
        fh.flush()


DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}


def bench_tower(calls, fh, dtypes):
    cfg = TextConfig()
    g = torch.Generator().manual_seed(0)
    for name in dtypes:
        dtype = DTYPES[name]
        tower = OpenCLIPTextEncoder(cfg, dtype, "cuda").init_synthetic()
        for B in (1, 16):
            tokens = torch.zeros((B, cfg.context), dtype=torch.int64)
            tokens[:, 0] = 49406
            tokens[:, 1:20] = torch.randint(1, 49000, (B, 19), generator=g)
            tokens[:, 20] = 49407
            for _ in range(3):
                out = tower.encode_tokens(tokens)
            torch.cuda.synchronize()
            wall, dev = [], []
            for _ in range(calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                out = tower.encode_tokens(tokens)
                e1.record()
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
                dev.append(e0.elapsed_time(e1))
            emit({"what": "tower_encode_tokens", "dtype": name, "batch": B, "layers_run": cfg.blocks_run(),
                  "width": cfg.width, "calls": calls, "wall_ms_median": round(statistics.median(wall), 3),
                  "wall_ms_min": round(min(wall), 3), "wall_ms_max": round(max(wall), 3),
                  "event_ms_median": round(statistics.median(dev), 3),
                  "finite": bool(torch.isfinite(out.float()).all())}, fh)
        del tower
        torch.cuda.empty_cache()


def bench_attention(calls, reps, fh, dtypes):
    heads, dh, l = 16, 64, 77
    C = heads * dh
    for name in dtypes:
        dtype = DTYPES[name]
        for B in (1, 16):
            qkv = torch.randn(B * l, 3 * C, device="cuda").to(dtype)
            q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
            o = torch.empty(B * l, C, dtype=dtype, device="cuda")
            sc = dh ** -0.5
            fns = {"causal": lambda: ops.attention_causal(q, k, v, o, batch=B, heads=heads, l=l, dh=dh, scale=sc),
                   "noncausal": lambda: ops.attention(q, k, v, o, batch=B, heads=heads, lq=l, lk=l, dh=dh, scale=sc)}
            for fn in fns.values():
                for _ in range(reps):
                    fn()
            torch.cuda.synchronize()
            us = {n: [] for n in fns}
            for _ in range(calls):
                for n, fn in fns.items():  # alternating
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(reps):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    us[n].append(e0.elapsed_time(e1) * 1e3 / reps)
            rec = {"what": "attention_l77_h16", "dtype": name, "batch": B, "samples": calls,
                   "launches_per_sample": reps}
            for n, xs in us.items():
                rec[n + "_us_median"] = round(statistics.median(xs), 2)
                rec[n + "_us_min"] = round(min(xs), 2)
                rec[n + "_us_max"] = round(max(xs), 2)
            emit(rec, fh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", type=str, default="")
    ap.add_argument("--only", type=str, default="", choices=["", "tower", "attention"])
    ap.add_argument("--dtype", type=str, default="", choices=["", "bf16", "fp32"], help="default: both")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("text_bench.py needs the GPU: it measures, it does not estimate")
    fh = open(args.out, "w") if args.out else None
    dtypes = [args.dtype] if args.dtype else list(DTYPES)
    if args.only in ("", "attention"):
        bench_attention(args.calls, args.reps, fh, dtypes)
    if args.only in ("", "tower"):
        bench_tower(args.calls, fh, dtypes)


if __name__ == "__main__":
    main()
