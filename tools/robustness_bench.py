"""Time the bitstream robustness sweep of one image both ways, in one process on one device:

  * run_bitstream_robustness — every corrupted body entropy-decoded alone (20 stage round trips at batch 1 each),
    then one relay decode of all survivors;
  * run_robustness — the variants entropy-decoded in fault-isolating chunks of --batch_size, the survivors
    relay-decoded in chunks of the same size.

One synthetic 512x512 image, the reference's default sweep (rates 0,0.1,0.5,1,2,5,10 percent x 5 seeds = 35
variants), seeded synthetic weights. Two figures per function: the entropy-decode part alone and the whole sweep
(encode, corruption, entropy decode, relay decode, scoring). Both functions of a pair run once untimed first (launch
plans recorded, tiles tuned) and are then timed alternately, old, new, old, new ..., --repeats times each between
device synchronisations; every sample, the medians, their ratio and the smallest and largest per-repeat ratio go
into the result. The old function is unchanged by the new path, so it is the yardstick. Prints one JSON line.
--relay_by_batch measures relay_decode_u8 by batch size instead (what a padded relay row costs).

    python tools/robustness_bench.py [--dtype bf16|fp32] [--rate_gain 1.0] [--batch_size 8] [--repeats 7]
        [--sampler ddim] [--relay_by_batch] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sampler", default="ddim", choices=["ddim", "ddpm"])
    ap.add_argument("--error_type", default="random", choices=["random", "burst"])
    ap.add_argument("--rate_gain", type=float, default=1.0,
                    help="the synthetic weights' bpp knob: 1.0 codes ~4 bpp (every flipped stream fails early), "
                         "0.4 a stream of the codec's real size, of which many flipped variants decode")
    ap.add_argument("--relay_by_batch", action="store_true",
                    help="instead of the sweep: relay_decode_u8 at batch 1, 2, 3, 4, 5, 6, 8 (the cost of a padded row)")
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from rdeic_amd import bitstream, ops, robustness as R
    from rdeic_amd.rdeic import RDEIC
    from rdeic_amd.synthetic import synth_context, synth_image
    rates = [r / 100.0 for r in (0, 0.1, 0.5, 1, 2, 5, 10)]
    seeds = [231 + k for k in range(5)]
    m = RDEIC(compute_dtype=torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    m.init_synthetic(rate_gain=args.rate_gain)
    img = torch.from_numpy(synth_image(args.size, args.size, 231)[None]).cuda()
    ctx = synth_context().cuda()
    body = m.compress_images(img)[0]
    shape0 = bitstream.unpack_body(body)[1]
    variants = [R.Corruptor("bitstream", args.error_type, rate, seed).corrupt_bytes(body)
                for rate in rates for seed in seeds]

    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def timed_pair(old_fn, new_fn):
        """Both once untimed (plans recorded, tiles tuned), then alternating old, new, old, new ... so that a
        drift of the box lands on both alike. -> (old samples, new samples, last old result, last new result)."""
        old_fn(), new_fn()
        t_old, t_new = [], []
        for _ in range(args.repeats):
            t, r_old = once(old_fn)
            t_old.append(t)
            t, r_new = once(new_fn)
            t_new.append(t)
        return t_old, t_new, r_old, r_new

    def stats(old_s, new_s):
        ms = lambda v: [round(x * 1e3, 2) for x in v]  # noqa: E731
        return {"old_ms": ms(old_s), "new_ms": ms(new_s), "old_median_ms": round(statistics.median(old_s) * 1e3, 2),
                "new_median_ms": round(statistics.median(new_s) * 1e3, 2),
                "ratio": round(statistics.median(old_s) / statistics.median(new_s), 3),
                # per repeat, the old sample over the new one taken right after it
                "ratio_min": round(min(o / n for o, n in zip(old_s, new_s)), 3),
                "ratio_max": round(max(o / n for o, n in zip(old_s, new_s)), 3)}

    if args.relay_by_batch:
        # what a padded relay row costs: relay_decode_u8 of the clean latent repeated B times
        lat, hint = m.decompress_bodies([body])
        table = {}
        for B in (1, 2, 3, 4, 5, 6, 8):
            ins = (lat.expand(B, -1, -1, -1).contiguous(), hint.expand(B, -1, -1, -1).contiguous(), ctx,
                   ops.nchw_to_nhwc(torch.randn((B, 4, args.size // 8, args.size // 8),
                                                generator=torch.Generator().manual_seed(1)).cuda(), torch.float32))
            m.relay_decode_u8(*ins, 2, "ddim")  # records the plan of this batch size
            table[B] = round(statistics.median(once(lambda: m.relay_decode_u8(*ins, 2, "ddim"))[0]
                                               for _ in range(args.repeats)) * 1e3, 2)
        res = {"tool": "robustness_bench", "what": "relay_by_batch", "dtype": args.dtype, "rate_gain": args.rate_gain,
               "size": args.size, "sampler": "ddim", "steps": 2, "repeats": args.repeats, "relay_ms_by_batch": table}
    else:
        kw = dict(steps=2, sampler=args.sampler, noise_seed=231)
        dec = timed_pair(lambda: [R.try_decompress(m, b, shape0) for b in variants],
                         lambda: R.decode_isolated(m, variants, shape0, args.batch_size))
        swp = timed_pair(lambda: R.run_bitstream_robustness(m, img, ctx, args.error_type, rates, seeds, **kw),
                         lambda: R.run_robustness(m, img, ctx, "bitstream", args.error_type, rates, seeds,
                                                  batch_size=args.batch_size, **kw))
        old_dec, new_dec, old, new = dec[2], dec[3], swp[2], swp[3]
        fail_old = [isinstance(r, Exception) for r in old_dec]
        same_dec = fail_old == [isinstance(r, Exception) for r in new_dec] and all(
            torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(old_dec, new_dec)
            if not isinstance(a, Exception))
        same_rec = len(old) == len(new) and all(
            {k: v for k, v in a.items() if k != "error"} == {k: v for k, v in b.items() if k != "error"}
            for a, b in zip(old, new))
        res = {"tool": "robustness_bench", "dtype": args.dtype, "rate_gain": args.rate_gain, "size": args.size,
               "sampler": args.sampler, "error_type": args.error_type, "variants": len(variants),
               "batch_size": args.batch_size, "repeats": args.repeats, "body_bytes": len(body),
               "decode_failures": int(np.sum(fail_old)),
               "entropy_decode": stats(dec[0], dec[1]),  # old = serial try_decompress, new = decode_isolated
               "sweep": stats(swp[0], swp[1]),  # old = run_bitstream_robustness, new = run_robustness
               "same_latents": bool(same_dec), "same_records": bool(same_rec)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
