"""Protected streams measured: what protection buys in the robustness sweep, what it costs in rate, and what it costs
in host time beside one relay decode. One synthetic 512x512 image and the seeded synthetic weights (no checkpoint
ships), the default sweep of run_robustness.py (rates 0,0.1,0.5,1,2,5,10 percent x 5 seeds), one process, one device.
Prints JSON lines, one per measurement:

  * what "sweep": per (error type, protection) the failures, FEC failures, mean PSNR and mean corrected bytes per
    rate, the stream sizes and the rate overhead. random: unprotected, rs:16, rs:32, rs:64; burst: those and rs:32:8.
  * what "host": protect / recover of the image's own body in ms (median of --repeats), clean and with t byte errors in
    every codeword, for rs:16, rs:32, rs:64.
  * what "pairs": the whole sweep (corruption, recovery, entropy decode, relay decode, scoring) without and with
    rs:32, timed alternately between device synchronisations after one untimed run of each.

    python tools/fec_bench.py [--rate_gain 1.0] [--dtype fp32|bf16] [--sampler ddpm|ddim] [--repeats 5] [--out FILE]
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


def main(argv=None) -> list:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate_gain", type=float, default=1.0,
                    help="the synthetic weights' bpp knob (1.0: a 129 KB stream at 512x512; 0.4: 2.5 KB, the codec's "
                         "real size)")
    ap.add_argument("--dtype", default="fp32", choices=["bf16", "fp32"])
    ap.add_argument("--sampler", default="ddpm", choices=["ddim", "ddpm"])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: sweep, host, pairs")
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from rdeic_amd import fec, robustness as R
    from rdeic_amd.rdeic import RDEIC
    from rdeic_amd.synthetic import synth_context, synth_image
    skip = set(args.skip.split(","))
    rates = [r / 100.0 for r in (0, 0.1, 0.5, 1, 2, 5, 10)]
    seeds = [231 + k for k in range(5)]
    m = RDEIC(compute_dtype=torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    m.init_synthetic(rate_gain=args.rate_gain)
    img = torch.from_numpy(synth_image(args.size, args.size, 231)[None]).cuda()
    ctx = synth_context().cuda()
    body = m.compress_images(img)[0]
    base = {"tool": "fec_bench", "rate_gain": args.rate_gain, "dtype": args.dtype, "sampler": args.sampler,
            "size": args.size, "body_bytes": len(body)}
    lines = []

    def emit(rec):
        lines.append(json.dumps({**base, **rec}))
        print(lines[-1], flush=True)

    def sweep(error_type, spec):
        return R.run_robustness(m, img, ctx, "bitstream", error_type, rates, seeds, steps=2, sampler=args.sampler,
                                noise_seed=231, batch_size=args.batch_size, bodies=[body], fec=spec)

    if "sweep" not in skip:
        for error_type, specs in (("random", [None, "rs:16", "rs:32", "rs:64"]),
                                  ("burst", [None, "rs:16", "rs:32", "rs:64", "rs:32:8"])):
            for spec in specs:
                recs = sweep(error_type, spec)
                rows = R.summary_by_rate(recs)
                size = len(fec.protect(body, spec)) if spec else len(body)
                emit({"what": "sweep", "error_type": error_type, "fec": spec or "none", "stream_bytes": size,
                      "bpp": recs[0]["bpp"], "overhead": round(size / len(body) - 1.0, 4),
                      "rates_percent": [row["error_rate"] for row in rows],
                      "failed": [row["decode_failed"] for row in rows],
                      "fec_failed": [row.get("fec_failed") for row in rows],
                      "psnr_mean": [round(row["psnr"][0], 3) for row in rows],
                      "corrected_mean": [row.get("fec_corrected") for row in rows]})

    def median_ms(fn):
        fn()
        samples = []
        for _ in range(max(args.repeats, 21)):
            t0 = time.perf_counter()
            fn()
            samples.append(time.perf_counter() - t0)
        return round(statistics.median(samples) * 1e3, 4)

    if "host" not in skip:
        rng = np.random.default_rng(1)
        for spec in ("rs:16", "rs:32", "rs:64"):
            p = fec.parse_fec(spec)
            clean = fec.protect(body, p)
            bad = bytearray(clean)
            for at in range(46, len(clean), 255):  # depth 1: codewords lie one after the other
                end = min(at + 255, len(clean))
                for pos in rng.choice(np.arange(at, end), min(p.nroots // 2, end - at), replace=False):
                    bad[pos] ^= 0x5a
            bad = bytes(bad)
            got, st = fec.recover(bad)
            assert got == body and st.uncorrectable == 0
            emit({"what": "host", "fec": spec, "stream_bytes": len(clean), "codewords": st.codewords,
                  "protect_ms": median_ms(lambda: fec.protect(body, p)),
                  "recover_clean_ms": median_ms(lambda: fec.recover(clean)),
                  "recover_t_errors_ms": median_ms(lambda: fec.recover(bad)), "bytes_corrected": st.corrected})

    if "pairs" not in skip:
        def once(spec):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = sweep("random", spec)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out
        once(None), once("rs:32")
        t_plain, t_fec = [], []
        for _ in range(args.repeats):
            t_plain.append(once(None)[0])
            t_fec.append(once("rs:32")[0])
        ms = lambda v: [round(x * 1e3, 2) for x in v]  # noqa: E731
        emit({"what": "pairs", "error_type": "random", "fec": "rs:32", "plain_ms": ms(t_plain), "fec_ms": ms(t_fec),
              "plain_median_ms": round(statistics.median(t_plain) * 1e3, 2),
              "fec_median_ms": round(statistics.median(t_fec) * 1e3, 2)})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    main()
