"""Throughput of the image-list data path (rdeic_amd/data.py) on one GPU.

Writes a seeded set of PNG and JPEG files of the satellite list's typical sizes to a temporary directory and prints
one JSON line per measurement:
  * loader images/s (random 512 crops, hflip) with the resize chain on the device and with host_resize (PIL on the
    decode threads), at 2, 4 and 16 decode threads, as alternating pairs;
  * train.py steps/s (config 5, bf16, captured step) fed from those files against the synthetic pool, as
    alternating pairs (--train-steps 0 skips it).

  python tools/data_bench.py [--pairs 3] [--batches 24] [--train-steps 40] > profiles/data_bench.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(2040, 1356), (1356, 2040), (2040, 1536), (1024, 1024), (1500, 1000), (2040, 1152)]  # (w, h)


def write_files(td: str, n: int, seed: int):
    from PIL import Image

    from rdeic_amd.synthetic import synth_image
    paths = []
    for i in range(n):
        w, h = SIZES[i % len(SIZES)]
        img = Image.fromarray(synth_image(h, w, seed + i))
        p = os.path.join(td, f"{i}.png" if i % 2 == 0 else f"{i}.jpg")
        img.save(p, **({} if p.endswith(".png") else {"quality": 92}))
        paths.append(p)
    return paths


def loader_rate(paths, threads: int, host_resize: bool, batches: int, batch_size: int) -> float:
    from rdeic_amd.data import ImageListLoader
    ld = ImageListLoader(paths, 512, "random", True, False, batch_size, True, True, 231, device="cuda",
                         threads=threads, host_resize=host_resize)
    it = ld.forever()
    for _ in range(2):
        next(it)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(batches):
        next(it)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    it.close()
    ld.close()
    return batches * batch_size / dt


def train_rate(td: str, lst, steps: int, warm: int) -> float:
    """Steps/s of train.main between step `warm` and the last one (the capture and the first replays left out)."""
    import train
    data = {"out_size": 512, "batch_size": 1, "n_images": 16}
    if lst:
        data = {"train": dict(file_list=lst, out_size=512, crop_type="random", use_hflip=True, use_rot=False,
                              batch_size=1, shuffle=True, drop_last=True, num_workers=0)}
    cfg = {"data": data,
           "model": {"learning_rate": 2e-5, "l_guide_weight": 3.0, "l_bpp_weight": 1.0, "used_timesteps": 300,
                     "sd_locked": True, "is_refine": False, "precision": "bf16", "resume": None},
           "lightning": {"seed": 231, "trainer": {"max_steps": steps, "log_every_n_steps": 1},
                         "checkpoint": {"every_n_train_steps": 0}}}
    p = os.path.join(td, "files.yaml" if lst else "synthetic.yaml")
    with open(p, "w") as f:
        yaml.safe_dump(cfg, f)
    stdout, sys.stdout = sys.stdout, open(os.devnull, "w")  # the per-step records are not this tool's output
    try:
        recs = train.main(["--config", p])
    finally:
        sys.stdout.close()
        sys.stdout = stdout
    t = {r["global_step"]: r["global_step"] / r["it_per_s"] for r in recs}
    return (steps - warm) / (t[steps] - t[warm])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=24)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--batches", type=int, default=24)
    ap.add_argument("--batch-size", type=int, default=4)
    ap.add_argument("--threads", default="2,4,16")
    ap.add_argument("--train-steps", type=int, default=40)
    args = ap.parse_args(argv)
    with tempfile.TemporaryDirectory() as td:
        t0 = time.perf_counter()
        paths = write_files(td, args.files, 4000)
        lst = os.path.join(td, "files.list")
        with open(lst, "w") as f:
            f.write("\n".join(paths) + "\n")
        print(json.dumps({"files": len(paths), "write_s": round(time.perf_counter() - t0, 2),
                          "mean_file_mb": round(float(np.mean([os.path.getsize(p) for p in paths])) / 2 ** 20, 2)}),
              flush=True)
        for threads in [int(t) for t in args.threads.split(",")]:
            for pair in range(args.pairs):
                for host in (False, True):
                    r = loader_rate(paths, threads, host, args.batches, args.batch_size)
                    print(json.dumps({"loader": "host_resize" if host else "device", "threads": threads,
                                      "pair": pair, "images_per_s": round(r, 2)}), flush=True)
        if args.train_steps:
            warm = max(2, args.train_steps // 4)
            for pair in range(args.pairs):
                for src in ("files", "synthetic"):
                    r = train_rate(td, lst if src == "files" else None, args.train_steps, warm)
                    print(json.dumps({"train": src, "pair": pair, "steps_per_s": round(r, 3)}), flush=True)


if __name__ == "__main__":
    main()
