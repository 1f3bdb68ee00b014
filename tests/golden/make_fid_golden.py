"""Generates tests/golden/fid_tower.npz: the float64 restatement's pool3 features (tests/fid_ref.py) of two seeded
64x48 uint8 images under seeded_inception(0), and the float32 yardstick: the worst absolute error of the same
restatement run in float32 on the CPU, with the largest |feature|. The device tower is held against the yardstick
read from the file, never against its own output.

    python tests/golden/make_fid_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import fid_ref  # noqa: E402
from rdeic_amd.fid import seeded_inception  # noqa: E402


def main():
    sd = seeded_inception(0)
    rs = np.random.RandomState(20261020)
    # smooth structure plus noise, so the resize and the stem see both
    yy, xx = np.mgrid[0:64, 0:48]
    imgs = []
    for k in range(2):
        base = 127 + 90 * np.sin(xx[..., None] * (0.11 + 0.05 * k) + np.arange(3)) * np.cos(yy[..., None] * 0.07 * (k + 1))
        imgs.append(np.clip(base + rs.normal(0, 20, base.shape), 0, 255).astype(np.uint8))
    imgs = np.stack(imgs)
    with torch.no_grad():
        f64 = fid_ref.tower(imgs, sd, torch.float64).numpy()
        f32 = fid_ref.tower(imgs, sd, torch.float32).numpy().astype(np.float64)
    err = float(np.abs(f32 - f64).max())
    out = os.path.join(HERE, "fid_tower.npz")
    np.savez_compressed(out, images=imgs, features=f64, f32_max_abs_err=np.float64(err),
                        max_abs_feature=np.float64(np.abs(f64).max()))
    print(f"{out}: features {f64.shape}, max |f| {np.abs(f64).max():.4f}, mean {f64.mean():.4f}, "
          f"zeros {(f64 == 0).mean():.3f}, float32 worst abs err {err:.3e}, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
