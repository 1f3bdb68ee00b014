"""Golden vectors for the image-list dataset, from the reference's own LICDataset (dataset/licdataset.py with
utils/image/common.py) run where the reference tree is. Output: tests/golden/data_lic.npz.

Four small generated images (landscape, odd-sized, portrait, and one large enough for a BOX halving) go through
LICDataset with crop_type center and random at out_size 32, hflip on, rotation off and on. random.randrange /
random.random are patched to record every draw, so a test can replay the chain with exactly those values. cv2 is
not installed here; the only cv2 call on the path is the in-place cv2.flip of augment(), and the numpy stand-in
below does the same. The outputs are mapped back from the dataset's float [-1, 1] to uint8.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_data_golden.py
"""
import os
import random
import sys
import tempfile
import types

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden import refload  # noqa: E402

SIZES = [(61, 47), (45, 39), (47, 61), (90, 81)]  # (w, h)
OUT = 32
CASES = [("center", True, False), ("random", True, False), ("random", True, True)]  # crop_type, hflip, rot


def _flip(src, code, dst=None):
    out = src[:, ::-1].copy() if code == 1 else src[::-1].copy()
    if dst is None:
        return out
    dst[...] = out
    return dst


def gen_image(w, h, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([xx * 255.0 / w, yy * 255.0 / h, (xx + yy) % 64 * 4.0], axis=-1)
    return np.clip(base + rng.normal(0, 24, (h, w, 3)), 0, 255).round().astype(np.uint8)


def main():
    sys.modules.setdefault("cv2", types.SimpleNamespace(flip=_flip))
    if refload.REF not in sys.path:
        sys.path.insert(0, refload.REF)
    from dataset.licdataset import LICDataset
    out = {"pillow_version": np.array(PIL.__version__), "out_size": np.array(OUT),
           "cases": np.array([f"{c}/{int(hf)}/{int(rot)}" for c, hf, rot in CASES])}
    with tempfile.TemporaryDirectory() as td:
        paths = []
        for i, (w, h) in enumerate(SIZES):
            img = gen_image(w, h, 100 + i)
            out[f"img{i}"] = img
            paths.append(os.path.join(td, f"{i}.png"))
            Image.fromarray(img).save(paths[-1])
        lst = os.path.join(td, "list.txt")
        with open(lst, "w") as f:
            f.write("\n".join(paths) + "\n\n")
        real_randrange, real_random = random.randrange, random.random
        for ci, (crop, hf, rot) in enumerate(CASES):
            ds = LICDataset(lst, OUT, crop, hf, rot)
            for i in range(len(SIZES)):
                log = []

                def rr(*a, _log=log):
                    v = real_randrange(*a)
                    _log.append(float(v))
                    return v

                def rd(_log=log):
                    v = real_random()
                    _log.append(v)
                    return v

                random.seed(7000 + 10 * ci + i)
                random.randrange, random.random = rr, rd
                try:
                    item = ds[i]
                finally:
                    random.randrange, random.random = real_randrange, real_random
                u8 = np.round((item["jpg"].astype(np.float64) + 1.0) * 127.5)
                assert np.abs((u8 / 255.0).astype(np.float32) * 2 - 1 - item["jpg"]).max() < 1e-6
                out[f"out{ci}_{i}"] = u8.astype(np.uint8)
                out[f"draws{ci}_{i}"] = np.array(log, dtype=np.float64)
    dst = os.path.join(HERE, "data_lic.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
