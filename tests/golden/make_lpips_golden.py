"""The learned LPIPS `lin` heads (AlexNet and VGG16, v0.1) as a test fixture, read as data from the reference's
weight/lpips/alex.pth and vgg.pth (state dicts of five `lin<k>.model.1.weight` tensors [1, C, 1, 1] each;
nothing of the reference is imported). Output: tests/golden/lpips_lin.npz with alex_lin0..4 and vgg_lin0..4.

    python tests/golden/make_lpips_golden.py REFERENCE_CHECKOUT
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CHANNELS = {"alex": (64, 192, 384, 256, 256), "vgg": (64, 128, 256, 512, 512)}


def main(ref: str) -> None:
    out = {}
    for net, chans in CHANNELS.items():
        sd = torch.load(os.path.join(ref, "weight", "lpips", f"{net}.pth"), map_location="cpu", weights_only=True)
        for k, c in enumerate(chans):
            v = sd[f"lin{k}.model.1.weight"]
            assert tuple(v.shape) == (1, c, 1, 1) and v.dtype == torch.float32, (net, k, tuple(v.shape))
            out[f"{net}_lin{k}"] = v.reshape(c).numpy()
    path = os.path.join(HERE, "lpips_lin.npz")
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
