"""The device resize / crop / flip chain (csrc/image_ops.hip through rdeic_amd/data.py) against the PIL chain
computed here, torch.equal on uint8: every resize and plan shape of tests/test_data_cpu.py, crops at the far
border, the eight flip / transpose combinations, sources with 4-aligned and with odd row strides, a window wide
enough for several blocks per row, three sources of different sizes into one [3, 32, 32, 3] batch, the fixture
of the reference's LICDataset, and the loader's own device path. Every output is a slice of a larger allocation
filled with a canary value that must be unchanged outside the slice."""
import itertools
import os

import numpy as np
import pytest
import torch
from PIL import Image

from rdeic_amd import data as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "data_lic.npz")
CANARY = 0xA5

BOX_CASES = [((203, 135), (101, 67)), ((101, 67), (50, 33)), ((97, 131), (48, 65))]
BICUBIC_CASES = [((77, 53), (40, 28)), ((53, 77), (36, 52)), ((64, 40), (70, 44)), ((203, 135), (61, 41)),
                 ((33, 47), (32, 46))]
# (source (w, h), smaller side): the plan-structure rows, one with both crop maxima above zero, and a source whose
# halved rows (1200 bytes) take more than one block of the vertical pass and six tiles of the horizontal one
CHAIN_CASES = [((300, 131), 32), ((64, 64), 32), ((32, 32), 32), ((40, 33), 32), ((203, 135), 40), ((800, 96), 40)]
S = 32


def noise_image(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def pil_chain(img, d, out_size):
    """The reference's random_crop_arr / center_crop_arr and augment, restated on PIL and numpy."""
    pil = Image.fromarray(img)
    while min(*pil.size) >= 2 * d.smaller_dim_size:
        pil = pil.resize(tuple(x // 2 for x in pil.size), resample=Image.BOX)
    scale = d.smaller_dim_size / min(*pil.size)
    pil = pil.resize(tuple(round(x * scale) for x in pil.size), resample=Image.BICUBIC)
    arr = np.array(pil)[d.crop_y:d.crop_y + out_size, d.crop_x:d.crop_x + out_size]
    return flips(arr, d)


def flips(arr, d):
    if d.hflip:
        arr = arr[:, ::-1]
    if d.vflip:
        arr = arr[::-1]
    if d.rot90:
        arr = arr.transpose(1, 0, 2)
    return np.ascontiguousarray(arr)


def upload(img, plan, padded):
    """(raw bytes on the device, row stride, device tables, offsets) as the loader lays them out."""
    h, w = img.shape[:2]
    stride = D._r4(w * 3) if padded else w * 3
    host = np.zeros((h, stride), np.uint8)
    host[:, :w * 3] = img.reshape(h, w * 3)
    tables, offs = D.plan_tables(plan)
    return torch.from_numpy(host).cuda().view(-1), stride, torch.from_numpy(tables.copy()).cuda(), offs


def run_device(img, plan, d, out_shape, *, padded=True, offset=7, crop_type="random", window=None, out_size=S):
    """The chain into a slice (at byte `offset`) of a canary-filled allocation; checks the canary."""
    from rdeic_amd import ops
    raw, stride, tables, offs = upload(img, plan, padded)
    n = int(np.prod(out_shape))
    big = torch.full((n + 4096,), CANARY, dtype=torch.uint8, device="cuda")
    dst = big[offset:offset + n].view(out_shape)
    D.process_device(raw, (img.shape[1], img.shape[0]), stride, tables, offs, plan, d, out_size, crop_type, dst,
                     ops.stream_ptr(), window=window)
    torch.cuda.synchronize()
    assert bool((big[:offset] == CANARY).all()) and bool((big[offset + n:] == CANARY).all()), "wrote outside the slot"
    return dst.cpu()


NOFLIP = dict(hflip=False, vflip=False, rot90=False)


@pytest.mark.parametrize("padded", [True, False])
@pytest.mark.parametrize("filt,size,out", [(D.BOX, *c) for c in BOX_CASES] + [(D.BICUBIC, *c) for c in BICUBIC_CASES])
def test_resize_equals_pil(gpu, filt, size, out, padded):
    img = noise_image(*size, seed=size[0] + out[0])
    want = np.array(Image.fromarray(img).resize(out, resample=Image.BOX if filt == D.BOX else Image.BICUBIC))
    passes = (D.Pass("h", size[0], out[0], *D.coeff_tables(size[0], out[0], filt)),
              D.Pass("v", size[1], out[1], *D.coeff_tables(size[1], out[1], filt)))
    plan = (D.Stage(filt, size, out, passes),)
    d = D.CropDraws(0, 0, 0, **NOFLIP)
    got = run_device(img, plan, d, want.shape, padded=padded, offset=64 if padded else 7,
                     window=(0, 0, out[1], out[0]))
    assert torch.equal(got, torch.from_numpy(want))
    # an interior window: only those rows and columns are computed
    wy, wx, wh, ww = out[1] // 3, out[0] // 4, out[1] // 2, out[0] // 2 + 1
    got = run_device(img, plan, d, (wh, ww, 3), padded=padded, window=(wy, wx, wh, ww))
    assert torch.equal(got, torch.from_numpy(want[wy:wy + wh, wx:wx + ww].copy()))


@pytest.mark.parametrize("size,smaller", CHAIN_CASES)
def test_chain_equals_pil_at_the_corners(gpu, size, smaller):
    img = noise_image(*size, seed=size[0] * 7 + smaller)
    w, h = D.resized_size(size, smaller)
    plan = D.resize_plan(size, smaller)
    for (cy, cx), padded in zip([(0, 0), (h - S, w - S), ((h - S) // 2, (w - S) // 2)], [True, False, True]):
        d = D.CropDraws(smaller, cy, cx, **NOFLIP)
        got = run_device(img, plan, d, (S, S, 3), padded=padded, offset=64 if cy else 5)
        assert torch.equal(got, torch.from_numpy(pil_chain(img, d, S))), (size, smaller, cy, cx)


@pytest.mark.parametrize("hflip,vflip,rot90", list(itertools.product([False, True], repeat=3)))
def test_flips_and_transpose(gpu, hflip, vflip, rot90):
    size, smaller = (203, 135), 40
    img = noise_image(*size, seed=11)
    d = D.CropDraws(smaller, 3, 21, hflip, vflip, rot90)
    got = run_device(img, D.resize_plan(size, smaller), d, (S, S, 3))
    assert torch.equal(got, torch.from_numpy(pil_chain(img, d, S)))
    # crop_type none: the whole (non-square) image through the flips alone
    src = noise_image(128, 64, seed=12)
    want = flips(src, d)
    got = run_device(src, (), d, want.shape, crop_type="none", out_size=64)
    assert torch.equal(got, torch.from_numpy(want))


def test_three_sources_into_one_batch(gpu):
    from rdeic_amd import ops
    cases = [((300, 131), 32, (0, 43)), ((40, 33), 32, (0, 7)), ((203, 135), 40, (8, 28))]
    big = torch.full((5, S, S, 3), CANARY, dtype=torch.uint8, device="cuda")
    batch = big[1:4]
    want = []
    for b, (size, smaller, (cy, cx)) in enumerate(cases):
        img = noise_image(*size, seed=20 + b)
        d = D.CropDraws(smaller, cy, cx, hflip=b == 1, vflip=False, rot90=b == 2)
        plan = D.resize_plan(size, smaller)
        raw, stride, tables, offs = upload(img, plan, True)
        D.process_device(raw, size, stride, tables, offs, plan, d, S, "random", batch[b], ops.stream_ptr())
        want.append(pil_chain(img, d, S))
    torch.cuda.synchronize()
    assert torch.equal(batch.cpu(), torch.from_numpy(np.stack(want)))
    assert bool((big[0] == CANARY).all()) and bool((big[4] == CANARY).all())


def test_fixture_of_the_reference_dataset(gpu):
    g = np.load(GOLD)
    n = 0
    for ci, case in enumerate(g["cases"]):
        crop, hf, rot = str(case).split("/")
        for i in range(4):
            img = g[f"img{i}"]
            size = (img.shape[1], img.shape[0])
            log = list(g[f"draws{ci}_{i}"])
            if crop == "random":
                smaller, cy, cx = int(log.pop(0)), int(log.pop(0)), int(log.pop(0))
            else:
                smaller = S
                w, h = D.resized_size(size, smaller)
                cy, cx = (h - S) // 2, (w - S) // 2
            hflip = bool(int(hf)) and log.pop(0) < 0.5
            vflip = bool(int(rot)) and log.pop(0) < 0.5
            rot90 = bool(int(rot)) and log.pop(0) < 0.5
            d = D.CropDraws(smaller, cy, cx, bool(hflip), bool(vflip), bool(rot90))
            got = run_device(img, D.resize_plan(size, smaller), d, (S, S, 3), crop_type=crop)
            assert torch.equal(got, torch.from_numpy(g[f"out{ci}_{i}"])), (ci, i)
            n += 1
    assert n == 12


def test_loader_device_path_equals_host_path(gpu, tmp_path):
    sizes = [(300, 131), (70, 50), (45, 66), (203, 135), (64, 64), (90, 81), (33, 47)]
    paths = []
    for i, (w, h) in enumerate(sizes):
        paths.append(str(tmp_path / f"{i}.png"))
        Image.fromarray(noise_image(w, h, 70 + i)).save(paths[-1])
    kw = dict(out_size=S, crop_type="random", use_hflip=True, use_rot=True, batch_size=3, shuffle=True,
              drop_last=False, seed=9, threads=2)
    dev = D.ImageListLoader(paths, device="cuda", **kw)
    host = D.ImageListLoader(paths, device="cpu", host_resize=True, **kw)
    pin = D.ImageListLoader(paths, device="cuda", host_resize=True, **kw)
    for epoch in range(2):
        got, want, got_pin = list(dev), list(host), list(pin)
        assert [tuple(b.shape) for b in got] == [(3, S, S, 3), (3, S, S, 3), (1, S, S, 3)]
        for a, b, c in zip(got, want, got_pin):
            assert a.is_cuda and a.dtype == torch.uint8
            assert torch.equal(a.cpu(), b) and torch.equal(c.cpu(), b)
    # a staging slot smaller than the image is replaced by a larger one on the consumer thread
    small = D.ImageListLoader(paths, device="cuda", **kw)
    small._cap = 1024
    host.seek(0)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(list(small), list(host)))
    for l in (dev, host, pin, small):
        l.close()
