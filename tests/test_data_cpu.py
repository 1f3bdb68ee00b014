"""The image-list dataset's host side (rdeic_amd/data.py), without a GPU.

* resize_plan's int32 tables, evaluated by the small numpy integer evaluator below (horizontal pass first, uint8
  intermediate, clip8((2^21 + sum kk * px) >> 22)), equal PIL.Image.resize bit for bit for BOX and BICUBIC.
* the plan's structure: halvings, dropped stages and passes.
* the whole chain (plan, crop, flips) from the draws recorded in tests/golden/data_lic.npz equals what the
  reference's LICDataset returned (tests/golden/make_data_golden.py), through PIL and through the tables.
* draw_crop keeps the reference's ranges; the loader's order, sharding and seek.
* train.py builds no loader for a config without data.train.
"""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from rdeic_amd import data as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "data_lic.npz")

BOX_CASES = [((203, 135), (101, 67)), ((101, 67), (50, 33)), ((97, 131), (48, 65))]
BICUBIC_CASES = [((77, 53), (40, 28)), ((53, 77), (36, 52)), ((64, 40), (70, 44)), ((203, 135), (61, 41)),
                 ((33, 47), (32, 46))]


def noise_image(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def eval_axis(arr, bounds, kk, axis):
    """One resampling pass of an [h][w][3] uint8 array along `axis` (0: vertical, 1: horizontal)."""
    a = np.moveaxis(arr.astype(np.int64), axis, 0)
    out = np.empty((bounds.shape[0],) + a.shape[1:], dtype=np.int64)
    for o in range(bounds.shape[0]):
        lo, n = int(bounds[o, 0]), int(bounds[o, 1])
        acc = np.full(a.shape[1:], 1 << 21, dtype=np.int64)
        for t in range(n):
            acc += int(kk[o, t]) * a[lo + t]
        out[o] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def eval_plan(arr, plan):
    for st in plan:
        for p in st.passes:
            arr = eval_axis(arr, p.bounds, p.kk, 1 if p.axis == "h" else 0)
    return arr


def resize_tables(arr, out, filt):
    h, w = arr.shape[:2]
    if out[0] != w:
        arr = eval_axis(arr, *D.coeff_tables(w, out[0], filt), 1)
    if out[1] != h:
        arr = eval_axis(arr, *D.coeff_tables(h, out[1], filt), 0)
    return arr


@pytest.mark.parametrize("size,out", BOX_CASES)
def test_box_tables_equal_pil(size, out):
    img = noise_image(*size, seed=size[0])
    want = np.array(Image.fromarray(img).resize(out, resample=Image.BOX))
    assert np.array_equal(resize_tables(img, out, D.BOX), want)


@pytest.mark.parametrize("size,out", BICUBIC_CASES)
def test_bicubic_tables_equal_pil(size, out):
    img = noise_image(*size, seed=size[1])
    want = np.array(Image.fromarray(img).resize(out, resample=Image.BICUBIC))
    assert np.array_equal(resize_tables(img, out, D.BICUBIC), want)


def test_coefficient_sum_cannot_overflow_int32():
    for (size, out), filt in [(c, D.BOX) for c in BOX_CASES] + [(c, D.BICUBIC) for c in BICUBIC_CASES]:
        for i, o in zip(size, out):
            _, kk = D.coeff_tables(i, o, filt)
            assert 255 * int(np.abs(kk.astype(np.int64)).sum(1).max()) + (1 << 21) < 2 ** 31


def test_plan_structure():
    plan = D.resize_plan((300, 131), 32)  # 300x131 -> 150x65 -> 75x32, and 75x32 is already the size
    assert [(s.filter, s.in_size, s.out_size) for s in plan] == [(D.BOX, (300, 131), (150, 65)),
                                                                  (D.BOX, (150, 65), (75, 32))]
    assert all([p.axis for p in s.passes] == ["h", "v"] for s in plan)
    plan = D.resize_plan((64, 64), 32)
    assert [(s.filter, s.out_size) for s in plan] == [(D.BOX, (32, 32))]
    assert D.resize_plan((32, 32), 32) == ()
    plan = D.resize_plan((40, 33), 32)
    assert [(s.filter, s.in_size, s.out_size) for s in plan] == [(D.BICUBIC, (40, 33), (39, 32))]
    assert [p.axis for p in plan[0].passes] == ["h", "v"]  # the horizontal pass runs first
    assert [(p.in_size, p.out_size) for p in plan[0].passes] == [(40, 39), (33, 32)]
    assert D.resize_plan((40, 32), 32) == ()  # scale 1: both sides keep their size


def _fixture_cases():
    g = np.load(GOLD)
    S = int(g["out_size"])
    for ci, case in enumerate(g["cases"]):
        crop, hf, rot = str(case).split("/")
        for i in range(4):
            yield g, S, ci, i, crop, bool(int(hf)), bool(int(rot))


def draws_from_log(log, size, out_size, crop, hf, rot):
    """The reference's recorded random values, in its order of use, as CropDraws."""
    log = list(log)
    if crop == "random":
        smaller, cy, cx = int(log.pop(0)), int(log.pop(0)), int(log.pop(0))
    else:
        smaller = out_size
        w, h = D.resized_size(size, smaller)
        cy, cx = (h - out_size) // 2, (w - out_size) // 2
    hflip = hf and log.pop(0) < 0.5
    vflip = rot and log.pop(0) < 0.5
    rot90 = rot and log.pop(0) < 0.5
    assert not log
    return D.CropDraws(smaller, cy, cx, bool(hflip), bool(vflip), bool(rot90))


def test_whole_chain_equals_reference_dataset():
    n = 0
    for g, S, ci, i, crop, hf, rot in _fixture_cases():
        img = g[f"img{i}"]
        size = (img.shape[1], img.shape[0])
        d = draws_from_log(g[f"draws{ci}_{i}"], size, S, crop, hf, rot)
        want = g[f"out{ci}_{i}"]
        got = D.process_host(Image.fromarray(img), d, S, crop)
        assert np.array_equal(got, want), (ci, i, "PIL chain")
        full = eval_plan(img, D.resize_plan(size, d.smaller_dim_size))
        assert (full.shape[1], full.shape[0]) == D.resized_size(size, d.smaller_dim_size)
        got = D.flip_host(full[d.crop_y:d.crop_y + S, d.crop_x:d.crop_x + S], d)
        assert np.array_equal(got, want), (ci, i, "tables")
        n += 1
    assert n == 12


def test_draw_crop_ranges():
    seen = {"s": set(), "s256": set(), "h": set(), "v": set(), "r": set()}
    for i in range(400):
        rng = D.image_rng(5, 0, i)
        d = D.draw_crop(rng, (200, 150), 32, "random", True, True)
        assert 32 <= d.smaller_dim_size <= 40  # [ceil(32 / 1.0), ceil(32 / 0.8)]
        w, h = D.resized_size((200, 150), d.smaller_dim_size)
        assert min(w, h) == d.smaller_dim_size
        assert 0 <= d.crop_y <= h - 32 and 0 <= d.crop_x <= w - 32
        seen["s"].add(d.smaller_dim_size), seen["h"].add(d.hflip), seen["v"].add(d.vflip), seen["r"].add(d.rot90)
        d = D.draw_crop(D.image_rng(5, 1, i), (900, 700), 256, "random", True, False)
        assert 512 <= d.smaller_dim_size <= 640  # the 256 branch: fractions 0.4 to 0.5
        assert not d.vflip and not d.rot90
        seen["s256"].add(d.smaller_dim_size)
    assert seen["s"] == set(range(32, 41)) and min(seen["s256"]) < 530 and max(seen["s256"]) > 620
    assert seen["h"] == seen["v"] == seen["r"] == {False, True}
    d = D.draw_crop(D.image_rng(5, 0, 0), (200, 150), 32, "center", False, False)
    assert d == D.CropDraws(32, 0, (43 - 32) // 2, False, False, False)
    # keyed by (seed, epoch, index) only
    assert D.draw_crop(D.image_rng(5, 2, 9), (200, 150), 32, "random", True, True) == \
        D.draw_crop(D.image_rng(5, 2, 9), (200, 150), 32, "random", True, True)


@pytest.fixture(scope="module")
def file_list(tmp_path_factory):
    td = tmp_path_factory.mktemp("imgs")
    paths = []
    for i in range(11):
        w, h = [(70, 50), (45, 66), (64, 64)][i % 3]
        p = td / f"{i}.png"
        Image.fromarray(noise_image(w, h, 50 + i)).save(p)
        paths.append(str(p))
    lst = td / "list.txt"
    lst.write_text("\n".join(paths[:5]) + "\n\n  \n" + "\n".join(paths[5:]) + "\n")
    return str(lst), paths


def _loader(lst, **kw):
    args = dict(out_size=32, crop_type="random", use_hflip=True, use_rot=True, batch_size=2, shuffle=True,
                drop_last=False, seed=3, rank=0, world=1, device="cpu", threads=2, host_resize=True)
    args.update(kw)
    return D.ImageListLoader(lst, **args)


def test_file_list_and_sharding(file_list):
    lst, paths = file_list
    assert D.load_file_list(lst) == paths
    l0, l1 = _loader(lst, rank=0, world=2), _loader(lst, rank=1, world=2)
    for epoch in (0, 1):
        a, b = l0.epoch_indices(epoch), l1.epoch_indices(epoch)
        assert not set(a) & set(b) and sorted(list(a) + list(b)) == list(range(11))
    assert not np.array_equal(l0.epoch_indices(0), l0.epoch_indices(1))
    assert list(_loader(lst, shuffle=False).epoch_indices(4)) == list(range(11))
    assert len(_loader(lst)) == 6 and len(_loader(lst, drop_last=True)) == 5
    assert len(_loader(lst, rank=1, world=2, drop_last=True)) == 2  # 5 images
    for l in (l0, l1):
        l.close()


def test_loader_batches_seek_and_determinism(file_list):
    lst, paths = file_list
    a, b = _loader(lst), _loader(lst)
    ea, eb = list(a), list(b)
    assert len(ea) == 6 and ea[0].shape == (2, 32, 32, 3) and ea[0].dtype == torch.uint8
    assert ea[-1].shape[0] == 1  # drop_last false keeps the short batch
    assert all(torch.equal(x, y) for x, y in zip(ea, eb))
    # the batches are the chain of their images under the (seed, epoch, index) draws
    idx = a.batch_indices(0, 1)
    for j, i in enumerate(idx):
        img = Image.open(paths[i]).convert("RGB")
        d = D.draw_crop(D.image_rng(3, 0, int(i)), img.size, 32, "random", True, True)
        assert np.array_equal(ea[1][j].numpy(), D.process_host(img, d, 32, "random"))
    # a second epoch differs, and seek lands where the uninterrupted run would be
    e1 = list(a)
    assert a.epoch == 2 and not torch.equal(e1[0], ea[0])
    s = _loader(lst)
    s.seek(6 + 2)
    got = list(s)
    assert len(got) == 4 and all(torch.equal(x, y) for x, y in zip(got, e1[2:]))
    # forever() crosses the epoch boundary in the same order
    f = _loader(lst)
    f.seek(4)
    it = f.forever()
    assert all(torch.equal(next(it), want) for want in ea[4:] + e1[:2])
    it.close()
    for l in (a, b, s, f):
        l.close()


def test_passthrough_needs_multiples_of_64_and_equal_sides(tmp_path):
    for name, (w, h) in {"a": (128, 64), "b": (64, 64), "c": (70, 64)}.items():
        Image.fromarray(noise_image(w, h, 1)).save(tmp_path / f"{name}.png")
    mk = lambda names: D.ImageListLoader([str(tmp_path / f"{n}.png") for n in names], out_size=64, crop_type="none",
                                         use_hflip=False, use_rot=False, batch_size=2, shuffle=False,
                                         drop_last=False, seed=0, device="cpu", threads=1, host_resize=True)
    assert next(iter(mk("bb"))).shape == (2, 64, 64, 3)
    with pytest.raises(ValueError, match="multiples of 64"):
        next(iter(mk("bc")))
    with pytest.raises(ValueError, match="equal sides"):
        next(iter(mk("ab")))
    with pytest.raises(ValueError, match="host_resize"):
        D.ImageListLoader([str(tmp_path / "a.png")], 64, "none", False, False, 1, False, False, 0, device="cpu")


def test_config_without_data_train_builds_no_loader(file_list):
    import yaml

    import train
    with open(os.path.join(ROOT, "configs", "finetune_ood.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert train.data_loaders(cfg, 231, 0, 1, torch.device("cpu")) == (None, None)
    cfg["data"]["train"] = dict(file_list=file_list[0], out_size=32, crop_type="random", use_hflip=True,
                                use_rot=False, batch_size=2, shuffle=True, drop_last=True, num_workers=2,
                                host_resize=True)
    tr, va = train.data_loaders(cfg, 231, 0, 1, torch.device("cpu"))
    assert va is None and isinstance(tr, D.ImageListLoader) and len(tr) == 5 and tr.threads == 2
    tr.close()
    for name in ("finetune_ood_files.yaml", "refine_files.yaml"):
        with open(os.path.join(ROOT, "configs", name)) as f:
            c = yaml.safe_load(f)
        assert c["data"]["train"]["crop_type"] == "random" and c["data"]["train"]["out_size"] == 512
        assert c["data"]["train"]["use_hflip"] is True
