"""The shared sequential tower (rdeic_amd/tower.py) without a device: the backward plan of the two tables, the one
weight-file loader, and the size rules against the LPIPS / DISTS delegations."""
import numpy as np
import pytest
import torch

from rdeic_amd import dists as D
from rdeic_amd import lpips as L
from rdeic_amd import tower


def _kinds(plan):
    """(kind, index of the op's input activation, number): the conv's or the tap's; a pool carries the number of the
    convs before it, which nothing reads."""
    return [(op[0], i, j) for op, i, j in plan]


def test_backward_plan_alex():
    # acts: 0 prep, 1 conv0, 2 pool, 3 conv1, 4 pool, 5 conv2, 6 conv3, 7 conv4
    want = [("tap", 7, 4), ("conv", 6, 4), ("tap", 6, 3), ("conv", 5, 3), ("tap", 5, 2), ("conv", 4, 2),
            ("pool", 3, 2), ("tap", 3, 1), ("conv", 2, 1), ("pool", 1, 1), ("tap", 1, 0), ("conv", 0, 0)]
    plan = tower.backward_plan(L.NETS["alex"], 0)
    assert _kinds(plan) == want
    assert plan[1][0] == ("conv", 10, 256, 3, 1, 1) and plan[6][0] == ("pool", 3, 2)  # the table's own tuples
    assert _kinds(tower.backward_plan(L.NETS["alex"], 1)) == [(k, i, j + (k == "tap")) for k, i, j in want]


def test_backward_plan_vgg():
    # acts: 0 prep, 1-2 convs, 3 pool, 4-5 convs, 6 pool, 7-9 convs, 10 pool, 11-13 convs, 14 pool, 15-17 convs
    want = [("tap", 17, 5), ("conv", 16, 12), ("conv", 15, 11), ("conv", 14, 10), ("pool", 13, 10),
            ("tap", 13, 4), ("conv", 12, 9), ("conv", 11, 8), ("conv", 10, 7), ("pool", 9, 7),
            ("tap", 9, 3), ("conv", 8, 6), ("conv", 7, 5), ("conv", 6, 4), ("pool", 5, 4),
            ("tap", 5, 2), ("conv", 4, 3), ("conv", 3, 2), ("pool", 2, 2),
            ("tap", 2, 1), ("conv", 1, 1), ("conv", 0, 0)]
    assert _kinds(tower.backward_plan(L.NETS["vgg"], 1)) == want  # DISTS: tap 0 is the raw image
    assert _kinds(tower.backward_plan(L.NETS["vgg"], 0)) == [(k, i, j - (k == "tap")) for k, i, j in want]


def test_load_state_file(tmp_path):
    sd = {"a": torch.arange(6, dtype=torch.float32).reshape(2, 3), "b": torch.tensor([1.5])}
    np.savez(tmp_path / "w.npz", **{k: v.numpy() for k, v in sd.items()})
    torch.save(sd, tmp_path / "w.pt")
    torch.save({"state_dict": sd, "epoch": 3}, tmp_path / "nest.pt")
    for name in ("w.npz", "w.pt", "nest.pt"):
        got = tower.load_state_file(str(tmp_path / name), "LPIPS")
        assert sorted(got) == ["a", "b"], name
        assert all(torch.equal(got[k], sd[k]) for k in sd), name
    assert tower.load_state(sd, "LPIPS") is sd and sorted(tower.load_state(tmp_path / "w.pt", "LPIPS")) == ["a", "b"]
    missing = str(tmp_path / "none.pth")
    for what in ("LPIPS", "DISTS", "Inception"):
        with pytest.raises(FileNotFoundError) as e:
            tower.load_state_file(missing, what)
        assert str(e.value) == f"{what} weights not found: {missing}"
    from rdeic_amd import fid as F
    for load, what in ((lambda p: L.load_lin("alex", p), "LPIPS"), (D.load_weights, "DISTS"),
                       (F.load_inception, "Inception")):
        with pytest.raises(FileNotFoundError) as e:
            load(missing)
        assert str(e.value) == f"{what} weights not found: {missing}"


# VGG's 64-channel full-size maps decide: 2048 x 2048 is exactly 2^30 bytes per image, the first size at which a pair
# does not fit; 2897 x 2897 is the first square whose single image passes 2^31 bytes; at 8 x 8 DISTS's MAX_PAIRS caps
# (image_bytes below confirms each)
SIZES = [(8, 8), (16, 16), (31, 31), (35, 47), (96, 80), (512, 768), (2047, 2048), (2048, 2048), (2896, 2896),
         (2897, 2897)]


def test_size_rules_agree_with_the_delegations():
    assert tower.MAX_TENSOR_BYTES == L.MAX_TENSOR_BYTES == D.MAX_TENSOR_BYTES == 2 ** 31
    seen = set()
    rules = [(lambda h, w: L.image_bytes("vgg", h, w), lambda h, w: L.chunk_pairs("vgg", h, w),
              lambda h, w: L.split_pair("vgg", h, w), None, "LPIPS(vgg)", L.MIN_SIZE["vgg"]),
             (lambda h, w: L.image_bytes("alex", h, w), lambda h, w: L.chunk_pairs("alex", h, w),
              lambda h, w: L.split_pair("alex", h, w), None, "LPIPS(alex)", L.MIN_SIZE["alex"]),
             (D.image_bytes, D.chunk_pairs, D.split_pair, D.MAX_PAIRS, "DISTS", 1)]
    for image_bytes, chunk_pairs, split_pair, cap, who, min_size in rules:
        for h, w in SIZES:
            if h < min_size:
                continue
            per = image_bytes(h, w)
            if per >= 2 ** 31:
                seen.add("refused")
                with pytest.raises(ValueError, match=f"{h}x{w}: one image's activation reaches 2\\^31 bytes"):
                    chunk_pairs(h, w)
                with pytest.raises(ValueError, match="reaches 2\\^31 bytes"):
                    tower.chunk_pairs(per, cap)
                assert split_pair(h, w) and tower.split_pair(per)
                continue
            want = max(1, ((2 ** 31 - 1) // per) // 2)  # the rule, restated
            want = want if cap is None else min(cap, want)
            assert chunk_pairs(h, w) == tower.chunk_pairs(per, cap) == want, (who, h, w)
            assert split_pair(h, w) == tower.split_pair(per) == (2 * per >= 2 ** 31), (who, h, w)
            seen.add("split" if split_pair(h, w) else "whole")
            if who == "DISTS" and want == cap:
                seen.add("capped")
    assert seen == {"refused", "split", "whole", "capped"}
    assert not D.split_pair(2047, 2048) and D.split_pair(2048, 2048)  # where it turns
