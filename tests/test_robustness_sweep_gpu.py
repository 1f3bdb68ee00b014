"""The batched robustness sweep on the device (synthetic weights): fault isolation of the batched entropy decode,
run_robustness against run_bitstream_robustness, the latent error space, and the run_robustness.py CLI."""
import csv
import functools
import math
import os

import numpy as np
import pytest
import torch

from rdeic_amd import robustness as R

pytestmark = pytest.mark.gpu

COLUMNS = ["image_id", "error_space", "error_type", "error_rate", "seed", "bpp", "psnr", "ssim", "ms_ssim", "lpips",
           "decode_failed"]


def _model(dtype=torch.float32, rate_gain=0.4):
    from rdeic_amd.rdeic import RDEIC
    return RDEIC(compute_dtype=dtype).init_synthetic(rate_gain=rate_gain)


def _images(h, w, n, seed=231):
    from rdeic_amd.synthetic import synth_image
    return torch.from_numpy(np.stack([synth_image(h, w, seed + i) for i in range(n)])).cuda()


# (rate, seed) of the four bit-flipped bodies, fixed after a run on an MI355X. Alone, in fp32 / bf16: the first decodes
# in both, the second fails in a rANS stage in both (BitstreamError), the third fails in a stage in fp32 and decodes in
# bf16, the fourth has its string count flipped in both (IndexError before any device work).
FLIPS = ((0.0001, 232), (0.001, 237), (0.0003, 233), (0.001, 232))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_isolated_decode_flags_what_fails_alone_and_keeps_the_survivors_bits(gpu, dtype):
    from rdeic_amd import _lib, bitstream
    # rate_gain 1.0: a 6 KB body, so that a flipped bit lands in the rANS stream and not in the 20 header bytes (at
    # rate_gain 0.4 the body has 56 bytes, and in a probe of 48 flipped variants none failed inside a stage)
    m = _model(dtype, rate_gain=1.0)
    bodies = m.compress_images(_images(128, 128, 2))
    body = bodies[0]
    shape0 = bitstream.unpack_body(body)[1]
    before = [t.clone() for t in m.decompress_bodies([body])]
    hdr = bytearray(body)
    hdr[0] ^= 0x80  # the header's first word (z height)
    batch = [body, body, body[:2 * len(body) // 3], bytes(hdr)]  # 2 clean, 1 truncated, 1 flipped header word
    batch += [R.Corruptor("bitstream", "random", rate, seed).corrupt_bytes(body)
              for rate, seed in FLIPS]
    assert len(batch) == 8 and len(set(batch)) == 7  # every corrupted body differs from the clean one and the others
    lat, hint, errors = m.decompress_bodies(batch, isolate=True, expect_shape=shape0)
    solo = [R.try_decompress(m, b, shape0) for b in batch]
    print(f"\n[isolate {dtype}] body {len(body)} bytes; alone: "
          f"{['fail' if isinstance(s, Exception) else 'ok' for s in solo]}")
    assert errors[0] is None and errors[1] is None and errors[2] is not None and isinstance(errors[3], ValueError)
    # the path this is about runs: a bit-flipped body fails inside a rANS stage (a nonzero status, zeros from there
    # on) next to a bit-flipped body that decodes, whose bits are compared with its solo decode below
    assert any(isinstance(e, _lib.BitstreamError) for e in errors[4:]) and any(e is None for e in errors[4:])
    assert lat.shape[0] == 8 and hint.shape[0] == 8 and torch.isfinite(lat).all() and torch.isfinite(hint.float()).all()
    for k, (s, e) in enumerate(zip(solo, errors)):
        assert isinstance(s, Exception) == (e is not None), (k, s, e)
        if e is None:
            assert torch.equal(lat[k:k + 1], s[0]) and torch.equal(hint[k:k + 1], s[1]), k
        else:
            assert type(e) is type(s), (k, s, e)
    # the decoder and its plans are intact: the clean body decodes to the bits it had before
    after = m.decompress_bodies([body])
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])
    # with nothing to isolate the batch is the plain batch
    clean = [bodies[k % 2] for k in range(8)]
    plain = m.decompress_bodies(clean)
    lat2, hint2, err2 = m.decompress_bodies(clean, isolate=True)
    assert err2 == [None] * 8 and torch.equal(lat2, plain[0]) and torch.equal(hint2, plain[1])
    assert torch.equal(lat2[0:1], before[0]) and torch.equal(hint2[0:1], before[1])
    # every body unparseable: no device work, every error reported
    none = m.decompress_bodies([body[:5], b""], isolate=True, expect_shape=shape0)
    assert none[0] is None and none[1] is None and all(isinstance(e, Exception) for e in none[2])
    # without expect_shape an implausible first header is that body's own failure, not the batch's
    lat3, hint3, err3 = m.decompress_bodies([bytes(hdr), body], isolate=True)
    assert isinstance(err3[0], ValueError) and "implausible" in str(err3[0]) and err3[1] is None
    assert torch.equal(lat3[1:2], before[0]) and torch.equal(hint3[1:2], before[1])


# Chosen on an MI355X so that the corrupted rows hold both outcomes (the test asserts it).
EQ_RATES = [0.0, 0.002, 0.02]
EQ_SEEDS = [231, 232, 233]


def test_run_robustness_equals_run_bitstream_robustness(gpu):
    from rdeic_amd.synthetic import synth_context
    m = _model()
    img = _images(192, 256, 2)
    ctx = synth_context().cuda()
    old = R.run_bitstream_robustness(m, img, ctx, "random", EQ_RATES, EQ_SEEDS, steps=2, sampler="ddim", noise_seed=77)
    new = R.run_robustness(m, img, ctx, "bitstream", "random", EQ_RATES, EQ_SEEDS, steps=2, sampler="ddim",
                           noise_seed=77, batch_size=4)
    assert len(old) == len(new) == 2 * 3 * 3
    corrupted = [r for r in old if r["error_rate"] > 0]
    print(f"\n[equivalence] corrupted rows failed: {[int(r['decode_failed']) for r in corrupted]}")
    for a, b in zip(old, new):
        assert list(a) == list(b), (a, b)
        for k in a:
            if k != "error":
                assert type(a[k]) is type(b[k]) and a[k] == b[k], (k, a, b)
    assert any(r["decode_failed"] for r in corrupted) and any(not r["decode_failed"] for r in corrupted)
    for r in new:
        if r["decode_failed"]:
            assert (r["psnr"], r["ssim"], r["ms_ssim"], r["lpips"]) == (0.0, 0.0, 0.0, 1.0) and r["error"]
        else:
            # a corrupted stream that decodes may decode to anything: only the clean rows have a quality to speak of
            assert math.isfinite(r["psnr"]) and r["psnr"] > 0.0 and "error" not in r
    for r in new:
        if r["error_rate"] == 0.0:
            # (the seeded synthetic weights reconstruct poorly: MS-SSIM's relu'd contrast term can be exactly 0)
            assert not r["decode_failed"] and r["psnr"] > 5.0 and math.isfinite(r["ssim"]) and 0.0 <= r["ms_ssim"] <= 1.0


@pytest.mark.parametrize("error_type", ["additive", "mask_replace"])
def test_latent_space_rows(gpu, error_type):
    from rdeic_amd import ops
    from rdeic_amd.synthetic import synth_context
    m = _model()
    img = _images(192, 256, 1)
    ctx = synth_context().cuda()
    kw = dict(steps=2, sampler="ddim", noise_seed=9, batch_size=4)
    recs = R.run_robustness(m, img, ctx, "latent", error_type, [0.0, 0.1], [231, 232, 233], **kw)
    assert len(recs) == 6 and not any(r["decode_failed"] for r in recs)
    assert all(list(r) == COLUMNS and r["error_space"] == "latent" and r["error_type"] == error_type for r in recs)
    # the clean decode with each job's own noise: what the rate-0 rows have to be
    body = m.compress_images(img)[0]
    c_lat, hint = m.decompress_bodies([body])
    noise = torch.randn((6, 4, 24, 32), generator=torch.Generator().manual_seed(9))
    for k in range(3):
        out = m.relay_decode_u8(c_lat, hint, ctx, ops.nchw_to_nhwc(noise[k:k + 1].cuda(), torch.float32), 2, "ddim")
        want = R.score_crop(out, img)
        assert recs[k]["error_rate"] == 0.0 and recs[k]["seed"] == 231 + k
        assert {key: recs[k][key] for key in want} == want, k
        assert recs[k]["bpp"] == 8.0 * len(body) / (192 * 256)
    for k in range(3, 6):
        assert recs[k]["error_rate"] == 10.0 and math.isfinite(recs[k]["psnr"]) and recs[k]["psnr"] > 0
        assert all(recs[k]["psnr"] != recs[j]["psnr"] for j in range(3))
    assert len({r["psnr"] for r in recs}) == 6
    assert R.run_robustness(m, img, ctx, "latent", error_type, [0.0, 0.1], [231, 232, 233], **kw) == recs


# ------------------------------------------------------------------ CLI
@pytest.fixture()
def one_model(monkeypatch):
    """Every run_robustness.main of this module shares one synthetic model (the load dominates a run)."""
    import inference
    monkeypatch.setattr(inference, "load_model", _load_once(inference.load_model))


@functools.lru_cache(maxsize=None)
def _load_once(load):
    return functools.lru_cache(maxsize=None)(load)


def _rows(path):
    with open(path, newline="") as f:
        r = csv.reader(f)
        header = next(r)
        return header, [dict(zip(header, row)) for row in r]


def test_run_robustness_cli(gpu, tmp_path, one_model, monkeypatch, capsys):
    import run_robustness as cli
    from PIL import Image
    from rdeic_amd.rdeic import RDEIC
    from rdeic_amd.synthetic import synth_image
    os.makedirs(tmp_path / "in")
    Image.fromarray(synth_image(192, 256, 50)).save(tmp_path / "in" / "a.png")
    Image.fromarray(synth_image(180, 250, 51)).save(tmp_path / "in" / "b.png")  # padded to 192x256, cropped back
    base = ["--data", str(tmp_path / "in"), "--rates", "0,2", "--num_seeds", "2", "--cache_dir", str(tmp_path / "enc"),
            "--batch_size", "4"]
    recs = cli.main(base + ["--output_csv", str(tmp_path / "o1" / "r.csv"), "--save_recon", "--recon_dir",
                            str(tmp_path / "recon")])
    assert "Encoded 2 images" in capsys.readouterr().out
    header, rows = _rows(tmp_path / "o1" / "r.csv")
    assert header == COLUMNS and len(rows) == len(recs) == 8
    assert [(r["image_id"], float(r["error_rate"]), int(r["seed"])) for r in rows] == \
        [(i, p, s) for i in ("a", "b") for p in (0.0, 2.0) for s in (231, 232)]
    for r in rows:
        nbytes = (tmp_path / "enc" / r["image_id"]).stat().st_size
        assert abs(float(r["bpp"]) - 8.0 * nbytes / (192 * 256)) < 1e-12
        assert (r["error_space"], r["error_type"]) == ("bitstream", "random")
        if r["decode_failed"] == "True":
            assert (float(r["psnr"]), float(r["ssim"]), float(r["ms_ssim"]), float(r["lpips"])) == (0, 0, 0, 1)
            continue
        assert r["lpips"] == "nan" and math.isfinite(float(r["psnr"])) and math.isfinite(float(r["ssim"]))
        # 180 rows are no multiple of 16: SSIM alone, as ood.score_image has it
        assert math.isfinite(float(r["ms_ssim"])) == (r["image_id"] == "a")
        recon = tmp_path / "recon" / r["image_id"] / f"r_{float(r['error_rate']):.1f}" / f"seed_{r['seed']}" / "recon.png"
        assert np.array(Image.open(recon)).shape == ((192, 256, 3) if r["image_id"] == "a" else (180, 250, 3))
    assert all(r["decode_failed"] == "False" for r in rows if float(r["error_rate"]) == 0.0)

    # a second run decodes from the cached streams: the encoder is not called, the table is the same
    def no_encode(self, img):
        raise AssertionError("the cached stream was encoded again")

    with monkeypatch.context() as mp:
        mp.setattr(RDEIC, "compress_images", no_encode)
        cli.main(base + ["--output_csv", str(tmp_path / "o2" / "r.csv")])
    assert "Encoded 0 images" in capsys.readouterr().out
    assert (tmp_path / "o2" / "r.csv").read_bytes() == (tmp_path / "o1" / "r.csv").read_bytes()

    lat = cli.main(base + ["--output_csv", str(tmp_path / "o3" / "r.csv"), "--error_space", "latent", "--error_type",
                           "additive", "--thresholds_dir", str(tmp_path / "thr")])
    assert len(lat) == 8 and not any(r["decode_failed"] for r in lat)
    header, rows = _rows(tmp_path / "o3" / "r.csv")
    assert header == COLUMNS and {r["error_space"] for r in rows} == {"latent"}
    _, thr = _rows(tmp_path / "thr" / "latent_additive_failure_thresholds.csv")
    assert [t["metric"] for t in thr] == ["psnr", "ssim", "ms_ssim", "lpips"]
    assert (tmp_path / "thr" / "latent_additive_failure_thresholds.txt").read_text().startswith("RDEIC Robustness")
    assert "=== Summary ===" in capsys.readouterr().out
