"""The host side of the robustness sweep: the per-stream status decode (rdeic_rans_decode_batch_status), the
threshold / summary tables against the reference's published indicators (tests/golden/robustness_tables/, recorded
results of the reference's own runs), the NHWC latent corruption order, the JPEG2000 baseline with host PSNR, and the
two CLIs' argument parsing."""
import os

import numpy as np
import pytest
import torch

from rdeic_amd import coders
from rdeic_amd import robustness as R

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TABLES = os.path.join(GOLD, "robustness_tables")
PAIRS = [("robustness_results.csv", "bitstream_random_failure_thresholds.csv"),
         ("robustness_bitstream_burst.csv", "bitstream_burst_failure_thresholds.csv"),
         ("robustness_latent_additive.csv", "latent_additive_failure_thresholds.csv")]


# ------------------------------------------------------------------ tables
@pytest.mark.parametrize("results,published", PAIRS)
def test_failure_thresholds_match_the_published_tables(results, published):
    import csv
    rows = R.failure_thresholds(R.read_csv(os.path.join(TABLES, results)))
    with open(os.path.join(TABLES, published), newline="") as f:
        want = list(csv.DictReader(f))
    assert [r["metric"] for r in rows] == [w["metric"] for w in want] == ["psnr", "ssim", "ms_ssim", "lpips"]
    for r, w in zip(rows, want):
        assert r["threshold"] == float(w["threshold"])
        if w["failure_rate"] == ">10%":
            assert r["failure_rate"] == ">10%"
        else:
            assert r["failure_rate"] == float(w["failure_rate"])
        assert abs(r["metric_at_failure"] - float(w["metric_at_failure"])) <= 1e-9 * abs(float(w["metric_at_failure"]))


def test_threshold_files_are_written_as_published(tmp_path):
    recs = R.read_csv(os.path.join(TABLES, "robustness_latent_additive.csv"))
    R.write_failure_thresholds(recs, str(tmp_path), prefix="latent_additive_")
    import csv
    with open(tmp_path / "latent_additive_failure_thresholds.csv", newline="") as f:
        got = list(csv.DictReader(f))
    with open(os.path.join(TABLES, "latent_additive_failure_thresholds.csv"), newline="") as f:
        want = list(csv.DictReader(f))
    assert [(g["metric"], g["threshold"], g["failure_rate"]) for g in got] == \
        [(w["metric"], w["threshold"], w["failure_rate"]) for w in want]
    txt = (tmp_path / "latent_additive_failure_thresholds.txt").read_text()
    assert txt.startswith("RDEIC Robustness Failure Thresholds\n" + "=" * 50 + "\n\nPSNR:\n  Threshold: 25.0\n")
    assert "LPIPS:\n  Threshold: 0.3\n  Failure at: >10%% error rate\n  Value at failure: 0.2709\n" in txt


@pytest.mark.parametrize("results", [p[0] for p in PAIRS])
def test_summary_by_rate_is_the_groupby(results):
    recs = R.read_csv(os.path.join(TABLES, results))
    rates = sorted({r["error_rate"] for r in recs})
    table = R.summary_by_rate(recs)
    assert [row["error_rate"] for row in table] == rates and len(rates) >= 6
    for row in table:
        sel = [r for r in recs if r["error_rate"] == row["error_rate"]]
        assert row["decode_failed"] == sum(r["decode_failed"] for r in sel)
        for m in ("psnr", "ssim", "ms_ssim", "lpips"):
            v = np.array([r[m] for r in sel], dtype=np.float64)
            v = v[~np.isnan(v)]
            assert np.isclose(row[m][0], v.mean(), rtol=1e-12, atol=0)
            assert np.isclose(row[m][1], np.sqrt(((v - v.mean()) ** 2).sum() / (v.size - 1)), rtol=1e-9, atol=1e-15)
    assert len(R.format_summary(recs).splitlines()) == 1 + len(rates)


def test_summary_skips_nan_and_none():
    recs = [{"error_rate": 0.0, "psnr": 30.0, "ssim": float("nan"), "ms_ssim": None, "lpips": 0.1, "decode_failed": False},
            {"error_rate": 0.0, "psnr": 20.0, "ssim": 0.5, "ms_ssim": None, "lpips": 0.2, "decode_failed": True}]
    (row,) = R.summary_by_rate(recs)
    assert row["psnr"] == (25.0, float(np.std([30.0, 20.0], ddof=1))) and row["decode_failed"] == 1
    assert row["ssim"][0] == 0.5 and np.isnan(row["ssim"][1])
    assert np.isnan(row["ms_ssim"][0]) and np.isnan(row["ms_ssim"][1])
    thr = {r["metric"]: r for r in R.failure_thresholds(recs)}
    assert thr["psnr"]["failure_rate"] == ">10%" and thr["psnr"]["metric_at_failure"] == 25.0
    assert thr["ssim"]["failure_rate"] == 0.0 and thr["ssim"]["metric_at_failure"] == 0.5


def test_records_csv_round_trip(tmp_path):
    recs = [{"image_id": "a", "error_space": "bitstream", "error_type": "random", "error_rate": 0.5, "seed": 231,
             "bpp": 0.125, "psnr": 21.5, "ssim": float("nan"), "ms_ssim": 0.75, "lpips": None, "decode_failed": False,
             "dists": 0.25, "error": "dropped"}]
    R.write_records_csv(recs, str(tmp_path / "r.csv"))
    text = (tmp_path / "r.csv").read_text().splitlines()
    assert text[0] == "image_id,error_space,error_type,error_rate,seed,bpp,psnr,ssim,ms_ssim,lpips,dists,decode_failed"
    (back,) = R.read_csv(str(tmp_path / "r.csv"))
    assert back["seed"] == 231 and back["decode_failed"] is False and back["psnr"] == 21.5 and back["dists"] == 0.25
    assert np.isnan(back["ssim"]) and np.isnan(back["lpips"])


# ------------------------------------------------------------------ status decode
@pytest.fixture(scope="module")
def streams():
    t = coders.GaussianTables()
    rng = np.random.default_rng(17)
    count, n = 4, 1500  # two stages of 750 symbols per stream
    idx = rng.integers(0, t.levels, size=(count, n), dtype=np.int32)
    sym = np.rint(rng.standard_normal((count, n)) * t.scale_table.numpy()[idx]).astype(np.int32)
    return t, idx, sym, coders.rans_encode_batch(sym, idx, t, threads=2)


def _flip_until_bad(t, idx, data):
    """Flip more and more bits (fixed seeds) until the stream reports EBADMSG over all of its symbols."""
    for seed in range(200):
        bad = R.bit_flip_bytes(data, 0.02, seed)
        d = coders.RansDecoder(bad)
        status = np.zeros(1, dtype=np.int32)
        coders.rans_decode_batch([d], idx[None], t, status=status)
        d.close()
        if status[0] == -74:
            return bad
    raise AssertionError("no flipped stream failed")


def test_status_decode_isolates_failed_streams(streams):
    t, idx, sym, enc = streams
    n, half = idx.shape[1], idx.shape[1] // 2
    trunc = enc[1][:len(enc[1]) // 2 + 1]
    while len(trunc) % 4 == 0:
        trunc = trunc[:-1]
    flipped = _flip_until_bad(t, idx[2], enc[2])
    datas = [enc[0], trunc, flipped, enc[3]]
    ref_decs = [coders.RansDecoder(enc[i]) for i in (0, 3)]
    decs = [coders.RansDecoder(d) for d in datas]
    try:
        status = np.zeros(4, dtype=np.int32)
        out1 = np.full((4, half), 7, dtype=np.int32)  # stale values the call has to overwrite
        first = np.ascontiguousarray(idx[:, :half])
        coders.rans_decode_batch(decs, first, t, out=out1, status=status)
        ref1 = coders.rans_decode_batch(ref_decs, np.ascontiguousarray(idx[[0, 3], :half]), t)
        assert status[0] == 0 and status[3] == 0
        assert status[1] == -74  # a length that is no multiple of 4 is bad from the first symbol on
        assert np.array_equal(out1[[0, 3]], ref1) and np.array_equal(ref1, sym[[0, 3], :half])
        assert not out1[1].any()
        if status[2] != 0:
            assert not out1[2].any()
        # second stage: the failed streams stay skipped, the clean ones continue where they were
        after_first = status.copy()
        out2 = np.full((4, n - half), 7, dtype=np.int32)
        second = np.ascontiguousarray(idx[:, half:])
        coders.rans_decode_batch(decs, second, t, out=out2, status=status)
        ref2 = coders.rans_decode_batch(ref_decs, np.ascontiguousarray(idx[[0, 3], half:]), t)
        assert np.array_equal(out2[[0, 3]], ref2) and np.array_equal(ref2, sym[[0, 3], half:])
        assert status[0] == 0 and status[3] == 0 and status[1] == -74 and status[2] == -74
        assert after_first[2] in (0, -74) and not out2[1].any() and not out2[2].any()
        # a stream that is marked failed on entry is not decoded, whatever its handle holds
        fresh = coders.RansDecoder(enc[0])
        marked = np.array([-22], dtype=np.int32)
        out3 = np.full((1, half), 7, dtype=np.int32)
        coders.rans_decode_batch([fresh], first[:1], t, out=out3, status=marked)
        assert marked[0] == -22 and not out3.any()
        marked[0] = 0
        coders.rans_decode_batch([fresh], first[:1], t, out=out3, status=marked)  # its state was not advanced
        assert marked[0] == 0 and np.array_equal(out3[0], sym[0, :half])
        fresh.close()
    finally:
        for d in decs + ref_decs:
            d.close()


def test_status_decode_null_handle_and_bad_index(streams):
    t, idx, sym, enc = streams
    d = coders.RansDecoder(enc[0])
    try:
        two = np.ascontiguousarray(idx[[1, 0], :100])  # row 1 holds stream 0's own indexes
        two[1, 50] = t.levels  # an index outside the tables: that stream's own EINVAL
        status = np.zeros(2, dtype=np.int32)
        out = np.full((2, 100), 7, dtype=np.int32)
        coders.rans_decode_batch([None, d], two, t, out=out, status=status)
        assert status[0] == 0 and not out[0].any()  # no decoder: skipped, zeros, status untouched
        assert status[1] == -22 and not out[1].any()
        with pytest.raises(ValueError):
            coders.rans_decode_batch([d], two[:1], t, status=np.zeros(1, dtype=np.int64))
    finally:
        d.close()
    # the unchanged call still raises for the batch
    bad = coders.RansDecoder(enc[1][:7])
    with pytest.raises(ValueError):
        coders.rans_decode_batch([bad], np.ascontiguousarray(idx[:1, :10]), t)
    bad.close()


# ------------------------------------------------------------------ latent layout
def test_nhwc_latent_corruption_is_the_reference_order():
    g = np.load(os.path.join(GOLD, "corruptors.npz"))
    import re
    cases = sorted({k.split("_")[0] for k in g.files if re.match(r"lat\d+_", k)})
    seeds = sorted({int(g[c + "_seed"]) for c in cases}) + [231]
    assert cases
    nchw = torch.from_numpy(g["latent"]).float()
    if nchw.dim() == 3:
        nchw = nchw[None]
    nhwc = nchw.permute(0, 2, 3, 1).contiguous()
    for mode in ("mask_replace", "additive"):
        for seed in seeds:
            for rate in (0.0, 0.05, 0.5):
                want = R.latent_corrupt(nchw, mode, rate, seed).permute(0, 2, 3, 1)
                got = R.corrupt_latent_nhwc(nhwc, mode, rate, seed)
                assert got.shape == nhwc.shape and got.is_contiguous() and torch.equal(got, want), (mode, seed, rate)
                if rate:
                    assert not torch.equal(got, nhwc)
                    # corrupting the NHWC tensor as it lies in memory puts the draws on other elements
                    assert not torch.equal(R.latent_corrupt(nhwc, mode, rate, seed), want)


def test_error_pairs():
    for space, kind in (("bitstream", "random"), ("bitstream", "burst"), ("latent", "mask_replace"),
                        ("latent", "additive")):
        R.check_error_pair(space, kind)
    for space, kind in (("bitstream", "additive"), ("bitstream", "mask_replace"), ("latent", "random"),
                        ("latent", "burst"), ("pixels", "random")):
        with pytest.raises(ValueError):
            R.check_error_pair(space, kind)


# ------------------------------------------------------------------ JPEG2000
def _need_j2k():
    from rdeic_amd import jpeg2000 as J
    if not J.available():
        pytest.skip("Pillow without OpenJPEG")
    return J


@pytest.fixture(scope="module")
def j2k_run():
    J = _need_j2k()
    from rdeic_amd.synthetic import synth_image
    img = synth_image(256, 384, 231)
    kw = dict(target_bpp=0.5, error_type="random", rates=[0.0, 0.001, 0.1], seeds=list(range(231, 236)))
    return J, img, J.run_jpeg2000_robustness([img], ["synth"], **kw), J.run_jpeg2000_robustness([img], ["synth"], **kw)


def test_jpeg2000_rows(j2k_run):
    J, img, recs, again = j2k_run
    assert len(recs) == 15 and all(list(r)[:11] == J.COLUMNS for r in recs)
    assert [(r["error_rate"], r["seed"]) for r in recs] == [(p, s) for p in (0.0, 0.1, 10.0) for s in range(231, 236)]
    bpp = recs[0]["bpp"]
    print(f"\n[jpeg2000] achieved {bpp:.4f} bpp for a target of 0.5; decoded rows per rate: "
          f"{[sum(not r['decode_failed'] for r in recs if r['error_rate'] == p) for p in (0.0, 0.1, 10.0)]}")
    assert 0.9 * 0.5 <= bpp <= 1.02 * 0.5 and all(r["bpp"] == bpp for r in recs)
    clean = [r for r in recs if r["error_rate"] == 0.0]
    assert all(not r["decode_failed"] and "error" not in r for r in clean)
    assert all({k: r[k] for k in r if k != "seed"} == {k: clean[0][k] for k in clean[0] if k != "seed"} for r in clean)
    assert 10.0 < clean[0]["psnr"] < 100.0
    for r in recs:
        if r["error_rate"] == 10.0:
            assert r["decode_failed"] and r["psnr"] == 0.0 and r["lpips"] == 1.0 and r["ssim"] == r["ms_ssim"] == 0.0
        if r["decode_failed"]:
            assert r["psnr"] == 0.0 and r["lpips"] == 1.0 and r["error"] and " at 0x" not in r["error"]
    # two runs, the same records, the error texts included (the NaN columns are one object, equal by identity)
    assert recs == again


def test_jpeg2000_unrecognisable_stream_fails_with_a_fixed_text():
    J = _need_j2k()
    from PIL import UnidentifiedImageError
    texts = set()
    for _ in range(3):
        with pytest.raises(UnidentifiedImageError) as e:
            J.decode(bytes(range(256)) * 4, 10 ** 6)
        texts.add(str(e.value))
    assert texts == {"cannot identify the codestream"}


def test_jpeg2000_codec_round_trip_and_oversize_header():
    J = _need_j2k()
    import struct
    from rdeic_amd.synthetic import synth_image
    img = synth_image(64, 96, 5)
    data = J.encode(img, 4.0)
    assert data[:2] == b"\xff\x4f" and J.siz_size(data) == (64, 96)
    dec = J.decode(data, 4 * 64 * 96)
    assert dec.shape == img.shape and dec.dtype == np.uint8 and R.psnr_u8(dec, img) > 25.0
    # SIZ fields patched to 4x the height and a little more width: over 4x the pixels, refused before the decode
    big = data[:8] + struct.pack(">2I", 100, 4 * 64) + data[16:]
    assert J.siz_size(big) == (256, 100)
    with pytest.raises(ValueError, match="header announces"):
        J.decode(big, 4 * 64 * 96)
    huge = data[:8] + struct.pack(">2I", 20000, 20000) + data[16:]
    with pytest.raises(ValueError, match="header announces"):
        J.decode(huge, 4 * 64 * 96)
    # exactly 4x is not over the limit: the guard lets it through to the decoder (which may refuse it itself)
    assert J.siz_size(data[:8] + struct.pack(">2I", 96, 256) + data[16:]) == (256, 96)
    assert J.siz_size(b"\x00" * 40) is None

    def rows(patched):
        orig = J.encode
        J.encode = lambda im, bpp: patched
        try:
            return J.run_jpeg2000_robustness([img], ["x"], 4.0, "random", [0.0], [1])
        finally:
            J.encode = orig

    (row,) = rows(huge)
    assert row["decode_failed"] and row["psnr"] == 0.0 and row["lpips"] == 1.0 and "header announces" in row["error"]
    (row,) = rows(data)
    assert not row["decode_failed"] and row["psnr"] == min(R.psnr_u8(dec, img), 100.0)


# ------------------------------------------------------------------ CLI parsing
def test_run_robustness_cli_defaults_are_the_references():
    import run_robustness as cli
    a = cli.parse_args(["--data", "x"])
    want = dict(error_space="bitstream", error_type="random", rates="0,0.1,0.5,1,2,5,10", num_seeds=5, burst_len=8.0,
                sampler="ddpm", steps=2, guidance_scale=1.0, output_csv="indicators/robustness_results.csv",
                cache_dir="encodings/", recon_dir="outputs/robustness/", save_recon=False, force_encode=False, seed=231,
                device="cuda", suppress_warnings=False)
    assert {k: getattr(a, k) for k in want} == want
    assert a.rate_list == [0.0, 0.001, 0.005, 0.01, 0.02, 0.05, 0.1]
    assert a.batch_size == 8 and a.dtype == "fp32" and a.ckpt == "" and a.thresholds_dir == ""
    a = cli.parse_args(["--data", "x", "--error_space", "latent", "--error_type", "additive", "--rates", "0,2"])
    assert (a.error_space, a.error_type, a.rate_list) == ("latent", "additive", [0.0, 0.02])


@pytest.mark.parametrize("space,kind", [("bitstream", "additive"), ("bitstream", "mask_replace"), ("latent", "random"),
                                        ("latent", "burst")])
def test_run_robustness_cli_refuses_invalid_pairs(space, kind, capsys):
    import run_robustness as cli
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["--data", "x", "--error_space", space, "--error_type", kind])
    assert e.value.code == 2 and kind in capsys.readouterr().err


def test_run_jpeg2000_cli_defaults_are_the_references(capsys):
    import run_jpeg2000_robustness as cli
    a = cli.parse_args(["--data", "x"])
    want = dict(target_bpp=0.12, error_type="random", rates="0,0.1,0.5,1,2,5,10", num_seeds=5, burst_len=8.0,
                output_csv="indicators/jpeg2000_robustness.csv", output_dir="outputs/jpeg2000_robustness/",
                save_recon=False, seed=231)
    assert {k: getattr(a, k) for k in want} == want
    with pytest.raises(SystemExit):
        cli.parse_args(["--data", "x", "--error_type", "additive"])
    capsys.readouterr()
