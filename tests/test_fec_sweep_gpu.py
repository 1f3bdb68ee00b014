"""The robustness sweep over protected streams on the device (synthetic weights): rows that recover are the clean
sweep's rows, rows that do not are failure rows the entropy decoder never saw, the library agrees with the plain-Python
restatement about which is which, the unprotected sweep at the same rate is worse, and inference.process round-trips
through a protected file."""
import numpy as np
import pytest
import torch

from rdeic_amd import fec
from rdeic_amd import robustness as R
from tests import fec_ref

pytestmark = pytest.mark.gpu

H, W = 192, 256  # the size of the existing sweep test: SSIM needs 176 pixels
SEEDS = [231, 232, 233]
SPEC = "rs:32:4"
# the corruptors flip int(8 * bytes * rate) bits. R_LO: 0.2 % of the bits is about 4 byte errors per 255-byte codeword
# (a handful in all in a stream of one short codeword), far inside t = 16: P(Bin(255, 0.016) > 16) < 1e-5. R_HI: 5 % of
# the bits hits a third of the bytes, 85 of 255 and 5 times t: no codeword survives (the tail at 2 % is 0.999 already).
R_LO, R_HI = 0.002, 0.05
METRICS = ("psnr", "ssim", "ms_ssim", "lpips", "decode_failed")
KW = dict(steps=2, sampler="ddim", noise_seed=77, batch_size=4)


@pytest.fixture(scope="module")
def setup(gpu):
    from rdeic_amd.rdeic import RDEIC
    from rdeic_amd.synthetic import synth_context, synth_image
    # rate_gain 1.0: bodies of several KB, so the protected stream has many codewords and several interleave groups
    m = RDEIC(compute_dtype=torch.float32).init_synthetic(rate_gain=1.0)
    img = torch.from_numpy(np.stack([synth_image(H, W, 231 + i) for i in range(2)])).cuda()
    ctx = synth_context().cuda()
    bodies = m.compress_images(img)
    clean = R.run_robustness(m, img, ctx, "bitstream", "random", [0.0, 0.0], SEEDS, bodies=bodies, **KW)
    return m, img, ctx, bodies, clean


def _expected(bodies, rates):
    """(recoverable, corrupted byte count) per (image, rate, seed) in the sweep's order, from the restatement alone"""
    p = fec.parse_fec(SPEC)
    out = []
    for body in bodies:
        stream = fec_ref.protect(body, p.nroots, p.depth)
        for rate in rates:
            for seed in SEEDS:
                bad = R.Corruptor("bitstream", "random", rate, seed).corrupt_bytes(stream)
                errs = fec_ref.errors_per_codeword(stream, bad, p.nroots, p.depth, len(body))
                out.append((fec_ref.recoverable(stream, bad, p.nroots, p.depth, len(body)), sum(errs)))
    return out


def test_recovered_rows_are_the_clean_sweeps_rows(setup):
    m, img, ctx, bodies, clean = setup
    recs = R.run_robustness(m, img, ctx, "bitstream", "random", [0.0, R_LO], SEEDS, bodies=bodies, fec=SPEC, **KW)
    want = _expected(bodies, [0.0, R_LO])
    assert len(recs) == len(clean) == len(want) == 12 and all(ok for ok, _ in want)
    print(f"\n[fec sweep] bodies {[len(b) for b in bodies]} bytes; corrected at {R_LO}: "
          f"{[r['fec_corrected'] for r in recs if r['error_rate'] > 0]}; clean psnr {clean[0]['psnr']:.2f}")
    for r, c, (ok, nerr), i in zip(recs, clean, want, [0] * 6 + [1] * 6):
        assert list(r) == R.COLUMNS + R.FEC_COLUMNS and "error" not in r
        # same job count, every payload clean: the noise rule gives every job the noise it has in the clean sweep
        assert not r["decode_failed"] and {k: r[k] for k in METRICS} == {k: c[k] for k in METRICS}
        size = fec.parse_fec(SPEC).encoded_size(len(bodies[i]))
        assert size == len(fec.protect(bodies[i], SPEC)) == 46 + len(bodies[i]) + 32 * -(-len(bodies[i]) // 223)
        assert r["bpp"] == 8.0 * size / (H * W) and r["bpp_payload"] == c["bpp"] == 8.0 * len(bodies[i]) / (H * W)
        assert r["fec"] == "rs:32:4" and r["fec_failed"] == 0 and r["fec_corrected"] == nerr
        assert (r["fec_corrected"] > 0) == (r["error_rate"] > 0)
        assert r["image_id"] == c["image_id"] and r["seed"] == c["seed"]


def test_unrecoverable_rows_are_failure_rows_and_the_library_agrees_with_the_restatement(setup):
    m, img, ctx, bodies, clean = setup
    recs = R.run_robustness(m, img, ctx, "bitstream", "random", [R_LO, R_HI], SEEDS, bodies=bodies, fec=SPEC, **KW)
    want = _expected(bodies, [R_LO, R_HI])
    assert [r["fec_failed"] for r in recs] == [int(not ok) for ok, _ in want]  # the library agrees, row by row
    assert any(ok for ok, _ in want) and any(not ok for ok, _ in want)  # and both kinds occur
    for r, (ok, nerr) in zip(recs, want):
        assert ok == (r["error_rate"] == R_LO * 100)
        if ok:
            assert not r["decode_failed"] and r["psnr"] > 0.0 and r["fec_corrected"] == nerr and "error" not in r
            continue
        assert r["decode_failed"] and (r["psnr"], r["ssim"], r["ms_ssim"], r["lpips"]) == (0.0, 0.0, 0.0, 1.0)
        assert r["error"].startswith("FecError: rdeic_fec_decode failed: -74") and "0x" not in r["error"]
    again = R.run_robustness(m, img, ctx, "bitstream", "random", [R_LO, R_HI], SEEDS, bodies=bodies, fec=SPEC, **KW)
    assert again == recs
    with pytest.raises(ValueError, match="latent"):
        R.run_robustness(m, img, ctx, "latent", "additive", [0.0], SEEDS, bodies=bodies, fec=SPEC, **KW)


def test_the_unprotected_sweep_at_the_low_rate_is_worse(setup):
    m, img, ctx, bodies, clean = setup
    recs = R.run_robustness(m, img, ctx, "bitstream", "random", [0.0, R_LO], SEEDS, bodies=bodies, **KW)
    assert all(list(r)[:11] == R.COLUMNS and not set(r) & set(R.FEC_COLUMNS) for r in recs)
    hit = [r for r in recs if r["error_rate"] > 0]
    floor = min(r["psnr"] for r in recs if r["error_rate"] == 0)
    print(f"\n[fec sweep] unprotected at {R_LO}: {sum(r['decode_failed'] for r in hit)} of {len(hit)} failed, psnr "
          f"{[round(r['psnr'], 2) for r in hit]} against a clean floor of {floor:.2f}")
    assert any(r["decode_failed"] or r["psnr"] < floor for r in hit)


def test_inference_process_round_trips_through_a_protected_file(setup, tmp_path):
    import inference
    from rdeic_amd.synthetic import synth_image
    m, img, ctx, bodies, clean = setup
    x = synth_image(H, W, 231)
    outs = {}
    for name, kw in (("plain", {}), ("fec", {"fec": SPEC}), ("params", {"fec": fec.FecParams(32, 4)})):
        gen = torch.Generator().manual_seed(231)
        preds, bpp = inference.process(m, [x], "ddim", 2, str(tmp_path / name), 1.0, [ctx], gen, **kw)
        outs[name] = (preds[0], bpp, (tmp_path / name).read_bytes())
    body = outs["plain"][2]
    assert outs["fec"][2] == outs["params"][2] == fec.protect(body, SPEC) and fec.recover(outs["fec"][2])[0] == body
    assert len(outs["fec"][2]) == 46 + len(body) + 32 * -(-len(body) // 223)
    assert outs["plain"][1] == 8.0 * len(body) / (H * W) and outs["fec"][1] == 8.0 * len(outs["fec"][2]) / (H * W)
    assert np.array_equal(outs["fec"][0], outs["plain"][0]) and np.array_equal(outs["params"][0], outs["plain"][0])
    # protection is said, never detected: a plain body read as a protected stream is refused on the host
    with pytest.raises(fec.FecError):
        m.apply_condition_decompress(str(tmp_path / "plain"), fec=SPEC)
    # a damaged protected file is repaired on the way in
    bad = R.bit_flip_bytes(outs["fec"][2], R_LO, 231)
    (tmp_path / "bad").write_bytes(bad)
    a, b = m.apply_condition_decompress(str(tmp_path / "bad"), fec=SPEC)
    c, d = m.apply_condition_decompress(str(tmp_path / "fec"), fec=SPEC)
    assert bad != outs["fec"][2] and torch.equal(a, c) and torch.equal(b, d)
