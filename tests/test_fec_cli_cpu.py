"""Protected streams in the command-line tools, host side: the --fec spec, what the CLIs refuse at start-up, the
JPEG2000 baseline under protection (host scoring), and the tables' extra columns."""
import numpy as np
import pytest

from rdeic_amd import fec
from rdeic_amd import robustness as R


def test_parse_fec_accepts_and_refuses():
    assert fec.parse_fec("rs:32") == fec.FecParams(32, 1)
    assert fec.parse_fec("rs:32:4") == fec.FecParams(32, 4)
    assert fec.parse_fec(" rs:2:255 ") == fec.FecParams(2, 255)
    assert fec.parse_fec("rs:64").spec == "rs:64:1" and fec.parse_fec(fec.FecParams(16, 8).spec) == fec.FecParams(16, 8)
    assert fec.as_params(None) is None and fec.as_params("rs:16:2") == fec.FecParams(16, 2)
    assert fec.as_params(fec.FecParams(8)) == fec.FecParams(8, 1)
    for bad in ("", "rs", "rs:", "rs:31", "rs:0", "rs:66", "rs:32:0", "rs:32:256", "rs:32:4:1", "ldpc:32", "32:4",
                "rs:a", "rs:32:b", "rs:3.5", "RS:32", "rs:-2"):
        with pytest.raises(ValueError) as e:
            fec.parse_fec(bad)
        assert repr(bad) in str(e.value) and ("rs:NROOTS" in str(e.value) or "from" in str(e.value)), bad
    with pytest.raises(ValueError):
        fec.protect(b"abc", None)


def test_clis_refuse_at_start_up(capsys):
    import inference
    import run_jpeg2000_robustness as j2k_cli
    import run_robustness as cli
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["--data", "x", "--fec", "rs:32", "--error_space", "latent", "--error_type", "additive"])
    assert e.value.code == 2 and "latent" in capsys.readouterr().err
    for parse, base in ((cli.parse_args, ["--data", "x"]), (j2k_cli.parse_args, ["--data", "x"]),
                        (inference.parse_args, ["--input", "x"])):
        with pytest.raises(SystemExit) as e:
            parse(base + ["--fec", "rs:33"])
        assert e.value.code == 2 and "rs:33" in capsys.readouterr().err
        assert parse(base + ["--fec", "rs:32:4"]).fec_params == fec.FecParams(32, 4)
        a = parse(base)
        assert a.fec == "" and a.fec_params is None
    a = cli.parse_args(["--data", "x", "--fec", "rs:16", "--error_type", "burst"])
    assert a.fec_params == fec.FecParams(16, 1) and a.error_space == "bitstream"


@pytest.fixture(scope="module")
def j2k():
    from rdeic_amd import jpeg2000 as J
    if not J.available():
        pytest.skip("Pillow without OpenJPEG")
    from rdeic_amd.synthetic import synth_image
    img = synth_image(256, 384, 231)
    # 0.1 % flipped bits: about 2 byte errors per 255-byte codeword, far inside what rs:32 corrects (16), and enough
    # to break an unprotected JPEG2000 codestream of 12 KB (about 100 flipped bits)
    kw = dict(target_bpp=1.0, error_type="random", rates=[0.0, 0.001], seeds=list(range(231, 237)))
    plain = J.run_jpeg2000_robustness([img], ["synth"], **kw)
    return J, img, kw, plain, J.run_jpeg2000_robustness([img], ["synth"], fec="rs:32", **kw)


def test_jpeg2000_rows_that_fail_unprotected_decode_under_fec(j2k):
    J, img, kw, plain, prot = j2k
    assert len(plain) == len(prot) == 12
    hit = [r for r in plain if r["error_rate"] > 0]
    print(f"\n[jpeg2000 fec] unprotected at 0.1 %: {sum(r['decode_failed'] for r in hit)} of {len(hit)} failed, "
          f"psnr {[round(r['psnr'], 1) for r in hit]} against {plain[0]['psnr']:.1f} clean")
    assert any(r["decode_failed"] for r in hit) and all(not r["decode_failed"] for r in plain[:6])
    clean_size = round(plain[0]["bpp"] * 256 * 384 / 8)
    for a, b in zip(plain, prot):
        assert list(b)[:11] == J.COLUMNS and list(b)[11:15] == R.FEC_COLUMNS and "error" not in b
        assert not b["decode_failed"] and b["fec_failed"] == 0 and b["fec"] == "rs:32:1"
        # every protected row decodes to what the clean codestream decodes to
        assert b["psnr"] == plain[0]["psnr"] > 20.0
        assert b["bpp_payload"] == a["bpp"]
        assert b["bpp"] == 8.0 * fec.FecParams(32).encoded_size(clean_size) / (256 * 384)
        assert (b["fec_corrected"] > 0) == (b["error_rate"] > 0)


def test_jpeg2000_without_the_flag_is_unchanged(j2k):
    J, img, kw, plain, _ = j2k
    assert all(list(r)[:11] == J.COLUMNS and not set(r) & set(R.FEC_COLUMNS) for r in plain)
    assert J.run_jpeg2000_robustness([img], ["synth"], fec=None, **kw) == plain
    # the rows are what the corruptors and the decoder give directly (the function's unprotected path, restated)
    stream = J.encode(img, kw["target_bpp"])
    for r in plain:
        data = stream if r["error_rate"] == 0 else R.bit_flip_bytes(stream, r["error_rate"] / 100, r["seed"])
        try:
            want = J.host_score(J.decode(data, J.MAX_PIXEL_FACTOR * 256 * 384), img)["psnr"]
            assert not r["decode_failed"] and r["psnr"] == want
        except AssertionError:
            raise
        except Exception:  # noqa: BLE001
            assert r["decode_failed"] and r["psnr"] == 0.0


def test_jpeg2000_unrecoverable_stream_is_a_failure_row(j2k):
    J, img, kw, _, _ = j2k
    recs = J.run_jpeg2000_robustness([img], ["synth"], 1.0, "random", [0.05], [231, 232], fec=fec.FecParams(16, 1))
    again = J.run_jpeg2000_robustness([img], ["synth"], 1.0, "random", [0.05], [231, 232], fec="rs:16")
    assert recs == again  # the error texts included: no addresses in them
    for r in recs:
        assert r["decode_failed"] and r["fec_failed"] == 1 and r["psnr"] == 0.0 and r["lpips"] == 1.0
        assert r["error"].startswith("FecError: ") and "uncorrectable" in r["error"]


def test_tables_carry_the_fec_columns_only_with_fec(j2k, tmp_path):
    J, img, kw, plain, prot = j2k
    R.write_records_csv(plain, str(tmp_path / "plain.csv"), J.COLUMNS)
    R.write_records_csv(prot, str(tmp_path / "prot.csv"), J.COLUMNS)
    assert (tmp_path / "plain.csv").read_text().splitlines()[0] == ",".join(J.COLUMNS)
    assert (tmp_path / "prot.csv").read_text().splitlines()[0] == ",".join(J.COLUMNS + R.FEC_COLUMNS)
    back = R.read_csv(str(tmp_path / "prot.csv"))
    assert [r["fec"] for r in back] == ["rs:32:1"] * 12 and back[-1]["fec_corrected"] == prot[-1]["fec_corrected"]
    rows = R.summary_by_rate(prot)
    assert [set(r) >= {"fec_corrected", "fec_failed"} for r in rows] == [True, True]
    assert rows[0]["fec_corrected"] == 0.0 and rows[0]["fec_failed"] == 0 and rows[1]["fec_failed"] == 0
    assert rows[1]["fec_corrected"] == np.mean([r["fec_corrected"] for r in prot[6:]]) > 0
    assert [(r["psnr"], r["fec_corrected"], r["fec_failed"]) for r in R.summary_by_rate(back)] == \
        [(r["psnr"], r["fec_corrected"], r["fec_failed"]) for r in rows]
    assert all("fec_failed" not in r for r in R.summary_by_rate(plain))
    text, plain_text = R.format_summary(prot).splitlines(), R.format_summary(plain).splitlines()
    assert text[0].endswith("fec_corrected mean  fec_failed") and plain_text[0].endswith("decode_failed")
    assert all(t.startswith(p[:10]) and len(t) > len(p) for t, p in zip(text, plain_text))
    bare = [{k: v for k, v in r.items() if k not in R.FEC_COLUMNS} for r in prot]
    assert [t["failure_rate"] for t in R.failure_thresholds(prot)] == \
        [t["failure_rate"] for t in R.failure_thresholds(bare)]
    mixed = R.summary_by_rate(J.run_jpeg2000_robustness([img], ["synth"], 1.0, "random", [0.05], [231], fec="rs:16"))
    assert mixed[0]["fec_failed"] == 1
