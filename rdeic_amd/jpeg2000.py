"""JPEG2000 baseline of the fault-robustness study (reference experiments/run_jpeg2000_robustness.py).

The reference shells out to `opj_compress -r (24 / target_bpp)` and `opj_decompress`. Those tools are not part of
this project's environment; Pillow bundles the same library (OpenJPEG), so the codec here is Pillow's JPEG2000
plugin: a raw .j2k codestream (`no_jp2`), one quality layer at the compression ratio 24 / target_bpp, the reversible
5/3 transform (`opj_compress` without -I). The corruptors are the project's byte corruptors (rdeic_amd/robustness.py),
bit-identical to the reference's. Parity of the achieved rate and of the decoder's tolerance with the command-line
tools is unpinned: both depend on the OpenJPEG build.

One deviation: a corrupted header that announces more than MAX_PIXEL_FACTOR x the original's pixel count is a decode
failure before any pixel is decoded. A flipped SIZ field can announce 10^8 pixels and more; Pillow then raises its
DecompressionBombError or spends minutes on the decode, and a sweep must not stall on one row.
"""
from __future__ import annotations

import io
import re
import struct
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .robustness import bit_flip_bytes, burst_flip_bytes, psnr_u8

COLUMNS = ["codec", "image_id", "error_type", "error_rate", "seed", "bpp", "psnr", "ssim", "ms_ssim", "lpips",
           "decode_failed"]
MAX_PIXEL_FACTOR = 4
NAN = float("nan")
# an object's address inside an exception's text (" at 0x7f..."): two runs of a sweep give the same records without it
_ADDRESS = re.compile(r" at 0x[0-9a-fA-F]+")


def available() -> bool:
    """Pillow is there and was built with OpenJPEG."""
    try:
        from PIL import features
        return bool(features.check_codec("jpg_2000"))
    except Exception:  # noqa: BLE001
        return False


def encode(img: np.ndarray, target_bpp: float) -> bytes:
    """uint8 [H,W,3] -> a .j2k codestream at about target_bpp (compression ratio 24 / target_bpp, as the
    reference's `opj_compress -r`; ratio 100 for a target of 0 or less, run_jpeg2000_robustness.py:97)."""
    from PIL import Image
    ratio = 24.0 / target_bpp if target_bpp > 0 else 100.0
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img, dtype=np.uint8)).save(
        buf, format="JPEG2000", quality_mode="rates", quality_layers=[ratio], no_jp2=True)
    return buf.getvalue()


def siz_size(data: bytes) -> Optional[Tuple[int, int]]:
    """(height, width) the codestream's SIZ segment announces (ISO 15444-1 A.5.1: SOC ff4f, SIZ ff51, Lsiz, Rsiz,
    Xsiz, Ysiz, XOsiz, YOsiz), or None when the stream does not start with SOC + SIZ."""
    if len(data) < 24 or data[:4] != b"\xff\x4f\xff\x51":
        return None
    xsiz, ysiz, xo, yo = struct.unpack_from(">4I", data, 8)
    return max(0, ysiz - yo), max(0, xsiz - xo)


def decode(data: bytes, max_pixels: Optional[int] = None) -> np.ndarray:
    """A .j2k codestream -> uint8 [H,W,3]. Raises on anything the decoder refuses, and ValueError before any pixel
    is decoded when the header announces more than max_pixels."""
    from PIL import Image, UnidentifiedImageError
    announced = siz_size(data)
    if max_pixels is not None and announced is not None and announced[0] * announced[1] > max_pixels:
        raise ValueError(f"header announces {announced[0]}x{announced[1]} pixels, more than {max_pixels}")
    try:
        im = Image.open(io.BytesIO(data))  # parses the header only
    except UnidentifiedImageError:
        # Pillow's own message names the BytesIO object with its address: not the same text in two runs
        raise UnidentifiedImageError("cannot identify the codestream") from None
    with im:
        if max_pixels is not None and im.size[0] * im.size[1] > max_pixels:
            raise ValueError(f"header announces {im.size[1]}x{im.size[0]} pixels, more than {max_pixels}")
        im.load()
        return np.array(im.convert("RGB"))


def host_score(pred: np.ndarray, target: np.ndarray) -> Dict:
    """PSNR on the host (the reference's 10 log10(1 / (mse + 1e-10)) on [0, 1] images caps at 100 dB: so does this);
    the device metrics are left NaN."""
    return {"psnr": min(psnr_u8(pred, target), 100.0), "ssim": NAN, "ms_ssim": NAN, "lpips": NAN}


def run_jpeg2000_robustness(images: Sequence[np.ndarray], image_ids: Sequence[str], target_bpp: float = 0.12,
                            error_type: str = "random", rates: Sequence[float] = (0.0,), seeds: Sequence[int] = (231,),
                            mean_burst_len: float = 8.0, score: Optional[Callable] = None,
                            recon_cb: Optional[Callable] = None, fec=None) -> List[Dict]:
    """run_jpeg2000_robustness.py:167-276: every uint8 [H,W,3] image is coded once, its codestream corrupted per
    (rate, seed) — rates as fractions — and decoded; one record per (image, rate, seed) with COLUMNS. Any exception
    on decode is the reference's failure row (psnr 0, ssim 0, ms_ssim 0, lpips 1). A decoded size other than the
    original's is resized with LANCZOS (:222-224). score(pred, target) -> {psnr, ssim, ms_ssim, lpips} of two uint8
    [H,W,3] arrays (host_score by default); recon_cb(record, pred) is called for every decoded row.
    fec (rdeic_amd.fec FecParams or "rs:NROOTS[:DEPTH]"): the protected codestream is what gets corrupted (rate 0
    included: it is recovered like the others); one that does not recover is a failure row with the FecError's text.
    bpp is then the protected rate, and every row carries robustness.FEC_COLUMNS after decode_failed."""
    from PIL import Image
    if error_type not in ("random", "burst"):
        raise ValueError(f"error_type {error_type!r} (random | burst)")
    if not available():
        raise RuntimeError("Pillow has no JPEG2000 codec (it was built without OpenJPEG)")
    score = score or host_score
    from . import fec as F
    fec = F.as_params(fec)
    records = []
    for img, name in zip(images, image_ids):
        h, w = img.shape[:2]
        clean = encode(img, target_bpp)
        bpp = 8.0 * len(clean) / (h * w)
        if fec is not None:
            bpp_payload, clean = bpp, F.protect(clean, fec)
            bpp = 8.0 * len(clean) / (h * w)
        for rate in rates:
            for seed in seeds:
                rec = {"codec": "JPEG2000", "image_id": name, "error_type": error_type, "error_rate": rate * 100,
                       "seed": seed, "bpp": bpp, "psnr": 0.0, "ssim": 0.0, "ms_ssim": 0.0, "lpips": 1.0,
                       "decode_failed": True}
                if fec is not None:
                    rec.update(fec=fec.spec, bpp_payload=bpp_payload, fec_corrected=0, fec_failed=0)
                try:
                    if rate == 0:
                        data = clean
                    elif error_type == "random":
                        data = bit_flip_bytes(clean, rate, seed)
                    else:
                        data = burst_flip_bytes(clean, rate, mean_burst_len, seed)
                    if fec is not None:
                        try:
                            data, st = F.recover(data)
                        except F.FecError as e:  # never handed to the JPEG2000 decoder
                            rec.update(fec_corrected=e.stats.corrected, fec_failed=1)
                            raise
                        rec["fec_corrected"] = st.corrected
                    pred = decode(data, MAX_PIXEL_FACTOR * h * w)
                    if pred.shape != img.shape:
                        pred = np.array(Image.fromarray(pred).resize((w, h), Image.LANCZOS))
                    rec.update(score(pred, img))
                    rec["decode_failed"] = False
                    if recon_cb is not None:
                        recon_cb(rec, pred)
                except Exception as e:  # noqa: BLE001 — the reference's convention (:262-276)
                    rec.update(psnr=0.0, ssim=0.0, ms_ssim=0.0, lpips=1.0, decode_failed=True,
                               error=_ADDRESS.sub("", f"{type(e).__name__}: {e}"))
                records.append(rec)
    return records
