"""Bitstream / latent robustness harness (experiments/corruptors.py, experiments/run_robustness.py).

The corruptors are host byte work on ~2.5 KB streams, so they stay on the CPU and consume numpy's
RandomState exactly as the reference does (bit-identical outputs, pinned by
tests/golden/corruptors.npz). The decode side runs the HIP path: each corrupted body is entropy-
decoded on its own (the decode-failure convention of run_robustness.py:277-297 — any exception is a
catastrophic failure with psnr 0 / lpips 1), then every body that decoded goes through one batched
relay-denoise + VAE-decode launch.

Latent corruption draws its randoms from a CPU generator seeded like the reference's
torch.manual_seed(seed) (identical to the reference on CPU tensors; the reference's CUDA-RNG draws
cannot be reproduced on another device, so on-device inputs are corrupted through the CPU copy).

run_robustness is the batched form of the sweep: the variants of an image are entropy-decoded
together with per-stream fault isolation (decode_isolated), the latent error space is covered, and
summary_by_rate / failure_thresholds restate the reference's tables. For the bitstream space it returns the
records run_bitstream_robustness returns, for images of at least 176 pixels a side whose sides are multiples of 16
(elsewhere the two differ in what they put where SSIM / MS-SSIM does not apply: see run_robustness).
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Dict, List, Literal, Optional, Sequence, Tuple

import numpy as np
import torch

from . import bitstream, ops


# ------------------------------------------------------------------ corruptors (corruptors.py)
def bit_flip_bytes(data: bytes, rate: float, seed: int = 42) -> bytes:
    """Flip int(8·len·rate) distinct bits chosen by RandomState(seed).choice (corruptors.py:13-45)."""
    if rate <= 0:
        return data
    rng = np.random.RandomState(seed)
    total_bits = len(data) * 8
    n = int(total_bits * rate)
    if n == 0:
        return data
    pos = rng.choice(total_bits, size=n, replace=False)
    buf = np.frombuffer(data, dtype=np.uint8).copy()
    # distinct positions: one XOR per bit, applied per byte with a scatter of bit masks
    np.bitwise_xor.at(buf, pos // 8, (1 << (pos % 8)).astype(np.uint8))
    return buf.tobytes()


def burst_flip_bytes(data: bytes, burst_rate: float, mean_burst_len: float = 8.0, seed: int = 42) -> bytes:
    """Bursts of geometric length from random starts until int(8·len·rate) distinct bits are
    flipped (corruptors.py:48-95); the RNG call order (randint, geometric) is the reference's."""
    if burst_rate <= 0:
        return data
    rng = np.random.RandomState(seed)
    total_bits = len(data) * 8
    target = int(total_bits * burst_rate)
    if target == 0:
        return data
    flipped = set()
    while len(flipped) < target:
        start = rng.randint(0, total_bits)
        blen = rng.geometric(1.0 / mean_burst_len)
        for off in range(blen):
            flipped.add((start + off) % total_bits)
            if len(flipped) >= target:
                break
    buf = np.frombuffer(data, dtype=np.uint8).copy()
    pos = np.fromiter(flipped, dtype=np.int64, count=len(flipped))
    np.bitwise_xor.at(buf, pos // 8, (1 << (pos % 8)).astype(np.uint8))
    return buf.tobytes()


def latent_corrupt(c_latent: torch.Tensor, mode: Literal["mask_replace", "additive"], rate: float, seed: int = 42,
                   valid_range: Tuple[float, float] = (-3.0, 3.0)) -> torch.Tensor:
    """corruptors.py:98-142. Randoms from a CPU generator seeded `seed` (== torch.manual_seed on CPU)."""
    if rate <= 0:
        return c_latent.clone()
    g = torch.Generator().manual_seed(seed)
    x = c_latent.detach().to("cpu", torch.float32)
    if mode == "mask_replace":
        mask = torch.rand(x.shape, generator=g) < rate
        repl = torch.rand(x.shape, generator=g) * (valid_range[1] - valid_range[0]) + valid_range[0]
        out = x.clone()
        out[mask] = repl[mask]
    elif mode == "additive":
        out = (x + torch.randn(x.shape, generator=g) * rate).clamp(valid_range[0], valid_range[1])
    else:
        raise ValueError(f"Unknown corruption mode: {mode}")
    return out.to(c_latent.device, c_latent.dtype)


def corrupt_bitstream_file(input_path: str, output_path: str, error_type: Literal["random", "burst"], rate: float,
                           seed: int = 42, mean_burst_len: float = 8.0) -> None:
    """corruptors.py:145-176."""
    with open(input_path, "rb") as f:
        data = f.read()
    with open(output_path, "wb") as f:
        f.write(Corruptor("bitstream", error_type, rate, seed, mean_burst_len).corrupt_bytes(data))


def estimate_latent_range(c_latent: torch.Tensor, margin: float = 0.5) -> Tuple[float, float]:
    """corruptors.py:179-194."""
    return c_latent.min().item() - margin, c_latent.max().item() + margin


@dataclass
class Corruptor:
    """corruptors.py:198-241 unified interface."""
    error_space: str
    error_type: str
    rate: float
    seed: int = 42
    mean_burst_len: float = 8.0
    valid_range: Tuple[float, float] = (-3.0, 3.0)

    def corrupt_bytes(self, data: bytes) -> bytes:
        if self.error_space != "bitstream":
            raise ValueError("corrupt_bytes only works with bitstream error_space")
        if self.error_type == "random":
            return bit_flip_bytes(data, self.rate, self.seed)
        if self.error_type == "burst":
            return burst_flip_bytes(data, self.rate, self.mean_burst_len, self.seed)
        raise ValueError(f"Invalid error_type for bitstream: {self.error_type}")

    def corrupt_latent(self, c_latent: torch.Tensor) -> torch.Tensor:
        if self.error_space != "latent":
            raise ValueError("corrupt_latent only works with latent error_space")
        if self.error_type not in ("mask_replace", "additive"):
            raise ValueError(f"Invalid error_type for latent: {self.error_type}")
        return latent_corrupt(c_latent, self.error_type, self.rate, self.seed, self.valid_range)


# ------------------------------------------------------------------ harness (run_robustness.py)
def psnr_u8(a: np.ndarray, b: np.ndarray) -> float:
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return float("inf") if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)


def try_decompress(model, body: bytes, expect_shape: Optional[Tuple[int, int]] = None):
    """One body through the entropy decoder. Returns (c_latent, guide_hint) NHWC or the exception
    (the reference's `except Exception` → decode_failed, run_robustness.py:277-297). A header whose
    latent shape differs from `expect_shape` is a failure too (the reconstruction could not be
    compared with the original)."""
    try:
        _, shape = bitstream.unpack_body(body)
        if expect_shape is not None and tuple(shape) != tuple(expect_shape):
            raise ValueError(f"corrupted header: latent shape {tuple(shape)} != {tuple(expect_shape)}")
        return model.decompress_bodies([body])
    except Exception as e:  # noqa: BLE001 — the reference's convention
        return e


@torch.no_grad()
def run_bitstream_robustness(model, img_u8: torch.Tensor, context: torch.Tensor, error_type: str,
                             rates: Sequence[float], seeds: Sequence[int], steps: int = 2, sampler: str = "ddim",
                             noise_seed: int = 231, image_ids: Optional[Sequence[str]] = None,
                             mean_burst_len: float = 8.0, lpips=None, dists=None) -> List[Dict]:
    """Encode each image once, corrupt its bitstream per (rate, seed), decode every corrupted body,
    relay-decode all survivors in one batch, and score PSNR against the original pixels. Returns
    one record per (image, rate, seed) with the reference's columns: PSNR, and SSIM / MS-SSIM on
    the device (rdeic_amd/metrics.py; images of at least 176 pixels a side). lpips: an rdeic_amd.lpips.LPIPS
    (it needs a backbone state dict, none ships with the project); every image that decoded is then scored
    in one batched call. Without it lpips stays None for those rows; failure rows carry 1.0 either way.
    dists: an rdeic_amd.dists.DISTS; with it every row carries a `dists` key (decoded rows scored in the same
    batched way, failure rows 1.0), without it no row has the key."""
    B, H, W, _ = img_u8.shape
    ids = list(image_ids) if image_ids is not None else [f"img{i}" for i in range(B)]
    bodies = model.compress_images(img_u8)
    ref = img_u8.cpu().numpy()
    shape0 = bitstream.unpack_body(bodies[0])[1]
    jobs, lat, hint = [], [], []
    for i in range(B):
        bpp = 8.0 * len(bodies[i]) / (H * W)  # 8 * filesize / (H * W) (rdeic.py:667-669)
        for rate in rates:
            for seed in seeds:
                body = Corruptor("bitstream", error_type, rate, seed, mean_burst_len).corrupt_bytes(bodies[i])
                r = try_decompress(model, body, shape0)
                rec = {"image_id": ids[i], "error_space": "bitstream", "error_type": error_type,
                       "error_rate": rate * 100, "seed": seed, "bpp": bpp, "psnr": 0.0, "ssim": None,
                       "ms_ssim": None, "lpips": None, "decode_failed": isinstance(r, Exception)}
                if dists is not None:
                    rec["dists"] = None
                if rec["decode_failed"]:  # the reference's failure row (run_robustness.py:280-295)
                    rec.update(ssim=0.0, ms_ssim=0.0, lpips=1.0, error=f"{type(r).__name__}: {r}")
                    if dists is not None:
                        rec["dists"] = 1.0
                else:
                    lat.append(r[0])
                    hint.append(r[1])
                jobs.append((i, rec))
    ok = [(i, rec) for i, rec in jobs if not rec["decode_failed"]]
    if ok:
        c_lat, gh = torch.cat(lat), torch.cat(hint)
        gen = torch.Generator().manual_seed(noise_seed)
        n = c_lat.shape[0]
        noise = ops.nchw_to_nhwc(torch.randn((n, 4, c_lat.shape[1], c_lat.shape[2]), generator=gen).to(c_lat.device),
                                 torch.float32)
        step_noise = None
        if sampler == "ddpm":
            step_noise = torch.stack([ops.nchw_to_nhwc(torch.randn((n, 4, c_lat.shape[1], c_lat.shape[2]),
                                                                   generator=gen).to(c_lat.device), torch.float32)
                                      for _ in range(steps)])
        out_d = model.relay_decode_u8(c_lat, gh, context, noise, steps, sampler, step_noise)
        out = out_d.cpu().numpy()
        tgt = img_u8.to(out_d.device)[torch.tensor([i for i, _ in ok], device=out_d.device)]
        ssim, ms_ssim = (None, None)
        if min(H, W) >= 176:  # 5 MS-SSIM scales need >= 11 pixels at the coarsest one
            from .metrics import ssim_ms_ssim
            ssim, ms_ssim = ssim_ms_ssim(out_d, tgt)
        lp = lpips(out_d, tgt) if lpips is not None else None
        ds = dists(out_d, tgt) if dists is not None else None
        for k, (i, rec) in enumerate(ok):
            rec["psnr"] = psnr_u8(out[k], ref[i])
            if lp is not None:
                rec["lpips"] = float(lp[k])
            if ds is not None:
                rec["dists"] = float(ds[k])
            if ssim is not None:
                rec["ssim"], rec["ms_ssim"] = float(ssim[k]), float(ms_ssim[k])
    return [rec for _, rec in jobs]


def write_csv(records: Sequence[Dict], path: str) -> None:
    """results CSV with the reference's column order (run_robustness.py:330-370)."""
    import csv
    cols = ["image_id", "error_space", "error_type", "error_rate", "seed", "bpp", "psnr", "ssim", "ms_ssim", "lpips",
            "decode_failed"]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=cols, extrasaction="ignore")
        w.writeheader()
        for r in records:
            w.writerow(r)


# ------------------------------------------------------------------ batched sweep (run_robustness.py:188-370)
BITSTREAM_TYPES = ("random", "burst")
LATENT_TYPES = ("mask_replace", "additive")
COLUMNS = ["image_id", "error_space", "error_type", "error_rate", "seed", "bpp", "psnr", "ssim", "ms_ssim", "lpips",
           "decode_failed"]
SUMMARY_METRICS = ("psnr", "ssim", "ms_ssim", "lpips")
# appended after decode_failed by a sweep over protected streams (run_robustness(fec=...)), and only by one
FEC_COLUMNS = ["fec", "bpp_payload", "fec_corrected", "fec_failed"]
# plot_robustness.py:136-143: the value a rate's mean has to cross, and on which side failure lies
THRESHOLDS = {"psnr": 25.0, "ssim": 0.85, "ms_ssim": 0.9, "lpips": 0.3}
HIGHER_BETTER = {"psnr": True, "ssim": True, "ms_ssim": True, "lpips": False}
NAN = float("nan")


def check_error_pair(error_space: str, error_type: str) -> None:
    """bitstream takes random | burst, latent takes mask_replace | additive (Corruptor's own rule)."""
    allowed = {"bitstream": BITSTREAM_TYPES, "latent": LATENT_TYPES}.get(error_space)
    if allowed is None:
        raise ValueError(f"error_space {error_space!r} (bitstream | latent)")
    if error_type not in allowed:
        raise ValueError(f"error_type {error_type!r} does not go with error_space {error_space!r} "
                         f"({' | '.join(allowed)})")


def corrupt_latent_nhwc(c_latent: torch.Tensor, mode: str, rate: float, seed: int = 42,
                        valid_range: Tuple[float, float] = (-3.0, 3.0)) -> torch.Tensor:
    """latent_corrupt on the project's NHWC latent [B,h,w,4], in the reference's NCHW element order: the CPU
    generator's k-th draw lands on the element it lands on in the reference's [B,4,h,w] tensor."""
    x = c_latent.permute(0, 3, 1, 2).contiguous()
    return latent_corrupt(x, mode, rate, seed, valid_range).permute(0, 2, 3, 1).contiguous()


def decode_isolated(model, bodies: Sequence[bytes], expect_shape: Tuple[int, int], batch_size: int = 8) -> List:
    """Entropy-decode many bodies of one latent shape in chunks of exactly `batch_size` (the launch plans key on the
    batch size: the tail chunk is padded by repeating its last body, and the padding rows are dropped). One entry
    per body: (c_latent [1,h,w,4], guide_hint [1,h,w,M]) or the exception that body raises alone."""
    out: List = []
    bs = max(1, int(batch_size))
    for s in range(0, len(bodies), bs):
        chunk = list(bodies[s:s + bs])
        real = len(chunk)
        chunk += [chunk[-1]] * (bs - real)
        lat, hint, errors = model.decompress_bodies(chunk, isolate=True, expect_shape=expect_shape)
        for k in range(real):
            out.append(errors[k] if errors[k] is not None else (lat[k:k + 1], hint[k:k + 1]))
    return out


def relay_decode_chunked(model, lat: Sequence[torch.Tensor], hint: Sequence[torch.Tensor], context: torch.Tensor,
                         noise_nchw: torch.Tensor, step_noise_nchw: Optional[torch.Tensor], steps: int, sampler: str,
                         batch_size: int = 8) -> torch.Tensor:
    """relay_decode_u8 of n single-row latents / hints in chunks of `batch_size`. The tail chunk is padded, by
    repeating its last row, to the next multiple of a quarter chunk: the relay is compute-bound per row (a padded row
    costs what a real one does, unlike in the entropy decode), so the padding is bounded to batch_size / 4 - 1 rows
    and the recorded plans to four batch sizes, whatever the survivor counts of a sweep are.
    noise_nchw [n,4,h,w] and step_noise_nchw [steps,n,4,h,w] are CPU tensors. -> uint8 [n,H,W,3]."""
    n, bs = len(lat), max(1, int(batch_size))
    granule = max(1, bs // 4)
    dev = lat[0].device
    outs = []
    for s in range(0, n, bs):
        idx = list(range(s, min(n, s + bs)))
        real = len(idx)
        idx += [idx[-1]] * (-(-real // granule) * granule - real)
        noise = ops.nchw_to_nhwc(noise_nchw[idx].to(dev), torch.float32)
        step = None
        if sampler == "ddpm":
            step = torch.stack([ops.nchw_to_nhwc(step_noise_nchw[t][idx].to(dev), torch.float32)
                                for t in range(steps)])
        out = model.relay_decode_u8(torch.cat([lat[k] for k in idx]), torch.cat([hint[k] for k in idx]), context,
                                    noise, steps, sampler, step)
        outs.append(out[:real])
    return torch.cat(outs)


def score_crop(pred: torch.Tensor, target: torch.Tensor, lpips=None, dists=None, pred_np: Optional[np.ndarray] = None,
               target_np: Optional[np.ndarray] = None) -> Dict:
    """The metric columns of one cropped reconstruction, uint8 [1,h,w,3] device tensors. PSNR as psnr_u8 has it
    (pred_np / target_np [h,w,3]: host copies the caller already holds); the device metrics by ood.score_image's
    rules (NaN where the crop's size rules a metric out). Without an LPIPS model lpips stays None, as in
    run_bitstream_robustness."""
    from . import metrics
    h, w = pred.shape[1:3]
    out = {"psnr": psnr_u8(pred[0].cpu().numpy() if pred_np is None else pred_np,
                           target[0].cpu().numpy() if target_np is None else target_np),
           "ssim": NAN, "ms_ssim": NAN, "lpips": None}
    if min(h, w) >= 176 and h % 16 == 0 and w % 16 == 0:
        s, ms = metrics.ssim_ms_ssim(pred, target)
        out.update(ssim=float(s[0]), ms_ssim=float(ms[0]))
    elif min(h, w) >= 176:
        out.update(ssim=float(metrics.ssim_levels(pred, target, 1)[0, 0, 0]))
    if lpips is not None:
        from .lpips import MIN_SIZE
        out["lpips"] = float(lpips(pred, target)[0]) if min(h, w) >= MIN_SIZE[lpips.net] else NAN
    if dists is not None:
        out["dists"] = float(dists(pred, target)[0])
    return out


@torch.no_grad()
def run_robustness(model, images: torch.Tensor, context: torch.Tensor, error_space: str, error_type: str,
                   rates: Sequence[float], seeds: Sequence[int], steps: int = 2, sampler: str = "ddpm",
                   noise_seed: int = 231, image_ids: Optional[Sequence[str]] = None, mean_burst_len: float = 8.0,
                   batch_size: int = 8, lpips=None, dists=None, orig_sizes: Optional[Sequence[Tuple[int, int]]] = None,
                   recon_cb=None, bodies: Optional[Sequence[bytes]] = None, fec=None) -> List[Dict]:
    """The reference's sweep (run_robustness.py:227-350) over uint8 images [B,H,W,3] already padded to multiples of
    64: one record per (image, rate, seed), rates as fractions, in that loop order, with the reference's columns
    (`dists` too with a DISTS model, `error` on a failure row).

    bitstream (random | burst): every image is encoded once (or its stream is given in `bodies`), corrupted per
    (rate, seed), and all variants are entropy-decoded in chunks of `batch_size` with per-stream fault isolation
    (decode_isolated): a variant that fails is the reference's failure row (psnr 0, ssim 0, ms_ssim 0, lpips 1).
    latent (mask_replace | additive): the clean stream is decoded once, c_latent is corrupted per (rate, seed) in
    the reference's NCHW order with valid_range (-3, 3), guide_hint is reused unchanged; no row can fail.
    The survivors are relay-decoded in job order in chunks of `batch_size` (relay_decode_chunked). The noise rule is
    run_bitstream_robustness's — one CPU generator seeded noise_seed, randn([n,4,h,w]) for the n survivors, then one
    such draw per ddpm step — so for the bitstream space the two functions return the same records where H, W >= 176
    and both are multiples of 16 (and no orig_sizes crop is asked for). Elsewhere only the SSIM columns differ: under
    176 pixels the old function leaves ssim / ms_ssim None and this one writes NaN, and at 176 and more but no
    multiple of 16 the old one calls ssim_ms_ssim on the whole batch where this one scores SSIM alone (ms_ssim NaN).
    Scores are taken on the crop [:h,:w] of orig_sizes[i] = (h, w) against the cropped original (:311-314).
    recon_cb(record, crop uint8 [h,w,3] numpy) is called for every decoded row.

    fec (rdeic_amd.fec FecParams or "rs:NROOTS[:DEPTH]"; bitstream space only): the stream that crosses the channel is
    the protected one. `bodies` stay the unprotected bodies; per (rate, seed) the protected stream is corrupted by the
    same corruptors and seeds, recovered (fec.recover), and only a recovered body reaches decode_isolated. A stream
    that does not recover is the failure row with the FecError's text as `error`. `bpp` is the protected stream's
    rate, and every row carries FEC_COLUMNS: fec (the spec), bpp_payload (the body's rate), fec_corrected (bytes the
    decoder corrected) and fec_failed (0 / 1)."""
    check_error_pair(error_space, error_type)
    from . import fec as F
    fec = F.as_params(fec)
    if fec is not None and error_space != "bitstream":
        raise ValueError("fec protects the bitstream: it does not go with error_space 'latent'")
    B, H, W, _ = images.shape
    ids = list(image_ids) if image_ids is not None else [f"img{i}" for i in range(B)]
    sizes = [tuple(s) for s in orig_sizes] if orig_sizes is not None else [(H, W)] * B
    if bodies is None:
        bodies = model.compress_images(images)
    shape0 = bitstream.unpack_body(bodies[0])[1]
    jobs: List[Tuple[int, Dict]] = []
    payload: List = []
    fec_stats: List = []
    if fec is not None:
        protected = [F.protect(b, fec) for b in bodies]
        recovered = []
        for i in range(B):
            for rate in rates:
                for seed in seeds:
                    data = Corruptor("bitstream", error_type, rate, seed, mean_burst_len).corrupt_bytes(protected[i])
                    try:
                        body, st = F.recover(data)
                        recovered.append(body)
                        payload.append(None)
                    except F.FecError as e:  # never handed to the entropy decoder
                        st = e.stats
                        payload.append(e)
                    fec_stats.append(st)
        decoded = iter(decode_isolated(model, recovered, shape0, batch_size) if recovered else [])
        payload = [r if r is not None else next(decoded) for r in payload]
    elif error_space == "bitstream":
        variants = [Corruptor("bitstream", error_type, rate, seed, mean_burst_len).corrupt_bytes(bodies[i])
                    for i in range(B) for rate in rates for seed in seeds]
        payload = decode_isolated(model, variants, shape0, batch_size)
    else:
        for i in range(B):
            c_lat, hint = model.decompress_bodies([bodies[i]])
            payload += [(corrupt_latent_nhwc(c_lat, error_type, rate, seed), hint) for rate in rates for seed in seeds]
    k = 0
    for i in range(B):
        bpp = 8.0 * len(bodies[i]) / (H * W)  # 8 * filesize / (padded H * W) (run_robustness.py:250-251)
        bpp_payload = bpp
        if fec is not None:
            bpp = 8.0 * len(protected[i]) / (H * W)  # the file a protected codec writes
        for rate in rates:
            for seed in seeds:
                r = payload[k]
                k += 1
                rec = {"image_id": ids[i], "error_space": error_space, "error_type": error_type,
                       "error_rate": rate * 100, "seed": seed, "bpp": bpp, "psnr": 0.0, "ssim": None, "ms_ssim": None,
                       "lpips": None, "decode_failed": isinstance(r, Exception)}
                if dists is not None:
                    rec["dists"] = None
                if rec["decode_failed"]:  # the reference's failure row (run_robustness.py:280-295)
                    rec.update(ssim=0.0, ms_ssim=0.0, lpips=1.0, error=f"{type(r).__name__}: {r}")
                    if dists is not None:
                        rec["dists"] = 1.0
                if fec is not None:
                    rec.update(fec=fec.spec, bpp_payload=bpp_payload, fec_corrected=fec_stats[k - 1].corrected,
                               fec_failed=int(isinstance(r, F.FecError)))
                jobs.append((i, rec))
    ok = [j for j in range(len(jobs)) if not jobs[j][1]["decode_failed"]]
    if ok:
        n = len(ok)
        h, w = payload[ok[0]][0].shape[1:3]
        gen = torch.Generator().manual_seed(noise_seed)
        noise = torch.randn((n, 4, h, w), generator=gen)
        step_noise = None
        if sampler == "ddpm":
            step_noise = torch.stack([torch.randn((n, 4, h, w), generator=gen) for _ in range(steps)])
        out_d = relay_decode_chunked(model, [payload[j][0] for j in ok], [payload[j][1] for j in ok], context, noise,
                                     step_noise, steps, sampler, batch_size)
        tgt = images.to(out_d.device)
        out, ref = out_d.cpu().numpy(), images.cpu().numpy()
        for m, j in enumerate(ok):
            i, rec = jobs[j]
            ch, cw = sizes[i]
            pred = out_d[m:m + 1, :ch, :cw, :].contiguous()
            rec.update(score_crop(pred, tgt[i:i + 1, :ch, :cw, :].contiguous(), lpips, dists, out[m, :ch, :cw],
                                  ref[i, :ch, :cw]))
            if recon_cb is not None:
                recon_cb(rec, np.ascontiguousarray(out[m, :ch, :cw]))
    return [rec for _, rec in jobs]


def write_records_csv(records: Sequence[Dict], path: str, columns: Optional[Sequence[str]] = None) -> None:
    """The results table of a sweep: COLUMNS (`dists` after `lpips` when the records carry it) or the given
    columns, then FEC_COLUMNS when the records carry them; a value that was not scored (None) is written as nan."""
    import csv
    cols = list(columns) if columns is not None else list(COLUMNS)
    if "dists" not in cols and any("dists" in r for r in records):
        cols.insert(cols.index("lpips") + 1, "dists")
    if any("fec" in r for r in records):
        cols += [c for c in FEC_COLUMNS if c not in cols]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=cols, restval=NAN, extrasaction="ignore")
        w.writeheader()
        for r in records:
            w.writerow({k: (NAN if v is None else v) for k, v in r.items()})


def read_csv(path: str) -> List[Dict]:
    """A results CSV (write_csv's, the reference's, or the JPEG2000 table) back into records: numbers as floats,
    seed as int, decode_failed as bool, empty cells as NaN."""
    import csv
    out = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            rec: Dict = {}
            for key, v in row.items():
                if key in ("image_id", "error_space", "error_type", "codec", "fec"):
                    rec[key] = v
                elif key == "decode_failed":
                    rec[key] = v.strip().lower() in ("true", "1")
                elif key == "seed":
                    rec[key] = int(v)
                else:
                    rec[key] = float(v) if v.strip() else NAN
            out.append(rec)
    return out


def _by_rate(records: Sequence[Dict], key: str) -> Dict[float, np.ndarray]:
    """{error rate: the finite-or-inf values of `key` at that rate (None and NaN dropped)}, rates ascending."""
    rates = sorted({float(r["error_rate"]) for r in records})
    out = {}
    for rate in rates:
        v = np.array([NAN if r.get(key) is None else float(r[key]) for r in records
                      if float(r["error_rate"]) == rate], dtype=np.float64)
        out[rate] = v[~np.isnan(v)]
    return out


def summary_by_rate(records: Sequence[Dict]) -> List[Dict]:
    """The reference's printed table (run_robustness.py:362-370, a groupby on error_rate): per error rate, ascending,
    {"error_rate", "<metric>": (mean, sample std with ddof 1) for psnr / ssim / ms_ssim / lpips, "decode_failed":
    count}. NaN (and None) values are skipped, as pandas does; a mean of nothing and a std of fewer than two are NaN.
    Where the records carry FEC_COLUMNS a row also has "fec_corrected": the mean, and "fec_failed": the count."""
    cols = {m: _by_rate(records, m) for m in SUMMARY_METRICS}
    with_fec = any("fec_failed" in r for r in records)
    out = []
    for rate in sorted({float(r["error_rate"]) for r in records}):
        row: Dict = {"error_rate": rate}
        for m in SUMMARY_METRICS:
            v = cols[m][rate]
            row[m] = (float(v.mean()) if v.size else NAN, float(v.std(ddof=1)) if v.size > 1 else NAN)
        row["decode_failed"] = sum(1 for r in records if float(r["error_rate"]) == rate and r["decode_failed"])
        if with_fec:
            at = [r for r in records if float(r["error_rate"]) == rate and "fec_failed" in r]
            row["fec_corrected"] = float(np.mean([r["fec_corrected"] for r in at])) if at else NAN
            row["fec_failed"] = sum(int(r["fec_failed"]) for r in at)
        out.append(row)
    return out


def format_summary(records: Sequence[Dict]) -> str:
    """summary_by_rate as text, values rounded to 4 places like the reference's `.round(4)`."""
    lines = ["error_rate  " + "  ".join(f"{m + ' mean':>13} {m + ' std':>11}" for m in SUMMARY_METRICS)
             + "  decode_failed"]
    table = summary_by_rate(records)
    with_fec = bool(table) and "fec_failed" in table[0]
    if with_fec:
        lines[0] += "  fec_corrected mean  fec_failed"
    for row in table:
        lines.append(f"{row['error_rate']:>10g}  " + "  ".join(f"{row[m][0]:>13.4f} {row[m][1]:>11.4f}"
                                                              for m in SUMMARY_METRICS)
                     + f"  {row['decode_failed']:>13d}")
        if with_fec:
            lines[-1] += f"  {row['fec_corrected']:>18.4f}  {row['fec_failed']:>10d}"
    return "\n".join(lines)


def failure_thresholds(records: Sequence[Dict]) -> List[Dict]:
    """plot_robustness.compute_failure_thresholds (:130-175): per metric, the first error rate (ascending) whose mean
    over all rows (NaN skipped) is below the threshold — above it for lpips; where no rate crosses, ">10%" with the
    last rate's mean. One row per metric: metric, threshold, failure_rate, metric_at_failure."""
    out = []
    for m, thr in THRESHOLDS.items():
        means = [(rate, float(v.mean()) if v.size else NAN) for rate, v in _by_rate(records, m).items()]
        hit = next(((rate, mean) for rate, mean in means if (mean < thr if HIGHER_BETTER[m] else mean > thr)), None)
        rate, mean = hit if hit is not None else (">10%", means[-1][1])
        out.append({"metric": m, "threshold": thr, "failure_rate": rate, "metric_at_failure": mean})
    return out


def write_failure_thresholds(records: Sequence[Dict], output_dir: str, prefix: str = "") -> List[Dict]:
    """<prefix>failure_thresholds.csv and .txt as the reference writes them (plot_robustness.py:177-193)."""
    import csv
    rows = failure_thresholds(records)
    os.makedirs(output_dir, exist_ok=True)
    with open(os.path.join(output_dir, f"{prefix}failure_thresholds.csv"), "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=["metric", "threshold", "failure_rate", "metric_at_failure"])
        w.writeheader()
        for r in rows:
            w.writerow(r)
    with open(os.path.join(output_dir, f"{prefix}failure_thresholds.txt"), "w") as f:
        f.write("RDEIC Robustness Failure Thresholds\n")
        f.write("=" * 50 + "\n\n")
        for r in rows:
            f.write(f"{r['metric'].upper()}:\n")
            f.write(f"  Threshold: {r['threshold']}\n")
            f.write(f"  Failure at: {r['failure_rate']}% error rate\n")
            f.write(f"  Value at failure: {r['metric_at_failure']:.4f}\n\n")
    return rows
