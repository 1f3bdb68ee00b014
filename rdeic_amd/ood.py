"""Out-of-domain evaluation harness (reference experiments/run_ood.py).

Per domain folder: every image is padded to a multiple of 64 (run_ood.py:324-330), compressed to its own stream
file `<cache_dir>/<domain>/<stem>` and decompressed from that file (:180-182, :333), relay-decoded (:228-276),
cropped back to its original size (:344) and scored against the un-padded original (:347-350): bpp, PSNR, SSIM,
MS-SSIM, LPIPS, NIQE, BRISQUE — the columns of ood_results_<domain>.csv / ood_results_all.csv (:356-362, :374-394).

What differs from the reference, all by design:
  * images are grouped by padded size and coded / decoded in batches (as inference_partition.py); every metric runs
    on the device (rdeic_amd/metrics.py). SSIM / MS-SSIM are NaN below 176 pixels a side, MS-SSIM also where H or W
    is no multiple of 16 (rdeic_image_ssim pools even sizes only; pyiqa's pooling floors), LPIPS is NaN without a
    backbone, NIQE / BRISQUE are NaN without their model files (none ships) or where the image is too small
    (NIQE: two 96x96 blocks) or odd-sized (BRISQUE: the half-size plane needs even H and W);
  * test-time augmentation (:184-219): the N candidates c_latent + randn * std are decoded in ONE batched
    relay_decode_u8 and scored in ONE batched LPIPS call against the padded original; the lowest wins (the first
    of equals, as the reference's strict <), the first candidate when no LPIPS model is loaded (:214-217);
  * all randoms come from a CPU generator seeded per image (seed + the image's index in sorted order), in the
    reference's draw order per candidate — the latent perturbation (:201), the q_sample noise (:253), then one
    draw per spaced-sampler step — so results do not depend on the batching;
  * guidance_scale is accepted and, as in the reference (unconditional_conditioning=None, :260, :266), has no effect;
  * a per-image failure prints and skips the image (:366-368).
"""
from __future__ import annotations

import csv
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import metrics, ops

COLUMNS = ["domain", "image_id", "bpp", "psnr", "ssim", "ms_ssim", "lpips", "niqe", "brisque"]
NAN = float("nan")


def pad64(img: np.ndarray) -> np.ndarray:
    """Zero-pad bottom / right to a multiple of 64 (reference utils/image/common.py:251-258)."""
    h, w = img.shape[:2]
    return np.pad(img, ((0, (-h) % 64), (0, (-w) % 64), (0, 0)), mode="constant", constant_values=0)


def _nhwc_randn(shape_nchw, gen: torch.Generator, device) -> torch.Tensor:
    return ops.nchw_to_nhwc(torch.randn(shape_nchw, generator=gen).to(device), torch.float32)


def image_draws(shape_nchw, seed: int, steps: int, sampler: str, candidates: int, device):
    """The randoms of one image from its own CPU generator, per candidate in the reference's order:
    (latent perturbation or None, q_sample noise, per-step noise [steps, ...] or None), NHWC fp32 on the device."""
    gen = torch.Generator().manual_seed(int(seed))
    out = []
    for _ in range(max(1, candidates)):
        pert = _nhwc_randn(shape_nchw, gen, device) if candidates > 1 else None
        noise = _nhwc_randn(shape_nchw, gen, device)
        step = torch.stack([_nhwc_randn(shape_nchw, gen, device) for _ in range(steps)]) if sampler == "ddpm" else None
        out.append((pert, noise, step))
    return out


def select_candidate(scores: Optional[np.ndarray]) -> int:
    """run_ood.py:196-219: the lowest LPIPS (first of equals); the first candidate without scores."""
    return 0 if scores is None else int(np.argmin(scores))


def columns(with_dists: bool = False) -> List[str]:
    """COLUMNS, with `dists` after `lpips` when a DISTS model scores the run."""
    if not with_dists:
        return list(COLUMNS)
    i = COLUMNS.index("lpips") + 1
    return COLUMNS[:i] + ["dists"] + COLUMNS[i:]


def score_image(pred: torch.Tensor, target: torch.Tensor, lpips=None, niqe_model=None, brisque_model=None,
                dists=None) -> Dict:
    """The metric columns of one cropped reconstruction against its original: uint8 [1,H,W,3] device tensors.
    dists: an rdeic_amd.dists.DISTS; the `dists` key is there only with it."""
    from .lpips import MIN_SIZE
    h, w = pred.shape[1:3]
    out = {"psnr": float(metrics.psnr(pred, target)[0]), "ssim": NAN, "ms_ssim": NAN, "lpips": NAN, "niqe": NAN,
           "brisque": NAN}
    if min(h, w) >= 176 and h % 16 == 0 and w % 16 == 0:
        # 5 MS-SSIM scales: >= 11 pixels at the coarsest one, and an even size at each of the four 2x2 poolings
        s, ms = metrics.ssim_ms_ssim(pred, target)
        out.update(ssim=float(s[0]), ms_ssim=float(ms[0]))
    elif min(h, w) >= 176:  # SSIM alone needs no pooling
        out.update(ssim=float(metrics.ssim_levels(pred, target, 1)[0, 0, 0]))
    if lpips is not None and min(h, w) >= MIN_SIZE[lpips.net]:
        out["lpips"] = float(lpips(pred, target)[0])
    if dists is not None:
        out["dists"] = float(dists(pred, target)[0])
    if niqe_model is not None:
        out["niqe"] = float(metrics.niqe(pred, niqe_model)[0])
    if brisque_model is not None and h % 2 == 0 and w % 2 == 0 and min(h, w) >= 8:
        out["brisque"] = float(metrics.brisque(pred, brisque_model)[0])
    return out


@torch.no_grad()
def run_domain(model, files: Sequence[str], context: torch.Tensor, domain: str = "", cache_dir: str = "encodings/ood",
               sampler: str = "ddpm", steps: int = 2, guidance_scale: float = 1.0, latent_noise_std: float = 0.0,
               num_noise_samples: int = 1, seed: int = 231, batch_size: int = 1, lpips=None, niqe_model=None,
               brisque_model=None, recon_dir: Optional[str] = None, dists=None, fid=None) -> List[Dict]:
    """One domain's images through the codec; one record per image (COLUMNS, and `dists` with a DISTS model), in
    sorted file order. The best-of-N candidate is chosen on LPIPS alone. fid: an rdeic_amd.fid.FidKid that takes
    every scored (reconstruction, original) pair; the records do not change with it."""
    from PIL import Image
    del guidance_scale  # no unconditional branch in the reference's call: no effect there either
    files = sorted(files)
    order = {f: k for k, f in enumerate(files)}
    stream_dir = os.path.join(cache_dir, domain)
    os.makedirs(stream_dir, exist_ok=True)
    if recon_dir:
        os.makedirs(recon_dir, exist_ok=True)
    tta = latent_noise_std > 0 and num_noise_samples > 1
    dev = model.device
    groups: Dict[Tuple[int, int], List[str]] = {}
    for f in files:
        try:
            with Image.open(f) as im:
                w, h = im.size
            groups.setdefault((-(-h // 64) * 64, -(-w // 64) * 64), []).append(f)
        except Exception as e:  # noqa: BLE001 — the reference's convention (:366-368)
            print(f"Error processing {f}: {e}")
    done: Dict[str, Dict] = {}
    for key in sorted(groups):
        H, W = key
        shape = (1, 4, H // 8, W // 8)
        paths = groups[key]
        for b0 in range(0, len(paths), max(1, batch_size)):
            batch, origs = [], []
            for f in paths[b0:b0 + max(1, batch_size)]:
                try:
                    origs.append(np.array(Image.open(f).convert("RGB")))
                    batch.append(f)
                except Exception as e:  # noqa: BLE001
                    print(f"Error processing {f}: {e}")
            if not batch:
                continue
            try:
                padded = torch.from_numpy(np.stack([pad64(o) for o in origs])).to(dev)
                bodies = model.compress_images(padded)
                stems = [os.path.splitext(os.path.basename(f))[0] for f in batch]
                read = []
                for stem, body in zip(stems, bodies):  # every image decodes from its own stream file (:180-182)
                    with open(os.path.join(stream_dir, stem), "wb") as fh:
                        fh.write(body)
                    with open(os.path.join(stream_dir, stem), "rb") as fh:
                        read.append(fh.read())
                c_lat, hint = model.decompress_bodies(read)
                draws = [image_draws(shape, seed + order[f], steps, sampler, num_noise_samples if tta else 1, dev)
                         for f in batch]
                if tta:
                    preds = []
                    for i in range(len(batch)):
                        lat = torch.cat([c_lat[i:i + 1] + (d[0] * latent_noise_std).to(c_lat.dtype) for d in draws[i]])
                        cand = model.relay_decode_u8(
                            lat, hint[i:i + 1].expand(len(draws[i]), *hint.shape[1:]).contiguous(), context,
                            torch.cat([d[1] for d in draws[i]]), steps, sampler,
                            torch.cat([d[2] for d in draws[i]], dim=1) if sampler == "ddpm" else None)
                        scores = lpips(cand, padded[i:i + 1].expand_as(cand).contiguous()) if lpips is not None else None
                        preds.append(cand[select_candidate(scores)])
                    out = torch.stack(preds)
                else:
                    out = model.relay_decode_u8(
                        c_lat, hint, context, torch.cat([d[0][1] for d in draws]), steps, sampler,
                        torch.cat([d[0][2] for d in draws], dim=1) if sampler == "ddpm" else None)
            except Exception as e:  # noqa: BLE001
                print(f"Error processing {', '.join(batch)}: {e}")
                continue
            for i, (f, orig, stem) in enumerate(zip(batch, origs, stems)):
                try:
                    h, w = orig.shape[:2]
                    pred = out[i:i + 1, :h, :w, :].contiguous()
                    rec = {"domain": domain, "image_id": stem,
                           "bpp": 8.0 * os.path.getsize(os.path.join(stream_dir, stem)) / (H * W)}
                    rec.update(score_image(pred, torch.from_numpy(orig[None]).to(dev), lpips, niqe_model,
                                           brisque_model, dists=dists))
                    if fid is not None:
                        fid.add(pred, torch.from_numpy(orig[None]).to(dev))
                    if recon_dir:
                        Image.fromarray(pred[0].cpu().numpy()).save(os.path.join(recon_dir, f"{stem}.png"))
                    done[f] = rec
                except Exception as e:  # noqa: BLE001
                    print(f"Error processing {f}: {e}")
    return [done[f] for f in files if f in done]


def write_csv(records: Sequence[Dict], path: str, with_dists: bool = False) -> None:
    """The reference's table (run_ood.py:356-362, :376-378): COLUMNS in order, NaN for what was not scored;
    with_dists adds the `dists` column after `lpips`."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=columns(with_dists), restval=NAN, extrasaction="ignore")
        w.writeheader()
        for r in records:
            w.writerow(r)


def summary(records: Sequence[Dict], with_dists: bool = False) -> Dict[str, Dict[str, Tuple[float, float]]]:
    """{domain: {column: (mean, sample std)}} over each domain's finite values (run_ood.py:396-405)."""
    out: Dict[str, Dict[str, Tuple[float, float]]] = {}
    for d in sorted({r["domain"] for r in records}):
        out[d] = {}
        for k in columns(with_dists)[2:]:
            v = np.array([r.get(k, NAN) for r in records if r["domain"] == d], dtype=np.float64)
            v = v[np.isfinite(v)]
            out[d][k] = (float(v.mean()) if v.size else NAN, float(v.std(ddof=1)) if v.size > 1 else NAN)
    return out
