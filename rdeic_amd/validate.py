"""Validation epochs of the training loop (the reference's model/rdeic.py:907-955: validation_step,
on_validation_epoch_start, validation_epoch_end) on the inference path.

Every validation image is coded to a real bitstream and decoded (RDEIC.codec_images: compress, entropy-code,
decompress, relay sampler, VAE decode), then scored on the device. Deviations from the reference, on purpose:
  * avg_bpp is 8 * len(body) / (H * W) of the real file body; the reference logs the estimate q_bpp + 14 / 64^2.
  * the initial and per-step sampler noise of an image come from a CPU generator seeded by (seed, image index),
    so a validation row depends on the weights only, not on rank count or on what ran before.
  * SSIM / MS-SSIM are rdeic_amd/metrics.py's (sides >= 176); LPIPS is scored only when an LPIPS model is given.
"""
from __future__ import annotations

import hashlib
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Optional

import numpy as np
import torch

from . import metrics, parallel
from .synthetic import relay_noise, synth_context


def noise_seed(seed: int, index: int) -> int:
    return int(seed) * 1000003 + int(index)


class Validator:
    """run(global_step) -> {"global_step", "avg_bpp", "usage", "avg_psnr", "avg_ssim", "avg_ms_ssim",
    ["avg_lpips"], ["avg_dists"], "images", "bodies_sha256"}.

    loader: an ImageListLoader over the whole validation list (rank 0, world 1); the images of its first epoch
    order (all of them, or its whole batches with drop_last, at most limit_batches batches) are sharded over the
    ranks with parallel.shard and the per-image rows gathered as bench.py's metric rows are. ft: the FineTuner
    whose parameters the model shares (sync_inference() runs first), or None for a model that is not training.
    usage is the fraction of VQ codes used over the epoch (compression_modules.py:221-226; the count restarts at
    every run, as on_validation_epoch_start), from the indices the decompress path decoded. last_rows
    ([images][bpp, psnr, ssim, ms_ssim(, lpips)(, dists)]) and last_bodies (this rank's) keep the latest run's detail."""

    def __init__(self, model, ft, loader, *, steps: int, sampler: str = "ddpm", lpips=None, dists=None,
                 save_dir: Optional[str] = None, seed: int = 231, limit_batches: Optional[int] = None, context=None):
        self.model, self.ft, self.loader = model, ft, loader
        self.steps, self.sampler, self.lpips, self.save_dir = int(steps), sampler, lpips, save_dir
        self.dists = dists  # an rdeic_amd.dists.DISTS: adds the per-image dists column and avg_dists, after LPIPS
        self.seed, self.limit_batches = int(seed), limit_batches
        self.context = context if context is not None else synth_context().to(model.device)
        self.last_rows = None
        self.last_bodies = []

    def _order(self) -> np.ndarray:
        ld = self.loader
        nb = len(ld) if self.limit_batches is None else min(len(ld), int(self.limit_batches))
        order = ld.epoch_indices(0)
        return order[:min(len(order), nb * ld.batch_size)]

    @torch.no_grad()
    def run(self, global_step: int) -> dict:
        import torch.distributed as dist
        model, ld = self.model, self.loader
        if self.ft is not None:
            self.ft.sync_inference()
        distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        rank, world = (dist.get_rank(), dist.get_world_size()) if distributed else (0, 1)
        order = self._order()
        g0, g1 = parallel.shard(len(order), rank, world)
        used = np.zeros(model.preprocess_model.codebook_size, dtype=np.int64)  # reset per validation epoch
        rows, bodies_all = [], []
        saver = ThreadPoolExecutor(1, thread_name_prefix="rdeic-valsave") if self.save_dir else None
        jobs = []
        if saver:
            out_dir = os.path.join(self.save_dir, "validation", str(global_step))
            os.makedirs(out_dir, exist_ok=True)
        try:
            for p0 in range(g0, g1, ld.batch_size):
                pos = range(p0, min(p0 + ld.batch_size, g1))
                idx = [int(order[p]) for p in pos]
                imgs = ld.load_batch(idx, epoch=0)
                B, H, W_, _ = imgs.shape
                draws = [relay_noise((1, 4, H // 8, W_ // 8), noise_seed(self.seed, i), self.steps) for i in idx]
                noise = torch.cat([d[0] for d in draws])
                step_noise = torch.cat([d[1] for d in draws], 1) if self.sampler == "ddpm" else None
                out, bodies = model.codec_images(imgs, self.context, noise, steps=self.steps, sampler=self.sampler,
                                                 step_noise_nchw=step_noise)
                zi = np.asarray(model.preprocess_model.last_z_idx).reshape(-1)
                used += np.bincount(zi, minlength=used.size)[:used.size]
                ps = metrics.psnr(out, imgs)
                ss, ms = metrics.ssim_ms_ssim(out, imgs)
                cols = [[8.0 * len(b) / (H * W_) for b in bodies], ps, ss, ms]
                if self.lpips is not None:
                    cols.append(metrics.lpips(out, imgs, self.lpips))
                if self.dists is not None:
                    cols.append(metrics.dists(out, imgs, self.dists))
                rows.append(np.stack([np.asarray(c, dtype=np.float64) for c in cols], axis=1))
                bodies_all += list(bodies)
                if saver:
                    host = out.cpu().numpy()
                    for b, p in enumerate(pos):
                        jobs.append(saver.submit(_save_png, host[b], os.path.join(out_dir, f"{p}.png")))
            for j in jobs:
                j.result()
        finally:
            if saver:
                saver.shutdown(wait=True)
        k = 4 + (self.lpips is not None) + (self.dists is not None)
        mine = torch.from_numpy(np.concatenate(rows) if rows else np.zeros((0, k))).to(torch.float32)
        digest = hashlib.sha256(b"".join(bodies_all)).hexdigest()
        if distributed:
            mine = parallel.gather_metrics(mine.to(model.device), len(order)).cpu()
            cnt = torch.from_numpy(used)
            cnt = cnt if dist.get_backend() == "gloo" else cnt.to(model.device)
            dist.all_reduce(cnt)
            used = cnt.cpu().numpy()
        allrows = mine.double().numpy()
        self.last_rows, self.last_bodies = allrows, bodies_all
        avg = allrows.mean(0) if len(allrows) else np.full(k, float("nan"))
        rec = {"global_step": int(global_step), "avg_bpp": float(avg[0]),
               "usage": float((used != 0).sum() / used.size), "avg_psnr": float(avg[1]), "avg_ssim": float(avg[2]),
               "avg_ms_ssim": float(avg[3])}
        if self.lpips is not None:
            rec["avg_lpips"] = float(avg[4])
        if self.dists is not None:
            rec["avg_dists"] = float(avg[k - 1])
        rec.update(images=int(len(allrows)), bodies_sha256=digest)  # this rank's bodies, in order
        return rec


def _save_png(arr: np.ndarray, path: str) -> None:
    from PIL import Image
    Image.fromarray(arr).save(path)
