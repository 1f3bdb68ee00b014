"""Adapter fine-tune CLI (the reference's train.py:10-28 with configs/finetune_ood.yaml) on MI355X.

  python train.py --config configs/finetune_ood.yaml [--max-steps N]
  python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 train.py --config ...

One process per GPU (RCCL): every rank trains on its own batches; gradients of the
control model + compressor are all-reduced in buckets from the backward (FineTuner.enable_ddp).
Data: with a `data.train` section (configs/finetune_ood_files.yaml, configs/refine_files.yaml; the reference's
dataset / data_loader keys) batches come from an image file list through rdeic_amd/data.py (PIL decode on threads,
the crop chain on the device), and a resumed run seeks the loader; without one, from a synthetic pool. With a
`data.val` section and lightning.trainer.val_check_interval, a validation epoch (rdeic_amd/validate.py, the
reference's model/rdeic.py:907-955) runs every that many steps and prints one JSON line (avg_bpp, usage, avg_psnr,
avg_ssim, avg_ms_ssim); validation.save_images writes validation/{global_step}/{idx}.png under checkpoint.dirpath.
Weights: random-init synthetic (rdeic_amd/weights.py) or `model.resume` (reference-named state
dict, loaded with safe loaders only). With `is_refine: true` (configs/refine.yaml, the reference's
configs/model/rdeic.yaml) the step is p_losses' refine branch: the relay sampler and the VAE decoder in the loop,
image MSE + 0.5 LPIPS(alex); it needs model.lpips_backbone / model.lpips_lin and runs eagerly. Logs the reference's
loss dict (T/loss, T/l_simple, T/l_bpp, T/q_bpp, T/l_emb, T/l_guide; refine: also T/l_mse, T/l_lpips) every
log_every_n_steps; with `model.l_dists_weight` > 0 (configs/refine_dists.yaml; needs model.dists_weights, optionally
model.dists_backbone) the refine loss adds l_guide_weight * l_dists_weight * DISTS and T/l_dists is logged too. It saves the trainable parameters (and the
AdamW state) every every_n_train_steps as safetensors.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


EMBED_PROB = "preprocess_model.quantize.embed_prob"


def load_state(path: str):
    """(state dict, metadata) with safe loaders only (safetensors, or torch.load weights_only)."""
    if path.endswith(".safetensors"):
        from safetensors import safe_open
        from safetensors.torch import load_file
        with safe_open(path, "pt") as f:
            meta = f.metadata() or {}
        return load_file(path), meta
    sd = torch.load(path, map_location="cpu", weights_only=True)
    meta = {"global_step": str(sd["global_step"])} if isinstance(sd.get("global_step"), int) else {}
    return sd.get("state_dict", sd), meta


def precision_dtype(precision):
    """The trainer precision of the config: 32 (the reference's finetune_ood.yaml) or bf16. Lightning's
    16 means fp16 autocast, which this path does not implement: refused rather than silently trained
    in another dtype."""
    p = str(precision).lower()
    if p in ("32", "32-true"):
        return torch.float32
    if p in ("bf16", "bf16-mixed", "bf16-true"):
        return torch.bfloat16
    raise SystemExit(f"precision {precision!r} is not supported (32 or bf16; fp16 autocast is not implemented)")


def save_checkpoint(ft, path: str, step: int) -> None:
    from safetensors.torch import save_file
    out = {n: ft.flat[o:o + k].view(ft.m.store.shapes[n]).detach().cpu().contiguous()
           for n, (o, k) in ft.offsets.items()}
    out[EMBED_PROB] = ft.embed_prob.cpu()
    out["optimizer.exp_avg"] = ft.exp_avg.cpu()
    out["optimizer.exp_avg_sq"] = ft.exp_avg_sq.cpu()
    save_file(out, path, metadata={"global_step": str(step)})


def make_loader(dc: dict, seed: int, rank: int, world: int, dev):
    """An ImageListLoader from a data.train / data.val section (the reference's dataset.params and data_loader
    keys; num_workers sizes the decode thread pool, 0 or absent: the cgroup share)."""
    from rdeic_amd.data import ImageListLoader
    return ImageListLoader(str(dc["file_list"]), int(dc["out_size"]), str(dc.get("crop_type", "center")),
                           bool(dc.get("use_hflip", False)), bool(dc.get("use_rot", False)),
                           int(dc.get("batch_size", 1)), bool(dc.get("shuffle", False)),
                           bool(dc.get("drop_last", True)), seed, rank, world, dev,
                           threads=int(dc.get("num_workers") or 0) or None,
                           host_resize=bool(dc.get("host_resize", False)))


def data_loaders(cfg: dict, seed: int, rank: int, world: int, dev):
    """(train loader, validation loader) of the optional data.train / data.val sections; None for an absent one.
    The validation list is not sharded by the loader (rank 0, world 1): the Validator shards it."""
    dc = cfg.get("data") or {}
    train = make_loader(dc["train"], seed, rank, world, dev) if dc.get("train") else None
    val = make_loader(dc["val"], seed, 0, 1, dev) if dc.get("val") else None
    return train, val


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "finetune_ood.yaml"))
    ap.add_argument("--max-steps", type=int, default=None)
    ap.add_argument("--eager", action="store_true", help="no hipGraph capture of the step (one GPU)")
    ap.add_argument("--attention", default=None, choices=["auto", "flash", "materialized"],
                    help="attention of the step (autograd.set_attention_impl; default: the library's)")
    args = ap.parse_args(argv)
    with open(args.config) as f:
        cfg = yaml.safe_load(f)
    from rdeic_amd import autograd, parallel
    if args.attention:
        autograd.set_attention_impl(args.attention)
    from rdeic_amd.finetune import CapturedStep, FineTuneConfig, FineTuner, nchw_draws_to_nhwc
    from rdeic_amd.rdeic import RDEIC
    from rdeic_amd.synthetic import refine_draws, synth_context, synth_image, train_draws

    mc, dc, lc = cfg["model"], cfg["data"], cfg["lightning"]
    dtype = precision_dtype(mc.get("precision", 32))
    seed = int(lc.get("seed", 231))
    if not mc.get("sd_locked", True):
        raise SystemExit("sd_locked: false (training the UNet decoder) is not supported")
    refine = bool(mc.get("is_refine", False))
    if refine:  # p_losses' refine branch trains on LPIPS(alex); no backbone weights ship with the project
        for key in ("lpips_backbone", "lpips_lin"):
            if not mc.get(key) or not os.path.isfile(str(mc[key])):
                raise SystemExit(f"is_refine: true needs model.{key}: the torchvision AlexNet state dict "
                                 f"(lpips_backbone) and the LPIPS lin heads (lpips_lin); got {mc.get(key)!r}")
    l_dists = float(mc.get("l_dists_weight") or 0.0)
    if l_dists > 0:  # the opt-in DISTS term of the refine loss; no weights ship with the project
        if not refine:
            raise SystemExit("model.l_dists_weight > 0 needs is_refine: true: the DISTS term is taken on the decoded "
                             "image, which the non-refine step does not have")
        if not mc.get("dists_weights") or not os.path.isfile(str(mc["dists_weights"])):
            raise SystemExit(f"l_dists_weight: {l_dists} needs model.dists_weights: the DISTS alpha / beta file "
                             f"(.pt / .pth / .npz; the VGG16 convs from it or from model.dists_backbone); got "
                             f"{mc.get('dists_weights')!r}")
        if mc.get("dists_backbone") and not os.path.isfile(str(mc["dists_backbone"])):
            raise SystemExit(f"model.dists_backbone: no such file {mc['dists_backbone']!r}")
    rank, world, local = parallel.init_from_env()
    dev = torch.device("cuda", local)
    model = RDEIC(compute_dtype=dtype, device=dev).init_synthetic()
    sd, meta = (load_state(mc["resume"]) if mc.get("resume") else ({}, {}))
    if sd:
        model.load_state_dict(sd, strict=False)
    lpips = None
    if refine:
        from rdeic_amd.lpips import LPIPS
        lpips = LPIPS("alex", backbone=str(mc["lpips_backbone"]), lin=str(mc["lpips_lin"]), device=dev)
    dists = None
    if l_dists > 0:
        from rdeic_amd.dists import DISTS
        dists = DISTS(str(mc["dists_weights"]), backbone=str(mc["dists_backbone"]) if mc.get("dists_backbone") else None,
                      device=dev)
    # the codebook-usage EMA travels with the weights (reference checkpoints and ours)
    ft = FineTuner(model, FineTuneConfig(learning_rate=float(mc["learning_rate"]),
                                         l_guide_weight=float(mc["l_guide_weight"]),
                                         l_bpp_weight=float(mc["l_bpp_weight"]),
                                         used_timesteps=int(mc["used_timesteps"]), is_refine=refine,
                                         fixed_step=int(mc.get("fixed_step", 2)), l_dists_weight=l_dists),
                   embed_prob=sd.get(EMBED_PROB), lpips=lpips, dists=dists)
    start = 0
    if "optimizer.exp_avg" in sd:  # one of train.py's own checkpoints: continue that run exactly
        start = int(meta.get("global_step", 0))
        ft.load_optimizer_state(sd["optimizer.exp_avg"], sd["optimizer.exp_avg_sq"], start)
    if world > 1:
        ft.enable_ddp()
    loader, val_loader = data_loaders(cfg, seed, rank, world, dev)
    if loader is not None:  # batches from image files; on resume the loader seeks, nothing is replayed
        S, B = loader.out_size, loader.batch_size
        loader.seek(start)
        batches = loader.forever()
    else:
        S, B = int(dc["out_size"]), int(dc["batch_size"])
        n_img = int(dc.get("n_images", 64))
        pool = torch.from_numpy(np.stack([synth_image(S, S, seed + 1000 * rank + i) for i in range(n_img)])).to(dev)
    ctx = synth_context().to(dev)
    tr = lc["trainer"]
    max_steps = args.max_steps if args.max_steps is not None else int(tr["max_steps"])
    log_every = int(tr.get("log_every_n_steps", 50))
    ck = lc.get("checkpoint", {})
    ck_every = int(ck.get("every_n_train_steps", 0))
    ck_dir = ck.get("dirpath", "./logs/ood_finetune")
    slice_ch = model.cfg["compression"]["slice_ch"]
    rng = np.random.default_rng(seed + rank)
    for _ in range(start if loader is None else 0):  # the batches the interrupted run already drew
        rng.integers(0, n_img, size=B)
    validator, val_every = None, int(tr.get("val_check_interval") or 0)
    if val_loader is not None and val_every:  # validation epochs (model/rdeic.py:907-955) every val_check_interval steps
        from rdeic_amd.validate import Validator
        save = bool((cfg.get("validation") or {}).get("save_images", False))
        validator = Validator(model, ft, val_loader, steps=ft.cfg.fixed_step if refine else 5, sampler="ddpm",
                              lpips=lpips, dists=dists, save_dir=ck_dir if save else None, seed=seed,
                              limit_batches=tr.get("limit_val_batches"), context=ctx)
    graph = None
    records = []
    t0 = time.perf_counter()
    for step in range(start + 1, max_steps + 1):
        idx = rng.integers(0, n_img, size=B) if loader is None else None
        dseed = seed * 1000003 + step * 131 + rank
        dr = nchw_draws_to_nhwc(refine_draws(B, S // 8, S // 8, slice_ch, dseed, ft.cfg.fixed_step) if refine else
                                train_draws(B, S // 8, S // 8, slice_ch, dseed, ft.cfg.used_timesteps), dev)
        batch = pool[torch.from_numpy(idx).to(dev)] if loader is None else next(batches)
        if world == 1 and not args.eager and not refine and graph is None:  # the refine step runs eagerly
            graph = CapturedStep(ft, batch, ctx, dr)  # one GPU: the step replays as one hipGraph
        d = graph.step(batch, dr) if graph is not None else ft.training_step(batch, ctx, dr)
        if rank == 0 and (step % log_every == 0 or step == max_steps):
            rec = {k: round(float(v), 6) for k, v in d.items()}
            rec.update(global_step=step, it_per_s=round((step - start) / (time.perf_counter() - t0), 4))
            records.append(rec)
            print(json.dumps(rec), flush=True)
        if rank == 0 and ck_every and step % ck_every == 0:
            os.makedirs(ck_dir, exist_ok=True)
            save_checkpoint(ft, os.path.join(ck_dir, f"ood_finetune_step={step}.safetensors"), step)
        if validator is not None and step % val_every == 0:  # every rank codes its shard of the list
            vrec = validator.run(step)
            if rank == 0:
                vrec = {k: (round(v, 6) if isinstance(v, float) else v) for k, v in vrec.items()}
                records.append(vrec)
                print(json.dumps(vrec), flush=True)
    if loader is not None:
        batches.close()
    for ld in (loader, val_loader):
        if ld is not None:
            ld.close()
    parallel.finish()
    return records


if __name__ == "__main__":
    main()
