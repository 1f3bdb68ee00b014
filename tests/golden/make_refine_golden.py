"""Golden vectors of ONE refine step (is_refine: True, fixed_step 2: the second branch of p_losses,
model/rdeic.py:837-879), produced by the REFERENCE's own modules and torch autograd on CPU, fp32, at 128x128
(16x16 latent), batch 1.

Run in the development container only (the reference does not exist on the GPU box):
    python -m tests.golden.make_refine_golden
Output (committed): tests/golden/refine_128.npz, refine_128_grads.npz, refine_128_adamw.npz.

The step restates get_input as make_train_golden.py does (VAE encode_hc under no_grad, the posterior sample,
Compression.forward in training mode, bpp), then RDEIC.forward with is_refine (t = used_timesteps - 1) and the
refine branch: x_T = q_sample(c_latent, t, noise), SpacedSampler.sample_grad(fixed_step) with the reference's
sampler class on the reference's NoiseEstimator / UNet, decode_first_stage_with_grad (1 / scale_factor,
post_quant_conv, Decoder), and loss = w l_mse + 0.5 w l_lpips + w l_guide (+ bpp + emb after T/loss is
recorded), with FineTuneConfig's default weights (l_guide_weight 3, l_bpp_weight 1, lr 2e-5, as train_128.npz),
then configure_optimizers' AdamW for one step.

LPIPS: the reference's model/lpips.py builds its backbone from torchvision, which is absent. The golden
therefore evaluates the loss with tests/lpips_ref.py's torch restatement of that file, seeded_backbone('alex')
and the published heads: the loss is parity-unpinned against torchvision's weights, as the metric is.

Stored: the draws, x_T, the samples, the decoded image, every loss term, the gradient of the image losses
(w l_mse + 0.5 w l_lpips) with respect to the samples, and per trainable tensor of the control model and the
compressor the gradient's sum, L2 norm and 4 seeded projections (train_proj). The whole gradients of
make_train_golden's 12 FULL_GRADS tensors go to refine_128_grads.npz and their AdamW-updated values to
refine_128_adamw.npz (files of their own, so that no fixture grows past a megabyte).
"""
from __future__ import annotations

import math
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import train_ref  # noqa: E402
from rdeic_amd.config import CONFIG  # noqa: E402
from rdeic_amd.synthetic import refine_draws, synth_context, synth_image  # noqa: E402
from tests import lpips_bwd_ref, lpips_ref  # noqa: E402
from tests.golden import refload  # noqa: E402
from tests.golden.make_golden import fill_module, schedule  # noqa: E402
from tests.golden.make_train_golden import FULL_GRADS  # noqa: E402
from tests.golden.train_proj import projections  # noqa: E402

SIZE = 128
SEED = 7
FIXED_STEP = 2
L_GUIDE, L_BPP, LR = 3.0, 1.0, 2e-5   # FineTuneConfig's defaults, as train_128.npz


def lpips_loss(image, target):
    """tests/lpips_ref.py's restatement of model/lpips.py:75-89 (inp_range (-1, 1)), NCHW, under autograd."""
    bb = lpips_ref.seeded_backbone("alex")
    with torch.no_grad():
        f1 = lpips_ref.taps("alex", bb, lpips_bwd_ref.scaling_layer_float(target))
    f0 = lpips_ref.taps("alex", bb, lpips_bwd_ref.scaling_layer_float(image))
    val = 0
    for a, b, lin in zip(f0, f1, lpips_ref.lin_heads("alex")):
        val = val + lpips_ref.layer_distance(a, b, lin)
    return val.mean()


def main():
    torch.set_num_threads(min(os.cpu_count() or 8, 32))
    R = refload.load()
    cfg = CONFIG
    unet = R.UNetModel(**cfg["unet"])
    ne = R.NoiseEstimator(**cfg["control"])
    enc = R.Encoder(**cfg["ddconfig"]).eval()
    dec = R.Decoder(**cfg["ddconfig"])
    quant_conv = torch.nn.Conv2d(8, 8, 1)
    post_quant_conv = torch.nn.Conv2d(4, 4, 1)
    comp = R.Compression(**cfg["compression"])
    for m, p in [(unet, "model.diffusion_model."), (ne, "control_model."), (enc, "first_stage_model.encoder."),
                 (dec, "first_stage_model.decoder."), (quant_conv, "first_stage_model.quant_conv."),
                 (post_quant_conv, "first_stage_model.post_quant_conv."), (comp, "preprocess_model.")]:
        fill_module(m, p)
    for m in (unet, enc, dec, quant_conv, post_quant_conv):
        m.requires_grad_(False)
    unet.train(), ne.train(), comp.train(), dec.train()
    sched = schedule(R)

    img = synth_image(SIZE, SIZE, 231)
    ctx = synth_context()
    hl = SIZE // 8
    dr = refine_draws(1, hl, hl, cfg["compression"]["slice_ch"], SEED, FIXED_STEP)
    out = {"image": img, "post_eps": dr["post_eps"].numpy(), "noise": dr["noise"].numpy(),
           "step_noise": np.stack([s.numpy() for s in dr["step_noise"]])}
    for i, s in enumerate(dr["slice_noise"]):
        out[f"slice_noise{i}"] = s.numpy()
    t0 = time.time()
    target = (torch.tensor(img[None] / 255.0, dtype=torch.float32).permute(0, 3, 1, 2).contiguous()) * 2 - 1
    with torch.no_grad():
        h_out, c = enc.forward_hc(target)
        moments = quant_conv(h_out)
        mean, logvar = torch.chunk(moments, 2, dim=1)
        std = torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0))
        x_start = cfg["scale_factor"] * (mean + std * dr["post_eps"])
        h = cfg["scale_factor"] * c
    train_ref.NOISE_QUEUE[:] = list(dr["slice_noise"])
    c_latent, lik, qlik, emb_loss, guide_hint = comp(h)
    assert not train_ref.NOISE_QUEUE
    N, _, H, W_ = x_start.shape
    num_pixels = N * H * W_ * 64
    bpp = sum((torch.log(l_).sum() / (-math.log(2) * num_pixels)) for l_ in lik)
    q_bpp = sum((torch.log(l_).sum() / (-math.log(2) * num_pixels)) for l_ in qlik)
    t = torch.ones((N,)).long() * cfg["used_timesteps"] - 1
    x_T = (sched["sqrt_alphas_cumprod"][t].view(-1, 1, 1, 1) * c_latent +
           sched["sqrt_one_minus_alphas_cumprod"][t].view(-1, 1, 1, 1) * dr["noise"])

    class Model:
        """The attributes SpacedSampler reads from RDEIC, and apply_model on the reference's networks."""
        num_timesteps, used_timesteps = cfg["timesteps"], cfg["used_timesteps"]
        linear_start, linear_end = cfg["linear_start"], cfg["linear_end"]
        parameterization = "eps"
        betas = torch.zeros(1)  # only .device is read
        calls = []

        def apply_model(self, x, ts, cond):
            self.calls.append(int(ts[0]))
            return ne(x=x, timesteps=ts, context=torch.cat(cond["c_crossattn"], 1), guide_hint=cond["guide_hint"],
                      base_model=unet)

    model = Model()
    smp = R.SpacedSampler(model)
    cond = dict(c_crossattn=[ctx], guide_hint=guide_hint)
    it = iter(dr["step_noise"])
    orig = torch.randn_like
    torch.randn_like = lambda x, *a, **kw: next(it).to(x.dtype)
    try:
        samples = smp.sample_grad(FIXED_STEP, tuple(x_T.shape), cond, unconditional_guidance_scale=1.0,
                                  unconditional_conditioning=None, x_T=x_T)
    finally:
        torch.randn_like = orig
    assert next(it, None) is None, "one draw per step, the masked last one included"
    samples.retain_grad()
    image = dec(post_quant_conv(1.0 / cfg["scale_factor"] * samples))
    mse = torch.nn.functional.mse_loss
    loss_simple = mse(x_start, samples, reduction="none").mean([1, 2, 3])
    loss = L_GUIDE * loss_simple.mean()
    loss_mse = mse(target, image, reduction="none").mean([1, 2, 3])
    loss = L_GUIDE * loss_mse.mean()
    loss_lpips = lpips_loss(image, target)
    loss = loss + L_GUIDE * loss_lpips * 0.5
    image_loss = loss
    loss_guide = mse(x_start, c_latent)
    loss = loss + L_GUIDE * loss_guide
    t_loss = loss.detach().clone()
    loss = loss + L_BPP * bpp
    loss = loss + L_BPP * emb_loss
    print(f"forward {time.time() - t0:.1f}s t={model.calls} total {loss.item():.6f} T/loss {t_loss.item():.6f} "
          f"simple {loss_simple.mean().item():.6f} mse {loss_mse.mean().item():.6f} lpips {loss_lpips.item():.6f} "
          f"guide {loss_guide.item():.6f} bpp {bpp.item():.4f} emb {emb_loss.item():.6f}")
    t0 = time.time()
    (d_samples,) = torch.autograd.grad(image_loss, samples, retain_graph=True)
    loss.backward()
    print(f"backward {time.time() - t0:.1f}s")
    for k, v in dict(total=loss, loss=t_loss, l_simple=loss_simple.mean(), l_mse=loss_mse.mean(), l_lpips=loss_lpips,
                     l_bpp=bpp, q_bpp=q_bpp, l_emb=emb_loss, l_guide=loss_guide).items():
        out["loss_" + k] = np.float64(v.item())
    out.update(x_start=x_start.numpy(), c_latent=c_latent.detach().numpy(), x_T=x_T.detach().numpy(),
               samples=samples.detach().numpy(), decoded=image.detach().numpy(), d_samples=d_samples.numpy(),
               eps_t=np.array(model.calls, dtype=np.int64), weights=np.array([L_GUIDE, L_BPP, LR]))
    names, sums, norms, projs, params = [], [], [], [], []
    full_g, full_p = {}, {}
    for mod, prefix in ((ne, "control_model."), (comp, "preprocess_model.")):
        for k, p in mod.named_parameters():
            full = prefix + k
            g = p.grad if p.grad is not None else torch.zeros_like(p)
            names.append(full)
            sums.append(g.double().sum().item())
            norms.append(g.double().norm().item())
            projs.append(projections(full, g))
            params.append((full, p))
            if full in FULL_GRADS:
                full_g["grad:" + full] = g.numpy().copy()
    out["grad_names"] = np.asarray(names)
    out["grad_sum"] = np.asarray(sums)
    out["grad_norm"] = np.asarray(norms)
    out["grad_proj"] = np.stack(projs)
    opt = torch.optim.AdamW([p for _, p in params], lr=LR)
    opt.step()
    for full, p in params:
        if full in FULL_GRADS:
            full_p["after_adamw:" + full] = p.detach().numpy().copy()
    assert len(full_g) == len(full_p) == len(FULL_GRADS)
    for suffix, d in (("", out), ("_grads", full_g), ("_adamw", full_p)):
        path = os.path.join(HERE, f"refine_{SIZE}{suffix}.npz")
        np.savez_compressed(path, **d)
        print("wrote", path, f"{os.path.getsize(path) / 1e6:.2f} MB")
    print(f"{len(names)} trainable tensors")


if __name__ == "__main__":
    main()
