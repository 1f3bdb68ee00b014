"""The refine step (is_refine: True, fixed_step 2; p_losses' second branch, model/rdeic.py:837-879) against the
reference's own autograd.

tests/golden/refine_128.npz holds one step of the REFERENCE modules (frozen UNetModel and VAE, NoiseEstimator and
Compression in training mode, SpacedSampler.sample_grad, Decoder; torch autograd, fp32, CPU;
tests/golden/make_refine_golden.py) at 128x128 with the synthetic weights, synthetic.refine_draws and the LPIPS
restatement of tests/lpips_ref.py (seeded AlexNet backbone, published heads). The HIP path runs the same step in
fp32 and must reproduce x_T, the samples, the decoded image, every loss term, the gradient of the image losses with
respect to the samples, the gradient of every trainable tensor (norm and 4 seeded projections within TOL of the
reference norm: the fine-tune step's fp32 summation-order bound, tests/test_finetune_gpu.py) and the AdamW update."""
import numpy as np
import pytest
import torch

from tests import lpips_ref as R

pytestmark = pytest.mark.gpu

GOLD = "tests/golden/refine_128.npz"
GOLD_GRADS = "tests/golden/refine_128_grads.npz"   # the whole gradients of 12 tensors
GOLD_ADAMW = "tests/golden/refine_128_adamw.npz"   # and their AdamW-updated values
TOL = 2e-3   # tests/test_finetune_gpu.py TOL
SEED = 7


def _lpips():
    from rdeic_amd.lpips import LPIPS
    return LPIPS("alex", backbone=R.seeded_backbone("alex"), lin=R.LIN_NPZ)


def _tuner(dtype, refine=True):
    from rdeic_amd.finetune import FineTuneConfig, FineTuner
    from rdeic_amd.rdeic import RDEIC
    m = RDEIC(compute_dtype=dtype).init_synthetic()
    if not refine:
        return FineTuner(m)
    return FineTuner(m, FineTuneConfig(used_timesteps=m.used_timesteps, is_refine=True, fixed_step=2), lpips=_lpips())


def _inputs(ft):
    from rdeic_amd.finetune import nchw_draws_to_nhwc
    from rdeic_amd.synthetic import refine_draws, synth_context, synth_image
    dr = refine_draws(1, 16, 16, ft.m.cfg["compression"]["slice_ch"], SEED, 2)
    img = torch.from_numpy(synth_image(128, 128, 231)).cuda()[None]
    return dr, img, synth_context().cuda(), nchw_draws_to_nhwc(dr, "cuda")


@pytest.fixture(scope="module")
def step(gpu):
    g = np.load(GOLD)
    ft = _tuner(torch.float32)
    dr, img, ctx, d = _inputs(ft)
    assert np.array_equal(dr["noise"].numpy(), g["noise"]) and np.array_equal(dr["post_eps"].numpy(), g["post_eps"])
    assert np.array_equal(np.stack([s.numpy() for s in dr["step_noise"]]), g["step_noise"])
    ft.zero_grad()
    x_start, h = ft.get_first_stage(img, d["post_eps"])
    target = ft.image_target(img)
    loss, ld = ft.refine_losses(x_start, h, ctx, target, d["noise"], d["slice_noise"], d["step_noise"])
    fw = {k: ft._last[k].detach() for k in ("c_latent", "x_T", "samples", "image")}
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: ft.grad[o:o + k].cpu() for n, (o, k) in ft.offsets.items()}
    # the image losses alone, from the samples (the decoder and LPIPS hold no trainable parameter)
    s = fw["samples"].clone().requires_grad_(True)
    image = ft.decode_first_stage_with_grad(s)
    w = ft.cfg.l_guide_weight
    il = w * ((image - target) ** 2).mean(dim=(1, 2, 3)).mean()
    il = il + w * ft.lpips.loss(image, target) * 0.5
    il.backward()
    d_samples = s.grad.permute(0, 3, 1, 2).cpu().numpy()
    ft.optimizer_step()
    torch.cuda.synchronize()
    params = {n: ft.flat[o:o + k].cpu() for n, (o, k) in ft.offsets.items()}
    fw = {k: v.permute(0, 3, 1, 2).float().cpu().numpy() for k, v in fw.items()}
    fw["x_start"] = x_start.permute(0, 3, 1, 2).cpu().numpy()
    return dict(g=g, ld={k: float(v.detach()) for k, v in ld.items()}, total=float(loss.detach()), grads=grads,
                params=params, fw=fw, d_samples=d_samples)


def _close(a, b, rtol, name):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)
    print(f"{name}: max rel err {err:.3e}")
    assert err < rtol, f"{name}: max rel err {err:.3e}"


def test_forward_intermediates(step):
    g, fw = step["g"], step["fw"]
    _close(fw["x_start"], g["x_start"], 1e-4, "x_start")
    _close(fw["x_T"], g["x_T"], 1e-4, "x_T")
    _close(fw["samples"], g["samples"], 1e-4, "samples")
    err = np.abs(fw["image"].astype(np.float64) - g["decoded"]).max()
    print(f"decoded image: max abs err {err:.3e}")
    assert err <= 1e-3  # the project's pixel bound


def test_loss_terms(step):
    g, ld = step["g"], step["ld"]
    for ours, ref in (("T/loss", "loss_loss"), ("T/l_simple", "loss_l_simple"), ("T/l_mse", "loss_l_mse"),
                      ("T/l_lpips", "loss_l_lpips"), ("T/l_bpp", "loss_l_bpp"), ("T/q_bpp", "loss_q_bpp"),
                      ("T/l_emb", "loss_l_emb"), ("T/l_guide", "loss_l_guide")):
        r = float(g[ref])
        print(f"{ours}: {ld[ours]:.8g} (reference {r:.8g})")
        assert abs(ld[ours] - r) <= 1e-4 * max(abs(r), 1e-3), (ours, ld[ours], r)
    r = float(g["loss_total"])
    assert abs(step["total"] - r) <= 1e-4 * abs(r)
    # T/loss is recorded before bpp and emb are added
    assert abs(step["total"] - (ld["T/loss"] + ld["T/l_bpp"] + ld["T/l_emb"])) <= 1e-5 * abs(r)


def test_gradient_of_the_image_losses_wrt_samples(step):
    g = step["g"]
    ref = g["d_samples"].astype(np.float64)
    err = np.linalg.norm(step["d_samples"].astype(np.float64) - ref) / np.linalg.norm(ref)
    print(f"d(image losses)/d samples: relative L2 error {err:.3e}")
    assert err <= TOL


def test_gradients_of_every_trainable_tensor(step):
    from tests.golden.train_proj import projections
    g, grads = step["g"], step["grads"]
    names = [str(n) for n in g["grad_names"]]
    assert sorted(names) == sorted(grads), "trainable tensor set differs from the reference's"
    bad, worst = [], (0.0, "")
    for i, n in enumerate(names):
        gr = grads[n]
        ref_norm = float(g["grad_norm"][i])
        norm = float(gr.double().norm())
        if ref_norm == 0.0:
            if norm != 0.0:
                bad.append((n, "nonzero", norm))
            continue
        err = max(abs(norm - ref_norm), np.abs(projections(n, gr) - g["grad_proj"][i]).max()) / ref_norm
        worst = max(worst, (err, n))
        if err > TOL:
            bad.append((n, err, ref_norm))
    print(f"worst gradient error against the reference: {worst[0]:.3e} ({worst[1]})")
    assert not bad, f"{len(bad)} / {len(names)} gradients off: {bad[:10]}"
    full = np.load(GOLD_GRADS)
    assert len(full.files) == 12
    for k in full.files:  # the 12 whole tensors
        _close(grads[k[5:]].numpy().reshape(full[k].shape), full[k], TOL, k)


def test_compressor_and_control_all_get_a_gradient(step):
    """The x_T path: q_sample(c_latent) carries the image losses into the compressor, guide_hint into the control
    model; no trainable tensor is left without a gradient."""
    zero = [n for n, gr in step["grads"].items() if float(gr.abs().max()) == 0.0]
    assert not zero, zero[:10]


def test_adamw_update(step):
    g, params = np.load(GOLD_ADAMW), step["params"]
    lr = 2e-5
    seen = 0
    for k in g.files:
        n = k[len("after_adamw:"):]
        diff = np.abs(params[n].numpy().reshape(g[k].shape) - g[k])
        # the first AdamW step moves each weight by ~lr * sign(grad): allow sign flips of tiny gradients
        assert (diff > 1e-6).mean() < 1e-3 and diff.max() <= 2.5 * lr, (n, diff.max(), (diff > 1e-6).mean())
        seen += 1
    assert seen == 12


def _run(dtype):
    ft = _tuner(dtype)
    _, img, ctx, d = _inputs(ft)
    ld = ft.training_step(img, ctx, d)
    torch.cuda.synchronize()
    return ft, {k: float(v) for k, v in ld.items()}


def test_two_eager_steps_are_bit_identical(gpu):
    a, la = _run(torch.float32)
    flat_a, grad_a = a.flat.clone(), a.grad.clone()  # the step leaves its gradients in ft.grad
    del a
    b, lb = _run(torch.float32)
    assert la == lb
    assert float(grad_a.abs().max()) > 0
    assert torch.equal(grad_a.view(torch.int32), b.grad.view(torch.int32))
    assert torch.equal(flat_a.view(torch.int32), b.flat.view(torch.int32))


def test_non_refine_step_is_untouched(step):
    """A non-refine FineTuner built after the refine step ran in this process still reproduces train_128.npz's
    loss terms: the refine code leaves no state behind."""
    from rdeic_amd.finetune import nchw_draws_to_nhwc
    from rdeic_amd.synthetic import synth_context, synth_image, train_draws
    g = np.load("tests/golden/train_128.npz")
    ft = _tuner(torch.float32, refine=False)
    dr = train_draws(1, 16, 16, ft.m.cfg["compression"]["slice_ch"], 5, ft.m.used_timesteps)
    img = torch.from_numpy(synth_image(128, 128, 231)).cuda()[None]
    ld = ft.training_step(img, synth_context().cuda(), nchw_draws_to_nhwc(dr, "cuda"))
    for ours, ref in (("T/loss", "loss_loss"), ("T/l_simple", "loss_l_simple"), ("T/l_bpp", "loss_l_bpp"),
                      ("T/q_bpp", "loss_q_bpp"), ("T/l_emb", "loss_l_emb"), ("T/l_guide", "loss_l_guide")):
        r = float(g[ref])
        assert abs(float(ld[ours]) - r) <= 1e-4 * max(abs(r), 1e-3), (ours, float(ld[ours]), r)


def test_captured_step_refuses_refine(step):
    from rdeic_amd.finetune import CapturedStep, FineTuneConfig, FineTuner
    ft = FineTuner.__new__(FineTuner)
    ft.buckets, ft.cfg = None, FineTuneConfig(is_refine=True)
    with pytest.raises(ValueError, match="refine"):
        CapturedStep(ft, None, None, {})


def test_bf16_refine_step_tracks_the_reference(gpu):
    """bf16: the step runs and is finite; l_guide / l_bpp within the bf16 step test's bounds
    (tests/test_finetune_gpu.py), l_mse and l_lpips within the 0.1 relative bound it uses for l_simple: they pass
    through the same bf16 UNet, twice, plus the decoder."""
    g = np.load(GOLD)
    _, ld = _run(torch.bfloat16)
    for k, v in ld.items():
        print(f"bf16 {k}: {v:.6g}")
    assert all(np.isfinite(v) for v in ld.values())
    for ours, ref, tol in (("T/l_guide", "loss_l_guide", 0.05), ("T/l_bpp", "loss_l_bpp", 0.05),
                           ("T/l_mse", "loss_l_mse", 0.1), ("T/l_lpips", "loss_l_lpips", 0.1)):
        r = float(g[ref])
        print(f"bf16 {ours}: {ld[ours]:.6g} against {r:.6g}: {abs(ld[ours] - r) / abs(r):.3e}")
        assert abs(ld[ours] - r) <= tol * abs(r), (ours, ld[ours], r)


def test_train_cli_runs_the_refine_step(gpu, tmp_path):
    """train.main with is_refine: true and LPIPS weights on disk: two eager steps at 128x128, the refine loss dict,
    a checkpoint."""
    import yaml

    import train
    bb = tmp_path / "alexnet.pth"
    torch.save(R.seeded_backbone("alex"), str(bb))
    cfg = {"data": {"out_size": 128, "batch_size": 1, "n_images": 2},
           "model": {"learning_rate": 2e-5, "l_guide_weight": 2.0, "l_bpp_weight": 1.0, "used_timesteps": 300,
                     "sd_locked": True, "is_refine": True, "fixed_step": 2, "precision": 32, "resume": None,
                     "lpips_backbone": str(bb), "lpips_lin": R.LIN_NPZ},
           "lightning": {"seed": 231, "trainer": {"max_steps": 2, "log_every_n_steps": 1},
                         "checkpoint": {"every_n_train_steps": 2, "dirpath": str(tmp_path / "ck")}}}
    p = tmp_path / "refine.yaml"
    p.write_text(yaml.safe_dump(cfg))
    recs = train.main(["--config", str(p)])
    assert [r["global_step"] for r in recs] == [1, 2]
    for r in recs:
        assert {"T/loss", "T/l_mse", "T/l_lpips", "T/l_simple", "T/l_guide", "T/l_bpp", "T/l_emb"} <= set(r)
        assert all(np.isfinite(v) for k, v in r.items() if k.startswith("T/")), r
        t_loss = 2.0 * (r["T/l_mse"] + 0.5 * r["T/l_lpips"] + r["T/l_guide"])
        assert abs(r["T/loss"] - t_loss) <= 1e-4 * abs(t_loss)
    assert (tmp_path / "ck" / "ood_finetune_step=2.safetensors").exists()
