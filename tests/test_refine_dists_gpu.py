"""The refine step's opt-in DISTS term (FineTuneConfig.l_dists_weight) at 128x128 in fp32 with the
synthetic weights: with the weight 0 the step is the parent's to the bit; with 0.5 the loss dict gains T/l_dists, T/loss
moves by the term, and the gradient that reaches the decoded image is the run-without's plus the stand-alone DISTS
gradient. The Validator's dists column is checked against metrics.dists on the images it decoded."""
import numpy as np
import pytest
import torch

from tests import dists_ref as DR
from tests import lpips_ref as R

pytestmark = pytest.mark.gpu

SEED = 7
W_DISTS = 0.5


def _dists():
    from rdeic_amd.dists import DISTS
    return DISTS(DR.seeded_weights(), backbone=DR.seeded_backbone())


def _step(**cfg):
    """One refine forward + backward of a fresh model; the decoded image's gradient is taken by a hook."""
    from rdeic_amd.finetune import FineTuneConfig, FineTuner, nchw_draws_to_nhwc
    from rdeic_amd.lpips import LPIPS
    from rdeic_amd.rdeic import RDEIC
    from rdeic_amd.synthetic import refine_draws, synth_context, synth_image
    m = RDEIC(compute_dtype=torch.float32).init_synthetic()
    dists = _dists() if cfg.get("l_dists_weight", 0.0) > 0 else None
    ft = FineTuner(m, FineTuneConfig(used_timesteps=m.used_timesteps, is_refine=True, fixed_step=2, **cfg),
                   lpips=LPIPS("alex", backbone=R.seeded_backbone("alex"), lin=R.LIN_NPZ), dists=dists)
    d = nchw_draws_to_nhwc(refine_draws(1, 16, 16, m.cfg["compression"]["slice_ch"], SEED, 2), "cuda")
    img = torch.from_numpy(synth_image(128, 128, 231)).cuda()[None]
    ft.zero_grad()
    x_start, h = ft.get_first_stage(img, d["post_eps"])
    target = ft.image_target(img)
    loss, ld = ft.refine_losses(x_start, h, synth_context().cuda(), target, d["noise"], d["slice_noise"],
                                d["step_noise"])
    image, seen = ft._last["image"], []
    image.register_hook(lambda g: seen.append(g.detach().clone()))
    loss.backward()
    torch.cuda.synchronize()
    return dict(ft=ft, ld={k: v.detach().clone() for k, v in ld.items()}, total=loss.detach().clone(),
                grad=ft.grad.clone(), image=image.detach().clone(), target=target, d_image=seen[0], dists=dists)


@pytest.fixture(scope="module")
def runs(gpu):
    return {"default": _step(), "zero": _step(l_dists_weight=0.0), "on": _step(l_dists_weight=W_DISTS)}


def test_weight_zero_is_the_default_step_to_the_bit(runs):
    a, b = runs["default"], runs["zero"]
    assert list(a["ld"]) == list(b["ld"]) and "T/l_dists" not in b["ld"]
    for k in a["ld"]:
        assert torch.equal(a["ld"][k], b["ld"][k]), k
    assert torch.equal(a["total"], b["total"]) and torch.equal(a["d_image"], b["d_image"])
    assert torch.equal(a["grad"].view(torch.int32), b["grad"].view(torch.int32)) and float(a["grad"].abs().max()) > 0


def test_loss_dict_with_the_term(runs):
    a, c = runs["default"], runs["on"]
    assert set(c["ld"]) == set(a["ld"]) | {"T/l_dists"}
    assert torch.equal(c["image"], a["image"])  # the forward up to the image is the same
    want = c["dists"].loss(c["image"], c["target"])
    assert torch.equal(c["ld"]["T/l_dists"], want) and float(want) > 0
    for k in a["ld"]:
        if k != "T/loss":
            assert torch.equal(a["ld"][k], c["ld"][k]), k
    w = c["ft"].cfg.l_guide_weight
    t_loss = float(a["ld"]["T/loss"]) + w * W_DISTS * float(want)
    print(f"T/loss {float(c['ld']['T/loss']):.8g} = {float(a['ld']['T/loss']):.8g} + {w} * {W_DISTS} * {float(want):.8g}")
    assert abs(float(c["ld"]["T/loss"]) - t_loss) <= 4 * 2.0 ** -24 * abs(t_loss)  # the sum's few fp32 roundings
    assert abs(float(c["total"]) - float(a["total"]) - w * W_DISTS * float(want)) <= 8 * 2.0 ** -24 * abs(float(c["total"]))


def test_gradient_reaching_the_decoded_image(runs):
    a, c = runs["default"], runs["on"]
    p = c["image"].clone().requires_grad_(True)
    c["dists"].loss(p, c["target"]).backward()
    w = c["ft"].cfg.l_guide_weight
    want = a["d_image"].double() + w * W_DISTS * p.grad.double()
    err = float((c["d_image"].double() - want).norm() / want.norm())
    share = float((w * W_DISTS * p.grad.double()).norm() / want.norm())
    print(f"d loss / d image: relative L2 error {err:.3e}; the DISTS term is {share:.3f} of its norm")
    assert share > 1e-3 and err <= 1e-5


def test_all_trainable_tensors_get_finite_gradients(runs):
    c = runs["on"]
    assert bool(torch.isfinite(c["grad"]).all())
    zero = [n for n, (o, k) in c["ft"].offsets.items() if float(c["grad"][o:o + k].abs().max()) == 0.0]
    assert not zero, zero[:10]
    assert not torch.equal(c["grad"], runs["default"]["grad"])


def test_finetuner_needs_a_model_for_a_positive_weight(gpu):
    from rdeic_amd.finetune import CapturedStep, FineTuneConfig, FineTuner
    ft = FineTuner.__new__(FineTuner)
    ft.buckets, ft.cfg = None, FineTuneConfig(is_refine=True, l_dists_weight=W_DISTS)
    with pytest.raises(ValueError, match="refine"):
        CapturedStep(ft, None, None, {})
    with pytest.raises(ValueError, match="DISTS"):  # refused before the model is touched
        FineTuner(None, FineTuneConfig(is_refine=True, l_dists_weight=W_DISTS), lpips=object())


def test_validator_reports_avg_dists(gpu, tmp_path, monkeypatch):
    from PIL import Image

    from rdeic_amd import metrics
    from rdeic_amd.data import ImageListLoader
    from rdeic_amd.rdeic import RDEIC
    from rdeic_amd.synthetic import synth_image
    from rdeic_amd.validate import Validator
    paths = []
    for i in range(2):
        paths.append(str(tmp_path / f"{i}.png"))
        Image.fromarray(synth_image(192, 192, 900 + i)).save(paths[-1])  # MS-SSIM's five scales need > 160 pixels
    (tmp_path / "files.list").write_text("\n".join(paths) + "\n")
    dev = torch.device("cuda")
    model = RDEIC(compute_dtype=torch.float32, device=dev).init_synthetic()
    real, seen = metrics.dists, []

    def recording(pred, tgt, m):
        seen.append(real(pred, tgt, m))
        return seen[-1]
    monkeypatch.setattr(metrics, "dists", recording)
    dm = _dists()
    loader = ImageListLoader(str(tmp_path / "files.list"), 192, "center", False, False, 1, False, True, 231,
                             device=dev, threads=2)
    try:
        v = Validator(model, None, loader, steps=2, seed=231, dists=dm)
        rec = v.run(0)
        plain = Validator(model, None, loader, steps=2, seed=231).run(0)
    finally:
        loader.close()
    vals = np.concatenate(seen)
    assert len(vals) == 2 and rec["images"] == 2 and (vals > 0).all()
    assert list(rec) == ["global_step", "avg_bpp", "usage", "avg_psnr", "avg_ssim", "avg_ms_ssim", "avg_dists",
                         "images", "bodies_sha256"]
    assert rec["avg_dists"] == float(vals.astype(np.float32).astype(np.float64).mean())  # rows travel as fp32
    assert np.array_equal(v.last_rows[:, 4], vals.astype(np.float32).astype(np.float64))
    assert "avg_dists" not in plain and {k: x for k, x in rec.items() if k != "avg_dists"} == plain
