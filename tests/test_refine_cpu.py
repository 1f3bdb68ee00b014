"""The refine step without a device: the draws, train.py's start-up refusals, and the composition of the golden's
loss terms (tests/golden/refine_128.npz, produced by tests/golden/make_refine_golden.py from the reference's
modules)."""
import os

import numpy as np
import pytest
import torch
import yaml

from rdeic_amd.config import CONFIG
from rdeic_amd.synthetic import refine_draws, train_draws

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refine_128.npz")
SLICE_CH = CONFIG["compression"]["slice_ch"]


def test_refine_draws_order_and_shapes():
    """One generator, the reference's order: post_eps, the slice noises, the x_T noise, one noise per sampler step
    (the masked last one included); no t."""
    d = refine_draws(2, 16, 12, SLICE_CH, 7, fixed_step=3)
    assert sorted(d) == ["noise", "post_eps", "slice_noise", "step_noise"]
    g = torch.Generator().manual_seed(7)
    assert torch.equal(d["post_eps"], torch.randn((2, 4, 16, 12), generator=g))
    assert len(d["slice_noise"]) == len(SLICE_CH)
    for s, c in zip(d["slice_noise"], SLICE_CH):
        assert torch.equal(s, torch.rand((2, c, 8, 6), generator=g) - 0.5)
        assert float(s.min()) >= -0.5 and float(s.max()) < 0.5
    assert torch.equal(d["noise"], torch.randn((2, 4, 16, 12), generator=g))
    assert len(d["step_noise"]) == 3
    for s in d["step_noise"]:
        assert torch.equal(s, torch.randn((2, 4, 16, 12), generator=g))


def test_train_draws_are_unchanged_by_the_refine_draws():
    a = train_draws(1, 16, 16, SLICE_CH, 5, 300)
    refine_draws(1, 16, 16, SLICE_CH, 5)
    b = train_draws(1, 16, 16, SLICE_CH, 5, 300)
    assert torch.equal(a["noise"], b["noise"]) and torch.equal(a["t"], b["t"])
    gold = np.load(os.path.join(os.path.dirname(GOLD), "train_128.npz"))
    assert np.array_equal(a["noise"].numpy(), gold["noise"])


def test_golden_draws_are_refine_draws():
    g = np.load(GOLD)
    d = refine_draws(1, 16, 16, SLICE_CH, 7, 2)
    assert np.array_equal(d["post_eps"].numpy(), g["post_eps"]) and np.array_equal(d["noise"].numpy(), g["noise"])
    assert np.array_equal(np.stack([s.numpy() for s in d["step_noise"]]), g["step_noise"])
    for i, s in enumerate(d["slice_noise"]):
        assert np.array_equal(s.numpy(), g[f"slice_noise{i}"])
    assert list(g["eps_t"]) == [299, 0]  # the model is evaluated at the kept timesteps, high to low


def test_golden_loss_composition():
    """loss = w l_mse + 0.5 w l_lpips + w l_guide (T/loss, which excludes bpp and emb and in which l_simple was
    overwritten), and the optimised total adds l_bpp_weight (bpp + emb)."""
    g = np.load(GOLD)
    w, wb, _ = g["weights"]
    v = {k[5:]: float(g[k]) for k in g.files if k.startswith("loss_")}
    t_loss = w * v["l_mse"] + 0.5 * w * v["l_lpips"] + w * v["l_guide"]
    assert abs(v["loss"] - t_loss) <= 1e-6 * abs(t_loss)
    assert abs(v["total"] - (v["loss"] + wb * (v["l_bpp"] + v["l_emb"]))) <= 1e-6 * abs(v["total"])
    assert v["l_bpp"] + v["l_emb"] > 1e-3 * v["loss"]  # so the two differ measurably
    assert abs(v["loss"] - (t_loss + w * v["l_simple"])) > 1e-3  # l_simple is logged, not added
    assert (g["grad_norm"] > 0).all()  # every trainable tensor of the compressor and the control model


def _config(tmp_path, **model):
    with open(os.path.join(os.path.dirname(os.path.dirname(GOLD)), "..", "configs", "refine.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["model"].update(model)
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def test_refine_config_holds_the_reference_values(tmp_path):
    with open(_config(tmp_path)) as f:
        mc = yaml.safe_load(f)["model"]
    assert mc["is_refine"] is True and mc["fixed_step"] == 2 and mc["sd_locked"] is True
    assert mc["used_timesteps"] == 300 and mc["l_guide_weight"] == 2.0 and mc["l_bpp_weight"] == 1.0
    assert mc["learning_rate"] == 2e-5 and mc["lpips_backbone"] is None and mc["lpips_lin"] is None


def test_train_refuses_refine_without_lpips_weights(tmp_path):
    import train
    with pytest.raises(SystemExit, match="lpips_backbone"):
        train.main(["--config", _config(tmp_path), "--max-steps", "1"])
    lin = os.path.join(os.path.dirname(GOLD), "lpips_lin.npz")
    with pytest.raises(SystemExit, match="lpips_backbone"):
        train.main(["--config", _config(tmp_path, lpips_lin=lin), "--max-steps", "1"])
    with pytest.raises(SystemExit, match="lpips_lin"):  # a backbone file, no heads
        train.main(["--config", _config(tmp_path, lpips_backbone=lin, lpips_lin="/nonexistent/alex.pth"),
                    "--max-steps", "1"])


def test_train_still_refuses_sd_unlocked(tmp_path):
    import train
    lin = os.path.join(os.path.dirname(GOLD), "lpips_lin.npz")
    with pytest.raises(SystemExit, match="sd_locked"):
        train.main(["--config", _config(tmp_path, sd_locked=False, lpips_backbone=lin, lpips_lin=lin),
                    "--max-steps", "1"])
    with pytest.raises(SystemExit, match="sd_locked"):
        train.main(["--config", _config(tmp_path, sd_locked=False, is_refine=False), "--max-steps", "1"])


def test_finetuner_config_defaults_and_lpips_requirement():
    from rdeic_amd.finetune import FineTuneConfig
    c = FineTuneConfig()
    assert c.is_refine is False and c.fixed_step == 2
    assert FineTuneConfig(is_refine=True, fixed_step=3).fixed_step == 3
