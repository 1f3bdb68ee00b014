"""The DISTS training loss without a device: the fp32 CPU restatement against fp64 (the yardstick the device
gradient is held to in tests/test_dists_bwd_gpu.py), the restatement's own consistency with the uint8 metric's, and
train.py's start-up refusals for the DISTS term."""
import os

import numpy as np
import pytest
import torch
import yaml

from tests import dists_bwd_ref as B
from tests import dists_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIN = os.path.join(ROOT, "tests", "golden", "lpips_lin.npz")  # any readable file stands in for the LPIPS weights


@pytest.mark.parametrize("case", B.CASES, ids=lambda c: "x".join(map(str, c)))
def test_fp32_restatement_stays_near_fp64(case):
    pred, target, l64, g64, l32, g32 = B.case(*case)
    rel, dl = B.rel_l2(g32, g64), abs(float(l32) - float(l64))
    print(f"DISTS loss {case}: fp64 loss {float(l64):.6e}, fp32 CPU gradient rel L2 {rel:.3e}, loss abs {dl:.1e}")
    assert g64.shape == pred.shape and torch.isfinite(g64).all() and float(g64.norm()) > 0
    assert rel <= B.CPU_FP32_GRAD_BOUND
    assert dl <= B.CPU_FP32_LOSS_BOUND


def test_float_restatement_matches_the_metrics_on_the_uint8_grid():
    """On images that sit on the uint8 grid the float-input loss is the mean of the uint8 metric's scores."""
    pred_u8, tgt_u8 = R.pairs(24, 20)
    bb, wt = R.seeded_backbone(0), R.seeded_weights(0)
    want = R.dists(bb, wt, pred_u8, tgt_u8).mean()
    to_f = lambda a: torch.from_numpy(a).double() / 127.5 - 1.0
    got, _ = B.loss_and_grad(bb, wt, to_f(pred_u8), to_f(tgt_u8), torch.float64)
    assert abs(float(got) - want) <= 1e-12


def test_identical_images_have_zero_loss_and_gradient():
    pred, _ = B.float_pair(1, 16, 16, 1)
    loss, grad = B.loss_and_grad(R.seeded_backbone(0), R.seeded_weights(0), pred, pred, torch.float64)
    assert abs(float(loss)) <= 1e-12 and float(grad.abs().max()) <= 1e-12


def _config(tmp_path, **model):
    with open(os.path.join(ROOT, "configs", "refine.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["model"].update(lpips_backbone=LIN, lpips_lin=LIN)
    cfg["model"].update(model)
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def test_train_refuses_a_dists_weight_without_weights(tmp_path):
    import train
    with pytest.raises(SystemExit, match="dists_weights"):
        train.main(["--config", _config(tmp_path, l_dists_weight=0.5), "--max-steps", "1"])
    with pytest.raises(SystemExit, match="dists_weights"):
        train.main(["--config", _config(tmp_path, l_dists_weight=0.5, dists_weights="/nonexistent/dists.pt"),
                    "--max-steps", "1"])


def test_train_refuses_a_dists_weight_outside_the_refine_step(tmp_path):
    import train
    with pytest.raises(SystemExit, match="l_dists_weight"):
        train.main(["--config", _config(tmp_path, l_dists_weight=0.5, is_refine=False, dists_weights=LIN),
                    "--max-steps", "1"])


def test_example_config_and_finetuner_requirement():
    from rdeic_amd.finetune import FineTuneConfig, FineTuner
    assert FineTuneConfig().l_dists_weight == 0.0 and FineTuneConfig(l_dists_weight=0.5).l_dists_weight == 0.5
    with pytest.raises(ValueError, match="DISTS"):  # refused at construction, before the model is touched
        FineTuner(None, FineTuneConfig(is_refine=True, l_dists_weight=0.5), lpips=object())
    with open(os.path.join(ROOT, "configs", "refine_dists.yaml")) as f:
        mc = yaml.safe_load(f)["model"]
    with open(os.path.join(ROOT, "configs", "refine.yaml")) as f:
        base = yaml.safe_load(f)["model"]
    assert mc["is_refine"] is True and mc["l_dists_weight"] > 0 and "dists_weights" in mc
    assert {k: v for k, v in mc.items() if k in base} == base  # the refine values, plus the DISTS keys
