"""train.py on image files with validation epochs (rdeic_amd/data.py, rdeic_amd/validate.py,
FineTuner.sync_inference), once with the captured step and once with --eager.

Three seeded PNGs (synth_image at 200x260, 260x200 and 192x192) are the training list (random 192 crops, hflip)
and the validation list (center crops). train.main runs 4 fp32 steps with val_check_interval 2:
1. validation rows exist at steps 2 and 4, finite, avg_bpp > 0, 0 < usage <= 1;
2. the step-4 checkpoint equals, bit for bit, that of the same run without data.val: validation does not
   perturb training;
3. a fresh RDEIC loaded from the step-2 checkpoint gives, through Validator, the bodies and metrics of the in-run
   validation at step 2: no stale packed weights, launch plans or tables in the training process;
4. resuming from the step-2 checkpoint reproduces the step-4 checkpoint bit for bit on file data (the loader
   seeks; nothing is replayed).
The runs are shared between the tests of one mode."""
import math
import os

import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
S = 192
SIZES = [(200, 260), (260, 200), (192, 192)]  # (w, h)


@pytest.fixture(scope="module")
def lists(tmp_path_factory):
    from PIL import Image

    from rdeic_amd.synthetic import synth_image
    td = tmp_path_factory.mktemp("val_imgs")
    paths = []
    for i, (w, h) in enumerate(SIZES):
        paths.append(str(td / f"{i}.png"))
        Image.fromarray(synth_image(h, w, 900 + i)).save(paths[-1])
    lst = td / "files.list"
    lst.write_text("\n".join(paths) + "\n")
    return str(lst)


def _section(lst, crop, hflip, shuffle):
    return dict(file_list=lst, out_size=S, crop_type=crop, use_hflip=hflip, use_rot=False, batch_size=1,
                shuffle=shuffle, drop_last=True, num_workers=2)


class Runs:
    """train.main runs of one mode, made on first use: full (with validation), plain (no data.val), resumed."""

    def __init__(self, tmp, lst, flags):
        self.tmp, self.lst, self.flags, self.done = tmp, lst, flags, {}

    def cfg(self, name, val, resume=None):
        data = {"train": _section(self.lst, "random", True, True)}
        if val:
            data["val"] = _section(self.lst, "center", False, False)
        cfg = {"data": data,
               "model": {"learning_rate": 2e-5, "l_guide_weight": 3.0, "l_bpp_weight": 1.0, "used_timesteps": 300,
                         "sd_locked": True, "is_refine": False, "precision": 32, "resume": resume},
               "lightning": {"seed": 231, "trainer": {"max_steps": 4, "log_every_n_steps": 1,
                                                      "val_check_interval": 2},
                             "checkpoint": {"every_n_train_steps": 2, "dirpath": str(self.tmp / name)}}}
        p = self.tmp / f"{name}.yaml"
        p.write_text(yaml.safe_dump(cfg))
        return str(p)

    def ck(self, name, step):
        return str(self.tmp / name / f"ood_finetune_step={step}.safetensors")

    def get(self, name):
        import train
        if name not in self.done:
            resume = self.ck("full", 2) if name == "resumed" else None
            if resume:
                self.get("full")
            self.done[name] = train.main(["--config", self.cfg(name, val=name != "plain", resume=resume)] + self.flags)
        return self.done[name]


@pytest.fixture(scope="module", params=["captured", "eager"])
def runs(request, gpu, lists, tmp_path_factory):
    return Runs(tmp_path_factory.mktemp(request.param), lists, ["--eager"] if request.param == "eager" else [])


def _same_checkpoint(a, b):
    from safetensors.torch import load_file
    x, y = load_file(a), load_file(b)
    assert set(x) == set(y)
    diff = [k for k in x if not torch.equal(x[k], y[k])]
    assert not diff, diff[:5]


def test_validation_rows(runs):
    recs = runs.get("full")
    train_rows = [r for r in recs if "T/loss" in r]
    val_rows = [r for r in recs if "avg_bpp" in r]
    assert [r["global_step"] for r in train_rows] == [1, 2, 3, 4]
    assert [r["global_step"] for r in val_rows] == [2, 4]
    for r in val_rows:
        print(r)
        assert r["images"] == 3 and "avg_lpips" not in r
        for k in ("avg_bpp", "usage", "avg_psnr", "avg_ssim", "avg_ms_ssim"):
            assert math.isfinite(r[k]), (k, r)
        assert r["avg_bpp"] > 0 and 0 < r["usage"] <= 1
    assert val_rows[0]["bodies_sha256"] != val_rows[1]["bodies_sha256"]  # the second epoch saw the updated weights


def test_validation_does_not_perturb_training(runs):
    runs.get("full"), runs.get("plain")
    assert all("avg_bpp" not in r for r in runs.get("plain"))
    _same_checkpoint(runs.ck("full", 4), runs.ck("plain", 4))


def test_fresh_model_reproduces_in_run_validation(runs, lists):
    import train
    from rdeic_amd.data import ImageListLoader
    from rdeic_amd.rdeic import RDEIC
    from rdeic_amd.validate import Validator
    in_run = [r for r in runs.get("full") if "avg_bpp" in r][0]
    dev = torch.device("cuda")
    model = RDEIC(compute_dtype=torch.float32, device=dev).init_synthetic()
    sd, meta = train.load_state(runs.ck("full", 2))
    assert meta["global_step"] == "2"
    model.load_state_dict(sd, strict=False)
    loader = ImageListLoader(lists, S, "center", False, False, 1, False, True, 231, device=dev, threads=2)
    rec = Validator(model, None, loader, steps=5, seed=231).run(2)
    loader.close()
    rec = {k: (round(v, 6) if isinstance(v, float) else v) for k, v in rec.items()}
    assert rec == in_run


def test_resume_on_files_is_bit_exact(runs):
    full, resumed = runs.get("full"), runs.get("resumed")
    assert [r["global_step"] for r in resumed if "T/loss" in r] == [3, 4]
    for a, b in zip([r for r in full if "T/loss" in r][2:], [r for r in resumed if "T/loss" in r]):
        assert a["T/loss"] == b["T/loss"], (a, b)
    assert [r for r in resumed if "avg_bpp" in r] == [r for r in full if "avg_bpp" in r][1:]
    _same_checkpoint(runs.ck("full", 4), runs.ck("resumed", 4))
