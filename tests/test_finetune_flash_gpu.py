"""The bf16 fine-tune step with each attention implementation forced ("flash": attention_bwd.hip's LSE forward
and recomputing backward; "materialized": P kept, strided GEMMs), so both stay exercised whatever the default.
Same assertions as test_finetune_gpu.test_bf16_step_tracks_the_reference (loss terms within bf16 tolerance of
the fp32 reference step in tests/golden/train_128.npz, > 0.9 update-direction agreement) and the same
captured-step criterion as test_captured_step_replays_the_eager_steps, at 128^2."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = "tests/golden/train_128.npz"
SIZE = 128


@pytest.fixture
def impl(request):
    from rdeic_amd import autograd as AG
    prev = AG.get_attention_impl()
    AG.set_attention_impl(request.param)
    yield request.param
    AG.set_attention_impl(prev)


@pytest.mark.parametrize("impl", ["flash", "materialized"], indirect=True)
def test_bf16_step_tracks_the_reference(gpu, impl):
    from tests.test_finetune_gpu import _run_step
    g = np.load(GOLD)
    ft, ld = _run_step(torch.bfloat16, size=SIZE)
    assert all(np.isfinite(v) for v in ld.values())
    for ours, ref, tol in (("T/l_simple", "loss_l_simple", 0.1), ("T/l_guide", "loss_l_guide", 0.05),
                           ("T/l_bpp", "loss_l_bpp", 0.05), ("T/l_emb", "loss_l_emb", 0.1)):
        r = float(g[ref])
        assert abs(ld[ours] - r) <= tol * abs(r), (impl, ours, ld[ours], r)
    # the update direction against the reference gradient: sign(p_after - p_before) ~ -sign(grad)
    names = [str(n) for n in g["grad_names"]]
    agree, total = 0, 0
    from rdeic_amd import weights as W
    from oracle import weights_cpu
    for n in names[:200]:
        o, k = ft.offsets[n]
        if ("grad:" + n) not in g.files:
            continue
        shape = tuple(g["grad:" + n].shape)
        scale, offset = W.init_spec(n, shape)
        p0 = torch.from_numpy(weights_cpu.fill_uniform(int(np.prod(shape)), W.param_seed(n), scale, offset))
        step = (ft.flat[o:o + k].cpu() - p0).numpy()
        ref_g = g["grad:" + n].reshape(-1)
        big = np.abs(ref_g) > 1e-3 * np.abs(ref_g).max()
        agree += int((np.sign(step[big]) == -np.sign(ref_g[big])).sum())
        total += int(big.sum())
    print(f"\n[finetune_flash] {impl}: update-direction agreement {agree / max(total, 1):.4f}, losses {ld}")
    assert total > 0 and agree / total > 0.9, (impl, agree, total)


@pytest.mark.parametrize("impl", ["flash"], indirect=True)
def test_captured_flash_step_replays_the_eager_steps(gpu, impl):
    """CapturedStep under "flash" reproduces two eager steps bit for bit: parameters, AdamW moments, VQ usage
    EMA and the loss dict."""
    from rdeic_amd.finetune import CapturedStep, FineTuner, nchw_draws_to_nhwc
    from rdeic_amd.rdeic import RDEIC
    from rdeic_amd.synthetic import synth_context, synth_image, train_draws
    ctx = synth_context().cuda()
    imgs = [torch.from_numpy(synth_image(SIZE, SIZE, 300 + i)).cuda()[None] for i in range(2)]
    runs = []
    for captured in (False, True):
        m = RDEIC(compute_dtype=torch.bfloat16).init_synthetic()
        ft = FineTuner(m)
        draws = [nchw_draws_to_nhwc(train_draws(1, SIZE // 8, SIZE // 8, m.cfg["compression"]["slice_ch"], 40 + i,
                                                m.used_timesteps), "cuda") for i in range(2)]
        cs = CapturedStep(ft, imgs[0], ctx, draws[0]) if captured else None
        losses = []
        for i in range(2):
            d = cs.step(imgs[i], draws[i]) if captured else ft.training_step(imgs[i], ctx, draws[i])
            losses.append({k: float(v.detach()) for k, v in d.items()})
        torch.cuda.synchronize()
        runs.append((ft.flat.cpu(), ft.exp_avg.cpu(), ft.exp_avg_sq.cpu(), ft.embed_prob.cpu(), losses))
    (p0, m0, v0, e0, l0), (p1, m1, v1, e1, l1) = runs
    assert torch.equal(p0, p1) and torch.equal(m0, m1) and torch.equal(v0, v1) and torch.equal(e0, e1)
    assert l0 == l1
    assert all(np.isfinite(v) for d in l0 for v in d.values())
