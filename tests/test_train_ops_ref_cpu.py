"""The per-op training tests have power: CPU checks of tests/train_ops_ref.py.

* The float64 VQ restatement reproduces tests/golden/vq_resume.npz (the reference module's own outputs) within
  the tolerances tests/test_train_cli_gpu.py uses.
* Mutants: a deliberately wrong variant of the REFERENCE against the good reference, at the shapes of
  tests/test_train_ops_gpu.py. mixed_err(mutant, ref) must exceed 4x the bound the GPU test applies to that tensor
  (gross mutants: the bf16 bound 4 err_Y + sum_noise(N), computed here from the CPU yardstick of the very function
  the GPU test of that shape runs; fine mutants: the fp32 bound). A gross mutant must be flagged at EVERY shape where it changes the arithmetic at all (a kernel
  flip does nothing to a 1x1 kernel). A fine mutant perturbs by ~1/N (unbiased variance over N elements), which
  no 1e-4 test can see at N = 17408 or at c = 2048, shapes the kernels' branches require: it is asserted at every
  shape with fewer than ~1000 elements per statistic, which includes a cpg = 288 > 256 GroupNorm shape added for it.
* Tie conditions of the quantisation and VQ inputs hold for the seeds used, with no element excluded."""
import os

import numpy as np
import pytest
import torch

from tests import train_ops_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 4.0
EPS = 1e-5


def _flag(name, tensor, mutant, ref, bnd):
    err = R.mixed_err(mutant, ref)
    print(f"mutant {name}: {tensor} err {err:.3e} vs {MARGIN:g} x bound {bnd:.3e}")
    return err > MARGIN * bnd


# --------------------------------------------------------------------------------------------- metric
def test_mixed_err_holds_small_elements_to_the_rms():
    ref = torch.zeros(1000, dtype=torch.float64)
    ref[0] = 100.0
    got = ref.clone()
    got[5] = 0.5  # invisible to max|a-b| / max|b| at 5e-3
    assert R.mixed_err(got, ref) > 0.1
    assert R.mixed_err(ref, ref) == 0.0
    z = torch.zeros(4)
    assert R.mixed_err(z, z) == 0.0 and R.mixed_err(z + 1e-30, z) == float("inf")
    assert R.mixed_err(torch.full((3,), float("nan")), torch.ones(3)) == float("inf")


def test_round_bf16_matches_the_format():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(100000, generator=g) * torch.tensor(10.0) ** torch.randint(-20, 20, (100000,), generator=g)
    x[:4] = torch.tensor([1.00390625, 1.01171875, 0.0, -1.00390625])  # ties: to even
    r = R.bf16_round_(x)
    assert torch.equal(r, x.to(torch.bfloat16).float())
    assert r[0] == 1.0 and r[1] == 1.015625 and r[3] == -1.0
    t = x[:10].clone().requires_grad_(True)
    R.round_bf16(t).backward(x[10:20])
    assert torch.equal(t.grad, R.bf16_round_(x[10:20]))


# ------------------------------------------------------------------------------------------- VQ golden
def test_vq_restatement_reproduces_reference_golden():
    from oracle import weights_cpu
    g = np.load(os.path.join(ROOT, "tests", "golden", "vq_resume.npz"))
    z4 = torch.from_numpy(g["z"]).double()
    B, D, hz, wz = z4.shape
    K = g["embed_prob0"].shape[0]
    E0 = torch.from_numpy(weights_cpu.fill_uniform(K * D, int(g["e_seed"]), float(g["e_scale"]), 0.0)).view(K, D)
    z, E = R.leaves((z4.permute(0, 2, 3, 1).reshape(-1, D), E0), torch.float64)
    zq, loss, E_new, ep, idx = R.vq_train_ref(z, E, torch.from_numpy(g["embed_prob0"]).double(), 0.25, 0.99, 0.07)
    r = torch.from_numpy(g["r"]).double().permute(0, 2, 3, 1).reshape(-1, D)
    (loss + (zq * r).sum()).backward()

    def rel(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))

    def nchw(t):
        return t.detach().view(B, hz, wz, D).permute(0, 3, 1, 2).numpy()
    rows = torch.from_numpy(g["rows"])
    assert np.array_equal(idx.view(B, hz, wz).numpy(), g["idx"])
    checks = {
        "embed_prob": (rel(ep, g["embed_prob_after"]), 1e-5),
        "z_q": (rel(nchw(zq), g["zq"]), 1e-6),
        "loss": (abs(float(loss.detach()) - float(g["loss"])) / abs(float(g["loss"])), 1e-5),
        "codebook rows": (rel(E_new[rows], g["E_after_rows"]), 1e-5),
        "codebook row sums": (rel(E_new.sum(1), g["E_after_rowsum"]), 1e-5),
        "dz": (rel(nchw(z.grad), g["dz"]), 1e-4),
        "dE rows": (rel(E.grad[rows], g["dE_rows"]), 1e-4),
        "dE row norms": (rel(E.grad.norm(dim=1), g["dE_rownorm"]), 1e-4),
    }
    for name, (err, tol) in checks.items():
        print(f"{name}: rel err {err:.2e}")
        assert err < tol, (name, err)


# ---------------------------------------------------------------------------------------- norm mutants
def _gn_no_xhat_term(x, gamma, beta, groups, eps, silu):
    n, c = x.shape[0], x.shape[1]
    xg = x.reshape(n, groups, -1)
    mean = xg.mean(2, keepdim=True)
    var = xg.var(2, unbiased=False, keepdim=True).detach()  # no d(rstd)/dx: drops xhat * mean(g * xhat)
    y = ((xg - mean) / torch.sqrt(var + eps)).reshape(x.shape) * gamma.view(1, c, 1, 1) + beta.view(1, c, 1, 1)
    return y * torch.sigmoid(y) if silu else y


def _gn_silu_no_u_term(x, gamma, beta, groups, eps, silu):
    y = R.group_norm_core(x, gamma, beta, groups, eps, False)
    return y * torch.sigmoid(y).detach()  # silu' = s instead of s (1 + u (1 - s))


def _gn_unbiased(x, gamma, beta, groups, eps, silu):
    n, c = x.shape[0], x.shape[1]
    xg = x.reshape(n, groups, -1)
    mean = xg.mean(2, keepdim=True)
    m = xg.shape[2]
    var = xg.var(2, unbiased=False, keepdim=True) * (m / max(m - 1, 1))
    y = ((xg - mean) / torch.sqrt(var + eps)).reshape(x.shape) * gamma.view(1, c, 1, 1) + beta.view(1, c, 1, 1)
    return y * torch.sigmoid(y) if silu else y


def _gn_shifted_groups(x, gamma, beta, groups, eps, silu):
    # group boundaries one channel late: channel ch belongs to group (ch - 1) // cpg
    xs = x.roll(-1, dims=1)
    return R.group_norm_core(xs, gamma.roll(-1), beta.roll(-1), groups, eps, silu).roll(1, dims=1)


def _norm_runs(kind, case, silu, core, bf16, passthrough=False, use_res=True):
    """(reference, mutant, bounds) of one norm case. Reference, yardstick and bounds come from the function the
    GPU test of this shape runs: test_group_norm / test_layer_norm (passthrough False) or the passthrough tests."""
    if kind == "gn":
        inputs, gy, gres = R.gn_inputs(case, 3, bf16)

        def fn(x, gamma, beta, r, core=R.group_norm_core):
            return R.group_norm_op(x, gamma, beta, case[2], EPS, silu, r=r, passthrough=passthrough, core=core)
    else:
        inputs, gy, gres = R.ln_inputs(case, 4, bf16)

        def fn(x, gamma, beta, r, core=R.layer_norm_core):
            return R.layer_norm_op(x, gamma, beta, EPS, r=r, passthrough=passthrough, core=core)
    names = ["y", "alias"] if passthrough else ["y"]
    gouts = [gy, gres] if passthrough else [gy]
    ref, yard = R.reference_and_yardstick(fn, inputs, gouts, names, bf16)
    op = "group_norm" if kind == "gn" else "layer_norm"
    bounds = R.case_bounds(op, ref, yard, bf16, R.gn_n_sum(case) if kind == "gn" else R.ln_n_sum(case))
    mgouts = [gy, gres if use_res else None] if passthrough else [gy]
    mut = R.run_op(lambda **kw: fn(core=core, **kw), inputs, mgouts, names, torch.float64, R.ident)
    return ref, mut, bounds


@pytest.mark.parametrize("case", R.GN_CASES, ids=str)
def test_group_norm_gross_mutants_flagged_at_bf16_bound(case):
    for silu in (False, True):
        ref, mut, b = _norm_runs("gn", case, silu, _gn_no_xhat_term, True)
        assert _flag("gn no xhat term", "dx", mut["dx"], ref["dx"], b["dx"][0])
        ref, mut, b = _norm_runs("gn", case, silu, R.group_norm_core, True, passthrough=True, use_res=False)
        assert _flag("gn dres omitted", "dx", mut["dx"], ref["dx"], b["dx"][0])
        assert _flag("gn dgamma/dbeta swapped", "dgamma", ref["dbeta"], ref["dgamma"], b["dgamma"][0])
        assert _flag("gn dgamma/dbeta swapped", "dbeta", ref["dgamma"], ref["dbeta"], b["dbeta"][0])
    ref, mut, b = _norm_runs("gn", case, True, _gn_silu_no_u_term, True)
    assert _flag("silu' without u(1-s)", "dx", mut["dx"], ref["dx"], b["dx"][0])
    assert _flag("silu' without u(1-s)", "dgamma", mut["dgamma"], ref["dgamma"], b["dgamma"][0])


def test_group_norm_fine_mutants_flagged_at_fp32_bound():
    caught = {"unbiased": [], "shifted": []}
    for case in R.GN_CASES:
        n, c, groups, h, w = case
        ref, mut, b = _norm_runs("gn", case, False, _gn_unbiased, False)
        if _flag("gn unbiased variance", "y", mut["y"], ref["y"], b["y"][0]):
            caught["unbiased"].append(case)
        ref, mut, b = _norm_runs("gn", case, False, _gn_shifted_groups, False)
        hit = _flag("gn group boundary off by one", "y", mut["y"], ref["y"], b["y"][0])
        assert hit == (c // groups > 1), case  # cpg = 1: every channel is its own group either way
        if hit:
            caught["shifted"].append(case)
    # 1/N relative change of the variance, half of it in y: visible at 4e-4 only below ~1000 elements per group
    small = {(2, 32, 32, 3, 11), (1, 320, 32, 8, 8), (3, 640, 32, 5, 7), (1, 576, 2, 1, 2)}
    assert small <= set(caught["unbiased"])
    assert len(caught["shifted"]) == 5


def _ln_no_xhat_term(x, gamma, beta, eps):
    mean = x.mean(1, keepdim=True)
    var = x.var(1, unbiased=False, keepdim=True).detach()
    return (x - mean) / torch.sqrt(var + eps) * gamma + beta


def _ln_unbiased(x, gamma, beta, eps):
    mean = x.mean(1, keepdim=True)
    var = x.var(1, unbiased=True, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma + beta


@pytest.mark.parametrize("case", R.LN_CASES, ids=str)
def test_layer_norm_gross_mutants_flagged_at_bf16_bound(case):
    ref, mut, b = _norm_runs("ln", case, False, _ln_no_xhat_term, True)
    assert _flag("ln no xhat term", "dx", mut["dx"], ref["dx"], b["dx"][0])
    ref, mut, b = _norm_runs("ln", case, False, R.layer_norm_core, True, passthrough=True, use_res=False)
    assert _flag("ln dres omitted", "dx", mut["dx"], ref["dx"], b["dx"][0])
    assert _flag("ln dgamma/dbeta swapped", "dgamma", ref["dbeta"], ref["dgamma"], b["dgamma"][0])
    assert _flag("ln dgamma/dbeta swapped", "dbeta", ref["dgamma"], ref["dbeta"], b["dbeta"][0])


def test_layer_norm_fine_mutant_flagged_at_fp32_bound():
    caught = []
    for case in R.LN_CASES:
        ref, mut, b = _norm_runs("ln", case, False, _ln_unbiased, False)
        if _flag("ln unbiased variance", "y", mut["y"], ref["y"], b["y"][0]):
            caught.append(case)
    assert {(1, 64), (5, 72), (1025, 320), (2500, 64)} <= set(caught)  # 1/(2c) > 4e-4 up to c = 320


# ---------------------------------------------------------------------------------------- conv mutants
CONV = R.conv_case_list()


@pytest.mark.parametrize("cid,case,n,h,w", CONV, ids=[c[0] for c in CONV])
def test_conv_dgrad_mutants_flagged_at_bf16_bound(cid, case, n, h, w):
    cin, cout, k, stride, pad, up2, ps, act, slope, use_emb, use_res, out_f32 = case
    inputs, gout = R.conv_inputs(case, n, h, w, 2, True)
    names = ["out"]
    ref, yard = R.reference_and_yardstick(R.conv_fn(case), inputs, [gout], names, True)
    b = R.case_bounds("conv", ref, yard, True, R.conv_n_sum(case, n, h, w))
    dz = R.conv_dz(case, inputs, gout)
    W = inputs["W"].double()
    good = R.conv_dgrad_manual(dz, W, case, (h, w))
    assert R.mixed_err(good, ref["dx"]) < 1e-12  # the hand-written dgrad is the autograd gradient
    if k > 1:
        assert _flag("dgrad without the kernel flip", "dx", R.conv_dgrad_manual(dz, W, case, (h, w), flip=False),
                     ref["dx"], b["dx"][0])
    if stride == 2:
        assert _flag("zero-insert at odd positions", "dx", R.conv_dgrad_manual(dz, W, case, (h, w), odd=True),
                     ref["dx"], b["dx"][0])
    if up2:
        assert _flag("sum-pool of 3 of 4 pixels", "dx", R.conv_dgrad_manual(dz, W, case, (h, w), pool_pixels=3),
                     ref["dx"], b["dx"][0])
    if use_res:
        assert _flag("dres omitted", "dres", torch.zeros_like(ref["dres"]), ref["dres"], b["dres"][0])
    if ps:
        # the PixelShuffle backward with sub-pixel order 2j + i permutes dz's channels, and with them db and dW
        dps = torch.nn.functional.pixel_shuffle(dz, 2)  # gradient at the shuffled resolution
        assert torch.equal(R.pixel_unshuffle2_ref(dps), dz)
        bad = R.pixel_unshuffle2_ref(dps, swapped=True)
        assert _flag("unshuffle order 2j + i", "db", bad.sum((0, 2, 3)), ref["db"], b["db"][0])


def test_layout_refs_against_torch():
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2, 3, 6, 10), generator=g, dtype=torch.float64)
    assert torch.equal(R.pixel_unshuffle2_ref(x), torch.nn.functional.pixel_unshuffle(x, 2))
    assert not torch.equal(R.pixel_unshuffle2_ref(x, swapped=True), R.pixel_unshuffle2_ref(x))
    assert R.mixed_err(R.sum_pool2_ref(x), torch.nn.functional.avg_pool2d(x, 2) * 4) < 1e-15
    assert R.mixed_err(R.sum_pool2_ref(x, 3), R.sum_pool2_ref(x)) > 0.1
    xs = torch.randn((2, 3, 5, 7), generator=g, dtype=torch.float64)
    # (k, stride, pad, up2) against F.unfold of the (upsampled) input; unfold orders (c, tap), im2col (tap, c)
    for k, stride, pad, up2 in ((3, 1, 1, False), (3, 2, 1, False), (3, 1, 1, True), (4, 2, 1, True), (1, 1, 0, False)):
        src = xs.repeat_interleave(2, 2).repeat_interleave(2, 3) if up2 else xs
        ho = (src.shape[2] + 2 * pad - k) // stride + 1
        wo = (src.shape[3] + 2 * pad - k) // stride + 1
        cols = R.im2col_ref(xs, k, k, stride, pad, ho, wo, up2)
        unf = torch.nn.functional.unfold(src, k, padding=pad, stride=stride)
        unf = unf.view(2, 3, k * k, ho * wo).permute(0, 3, 2, 1).reshape(2 * ho * wo, k * k * 3)
        assert torch.equal(cols, unf), (k, stride, pad, up2)
    z = R.zero_insert2_ref(xs)
    assert torch.equal(z[:, :, ::2, ::2], xs) and float(z.abs().sum()) == float(xs.abs().sum())


# ----------------------------------------------------------------------------- checkerboard: ties, mutants
CKBD_SEED = 7


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_ckbd_quantisation_inputs_are_away_from_ties(bf16):
    inputs, noise, gA, gN = R.ckbd_inputs(CKBD_SEED, bf16)
    y, pa, pn = inputs["y"], inputs["pa"], inputs["pn"]
    c = y.shape[1]
    ma = R.anchor_mask(y.shape[2], y.shape[3], torch.float32)
    mu = pa[:, c:] * ma + pn[:, c:] * (1 - ma)   # each position is quantised against its own half's mean: all of y
    f = R.quant_fracs(y, mu)
    ok = ((f >= 0.05) & (f <= 0.45)) | ((f >= 0.55) & (f <= 0.95))
    assert bool(ok.all()), f[~ok]
    # the case reaches what it claims: scales on both sides of 0.11 and the 1e-9 likelihood floor
    s = pa[:, :c] * ma + pn[:, :c] * (1 - ma)
    assert bool((s < 0.11).any()) and bool((s > 0.11).any()) and not bool((s == 0.11).any())
    from oracle import train_ref
    v = (y.double() + noise.double() - mu.double()).abs()
    sd = s.double().clamp_min(0.11)
    lik = train_ref.standardized_cumulative((0.5 - v) / sd) - train_ref.standardized_cumulative((-0.5 - v) / sd)
    assert bool((lik < 1e-9).any()) and bool((lik > 1e-9).any())
    # ... and no likelihood sits on the floor's decision boundary (an fp32 kernel could fall either side)
    assert float(((lik - 1e-9).abs() / 1e-9).min()) > 1e-3


def _ckbd_runs(bf16, **kw):
    inputs, noise, gA, gN = R.ckbd_inputs(CKBD_SEED, bf16)

    def fn(y, pa, pn, r, **extra):
        return R.ckbd_op(y, pa, pn, noise.to(y.dtype), r=r, **extra)
    names = ["anchor", "S", "non"]
    gouts = [gA, -0.7, gN]
    ref, yard = R.reference_and_yardstick(fn, inputs, gouts, names, bf16)
    b = R.case_bounds("ckbd", ref, yard, bf16, inputs["y"].numel())
    mut = R.run_op(lambda **a: fn(**a, **kw), inputs, gouts, names, torch.float64, R.ident)
    return ref, mut, b


def test_ckbd_mutants():
    ref, mut, b = _ckbd_runs(True, flipped=True)
    for t in ("anchor", "non", "dy", "dpa", "dpn"):
        assert _flag("anchor parity flipped", t, mut[t], ref[t], b[t][0])
    ref, mut, b = _ckbd_runs(False, lower_bound=R.plain_bound)
    assert R.mixed_err(mut["S"], ref["S"]) == 0.0  # a backward-only mutant
    assert _flag("LowerBound backward rule dropped", "dpa", mut["dpa"], ref["dpa"], b["dpa"][0])
    assert _flag("LowerBound backward rule dropped", "dpn", mut["dpn"], ref["dpn"], b["dpn"][0])
    assert _flag("LowerBound backward rule dropped", "dy", mut["dy"], ref["dy"], b["dy"][0])


# ------------------------------------------------------------------------------------- VQ: ties, mutant
@pytest.mark.parametrize("case", R.VQ_CASES, ids=str)
def test_vq_inputs_are_away_from_ties(case):
    z, E, ep, gz = R.vq_inputs(case, R.VQ_SEEDS[case])
    row_gap, code_gap = R.vq_gaps(z, E)
    print(f"vq {case}: nearest-code gap {row_gap:.3e}, closest-point gap {code_gap:.3e}")
    assert row_gap > 1e-3 and code_gap > 1e-3
    P, K, D = case
    a = torch.exp(-(ep.double() * 0.99 * K * 1000.0) - 1e-3)  # lower bound of the usage EMA: both regimes present
    assert float(a.max()) > 0.5 and float(a.min()) < 0.01


def test_vq_npos_mutant_flagged_at_fp32_bound():
    case = (192, 16, 8)  # P // K = 12
    ref, _ = R.vq_reference(case, R.VQ_SEEDS[case])
    mut, _ = R.vq_reference(case, R.VQ_SEEDS[case], npos_fixed=1)
    assert _flag("npos fixed at 1", "loss", mut["loss"], ref["loss"], R.FP32_BOUND["vq"])
    assert _flag("npos fixed at 1", "dE", mut["dE"], ref["dE"], R.FP32_BOUND["vq"])
    for case in R.VQ_CASES:  # the restatement's autograd quirk is what the header says: finite, non-trivial gradients
        ref, idx = R.vq_reference(case, R.VQ_SEEDS[case])
        assert all(bool(torch.isfinite(v).all()) for v in ref.values())
        assert float(ref["dE"].abs().max()) > 0 and len(torch.unique(idx)) > 1
