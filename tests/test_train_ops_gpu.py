"""Per-op checks of the training kernels (train.hip through rdeic_amd/autograd.py) against the float64
references of tests/train_ops_ref.py, in fp32 and in bf16, at the smallest shapes that reach each branch.

Metric and bounds are those of tests/train_ops_ref.py: mixed_err = max |got - ref| / (|ref| + rms(ref));
fp32 mode 1e-5 (conv / linear / GEMM / act / GEGLU) and 1e-4 (norms, checkerboard, VQ gradients); bf16 mode
4 x err_Y of the same tensor and case (the fp32 + RoundBF16 yardstick) + sum_noise(N) = sqrt(N) * 2^-24, the
fp32 summation-order noise of the case's longest sum (1e-6 at N = 300; arithmetic in train_ops_ref.py). Data
movement (im2col, zero_insert2, pixel_unshuffle2, ckbd_mask, the quantised checkerboard halves away from ties)
must be bit-exact. Every check prints `op, tensor, err_ours, err_Y, ratio`; tests/test_train_ops_ref_cpu.py shows
that these bounds flag wrong kernels.

Worst err_ours / err_Y per op, measured on an MI355X (bf16 mode; printed per op when the module finishes):
  op           rounded tensors   fp32-only tensors   fp32 mode, worst err / bound
  group_norm        1.00              1.72                  0.12
  layer_norm        1.00              2.02                  0.01
  conv              1.00              1.34                  0.21
  linear            1.00              1.72                  0.07
  gemm              1.00              0.89                  0.07
  act               1.00               -                    0.04
  geglu             1.00               -                    0.01
  ckbd              1.00              1.00                  0.03
  vq (fp32 only)     -                 -                    0.12
"rounded tensors": every tensor whose yardstick contains a bf16 rounding (err_Y 8e-5 .. 8e-3); the kernels round
the same fp32 value as the yardstick almost everywhere, so the worst element and its error coincide and the factor
4 is never used. "fp32-only tensors": parameter gradients and fp32 outputs computed from exact bf16 inputs, where
err_Y is the fp32 summation noise of the host's order (~1e-7, e.g. LayerNorm dgamma 1.3e-7 vs 6.2e-8) and the
ratio compares two summation orders; where err_Y was exactly 0 (demb, dres, some row sums) ours was 0 as well.
"""
import math

import pytest
import torch

from tests import train_ops_ref as R

pytestmark = pytest.mark.gpu
EPS = 1e-5
DTS = [False, True]
DT_IDS = ["fp32", "bf16"]
WORST = {}
ROUNDED_ERR_Y = 1e-5  # a yardstick with a bf16 rounding errs by >= 8e-5 in every case here, one without by <= 1e-6


def _dt(bf16):
    return torch.bfloat16 if bf16 else torch.float32


def _dev(t, bf16=False, nhwc=False):
    """An fp32 CPU tensor of compute-dtype values -> the kernel's tensor (exact cast)."""
    if t is None:
        return None
    if nhwc:
        t = t.permute(0, 2, 3, 1)
    return t.contiguous().to(_dt(bf16)).cuda()


def _nchw(t):
    return t.detach().permute(0, 3, 1, 2)


def _wide(t, pad_l, pad_r):
    """t as a channel slice of a wider tensor filled with a sentinel: (leaf-able wide tensor, slice)."""
    shape = tuple(t.shape[:-1]) + (t.shape[-1] + pad_l + pad_r,)
    wide = torch.full(shape, 3.0, dtype=t.dtype, device=t.device)
    wide[..., pad_l:pad_l + t.shape[-1]] = t
    return wide, slice(pad_l, pad_l + t.shape[-1])


class Checker:
    def __init__(self, op, case, bf16, n_sum=1):
        """n_sum: the longest sum behind one output element of the case (train_ops_ref.bound)."""
        self.op, self.case, self.bf16, self.n_sum, self.bad = op, case, bf16, n_sum, []

    def __call__(self, name, got, ref, yard=None):
        ey = R.mixed_err(yard, ref) if (self.bf16 and yard is not None) else 0.0
        bnd = R.bound(self.op, self.bf16, ey, self.n_sum)
        err = R.mixed_err(got.float() if got.dtype == torch.bfloat16 else got, ref)
        ratio = err / ey if ey > 0 else (0.0 if err == 0 else math.inf)
        print(f"{self.op}, {self.case} {'bf16' if self.bf16 else 'fp32'} {name}, err_ours {err:.3e}, err_Y {ey:.3e}, "
              f"ratio {ratio:.2f}, bound {bnd:.3e}")
        w = WORST.setdefault(self.op, {"rounded": 0.0, "fp32-only": 0.0, "fp32-only err_Y = 0, err_ours": 0.0,
                                       "fp32 mode err / bound": 0.0})
        if not self.bf16:
            w["fp32 mode err / bound"] = max(w["fp32 mode err / bound"], err / bnd)
        elif ey > ROUNDED_ERR_Y:
            w["rounded"] = max(w["rounded"], ratio)
        elif ey > 0:
            w["fp32-only"] = max(w["fp32-only"], ratio)
        else:
            w["fp32-only err_Y = 0, err_ours"] = max(w["fp32-only err_Y = 0, err_ours"], err)
        if not err <= bnd:
            self.bad.append((name, err, bnd))

    def all(self, got: dict, ref: dict, yard):
        for k, v in ref.items():
            self(k, got[k], v, None if yard is None else yard[k])

    def done(self):
        assert not self.bad, (self.op, self.case, self.bad)


@pytest.fixture(scope="module", autouse=True)
def _worst_ratio_table():
    yield
    for op, w in sorted(WORST.items()):  # the docstring's table
        print(f"\nworst, {op}: " + ", ".join(f"{k} {v:.3g}" for k, v in w.items()))


# ------------------------------------------------------------------------------------------ GroupNorm
def _gn_fn(case, silu, passthrough):
    def fn(x, gamma, beta, r):
        return R.group_norm_op(x, gamma, beta, case[2], EPS, silu, r=r, passthrough=passthrough)
    return fn


def _run_norm(kind, case, silu, bf16, inputs, gy, gres, passthrough, strided=False):
    """Our norm on the device -> dict like run_op's (NCHW / [rows, c], CPU)."""
    from rdeic_amd import autograd as AG
    gn = kind == "gn"
    x = _dev(inputs["x"], bf16, nhwc=gn)
    if strided:
        leaf, sl = _wide(x, 32, 32)
        leaf.requires_grad_(True)
        xo = leaf[..., sl]
    else:
        leaf = xo = x.requires_grad_(True)
    go, bo = _dev(inputs["gamma"]).requires_grad_(True), _dev(inputs["beta"]).requires_grad_(True)
    if gn:
        out = AG.group_norm(xo, go, bo, case[2], EPS, silu, passthrough)
    else:
        out = AG.layer_norm(xo, go, bo, EPS, passthrough)
    outs = out if passthrough else (out,)
    gys = [_dev(gy, bf16, nhwc=gn)] + ([_dev(gres, bf16, nhwc=gn)] if passthrough and gres is not None else [])
    torch.autograd.backward(list(outs[:len(gys)]), gys)
    torch.cuda.synchronize()
    dx = leaf.grad
    if strided:
        rest = dx.clone()
        rest[..., sl] = 0
        assert not bool(rest.any()), "gradient written outside the slice"
        dx = dx[..., sl]
    conv = _nchw if gn else (lambda t: t.detach())
    got = {"y": conv(outs[0]).cpu(), "dx": conv(dx).cpu(), "dgamma": go.grad.cpu(), "dbeta": bo.grad.cpu()}
    if passthrough:
        got["alias"] = conv(outs[1]).cpu()
    return got


@pytest.mark.parametrize("bf16", DTS, ids=DT_IDS)
@pytest.mark.parametrize("silu", [False, True], ids=["plain", "silu"])
@pytest.mark.parametrize("case", R.GN_CASES, ids=str)
def test_group_norm(gpu, case, silu, bf16):
    inputs, gy, _ = R.gn_inputs(case, 3, bf16)
    ref, yard = R.reference_and_yardstick(_gn_fn(case, silu, False), inputs, [gy], ["y"], bf16)
    got = _run_norm("gn", case, silu, bf16, inputs, gy, None, False)
    ck = Checker("group_norm", (case, silu), bf16, R.gn_n_sum(case))
    ck.all(got, ref, yard)
    ck.done()


@pytest.mark.parametrize("bf16", DTS, ids=DT_IDS)
def test_group_norm_channel_slice_of_wider_tensor(gpu, bf16):
    case = (1, 320, 32, 8, 8)  # pixel stride 384 != c
    inputs, gy, _ = R.gn_inputs(case, 31, bf16)
    ref, yard = R.reference_and_yardstick(_gn_fn(case, True, False), inputs, [gy], ["y"], bf16)
    got = _run_norm("gn", case, True, bf16, inputs, gy, None, False, strided=True)
    ck = Checker("group_norm", (case, "strided"), bf16, R.gn_n_sum(case))
    ck.all(got, ref, yard)
    ck.done()


@pytest.mark.parametrize("bf16", DTS, ids=DT_IDS)
def test_group_norm_large_mean_small_spread(gpu, bf16):
    case = (1, 320, 32, 8, 8)
    inputs, gy, _ = R.gn_inputs(case, 32, bf16, mean=6.0 if bf16 else 50.0, spread=0.5)
    ref, yard = R.reference_and_yardstick(_gn_fn(case, True, False), inputs, [gy], ["y"], bf16)
    got = _run_norm("gn", case, True, bf16, inputs, gy, None, False)
    ck = Checker("group_norm", (case, "large mean"), bf16, R.gn_n_sum(case))
    ck.all(got, ref, yard)
    ck.done()


@pytest.mark.parametrize("bf16", DTS, ids=DT_IDS)
@pytest.mark.parametrize("alias_grad", [True, False], ids=["dres", "no_dres"])
@pytest.mark.parametrize("case", [(2, 32, 32, 3, 11), (3, 640, 32, 5, 7)], ids=str)
def test_group_norm_passthrough(gpu, case, alias_grad, bf16):
    inputs, gy, gres = R.gn_inputs(case, 33, bf16)
    gouts = [gy, gres if alias_grad else None]
    ref, yard = R.reference_and_yardstick(_gn_fn(case, True, True), inputs, gouts, ["y", "alias"], bf16)
    got = _run_norm("gn", case, True, bf16, inputs, gy, gres if alias_grad else None, True)
    assert torch.equal(got["alias"].float(), inputs["x"])
    ck = Checker("group_norm", (case, "passthrough", alias_grad), bf16, R.gn_n_sum(case))
    ck.all(got, ref, yard)
    ck.done()


def _direct_views(params: dict, seed: int):
    """Give each parameter a pre-filled fp32 gradient view (slices of one flat buffer) and a notify hook that
    records (name, view at that moment). Returns (prefill clones, events)."""
    g = torch.Generator().manual_seed(seed)
    total = sum(p.numel() for p in params.values())
    flat = torch.randn(total + 2 * len(params), generator=g).cuda()
    pre, events, off = {}, [], 1
    for name, p in params.items():
        view = flat[off:off + p.numel()].view(p.shape)
        off += p.numel() + 2
        p._rdeic_gview = view
        p._rdeic_notify = (lambda t, name=name: events.append((name, t._rdeic_gview.detach().clone())))
        pre[name] = view.detach().clone().cpu()
    return pre, events, flat


def _check_direct(ck, params, pre, events, refs, yards, flat):
    """views = prefill + sum of the uses' gradients; .grad None; one notification each, at the full sum."""
    torch.cuda.synchronize()
    assert sorted(n for n, _ in events) == sorted(params), events
    used = torch.zeros_like(flat, dtype=torch.bool)
    for name, p in params.items():
        assert p.grad is None and p._rdeic_uses == 0
        want = pre[name].double() + sum(r["d" + name].double() for r in refs)
        yard = None if yards is None else pre[name] + sum(y["d" + name] for y in yards)
        ck("view " + name, p._rdeic_gview.cpu(), want, yard)
        at_notify = dict(events)[name]
        assert torch.equal(at_notify, p._rdeic_gview), f"{name} notified before its last gradient"
        used[(p._rdeic_gview.data_ptr() - flat.data_ptr()) // 4:][:p.numel()] = True
    return used


@pytest.mark.parametrize("bf16", DTS, ids=DT_IDS)
@pytest.mark.parametrize("kind", ["gn", "ln"])
def test_norm_direct_gradient_views_shared_by_two_norms(gpu, kind, bf16):
    from rdeic_amd import autograd as AG
    gn = kind == "gn"
    cases = [(1, 320, 32, 8, 8), (2, 320, 32, 3, 11)] if gn else [(5, 72), (1025, 72)]
    mk = R.gn_inputs if gn else R.ln_inputs
    runs = [mk(c, 40 + i, bf16) for i, c in enumerate(cases)]
    for inp, _, _ in runs[1:]:
        inp["gamma"], inp["beta"] = runs[0][0]["gamma"], runs[0][0]["beta"]
    refs, yards = [], []
    for c, (inp, gy, _) in zip(cases, runs):
        fn = _gn_fn(c, True, False) if gn else (lambda x, gamma, beta, r: R.layer_norm_op(x, gamma, beta, EPS, r=r))
        ref, yard = R.reference_and_yardstick(fn, inp, [gy], ["y"], bf16)
        refs.append(ref)
        yards.append(yard)
    params = {"gamma": _dev(runs[0][0]["gamma"]).requires_grad_(True),
              "beta": _dev(runs[0][0]["beta"]).requires_grad_(True)}
    pre, events, flat = _direct_views(params, 41)
    flat0 = flat.clone()
    ys, gys, xs = [], [], []
    for c, (inp, gy, _) in zip(cases, runs):
        x = _dev(inp["x"], bf16, nhwc=gn).requires_grad_(True)
        xs.append(x)
        ys.append(AG.group_norm(x, params["gamma"], params["beta"], c[2], EPS, True) if gn
                  else AG.layer_norm(x, params["gamma"], params["beta"], EPS))
        gys.append(_dev(gy, bf16, nhwc=gn))
    assert params["gamma"]._rdeic_uses == 2 and params["beta"]._rdeic_uses == 2 and not events
    torch.autograd.backward(ys, gys)
    ck = Checker("group_norm" if gn else "layer_norm", (kind, "direct views"), bf16,
                 sum((R.gn_n_sum if gn else R.ln_n_sum)(c) for c in cases))
    used = _check_direct(ck, params, pre, events, refs, yards if bf16 else None, flat)
    assert torch.equal(flat[~used], flat0[~used]), "wrote outside the gradient views"
    for x, ref, yard in zip(xs, refs, yards):
        ck("dx", (_nchw(x.grad) if gn else x.grad).cpu(), ref["dx"], None if yard is None else yard["dx"])
    ck.done()


# ------------------------------------------------------------------------------------------ LayerNorm
def _ln_fn(passthrough):
    def fn(x, gamma, beta, r):
        return R.layer_norm_op(x, gamma, beta, EPS, r=r, passthrough=passthrough)
    return fn


@pytest.mark.parametrize("bf16", DTS, ids=DT_IDS)
@pytest.mark.parametrize("case", R.LN_CASES, ids=str)
def test_layer_norm(gpu, case, bf16):
    inputs, gy, _ = R.ln_inputs(case, 4, bf16)
    ref, yard = R.reference_and_yardstick(_ln_fn(False), inputs, [gy], ["y"], bf16)
    got = _run_norm("ln", case, False, bf16, inputs, gy, None, False)
    ck = Checker("layer_norm", case, bf16, R.ln_n_sum(case))
    ck.all(got, ref, yard)
    ck.done()


@pytest.mark.parametrize("bf16", DTS, ids=DT_IDS)
def test_layer_norm_row_strided(gpu, bf16):
    case = (1025, 72)
    inputs, gy, _ = R.ln_inputs(case, 42, bf16)
    ref, yard = R.reference_and_yardstick(_ln_fn(False), inputs, [gy], ["y"], bf16)
    got = _run_norm("ln", case, False, bf16, inputs, gy, None, False, strided=True)
    ck = Checker("layer_norm", (case, "strided"), bf16, R.ln_n_sum(case))
    ck.all(got, ref, yard)
    ck.done()


@pytest.mark.parametrize("bf16", DTS, ids=DT_IDS)
@pytest.mark.parametrize("alias_grad", [True, False], ids=["dres", "no_dres"])
@pytest.mark.parametrize("case", [(5, 72), (1025, 320)], ids=str)
def test_layer_norm_passthrough(gpu, case, alias_grad, bf16):
    inputs, gy, gres = R.ln_inputs(case, 43, bf16)
    gouts = [gy, gres if alias_grad else None]
    ref, yard = R.reference_and_yardstick(_ln_fn(True), inputs, gouts, ["y", "alias"], bf16)
    got = _run_norm("ln", case, False, bf16, inputs, gy, gres if alias_grad else None, True)
    assert torch.equal(got["alias"].float(), inputs["x"])
    ck = Checker("layer_norm", (case, "passthrough", alias_grad), bf16, R.ln_n_sum(case))
    ck.all(got, ref, yard)
    ck.done()


def _ln_bwd_call(rows, c, dgamma: bool, dbeta: bool):
    from rdeic_amd import _lib, ops
    x = torch.randn((rows, c), device="cuda")
    dy = torch.randn((rows, c), device="cuda")
    gamma = torch.ones(c, device="cuda")
    dx = torch.full((rows, c), 7.0, device="cuda")
    dg = torch.full((c,), 7.0, device="cuda")
    db = torch.full((c,), 7.0, device="cuda")
    nws = max(int(_lib.load().rdeic_layernorm_bwd_ws_floats(rows, c)), 1)
    ws = torch.empty(nws, device="cuda")
    try:
        ops.call("rdeic_layernorm_bwd_res", x.data_ptr(), c, rows, c, gamma.data_ptr(), EPS, dy.data_ptr(), c, None, 0,
                 dx.data_ptr(), c, dg.data_ptr() if dgamma else None, db.data_ptr() if dbeta else None, 0,
                 ws.data_ptr(), nws, 0, ops.stream_ptr())
        code = 0
    except _lib.RdeicError as e:
        code = e.code
    torch.cuda.synchronize()
    return code, dx, dg, db


def test_layer_norm_rejects_what_it_cannot_run(gpu):
    code, dx, dg, db = _ln_bwd_call(3, 2049, True, True)   # one wave holds at most 32 x 64 columns
    assert code == -22 and bool((dx == 7).all())
    for dgamma, dbeta in ((True, False), (False, True)):   # the parameter gradients come as a pair
        code, dx, dg, db = _ln_bwd_call(3, 64, dgamma, dbeta)
        assert code == -22, "exactly one of dgamma / dbeta used to compute neither, silently"
        assert bool((dx == 7).all()) and bool((dg == 7).all()) and bool((db == 7).all())  # nothing launched
    code, dx, dg, db = _ln_bwd_call(3, 64, False, False)
    assert code == 0 and not bool((dx == 7).any())
    code, dx, dg, db = _ln_bwd_call(3, 64, True, True)
    assert code == 0 and not bool((dg == 7).any()) and not bool((db == 7).any())


# -------------------------------------------------------------------------------------- conv / linear
CONV = R.conv_case_list()


def _run_conv(case, n, h, w, bf16, inputs, gout, params=None):
    from rdeic_amd import autograd as AG
    cin, cout, k, stride, pad, up2, ps, act, slope, use_emb, use_res, out_f32 = case
    xo = _dev(inputs["x"], bf16, nhwc=True).requires_grad_(True)
    Wo = params["W"] if params else _dev(inputs["W"]).requires_grad_(True)
    bo = params["b"] if params else _dev(inputs["b"]).requires_grad_(True)
    eo = _dev(inputs["emb"]).requires_grad_(True) if use_emb else None
    ro = _dev(inputs["res"], bf16 and not out_f32, nhwc=True).requires_grad_(True) if use_res else None
    cfg = AG.ConvCfg(k, k, stride, pad, up2, ps, act, slope, out_f32=out_f32)
    out = AG.conv2d(xo, Wo, bo, emb=eo, res=ro, cfg=cfg)
    assert out.dtype == (torch.float32 if out_f32 else _dt(bf16))
    out.backward(_dev(gout, bf16 and not out_f32, nhwc=True))
    torch.cuda.synchronize()
    got = {"out": _nchw(out).cpu(), "dx": _nchw(xo.grad).cpu()}
    if params is None:
        got["dW"], got["db"] = Wo.grad.cpu(), bo.grad.cpu()
    if use_emb:
        got["demb"] = eo.grad.cpu()
    if use_res:
        got["dres"] = _nchw(ro.grad).cpu()
    return got


@pytest.mark.parametrize("bf16", DTS, ids=DT_IDS)
@pytest.mark.parametrize("cid,case,n,h,w", CONV, ids=[c[0] for c in CONV])
def test_conv(gpu, cid, case, n, h, w, bf16):
    inputs, gout = R.conv_inputs(case, n, h, w, 2, bf16)
    ref, yard = R.reference_and_yardstick(R.conv_fn(case), inputs, [gout], ["out"], bf16)
    got = _run_conv(case, n, h, w, bf16, inputs, gout)
    ck = Checker("conv", cid, bf16, R.conv_n_sum(case, n, h, w))
    ck.all(got, ref, yard)
    ck.done()


@pytest.mark.parametrize("bf16", DTS, ids=DT_IDS)
@pytest.mark.parametrize("views", ["weight+bias", "bias"])
def test_conv_direct_gradient_views(gpu, views, bf16):
    """weight + bias on views: the bias gradient comes from the weight-gradient GEMM's row sums (fuse_b);
    bias alone: col_sum in accumulate mode, the weight gradient through autograd as usual."""
    case, n, h, w = R.CONV_CASES_SMALL[0][:9] + (False, True, False), 2, 12, 10
    inputs, gout = R.conv_inputs(case, n, h, w, 50, bf16)
    ref, yard = R.reference_and_yardstick(R.conv_fn(case), inputs, [gout], ["out"], bf16)
    W = _dev(inputs["W"]).requires_grad_(True)
    b = _dev(inputs["b"]).requires_grad_(True)
    on_view = {"W": W, "b": b} if views == "weight+bias" else {"b": b}
    pre, events, flat = _direct_views(on_view, 51)
    flat0 = flat.clone()
    got = _run_conv(case, n, h, w, bf16, inputs, gout, params={"W": W, "b": b})
    ck = Checker("conv", ("direct views", views), bf16, R.conv_n_sum(case, n, h, w))
    used = _check_direct(ck, on_view, pre, events, [ref], [yard] if bf16 else None, flat)
    assert torch.equal(flat[~used], flat0[~used]), "wrote outside the gradient views"
    if views == "bias":
        ck("dW", W.grad.cpu(), ref["dW"], None if yard is None else yard["dW"])
    ck("dx", got["dx"], ref["dx"], None if yard is None else yard["dx"])
    ck.done()


def test_conv_stride2_backward_rejects_odd_input(gpu):
    from rdeic_amd import autograd as AG
    x = torch.randn((1, 7, 7, 16), device="cuda").requires_grad_(True)
    W = (torch.randn((16, 16, 3, 3), device="cuda") * 0.1).requires_grad_(True)
    out = AG.conv2d(x, W, None, cfg=AG.ConvCfg(3, 3, 2, 1))
    with pytest.raises(ValueError, match="even input size"):
        out.backward(torch.ones_like(out))


LINEAR_CASES = [(77, 64, 96, True, True, False), (1, 320, 320, False, False, False), (77, 64, 96, True, False, True)]


@pytest.mark.parametrize("bf16", DTS, ids=DT_IDS)
@pytest.mark.parametrize("case", LINEAR_CASES, ids=["bias_res", "one_row", "column_slice"])
def test_linear(gpu, case, bf16):
    from rdeic_amd import autograd as AG
    rows, cin, cout, use_b, use_res, sliced = case
    g = torch.Generator().manual_seed(60)
    inputs = dict(x=R.to_compute(torch.randn((rows, cin), generator=g), bf16),
                  W=R.to_compute(torch.randn((cout, cin), generator=g) / math.sqrt(cin), bf16),
                  b=torch.randn(cout, generator=g) * 0.1 if use_b else None,
                  res=R.to_compute(torch.randn((rows, cout), generator=g), bf16) if use_res else None)
    gout = R.to_compute(torch.randn((rows, cout), generator=g), bf16)
    ref, yard = R.reference_and_yardstick(lambda x, W, b, res, r: R.linear_op(x, W, b, res, r=r), inputs, [gout],
                                          ["out"], bf16)
    x = _dev(inputs["x"], bf16)
    if sliced:
        leaf, sl = _wide(x, 8, 24)
        leaf.requires_grad_(True)
        xo = leaf[:, sl]
    else:
        leaf = xo = x.requires_grad_(True)
    Wo = _dev(inputs["W"]).requires_grad_(True)
    bo = _dev(inputs["b"]).requires_grad_(True) if use_b else None
    ro = _dev(inputs["res"], bf16).requires_grad_(True) if use_res else None
    out = AG.linear(xo, Wo, bo, res=ro)
    out.backward(_dev(gout, bf16))
    torch.cuda.synchronize()
    got = {"out": out.detach().cpu(), "dx": (leaf.grad[:, sl] if sliced else leaf.grad).cpu(), "dW": Wo.grad.cpu()}
    if sliced:
        rest = leaf.grad.clone()
        rest[:, sl] = 0
        assert not bool(rest.any())
    if use_b:
        got["db"] = bo.grad.cpu()
    if use_res:
        got["dres"] = ro.grad.cpu()
    ck = Checker("linear", case, bf16, max(rows, cin, cout))
    ck.all(got, ref, yard)
    ck.done()


def _layout_call(name, src, n, h, w, c, dst):
    from rdeic_amd import ops
    ops.call(name, src.data_ptr(), n, h, w, c, src.stride(2), dst.data_ptr(), dst.stride(2), ops.dt_code(src),
             ops.stream_ptr())
    torch.cuda.synchronize()


@pytest.mark.parametrize("bf16", DTS, ids=DT_IDS)
def test_layout_kernels_exact(gpu, bf16):
    from rdeic_amd import ops
    g = torch.Generator().manual_seed(70)
    n, h, w, c = 2, 5, 7, 6  # odd w, strided sources (pixel stride 11)

    def src_of(shape_nchw):
        t = R.to_compute(torch.randn(shape_nchw, generator=g), bf16)
        wide, sl = _wide(_dev(t, bf16, nhwc=True), 2, 3)
        return t, wide[..., sl]
    # im2col: (k, stride, pad, up2); stride 2 on the (even) upsampled grid
    for k, stride, pad, up2 in ((3, 1, 1, False), (3, 2, 1, True), (1, 1, 0, False), (4, 2, 1, True), (5, 1, 2, False)):
        t, src = src_of((n, c, h, w))
        hi, wi = (2 * h, 2 * w) if up2 else (h, w)
        ho, wo = (hi + 2 * pad - k) // stride + 1, (wi + 2 * pad - k) // stride + 1
        K = k * k * c
        cols = torch.full((n * ho * wo, K + 3), 5.0, dtype=_dt(bf16), device="cuda")
        ops.call("rdeic_im2col", src.data_ptr(), n, h, w, c, src.stride(2), k, k, stride, pad, pad, ho, wo, int(up2),
                 cols.data_ptr(), K + 3, ops.dt_code(src), ops.stream_ptr())
        torch.cuda.synchronize()
        assert torch.equal(cols[:, :K].float().cpu(), R.im2col_ref(t, k, k, stride, pad, ho, wo, up2)), (k, stride, up2)
        assert bool((cols[:, K:] == 5).all())
    # zero_insert2: [n, h, w, c] -> [n, 2h, 2w, c]
    t, src = src_of((n, c, h, w))
    dst = torch.full((n, 2 * h, 2 * w, c + 2), 5.0, dtype=_dt(bf16), device="cuda")
    _layout_call("rdeic_zero_insert2", src, n, h, w, c, dst)
    assert torch.equal(_nchw(dst[..., :c]).float().cpu(), R.zero_insert2_ref(t)) and bool((dst[..., c:] == 5).all())
    # pixel_unshuffle2: [n, 2h, 2w, c] -> [n, h, w, 4c]
    t, src = src_of((n, c, 2 * h, 2 * w))
    dst = torch.full((n, h, w, 4 * c + 2), 5.0, dtype=_dt(bf16), device="cuda")
    _layout_call("rdeic_pixel_unshuffle2", src, n, h, w, c, dst)
    assert torch.equal(_nchw(dst[..., :4 * c]).float().cpu(), R.pixel_unshuffle2_ref(t))
    assert bool((dst[..., 4 * c:] == 5).all())
    # sum_pool2: [n, 2h, 2w, c] -> [n, h, w, c]; fp32 adds, then at most one rounding to the compute dtype
    t, src = src_of((n, c, 2 * h, 2 * w))
    dst = torch.full((n, h, w, c + 2), 5.0, dtype=_dt(bf16), device="cuda")
    _layout_call("rdeic_sum_pool2", src, n, h, w, c, dst)
    exact = R.sum_pool2_ref(t.double())
    mag = R.sum_pool2_ref(t.double().abs())
    err = (_nchw(dst[..., :c]).double().cpu() - exact).abs()
    allow = mag * 2.0 ** -22 + (exact.abs() * 2.0 ** -8 if bf16 else 0.0)  # bf16 unit roundoff 2^-8
    assert bool((err <= allow).all()), float((err / allow).max())
    assert bool((dst[..., c:] == 5).all())


# ----------------------------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("bf16,c_bf16", [(False, False), (True, False), (True, True)],
                         ids=["fp32", "bf16_c_fp32", "bf16_c_bf16"])
@pytest.mark.parametrize("layout", ["nn", "tt"])
def test_gemm_alpha_beta_batch_offsets_splitk(gpu, layout, bf16, c_bf16):
    from rdeic_amd import autograd as AG
    g = torch.Generator().manual_seed(80)
    m, n, k, b1, b2 = 70, 50, 100, 2, 3
    A = R.to_compute(torch.randn((b1, b2, m, k), generator=g), bf16)
    B = R.to_compute(torch.randn((b1, b2, k, n), generator=g), bf16)
    C0 = R.to_compute(torch.randn((b1, b2, m, n), generator=g), c_bf16)
    ref = 0.5 * A.double() @ B.double() + C0.double()
    yard = 0.5 * (A @ B) + C0
    yard = R.bf16_round_(yard) if c_bf16 else yard
    dt, cdt = _dt(bf16), _dt(c_bf16)

    def stored(T, trans, off):
        """[b2][b1] planes (so the two batch levels have different strides) at an odd element offset"""
        P = T.permute(1, 0, 2, 3)
        P = (P.transpose(2, 3) if trans else P).contiguous()
        buf = torch.zeros(P.numel() + 8, dtype=dt, device="cuda")
        buf[off:off + P.numel()] = P.reshape(-1).to(dt).cuda()
        return buf
    ta, tb = layout[0] == "t", layout[1] == "t"
    a_buf, b_buf = stored(A, ta, 1), stored(B, tb, 3)
    a_sm, a_sk = (1, m) if ta else (k, 1)
    b_sk, b_sn = (1, k) if tb else (n, 1)
    Cd = C0.to(cdt).cuda().contiguous()
    AG.gemm(a_buf, 1, a_sm, a_sk, b_buf, 3, b_sk, b_sn, Cd, 0, n, m=m, n=n, k=k, batch=b1 * b2, nb2=b2,
            a_bs=(m * k, b1 * m * k), b_bs=(k * n, b1 * k * n), c_bs=(b2 * m * n, m * n), alpha=0.5, beta=1.0)
    torch.cuda.synchronize()
    ck = Checker("gemm", (layout, "alpha beta nb2 offsets", "C bf16" if c_bf16 else "C fp32"), bf16, k)
    ck("C", Cd.cpu(), ref, yard if bf16 else None)
    if not c_bf16:
        # split-K with a short last plane (100 = 3 x 32 + 4), per head (nb2), with A's row sums per plane
        ks, planes = 32, 4
        Pd = torch.full((planes, b2, m, n), 9.0, device="cuda")
        Rs = torch.full((planes, m), 9.0, device="cuda")
        AG.gemm(a_buf, 1, a_sm, a_sk, b_buf, 3, b_sk, b_sn, Pd, 0, n, m=m, n=n, k=k, batch=planes * b2, nb2=b2,
                a_bs=(0, b1 * m * k), b_bs=(0, b1 * k * n), c_bs=(b2 * m * n, m * n), ksplit=ks)
        P1 = torch.full((planes, m, n), 9.0, device="cuda")  # the same planes of head 0 without nb2, with row sums
        AG.gemm(a_buf, 1, a_sm, a_sk, b_buf, 3, b_sk, b_sn, P1, 0, n, m=m, n=n, k=k, batch=planes,
                c_bs=(m * n, 0), ksplit=ks, rsum=Rs, rsum_bs=m)
        torch.cuda.synchronize()
        assert torch.equal(P1, Pd[:, 0]), "split-K planes differ between the nb2 = 1 and nb2 = 3 launches"
        for q in range(planes):
            kq = slice(q * ks, min(k, (q + 1) * ks))
            want = A[0, :, :, kq].double() @ B[0, :, kq].double()
            ck(f"split-K plane {q}", Pd[q].cpu(), want, (A[0, :, :, kq] @ B[0, :, kq]) if bf16 else None)
            ck(f"row sums plane {q}", Rs[q].cpu(), A[0, 0, :, kq].double().sum(1),
               A[0, 0, :, kq].sum(1) if bf16 else None)
    ck.done()


# --------------------------------------------------------------------------------------- act / GEGLU
def _act_values(rows, c, kind, bf16, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((rows, c), generator=g) * 2
    if kind == R.LEAKY:   # at and around 0
        z[0, :8] = torch.tensor([0.0, -0.0, 1e-3, -1e-3, 1e-20, -1e-20, 2.0 ** -126, -2.0 ** -126])
    else:                 # |z| up to 12: the tails of GELU' and SiLU'
        z[0] = torch.linspace(-12, 12, c)
        z[1] = -z[0] * 0.999
    return R.to_compute(z, bf16), R.to_compute(torch.randn((rows, c), generator=g), bf16)


@pytest.mark.parametrize("bf16", DTS, ids=DT_IDS)
@pytest.mark.parametrize("kind", [R.LEAKY, R.GELU, R.SILU], ids=["leaky", "gelu", "silu"])
def test_act(gpu, kind, bf16):
    from rdeic_amd import autograd as AG
    z, gy = _act_values(37, 72, kind, bf16, 90 + kind)
    ref, yard = R.reference_and_yardstick(lambda z, r: R.act_op(z, kind, 0.01, r=r), dict(z=z), [gy], ["out"], bf16)
    leaf, sl = _wide(_dev(z, bf16), 8, 8)  # row-strided input
    leaf.requires_grad_(True)
    out = AG.act(leaf[:, sl], kind, 0.01)
    out.backward(_dev(gy, bf16))
    torch.cuda.synchronize()
    ck = Checker("act", ("leaky", "gelu", "silu")[kind - 1], bf16)
    ck.all({"out": out.detach().cpu(), "dz": leaf.grad[:, sl].cpu()}, ref, yard)
    ck.done()


@pytest.mark.parametrize("bf16", DTS, ids=DT_IDS)
def test_geglu(gpu, bf16):
    from rdeic_amd import autograd as AG
    rows, c = 37, 40
    a, gy = _act_values(rows, c, R.LEAKY, bf16, 95)
    gate, _ = _act_values(rows, c, R.GELU, bf16, 96)
    x = torch.cat([a, gate], 1)
    ref, yard = R.reference_and_yardstick(lambda x, r: R.geglu_op(x, r=r), dict(x=x), [gy], ["out"], bf16)
    leaf, sl = _wide(_dev(x, bf16), 8, 8)  # row stride 96 != 2c
    leaf.requires_grad_(True)
    out = AG.geglu(leaf[:, sl])
    out.backward(_dev(gy, bf16))
    torch.cuda.synchronize()
    ck = Checker("geglu", (rows, c), bf16)
    ck.all({"out": out.detach().cpu(), "dx": leaf.grad[:, sl].cpu()}, ref, yard)
    ck.done()


# -------------------------------------------------------------------------------------- checkerboard
@pytest.mark.parametrize("bf16", DTS, ids=DT_IDS)
def test_checkerboard_slice(gpu, bf16):
    """(n, c, h, w) = (3, 5, 5, 6): odd h and c, params as slices of a wider tensor, scales on both sides of
    0.11, |y - mu| into the 1e-9 likelihood floor (tests/test_train_ops_ref_cpu.py asserts the inputs do that)."""
    from rdeic_amd import autograd as AG
    inputs, noise, gA, gN = R.ckbd_inputs(7, bf16)
    names = ["anchor", "S", "non"]
    ref, yard = R.reference_and_yardstick(lambda y, pa, pn, r: R.ckbd_op(y, pa, pn, noise.to(y.dtype), r=r), inputs,
                                          [gA, -0.7, gN], names, bf16)
    c = inputs["y"].shape[1]
    yo = _dev(inputs["y"], bf16, nhwc=True).requires_grad_(True)
    pal, sla = _wide(_dev(inputs["pa"], bf16, nhwc=True), 3, 4)
    pnl, sln = _wide(_dev(inputs["pn"], bf16, nhwc=True), 1, 2)
    pal.requires_grad_(True)
    pnl.requires_grad_(True)
    pao, pno = pal[..., sla], pnl[..., sln]
    anc = AG.CkbdAnchorFn.apply(yo, pao)
    S, qS, non = AG.CkbdLikFn.apply(yo, pao, pno, _dev(noise, False, nhwc=True))
    torch.autograd.backward([anc, S, non], [_dev(gA, bf16, nhwc=True), torch.tensor([-0.7], device="cuda"),
                                            _dev(gN, bf16, nhwc=True)])
    torch.cuda.synchronize()
    # the quantised halves are data movement plus an integer: exact away from ties
    ma = R.anchor_mask(5, 6, torch.float64)
    y64, mua, mun = inputs["y"].double(), inputs["pa"][:, c:].double(), inputs["pn"][:, c:].double()
    want_a = R.to_compute(((torch.round(y64 - mua) + mua) * ma).float(), bf16)
    want_n = R.to_compute(((torch.round(y64 - mun) + mun) * (1 - ma)).float(), bf16)
    assert torch.equal(_nchw(anc).float().cpu(), want_a) and torch.equal(_nchw(non).float().cpu(), want_n)
    got = {"anchor": _nchw(anc).cpu(), "S": S.detach().cpu().view(()), "non": _nchw(non).cpu(),
           "dy": _nchw(yo.grad).cpu(), "dpa": _nchw(pal.grad[..., sla]).cpu(), "dpn": _nchw(pnl.grad[..., sln]).cpu()}
    for leaf, sl in ((pal, sla), (pnl, sln)):
        rest = leaf.grad.clone()
        rest[..., sl] = 0
        assert not bool(rest.any())
    ck = Checker("ckbd", (3, 5, 5, 6), bf16, inputs["y"].numel())
    ck.all(got, ref, yard)
    ck.done()


@pytest.mark.parametrize("bf16", DTS, ids=DT_IDS)
def test_checkerboard_mask_exact(gpu, bf16):
    from rdeic_amd import autograd as AG
    g = torch.Generator().manual_seed(8)
    t = R.to_compute(torch.randn((3, 5, 5, 6), generator=g), bf16)
    gy = R.to_compute(torch.randn((3, 5, 5, 6), generator=g), bf16)
    for which in (0, 1):
        leaf, sl = _wide(_dev(t, bf16, nhwc=True), 2, 1)
        leaf.requires_grad_(True)
        out = AG.CkbdMaskFn.apply(leaf[..., sl], which)
        out.backward(_dev(gy, bf16, nhwc=True))
        torch.cuda.synchronize()
        assert torch.equal(_nchw(out).float().cpu(), R.ckbd_mask_ref(t, which))
        assert torch.equal(_nchw(leaf.grad[..., sl]).float().cpu(), R.ckbd_mask_ref(gy, which))


# ------------------------------------------------------------------------------------------------ VQ
VQ_GRID = {(96, 40, 24): (2, 6, 8), (192, 16, 8): (3, 8, 8), (64, 300, 512): (1, 8, 8)}


@pytest.mark.parametrize("case", R.VQ_CASES, ids=str)
def test_vq_train_step(gpu, case):
    """P = 96: not a power of two (the bitonic sort's +inf padding); P = 192 > K = 16: npos = 12;
    D = 512: the kernel's limit. embed_prob spread over the re-initialisation threshold."""
    from rdeic_amd import autograd as AG
    P, K, D = case
    seed = R.VQ_SEEDS[case]
    z, E, ep, gz = R.vq_inputs(case, seed)
    ref, idx = R.vq_reference(case, seed, gloss=1.3)
    B, hz, wz = VQ_GRID[case]
    zo = z.view(B, hz, wz, D).cuda().requires_grad_(True)
    Eo = E.clone().cuda().requires_grad_(True)
    epo = ep.clone().cuda()
    zq, loss = AG.VQTrainFn.apply(zo, Eo, epo, 0.25, 0.99, 0.07)
    torch.autograd.backward([zq, loss], [gz.view(B, hz, wz, D).cuda(), torch.tensor([1.3], device="cuda")])
    torch.cuda.synchronize()
    got = {"zq": zq.detach().view(P, D).cpu(), "loss": loss.detach().cpu(), "E_new": Eo.detach().cpu(),
           "embed_prob": epo.cpu(), "dz": zo.grad.view(P, D).cpu(), "dE": Eo.grad.cpu()}
    ck = Checker("vq", case, False)
    ck.all(got, ref, None)
    ck.done()
