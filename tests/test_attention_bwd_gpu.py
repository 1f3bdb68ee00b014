"""Training flash attention (rdeic_attention_fwd_lse / rdeic_attention_bwd, attention_bwd.hip) against float64
torch on the CPU, computed from the same bf16-rounded inputs (q, k, v, dO ~ N(0, 1), fixed seeds).

Checks per shape (the smallest shapes that reach every edge: ragged tails on both sides, cross-attention
with lk = 77, the query-chunked dK/dV path with an uneven last chunk, lq below a tile, both head dims):
  * LSE: |lse - truth| <= 1e-3 (an fp32 sum of <= 64 exact bf16 x bf16 products is off by ~2e-5 at these
    magnitudes; 1e-3 is 50x that and still separates ln from log2 or a missing scale);
  * o, dq, dk, dv: with err(x) = max|x - truth| / max|truth|, err_flash <= 2 err_materialized, the latter from
    the materialised AttentionFn on the same inputs (both paths round P and dS to bf16 once, at different
    points: errors of one order, not ordered);
  * bounds: guard rows around every output keep their sentinel, every in-range element (pre-filled with NaN)
    is finite;
  * dq-only and dk/dv-only calls equal the full call bit for bit; two runs are bit-identical;
  * memory, graph capture, and the implementation switch of rdeic_amd.autograd.

Measured on MI355X (test_matches_float64_truth prints them with -s; also DESIGN.md section 14): LSE abs error, then
err flash / err materialised for o, dq, dk, dv:
  2x3x200x200x64   9.3e-7  2.61e-3/4.61e-3  4.17e-3/4.17e-3  3.53e-3/5.01e-3  2.40e-3/2.40e-3
  1x2x256x77x64    6.5e-7  3.02e-3/3.47e-3  4.07e-3/4.00e-3  3.21e-3/4.76e-3  3.26e-3/3.26e-3
  1x1x1000x77x64   6.7e-7  2.40e-3/3.50e-3  3.18e-3/4.17e-3  3.37e-3/3.35e-3  3.09e-3/3.09e-3
  2x4x130x130x16   9.1e-7  3.06e-3/3.38e-3  3.30e-3/4.74e-3  1.81e-3/2.70e-3  2.61e-3/2.61e-3
  1x16x16x77x16    7.0e-7  2.49e-3/2.38e-3  4.21e-3/3.23e-3  2.76e-3/5.21e-3  3.59e-3/3.59e-3
  1x20x4x4x64      2.6e-7  3.14e-3/3.45e-3  4.04e-3/4.41e-3  5.15e-3/4.20e-3  3.36e-3/3.36e-3
  1x20x4x77x64     6.2e-7  2.20e-3/3.23e-3  4.11e-3/4.11e-3  4.16e-3/3.45e-3  3.75e-3/3.75e-3
(worst ratio 1.30). Peak memory of forward + backward at (1, 2, 4096, 4096, 64): 4.1 MiB."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

# batch, heads, lq, lk, dh
CASES = [
    (2, 3, 200, 200, 64),   # ragged tail on both sides
    (1, 2, 256, 77, 64),    # cross, ragged lk
    (1, 1, 1000, 77, 64),   # the query-chunked dK/dV path with an uneven last chunk
    (2, 4, 130, 130, 16),   # ragged tail at dh = 16
    (1, 16, 16, 77, 16),    # lq smaller than a tile, cross
    (1, 20, 4, 4, 64),      # the 128^2 step's deepest level, lq below any tile
    (1, 20, 4, 77, 64),     # the same level, cross
]
IDS = ["x".join(str(v) for v in c) for c in CASES]
GUARD = 4           # guard rows before and after every output
SENT16 = 0x7B7B     # sentinel bit pattern of the guard rows (bf16 outputs)
SENT32 = 0x7B7B7B7B  # ... and of the guard floats around the LSE


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _inputs(case, seed):
    batch, heads, lq, lk, dh = case
    g = torch.Generator().manual_seed(seed)
    c = heads * dh
    q, do = (torch.randn(batch * lq, c, generator=g).bfloat16() for _ in range(2))
    k, v = (torch.randn(batch * lk, c, generator=g).bfloat16() for _ in range(2))
    return q, k, v, do


def _truth(case, q, k, v, do):
    """float64 on the CPU: o, lse, dq, dk, dv in the kernels' layouts."""
    batch, heads, lq, lk, dh = case
    scale = dh ** -0.5

    def split(x, n):
        return x.double().view(batch, n, heads, dh).permute(0, 2, 1, 3)

    def merge(x, n):
        return x.permute(0, 2, 1, 3).reshape(batch * n, heads * dh)

    Q, K, V, DO = split(q, lq), split(k, lk), split(v, lk), split(do, lq)
    S = Q @ K.transpose(-1, -2) * scale
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    O = P @ V
    dV = P.transpose(-1, -2) @ DO
    dP = DO @ V.transpose(-1, -2)
    dS = P * (dP - (dP * P).sum(-1, keepdim=True)) * scale
    return dict(o=merge(O, lq), lse=lse.reshape(-1), dq=merge(dS @ K, lq), dk=merge(dS.transpose(-1, -2) @ Q, lk),
                dv=merge(dV, lk))


def _guarded(rows, cols):
    buf = torch.empty((rows + 2 * GUARD, cols), dtype=torch.bfloat16, device="cuda")
    _bits(buf).fill_(SENT16)
    buf[GUARD:GUARD + rows].fill_(float("nan"))
    return buf


def _guards_intact(buf, rows, sent):
    b = _bits(buf)
    return bool((b[:GUARD] == sent).all()) and bool((b[GUARD + rows:] == sent).all())


def _flash_raw(case, q, k, v, do, want_dq=True, want_dkv=True):
    """The C entries on guarded outputs. Returns the in-range outputs (clones) and whether every guard kept
    its sentinel."""
    from rdeic_amd import _lib, ops
    from rdeic_amd._lib import call
    batch, heads, lq, lk, dh = case
    c = heads * dh
    scale = dh ** -0.5
    sp = ops.stream_ptr()
    nl = batch * heads * lq
    ob = _guarded(batch * lq, c)
    lb = torch.empty(nl + 16, dtype=torch.float32, device="cuda")
    _bits(lb).fill_(SENT32)
    lb[8:8 + nl].fill_(float("nan"))
    o, lse = ob[GUARD:GUARD + batch * lq], lb[8:8 + nl]
    call("rdeic_attention_fwd_lse", q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
         o.data_ptr(), c, lse.data_ptr(), batch, heads, lq, lk, dh, scale, 1, sp)
    dqb = _guarded(batch * lq, c) if want_dq else None
    dkb = _guarded(batch * lk, c) if want_dkv else None
    dvb = _guarded(batch * lk, c) if want_dkv else None
    nws = int(_lib.load().rdeic_attention_bwd_workspace(batch, heads, lq, lk, dh))
    wsb = torch.empty(nws + 512, dtype=torch.uint8, device="cuda")
    wsb.fill_(0x7B)
    ptr = lambda b, rows: None if b is None else b[GUARD:GUARD + rows].data_ptr()  # noqa: E731
    call("rdeic_attention_bwd", q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
         o.data_ptr(), c, do.data_ptr(), do.stride(0), lse.data_ptr(), ptr(dqb, batch * lq), c, ptr(dkb, batch * lk), c,
         ptr(dvb, batch * lk), c, wsb.data_ptr() + 256, nws, batch, heads, lq, lk, dh, scale, 1, sp)
    torch.cuda.synchronize()
    intact = _guards_intact(ob, batch * lq, SENT16)
    intact &= bool((_bits(lb)[:8] == SENT32).all()) and bool((_bits(lb)[8 + nl:] == SENT32).all())
    intact &= bool((wsb[:256] == 0x7B).all()) and bool((wsb[256 + nws:] == 0x7B).all())
    out = dict(o=o.clone(), lse=lse.clone())
    for name, buf, rows in (("dq", dqb, batch * lq), ("dk", dkb, batch * lk), ("dv", dvb, batch * lk)):
        if buf is not None:
            intact &= _guards_intact(buf, rows, SENT16)
            out[name] = buf[GUARD:GUARD + rows].clone()
    out["intact"] = intact
    return out


def _autograd_run(impl, case, q, k, v, do):
    """o, dq, dk, dv of rdeic_amd.autograd.attention with the implementation forced."""
    from rdeic_amd import autograd as AG
    batch, heads, lq, lk, dh = case
    prev = AG.get_attention_impl()
    AG.set_attention_impl(impl)
    try:
        q, k, v = (t.detach().requires_grad_() for t in (q, k, v))
        o = AG.attention(q, k, v, batch, heads, dh ** -0.5)
        dq, dk, dv = torch.autograd.grad(o, (q, k, v), do)
        torch.cuda.synchronize()
    finally:
        AG.set_attention_impl(prev)
    return dict(o=o.detach(), dq=dq, dk=dk, dv=dv)


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs, the float64 truth and the full flash result of case i, computed once and shared (read-only)."""
    case = CASES[i]
    host = _inputs(case, 1234 + i)
    dev = tuple(t.cuda() for t in host)
    return dict(case=case, dev=dev, truth=_truth(case, *host), flash=_flash_raw(case, *dev))


def _err(x, truth):
    return float((x.double().cpu() - truth).abs().max() / truth.abs().max())


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_matches_float64_truth(gpu, i):
    c = _case(i)
    fl, tr = c["flash"], c["truth"]
    lse_err = float((fl["lse"].double().cpu() - tr["lse"]).abs().max())
    mat = _autograd_run("materialized", c["case"], *c["dev"])
    pairs = {n: (_err(fl[n], tr[n]), _err(mat[n], tr[n])) for n in ("o", "dq", "dk", "dv")}
    print(f"\n[attention_bwd] {IDS[i]}: lse err {lse_err:.2e}; flash / materialised: " +
          ", ".join(f"{n} {a:.2e} / {b:.2e}" for n, (a, b) in pairs.items()))
    assert lse_err <= 1e-3, lse_err
    for n, (a, b) in pairs.items():
        assert a <= 2 * b, (n, a, b)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_writes_every_element_and_nothing_else(gpu, i):
    fl = _case(i)["flash"]
    assert fl["intact"], "a guard row, the LSE guard or the workspace guard was overwritten"
    for n in ("o", "lse", "dq", "dk", "dv"):
        assert bool(torch.isfinite(fl[n]).all()), n


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_null_outputs_and_determinism(gpu, i):
    """dq-only and dk/dv-only calls, and a second full run, equal the full call bit for bit."""
    c = _case(i)
    fl = c["flash"]
    again = _flash_raw(c["case"], *c["dev"])
    only_q = _flash_raw(c["case"], *c["dev"], want_dkv=False)
    only_kv = _flash_raw(c["case"], *c["dev"], want_dq=False)
    assert again["intact"] and only_q["intact"] and only_kv["intact"]
    for n in ("o", "lse", "dq", "dk", "dv"):
        assert torch.equal(_bits(again[n]), _bits(fl[n])), n
    assert torch.equal(_bits(only_q["dq"]), _bits(fl["dq"])) and "dk" not in only_q
    assert torch.equal(_bits(only_kv["dk"]), _bits(fl["dk"])) and torch.equal(_bits(only_kv["dv"]), _bits(fl["dv"]))


def test_column_slices_of_one_qkv_tensor(gpu):
    """q, k, v as column slices of a single [rows, 3C] tensor (row stride 3C, not C), raw entries and autograd."""
    case = CASES[0]
    c = _case(0)
    q, k, v, do = c["dev"]
    qkv = torch.cat([q, k, v], 1)
    C = q.shape[1]
    qs, ks, vs = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    assert qs.stride(0) == 3 * C
    raw = _flash_raw(case, qs, ks, vs, do)
    assert raw["intact"]
    ag = _autograd_run("flash", case, qs, ks, vs, do)
    for n in ("o", "dq", "dk", "dv"):
        assert torch.equal(_bits(raw[n]), _bits(c["flash"][n])), n
        assert torch.equal(_bits(ag[n]), _bits(c["flash"][n])), n


def test_peak_memory_has_no_score_tensor(gpu):
    """(1, 2, 4096, 4096, 64): one fp32 score tensor is 128 MiB; the flash working set (eight [4096, 128] bf16
    tensors, LSE, workspace) is ~8-10 MiB. The materialised path fails this by construction."""
    from rdeic_amd import autograd as AG
    case = (1, 2, 4096, 4096, 64)
    q, k, v, do = (t.cuda() for t in _inputs(case, 99))
    prev = AG.get_attention_impl()
    AG.set_attention_impl("flash")
    try:
        q, k, v = (t.requires_grad_() for t in (q, k, v))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        o = AG.attention(q, k, v, 1, 2, 0.125)
        grads = torch.autograd.grad(o, (q, k, v), do)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
    finally:
        AG.set_attention_impl(prev)
    print(f"\n[attention_bwd] peak memory of fwd+bwd at {case}: {peak / 2**20:.1f} MiB")
    assert all(bool(torch.isfinite(g).all()) for g in grads)
    assert peak < 32 << 20, peak


def test_graph_capture_replays_the_eager_result(gpu):
    """fwd + bwd captured in one graph on a single stream and replayed twice equals the eager result bit for bit
    (no host sync, allocation or memset outside the stream in either entry). The chunked shape: four launches."""
    from rdeic_amd import autograd as AG
    case = CASES[2]
    c = _case(2)
    eager = _autograd_run("flash", case, *c["dev"])
    batch, heads, lq, lk, dh = case
    prev = AG.get_attention_impl()
    AG.set_attention_impl("flash")
    try:
        q, k, v = (t.clone().requires_grad_() for t in c["dev"][:3])
        do = c["dev"][3].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up on the capture stream
            torch.autograd.grad(AG.attention(q, k, v, batch, heads, dh ** -0.5), (q, k, v), do)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            o = AG.attention(q, k, v, batch, heads, dh ** -0.5)
            dq, dk, dv = torch.autograd.grad(o, (q, k, v), do)
        for _ in range(2):
            for t in (o, dq, dk, dv):
                t.detach().fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            for n, t in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv)):
                assert torch.equal(_bits(t.detach()), _bits(eager[n])), n
    finally:
        AG.set_attention_impl(prev)


class _ParentAttentionFn(torch.autograd.Function):
    """The materialised formulas as they stood before the flash path existed (the parent's AttentionFn body)."""

    @staticmethod
    def forward(ctx, q, k, v, batch, heads, scale):
        from rdeic_amd import autograd as AG
        from rdeic_amd._lib import call
        Lq, Lk, dh = q.shape[0] // batch, k.shape[0] // batch, q.shape[1] // heads
        dev, dt = q.device, q.dtype
        s = torch.empty((batch, heads, Lq, Lk), dtype=torch.float32, device=dev)
        ldq, ldk, ldv = q.stride(0), k.stride(0), v.stride(0)
        AG.gemm(q, 0, ldq, 1, k, 0, 1, ldk, s, 0, Lk, m=Lq, n=Lk, k=dh, batch=batch * heads, nb2=heads,
                a_bs=(Lq * ldq, dh), b_bs=(Lk * ldk, dh), c_bs=(heads * Lq * Lk, Lq * Lk))
        p = torch.empty((batch, heads, Lq, Lk), dtype=dt, device=dev)
        call("rdeic_softmax_rows", s.data_ptr(), batch * heads * Lq, Lk, float(scale), p.data_ptr(), AG._dt(q), AG._sp())
        o = AG._heads_gemm(p, Lk, 1, (heads * Lq * Lk, Lq * Lk), v, ldv, 1, (Lk * ldv, dh), m=Lq, n=dh, k=Lk,
                           batch=batch, heads=heads, dt=dt, dev=dev)
        ctx.dims = (batch, heads, Lq, Lk, dh, scale)
        ctx.save_for_backward(q, k, v, p)
        return o

    @staticmethod
    def backward(ctx, do):
        from rdeic_amd import autograd as AG
        from rdeic_amd._lib import call
        q, k, v, p = ctx.saved_tensors
        batch, heads, Lq, Lk, dh, scale = ctx.dims
        do = do.contiguous()
        dev, dt = q.device, q.dtype
        ldq, ldk, ldv, ldo = q.stride(0), k.stride(0), v.stride(0), do.stride(0)
        nb = batch * heads
        dp = torch.empty((batch, heads, Lq, Lk), dtype=torch.float32, device=dev)
        AG.gemm(do, 0, ldo, 1, v, 0, 1, ldv, dp, 0, Lk, m=Lq, n=Lk, k=dh, batch=nb, nb2=heads,
                a_bs=(Lq * ldo, dh), b_bs=(Lk * ldv, dh), c_bs=(heads * Lq * Lk, Lq * Lk))
        ds = torch.empty((batch, heads, Lq, Lk), dtype=dt, device=dev)
        call("rdeic_softmax_bwd_rows", p.data_ptr(), dp.data_ptr(), nb * Lq, Lk, float(scale), ds.data_ptr(), AG._dt(q),
             AG._sp())
        pl = (heads * Lq * Lk, Lq * Lk)
        dq = AG._heads_gemm(ds, Lk, 1, pl, k, ldk, 1, (Lk * ldk, dh), m=Lq, n=dh, k=Lk, batch=batch, heads=heads,
                            dt=dt, dev=dev)
        dk = AG._heads_gemm(ds, 1, Lk, pl, q, ldq, 1, (Lq * ldq, dh), m=Lk, n=dh, k=Lq, batch=batch, heads=heads,
                            dt=dt, dev=dev)
        dv = AG._heads_gemm(p, 1, Lk, pl, do, ldo, 1, (Lq * ldo, dh), m=Lk, n=dh, k=Lq, batch=batch, heads=heads,
                            dt=dt, dev=dev)
        return dq, dk, dv, None, None, None


@pytest.mark.parametrize("i,dtype", [(0, torch.bfloat16), (2, torch.bfloat16), (3, torch.float32)],
                         ids=["bf16-self", "bf16-cross-splitk", "fp32"])
def test_materialized_path_is_the_parents(gpu, i, dtype):
    """"materialized" forced: bit-equal to the parent's Function body (bf16, and fp32, which always takes it)."""
    case = CASES[i]
    batch, heads, lq, lk, dh = case
    q, k, v, do = (t.to(dtype) for t in _case(i)["dev"])
    ours = _autograd_run("materialized", case, q, k, v, do)
    qr, kr, vr = (t.detach().requires_grad_() for t in (q, k, v))
    o = _ParentAttentionFn.apply(qr, kr, vr, batch, heads, dh ** -0.5)
    dq, dk, dv = torch.autograd.grad(o, (qr, kr, vr), do)
    torch.cuda.synchronize()
    for n, t in (("o", o.detach()), ("dq", dq), ("dk", dk), ("dv", dv)):
        assert torch.equal(_bits(ours[n]), _bits(t)), n
    if dtype == torch.float32:  # "auto" keeps fp32 on the materialised path too
        auto = _autograd_run("auto", case, q, k, v, do)
        for n, t in (("o", o.detach()), ("dq", dq), ("dk", dk), ("dv", dv)):
            assert torch.equal(_bits(auto[n]), _bits(t)), n


def test_implementation_switch(gpu):
    from rdeic_amd import autograd as AG
    with pytest.raises(ValueError):
        AG.set_attention_impl("fused")
    case = CASES[3]
    q, k, v, do = _case(3)["dev"]
    with pytest.raises(ValueError):  # fp32 is not eligible
        _autograd_run("flash", case, q.float(), k.float(), v.float(), do.float())
    with pytest.raises(ValueError):  # head dim 32 is not eligible
        _autograd_run("flash", (2, 2, 130, 130, 32), q, k, v, do)
    ok = _autograd_run("flash", case, q, k, v, do)  # eligible: the flash kernels, bit-equal to the raw entries
    for n in ("o", "dq", "dk", "dv"):
        assert torch.equal(_bits(ok[n]), _bits(_case(3)["flash"][n])), n
