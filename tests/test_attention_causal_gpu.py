"""rdeic_attention_causal (attention_causal.hip) on the MI355X: against a float64 masked softmax on inputs
pre-rounded to the dtype (test_attention's own bounds), causality and repeatability bit for bit, the rows past
batch*l untouched, and the argument checks. q | k | v are column slices of one [rows, 3 * heads * 64] buffer, as
the text tower's fused in_proj leaves them."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DH = 64
DTYPES = [torch.float32, torch.bfloat16]
# both sides of every 16- and 64-wide tile edge, the tower's 77, and lengths over several query blocks
LENGTHS = [1, 15, 16, 17, 63, 64, 65, 77, 130, 300]


def _qkv(batch, heads, l, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch * l, 3 * heads * DH, generator=g).to(dtype)


def _run(qkv, batch, heads, l, extra_rows=0, fill=0.0):
    from rdeic_amd import ops
    C = heads * DH
    d = qkv.cuda()
    out = torch.full((batch * l + extra_rows, C), fill, dtype=qkv.dtype, device="cuda")
    ops.attention_causal(d[:, :C], d[:, C:2 * C], d[:, 2 * C:], out, batch=batch, heads=heads, l=l, dh=DH,
                         scale=DH ** -0.5)
    torch.cuda.synchronize()
    return out.cpu()


def _ref(qkv, batch, heads, l):
    """float64 softmax_{j <= i}(q_i . k_j / 8) v_j of the (already rounded) inputs."""
    C = heads * DH
    x = qkv.double().view(batch, l, 3, heads, DH)
    q, k, v = (x[:, :, j].transpose(1, 2) for j in range(3))  # [b, h, l, dh]
    s = q @ k.transpose(-1, -2) * DH ** -0.5
    s = s.masked_fill(torch.ones(l, l, dtype=torch.bool).triu_(1), float("-inf"))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(batch * l, C)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("l", LENGTHS)
def test_against_float64_masked_softmax(gpu, dtype, l):
    batch, heads = 2, 3
    qkv = _qkv(batch, heads, l, dtype, 100 + l)
    out = _run(qkv, batch, heads, l)
    ref = _ref(qkv, batch, heads, l)
    tol = 2e-5 if dtype == torch.float32 else 3e-2
    print(f"l={l} {dtype}: max |d| = {float((out.double() - ref).abs().max()):.3g}")
    torch.testing.assert_close(out.double(), ref, rtol=tol, atol=tol)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("l", [77, 130])
def test_causality_bitwise(gpu, dtype, l):
    batch, heads = 2, 3
    C = heads * DH
    qkv = _qkv(batch, heads, l, dtype, 7 + l)
    qkv.view(batch, l, 3, heads, DH)[:, :, 0, :, 0] = 1.0  # q[d = 0] = 1 in every row: see the key-0 poke below
    base = _run(qkv, batch, heads, l).view(batch, l, C)
    for m in (40, 65):
        poked = qkv.clone().view(batch, l, 3 * C)
        poked[:, m:, C:] = 1e4  # K and V rows >= m: large and finite (0 * 1e4 = 0, a leak would be huge)
        got = _run(poked.view(batch * l, 3 * C), batch, heads, l).view(batch, l, C)
        assert torch.equal(got[:, :m], base[:, :m]), f"rows < {m} see keys >= {m}"
        assert not torch.equal(got[:, m:], base[:, m:])
    # key 0 is visible to every row. Row 0 itself sees nothing else, so its softmax is 1 whatever k_0 is and its
    # output is v_0: changing K row 0 moves every row from 1 on, changing V row 0 moves every row
    tol = 2e-5 if dtype == torch.float32 else 3e-2
    torch.testing.assert_close(base[:, 0].float(), qkv.view(batch, l, 3 * C)[:, 0, 2 * C:].float(), rtol=tol, atol=tol)
    # (the pokes are sized so that no row can hide them in rounding: k_0[d = 0] += 64 raises every row's score of
    # key 0 by 64 * q[d = 0] / 8 = 8, i.e. its weight by e^8; v_0 += 100 moves a row by 100 times its weight)
    poked = qkv.clone().view(batch, l, 3, heads, DH)
    poked[:, 0, 1, :, 0] += 64
    got = _run(poked.view(batch * l, 3 * C), batch, heads, l).view(batch, l, C)
    assert torch.equal(got[:, 0], base[:, 0])
    changed = (got != base).view(batch, l, heads, DH).any(-1)  # per (batch, row, head)
    assert bool(changed[:, 1:].all()), "a row beyond 0 does not see key 0"
    poked = qkv.clone().view(batch, l, 3, heads, DH)
    poked[:, 0, 2] += 100
    got = _run(poked.view(batch * l, 3 * C), batch, heads, l).view(batch, l, C)
    assert bool((got != base).view(batch, l, heads, DH).any(-1).all()), "a row does not see value 0"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("l", [17, 77, 130])
def test_rows_past_the_end_are_untouched(gpu, dtype, l):
    batch, heads, extra, sentinel = 2, 3, 70, -777.0
    qkv = _qkv(batch, heads, l, dtype, 3 + l)
    out = _run(qkv, batch, heads, l, extra_rows=extra, fill=sentinel)
    assert bool((out[batch * l:] == sentinel).all())
    assert bool((out[:batch * l] != sentinel).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("l", [77, 130])
def test_repeats_and_batch_independence_bitwise(gpu, dtype, l):
    batch, heads = 3, 5
    C = heads * DH
    qkv = _qkv(batch, heads, l, dtype, 11 + l)
    a = _run(qkv, batch, heads, l)
    assert torch.equal(a, _run(qkv, batch, heads, l))  # two runs of the same call
    x = qkv.view(batch, l, 3, heads, DH)
    for b, h in ((1, 3), (2, 0), (0, 4)):
        alone = x[b, :, :, h].reshape(l, 3 * DH).contiguous()  # one (batch, head) in a buffer of its own
        got = _run(alone, 1, 1, l)
        assert torch.equal(got, a.view(batch, l, heads, DH)[b, :, h]), (b, h)


def test_bad_arguments_return_einval(gpu):
    from rdeic_amd import _lib
    lib = _lib.load()
    heads, l = 2, 77
    for dtype, code, bad_ld in ((torch.bfloat16, 1, 4), (torch.float32, 0, 2)):
        C = heads * DH
        buf = torch.zeros((l, 3 * C + 8), dtype=dtype, device="cuda")
        out = torch.full((l, C + 8), 5.0, dtype=dtype, device="cuda")
        es = buf.element_size()
        q, k, v, o = buf.data_ptr(), buf.data_ptr() + C * es, buf.data_ptr() + 2 * C * es, out.data_ptr()
        ld, ldo = buf.stride(0), out.stride(0)
        stream = torch.cuda.current_stream().cuda_stream

        def call(q=q, ldq=ld, k=k, ldk=ld, v=v, ldv=ld, o=o, ldo=ldo, batch=1, heads=heads, l=l, dh=DH):
            return lib.rdeic_attention_causal(q, ldq, k, ldk, v, ldv, o, ldo, batch, heads, l, dh, 0.125, code, stream)

        assert call() == 0
        for dh in (16, 32, 128, 512):
            assert call(dh=dh) == _lib.EINVAL
        for kw in (dict(ldq=ld + bad_ld), dict(ldk=ld + bad_ld), dict(ldv=ld + bad_ld), dict(ldo=ldo + 1),
                   dict(q=q + es), dict(k=k + es), dict(v=v + es), dict(o=o + es), dict(l=0), dict(batch=0),
                   dict(heads=0), dict(q=None)):
            assert call(**kw) == _lib.EINVAL, kw
        torch.cuda.synchronize()
        assert bool((out[:, C:] == 5.0).all())
