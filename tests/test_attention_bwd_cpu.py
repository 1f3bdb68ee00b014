"""Host side of the training flash attention (rdeic_attention_fwd_lse / rdeic_attention_bwd): the workspace
query and the argument validation, which both run before any device call (no GPU needed)."""
import ctypes as C

import pytest

from rdeic_amd import _lib

EINVAL = -22


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def host():
    """A 16-byte aligned host buffer: dummy non-null pointers (validation precedes any device call)."""
    raw = C.create_string_buffer(4096 + 16)
    base = (C.addressof(raw) + 15) // 16 * 16
    return raw, base


def test_workspace_is_monotone_in_lq_and_sized_for_slabs(lib):
    for batch, heads, lk, dh in ((1, 1, 77, 64), (1, 5, 77, 64), (1, 4, 77, 16), (2, 3, 200, 64), (1, 2, 4096, 64)):
        prev = 0
        for lq in (1, 4, 63, 64, 65, 200, 1000, 1024, 3300, 3392, 4096, 16384):
            ws = lib.rdeic_attention_bwd_workspace(batch, heads, lq, lk, dh)
            assert ws >= prev, (batch, heads, lq, lk, dh, ws, prev)
            assert ws >= batch * heads * lq * 4  # delta, one fp32 per query row
            prev = ws
    # cross-attention of one image (2 key blocks x 1 head): the query sweep is chunked, so the workspace
    # holds fp32 dK / dV slabs (at least two chunks of [lk][dh] each) next to delta
    ws = lib.rdeic_attention_bwd_workspace(1, 1, 1000, 77, 64)
    assert ws >= 1000 * 4 + 2 * 2 * 77 * 64 * 4
    # many key blocks: no slabs, and far below one fp32 score tensor
    assert lib.rdeic_attention_bwd_workspace(1, 2, 4096, 4096, 64) < 1 << 20


def _fwd(lib, p, **kw):
    a = dict(q=p, k=p, v=p, o=p, lse=p, batch=1, heads=2, lq=64, lk=77, dh=64, dtype=1)
    a.update(kw)
    c = a["heads"] * a["dh"]
    return lib.rdeic_attention_fwd_lse(a["q"], c, a["k"], c, a["v"], c, a["o"], c, a["lse"], a["batch"], a["heads"],
                                       a["lq"], a["lk"], a["dh"], 0.125, a["dtype"], None)


def _bwd(lib, p, **kw):
    a = dict(q=p, lse=p, dq=p, dk=p, dv=p, ws=p, ws_bytes=None, batch=1, heads=2, lq=64, lk=77, dh=64, dtype=1)
    a.update(kw)
    c = a["heads"] * a["dh"]
    need = lib.rdeic_attention_bwd_workspace(a["batch"], a["heads"], a["lq"], a["lk"], a["dh"])
    wsb = need if a["ws_bytes"] is None else a["ws_bytes"]
    return need, lib.rdeic_attention_bwd(a["q"], c, p, c, p, c, p, c, p, c, a["lse"], a["dq"], c, a["dk"], c, a["dv"],
                                         c, a["ws"], wsb, a["batch"], a["heads"], a["lq"], a["lk"], a["dh"], 0.125,
                                         a["dtype"], None)


def test_forward_rejects_bad_arguments_before_any_device_call(lib, host):
    _, p = host
    assert _fwd(lib, p, dh=32) == EINVAL
    assert _fwd(lib, p, dtype=0) == EINVAL
    assert _fwd(lib, p, lse=None) == EINVAL
    assert _fwd(lib, p, q=None) == EINVAL
    assert _fwd(lib, p, q=p + 2) == EINVAL  # misaligned


def test_backward_rejects_bad_arguments_before_any_device_call(lib, host):
    _, p = host
    assert _bwd(lib, p, dh=32)[1] == EINVAL
    assert _bwd(lib, p, dtype=0)[1] == EINVAL
    assert _bwd(lib, p, lse=None)[1] == EINVAL
    need, rc = _bwd(lib, p, ws_bytes=0)
    assert need > 0 and rc == EINVAL
    assert _bwd(lib, p, ws_bytes=need - 1)[1] == EINVAL
    assert _bwd(lib, p, ws=None)[1] == EINVAL
    assert _bwd(lib, p, dq=None, dk=None, dv=None)[1] == EINVAL  # nothing to compute
    assert _bwd(lib, p, dk=None)[1] == EINVAL  # dK and dV come as a pair
    assert _bwd(lib, p, q=p + 2)[1] == EINVAL
