"""The per-op codec tests have power: CPU checks of tests/codec_ops_ref.py.

* Goldens: from tests/golden/e2e_128.npz (the reference modules' own y, z, symbols and indexes) the checkerboard
  references reproduce the oracle's _stage_loop symbols and indexes for every stage of each phase, and from
  tests/golden/vq_resume.npz vq_argmin_ref reproduces oracle.model_ref.vq_quant's (and the reference module's) indexes.
* Mutants: a deliberately wrong variant of the REFERENCE must change the reference's output on the exact inputs
  tests/test_codec_ops_gpu.py feeds the kernel, at every shape / dtype / phase of that test (for a bit-exact GPU
  assertion any changed element is a failure there).
* Input conditions (planted half-integers, scales at table entries and below the bound, VQ ties and the threads
  they land in) hold for the seeds used, counted over all elements."""
import os
import types

import numpy as np
import pytest
import torch

from oracle import coders_ref as cr
from oracle import model_ref as mr
from tests import codec_ops_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float32, torch.bfloat16]
CKBD_ALL = list(R.CKBD_SHAPES) + [R.CKBD_LARGE]


def _changed(a, b):
    return not torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ goldens
def _compression_weights():
    """The synthetic weights of the compression model only (oracle.model_ref.synthetic_state_dict's recipe)."""
    from oracle import weights_cpu
    from rdeic_amd import weights as W
    sd = {}
    for name, shape in mr.param_shapes().items():
        if not name.startswith(mr.P) or not W.is_param(name) or "gaussian_conditional" in name \
                or name.endswith("scale_list"):
            continue
        scale, offset = W.init_spec(name, shape, 1.0)
        n = int(np.prod(shape))
        sd[name] = torch.from_numpy(weights_cpu.fill_uniform(n, W.param_seed(name, W.GLOBAL_SEED), scale,
                                                             offset)).view(shape)
    return sd


def test_checkerboard_refs_reproduce_stage_loop_on_golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "e2e_128.npz"))
    sd = _compression_weights()
    table = torch.from_numpy(g["scale_table"])
    assert torch.equal(table, cr.get_scale_table())
    for i in (0, 1):
        y, z = torch.from_numpy(g[f"img{i}_y"]), torch.from_numpy(g[f"img{i}_z"])
        zq, zidx = mr.vq_quant(sd, z)
        assert np.array_equal(zidx.numpy(), g[f"img{i}_z_idx"])
        hyper = mr.seq(sd, mr.P + "hyper_dec.hyper_dec", zq)
        _, S, I = mr._stage_loop(sd, hyper, y, types.SimpleNamespace(scale_table=table), "enc")
        assert np.array_equal(S, g[f"img{i}_symbols"]) and np.array_equal(I, g[f"img{i}_indexes"])
        assert len(set(S.tolist())) > 3 and len(set(I.tolist())) > 3  # not trivial
        # _stage_loop's walk, each half stage through the references
        y_hat_slices, off, pos = [], 0, 0
        n_half = y.shape[2] * y.shape[3] // 2
        for k, c in enumerate(mr.SLICE_CH):
            ctx = [] if k == 0 else [mr.channel_ctx(sd, k, torch.cat(y_hat_slices, 1))]
            params = mr.ep(sd, "entropy_parameters_anchor", k, torch.cat(ctx + [hyper], 1))
            halves = []
            for phase in (0, 1):
                if phase == 1:
                    lc = mr.conv(sd, f"{mr.P}local_context.{k}", halves[0])
                    params = mr.ep(sd, "entropy_parameters_nonanchor", k, torch.cat([lc] + ctx + [hyper], 1))
                sym, idx, half, _ = R.ckbd_encode_ref(y[:, off:off + c], params, phase, table)
                assert np.array_equal(sym[0].numpy(), S[pos:pos + c * n_half]), (i, k, phase)
                assert np.array_equal(idx[0].numpy(), I[pos:pos + c * n_half]), (i, k, phase)
                # the decoder's half of the stage gives the encoder's y_hat
                assert torch.equal(R.ckbd_dequant_ref(sym, params, phase)[0], half)
                halves.append(half)
                pos += c * n_half
            y_hat_slices.append(halves[0] + halves[1])
            off += c
        assert pos == S.size


def test_vq_argmin_ref_reproduces_vq_quant_on_golden():
    from oracle import weights_cpu
    g = np.load(os.path.join(ROOT, "tests", "golden", "vq_resume.npz"))
    z = torch.from_numpy(g["z"])
    K, D = g["embed_prob0"].shape[0], z.shape[1]
    assert K == R.vq_codebook_size()
    E = torch.from_numpy(weights_cpu.fill_uniform(K * D, int(g["e_seed"]), float(g["e_scale"]), 0.0)).view(K, D)
    _, want = mr.vq_quant({mr.P + "quantize.embedding.weight": E}, z)
    zf = z.permute(0, 2, 3, 1).reshape(-1, D)
    got = R.vq_argmin_ref(torch.einsum("bd,dn->bn", zf, E.t()), torch.sum(zf ** 2, dim=1), torch.sum(E ** 2, dim=1))
    assert torch.equal(got, want.reshape(-1))
    assert np.array_equal(got.numpy(), g["idx"].reshape(-1))
    assert got.unique().numel() > 10


def test_argmin_ref_non_finite_rule():
    """torch.argmin, which the reference's vq_quant calls: NaN is the minimum, the first one wins."""
    nan, inf = float("nan"), float("inf")
    d = torch.tensor([[inf] * 4, [1.0, nan, -inf, nan], [nan] * 4, [2.0, 1.0, 1.0, 3.0]])
    assert torch.argmin(d, 1).tolist() == [0, 1, 0, 1]


# ------------------------------------------------------------------------------------------------ mutants
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", CKBD_ALL)
def test_checkerboard_mutants_flagged(shape, dtype):
    if shape == R.CKBD_LARGE and dtype != torch.bfloat16:
        return  # the GPU test runs the large case in bf16 only
    n, hy, wy, c = shape
    y, params, table = R.ckbd_case(n, hy, wy, c, dtype)
    for phase in (0, 1):
        sym, idx, half, anchor = R.ckbd_encode_ref(y, params, phase, table, dtype)
        m = R.ckbd_encode_ref(y, params, phase, table, dtype, mutant="phase")
        assert _changed(m[0], sym) and _changed(m[1], idx) and _changed(m[2], half)
        m = R.ckbd_encode_ref(y, params, phase, table, dtype, mutant="half_away")
        assert _changed(m[0], sym) and _changed(m[2], half) and torch.equal(m[1], idx)
        for mutant in ("lt", "no_bound"):
            m = R.ckbd_encode_ref(y, params, phase, table, dtype, mutant=mutant)
            assert _changed(m[1], idx) and torch.equal(m[0], sym), mutant


@pytest.mark.parametrize("rows", R.VQ_ROWS)
@pytest.mark.parametrize("ncode", list(R.VQ_NCODES) + [R.vq_codebook_size()])
def test_last_min_argmin_flagged(rows, ncode):
    dot, zn, en = R.vq_case(rows, ncode)
    ref, mut = R.vq_argmin_ref(dot, zn, en), R.vq_argmin_ref(dot, zn, en, mutant="last_min")
    ties = R.vq_ties(rows, ncode)
    assert (ncode < 7) == (not ties)  # every case with room for a tie has one in every row
    for r, (a, b) in ties.items():
        assert ref[r] == a and mut[r] == b


def test_image_mutants_flagged():
    for dtype in DTYPES:
        x = R.x_to_u8_case(17 * 19).to(dtype)
        assert _changed(R.x_to_u8_ref(x, mutant="round"), R.x_to_u8_ref(x))
        u8 = (np.arange(768) % 256).astype(np.uint8)
        assert _changed(R.u8_to_x_ref(u8, dtype, mutant="div256"), R.u8_to_x_ref(u8, dtype))
    big = R.x_to_u8_case(R.GRID_CAP // 3 + 100)
    assert _changed(R.x_to_u8_ref(big, mutant="round"), R.x_to_u8_ref(big))


@pytest.mark.parametrize("shape", R.LAYOUT_SHAPES)
def test_mul_add_order_flagged(shape):
    x = R.layout_case(*shape)
    for dtype in DTYPES:
        for mul, add in R.LAYOUT_MULADD:
            changed = _changed(R.nchw_to_nhwc_ref(x, mul, add, dtype, mutant="add_first"),
                               R.nchw_to_nhwc_ref(x, mul, add, dtype))
            assert changed == (add != 0.0)  # with add = 0 both orders are the same function


@pytest.mark.parametrize("count", R.COUNTS)
def test_ddim_direction_on_x_flagged(count):
    x, e = R.pair_case(count, 1)
    assert _changed(R.ddim_step_ref(x, e, *R.DDIM_COEF, mutant="dir_on_x")[0], R.ddim_step_ref(x, e, *R.DDIM_COEF)[0])


@pytest.mark.parametrize("rows,cols", R.TRANSPOSE_SHAPES)
def test_transpose_ldout_as_cols_flagged(rows, cols):
    for dtype in DTYPES:
        src, ldin, ldout, in_bs, out_bs = R.transpose_case(rows, cols, dtype)
        out = torch.full((R.TRANSPOSE_BATCH * out_bs,), -7.0, dtype=dtype)
        args = (src, rows, cols, ldin, out, ldout, R.TRANSPOSE_BATCH, in_bs, out_bs)
        ref = R.transpose_ref(*args)
        # one column: the only output row starts at 0 whatever the leading dimension
        assert _changed(R.transpose_ref(*args, mutant="ldout_cols"), ref) == (cols > 1)
        dense = ref.as_strided((R.TRANSPOSE_BATCH, cols, rows), (out_bs, ldout, 1))
        assert torch.equal(dense, src.as_strided((R.TRANSPOSE_BATCH, rows, cols), (in_bs, ldin, 1)).transpose(1, 2))


# --------------------------------------------------------------------------------------- input conditions
def test_checkerboard_input_conditions():
    planted = {torch.float32: 0, torch.bfloat16: 0}
    for shape in R.CKBD_SHAPES:
        n, hy, wy, c = shape
        for dtype in DTYPES:
            y, params, table = R.ckbd_case(n, hy, wy, c, dtype)
            assert torch.equal(y, y.to(dtype).float()) and torch.equal(params, params.to(dtype).float())
            scales, means = params.chunk(2, 1)
            d = y - means  # fp32, as the kernel subtracts
            half = (d - torch.floor(d)) == 0.5
            planted[dtype] += int(half.sum())
            bound = R.f32(cr.SCALE_BOUND)
            for phase in (0, 1):  # both colours of every shape see each condition
                h, s = mr.squeeze(half.float(), phase) > 0, mr.squeeze(scales, phase)
                assert int(h.sum()) >= 10, (shape, dtype, phase)
                d_sq = mr.squeeze(d, phase)[h]
                assert (torch.floor(d_sq) % 2 == 0).any() and (torch.floor(d_sq) % 2 == 1).any()
                at_entry = (s[..., None] == table[:-1]).any(-1) & (s >= bound)
                assert int(at_entry.sum()) >= 5, (shape, dtype, phase)
                assert int((s < bound).sum()) >= 5, (shape, dtype, phase)
            assert (table[:-1] < bound).any()  # so that the bound moves an index
    assert planted[torch.float32] >= 300 and planted[torch.bfloat16] >= 300, planted


def test_vq_tie_conditions():
    seen = set()
    for ncode in list(R.VQ_NCODES) + [R.vq_codebook_size()]:
        for rows in R.VQ_ROWS:
            dot, zn, en = R.vq_case(rows, ncode)
            d = (zn[:, None] + en[None]) - 2 * dot
            for r, (a, b) in R.vq_ties(rows, ncode).items():
                lo = d[r].min()
                assert d[r, a] == lo and d[r, b] == lo and int((d[r] == lo).sum()) == 2  # exact, two-way
                seen.add((a, b))
    ta = lambda j: j % 256  # noqa: E731  the thread that owns code j
    assert any(ta(a) == ta(b) for a, b in seen)  # one thread, two loop trips
    assert any(ta(a) != ta(b) and (ta(a) < 128) != (ta(b) < 128) for a, b in seen)  # across the 128-split
    assert any(ta(a) != ta(b) and ta(a) >= 128 and ta(b) >= 128 for a, b in seen)  # both folded by the first step
    assert any(a < b and ta(a) > ta(b) for a, b in seen)  # the smallest index in the higher thread
    assert {(3, 259), (130, 700)} <= seen


def test_image_input_conditions():
    x = R.x_to_u8_case(17 * 19).view(-1)
    b = R.u8_boundary_values()
    assert b.numel() == 768 and torch.equal(x[:768], b)
    assert torch.isinf(x).sum() == 2 and torch.isnan(x).sum() == 1
    u8 = R.x_to_u8_ref(R.u8_boundary_values()[:256])
    below = R.x_to_u8_ref(R.u8_boundary_values()[256:512])
    assert set(u8.tolist()) | set(below.tolist()) == set(range(256))  # every output value is reached
    assert int((u8 != below).sum()) > 50  # neighbours straddle truncation steps
    for cols in R.SOFTMAX_COLS:
        s = R.softmax_case(cols) * R.SOFTMAX_SCALE
        assert abs(float(s.max()) - 80) < 1e-4 and (cols == 1 or abs(float(s.min()) + 80) < 1e-4)
