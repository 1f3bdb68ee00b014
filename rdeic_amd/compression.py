"""The RDEIC compressor (model/compression.py, model/compression_modules.py, utils/ckbd.py)
on the HIP kernels + host C++ coders, batched over images.

Nets (NHWC, reference parameter names under `preprocess_model.`):
  g_a  Encoder        compression_modules.py:7-24   (ResidualBlock / WithStride, res_blk.py:6-93)
  hyper_enc / dec     compression_modules.py:47-73  (ResidualBlockUpsample = subpel 1x1 + PixelShuffle,
                                                     fused into the conv store)
  ChannelContextEX    compression_modules.py:76-89  (5x5 convs + exact GELU)
  EntropyParametersEX compression_modules.py:91-104 (1x1 convs + GELU), local_context 5x5
  VectorQuantiser.quant / get_codebook_entry        compression_modules.py:309-338
  g_s Decoder + out   compression_modules.py:27-44, compression.py:21
Entropy stage (10 slices x {anchor, non-anchor}, compression.py:171-203 / 233-264):
  params -> rdeic_ckbd_encode (squeeze, build_indexes, round, dequantise, unsqueeze in one
  kernel) -> per-image symbol/index lists in the reference order -> C++ rANS (one stream per
  image, host threads). Torch.cat of [local_ctx, channel_ctx, hyper_params] is never
  materialised: producers write into channel slices of one context buffer and the first
  entropy-parameter conv gathers its two input segments directly.
The reference codes batch 1 per call (utils/ckbd.py:140 hard-codes batch 1 on decode); every
kernel here is batch-invariant (fixed reduction order), so a batched call produces exactly the
per-image streams and reconstructions of B single-image calls.

Host/GPU overlap: the batch is split into `coder_groups` image groups whose stage sequences run
interleaved (generators that yield at every host round trip), so while the host rANS-codes one
group's stage the GPU runs the stages the other group has queued. The GPU part of compress and of
decompress, with the host coder steps at their places in the sequence (plan.host_step), is
recorded once per shape as a launch plan and replayed (rdeic_amd/plan.py).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, coders, ops
from .params import ParamStore
from .plan import PlanCache, host_step

LEAK = 0.01


class Compression:
    def __init__(self, store: ParamStore, in_nc: int, out_nc: int, N: int, M: int, slice_num: int,
                 slice_ch: Sequence[int], codebook_size: int, prefix: str = "preprocess_model."):
        self.store, self.p = store, prefix
        self.N, self.M = N, M
        self.slice_num, self.slice_ch = slice_num, list(slice_ch)
        self.slice_off = [sum(self.slice_ch[:i]) for i in range(slice_num)]
        self.codebook_size = codebook_size
        p = prefix
        d = store
        # g_a
        self.g_a = []
        spec = [("rb", in_nc, M), ("rb", M, M), ("rb", M, M), ("rb", M, M), ("rbs", M, M), ("rb", M, M),
                ("rb", M, M), ("rb", M, M)]
        for i, (kind, ci, co) in enumerate(spec):
            self.g_a.append(self._declare_block(f"{p}encoder.g_a.{i}", kind, ci, co))
        d.declare_conv(f"{p}encoder.g_a.8", M, M, 3)
        self.g_a.append((f"{p}encoder.g_a.8", "conv", M, M))
        self.hyper_enc = [self._declare_block(f"{p}hyper_enc.hyper_enc.{i}", k, ci, co) for i, (k, ci, co) in
                          enumerate([("rb", M, N), ("rb", N, N), ("rbs", N, N), ("rbs", N, N)])]
        self.hyper_dec = [self._declare_block(f"{p}hyper_dec.hyper_dec.{i}", k, ci, co) for i, (k, ci, co) in
                          enumerate([("rbu", N, M), ("rbu", M, M), ("rb", M, M * 3 // 2), ("rb", M * 3 // 2, M * 2)])]
        d.declare_conv(f"{p}decoder.g_s.0", M, M, 3)
        self.g_s = [(f"{p}decoder.g_s.0", "conv", M, M)]
        for i, (k, ci, co) in enumerate([("rb", M, M)] * 3 + [("rbu", M, M)] + [("rb", M, M)] * 4):
            self.g_s.append(self._declare_block(f"{p}decoder.g_s.{i + 1}", k, ci, co))
        d.declare_conv(f"{p}out", out_nc, M, 3)
        for i, c in enumerate(self.slice_ch):
            d.declare_conv(f"{p}local_context.{i}", 2 * c, c, 5)
            if i:
                cin = sum(self.slice_ch[:i])
                d.declare_conv(f"{p}channel_context.{i}.fushion.0", 224, cin, 5)
                d.declare_conv(f"{p}channel_context.{i}.fushion.2", 128, 224, 5)
                d.declare_conv(f"{p}channel_context.{i}.fushion.4", 2 * c, 128, 5)
            for nm, cin in (("entropy_parameters_anchor", 2 * M + (2 * c if i else 0)),
                            ("entropy_parameters_nonanchor", 2 * M + (4 * c if i else 2 * c))):
                out = 2 * c
                d.declare_conv(f"{p}{nm}.{i}.fusion.0", out * 5 // 3, cin, 1)
                d.declare_conv(f"{p}{nm}.{i}.fusion.2", out * 4 // 3, out * 5 // 3, 1)
                d.declare_conv(f"{p}{nm}.{i}.fusion.4", out, out * 4 // 3, 1)
        d.declare(f"{p}quantize.embedding.weight", (codebook_size, N))
        self.tables = None
        self._en = None
        # image groups interleaved in the stage loops: measured on MI355X (B=16, 512^2) 2 groups cost
        # more GPU time (twice the small stage launches) than the host overlap saves, so 1
        self.coder_groups = 1
        self.use_plans = True
        self._plans = PlanCache()
        self._io = {}              # per-call host state read by the recorded host steps

    def _declare_block(self, pre, kind, ci, co):
        d = self.store
        if kind == "rb":
            d.declare_conv(pre + ".conv1", co, ci, 3)
            d.declare_conv(pre + ".conv2", co, co, 3)
            if ci != co:
                d.declare_conv(pre + ".adaptor", co, ci, 1)
        elif kind == "rbs":
            d.declare_conv(pre + ".conv1", co, ci, 3)
            d.declare_conv(pre + ".conv2", co, co, 3)
            d.declare_conv(pre + ".downsample", co, ci, 1)
        elif kind == "rbu":
            d.declare_conv(pre + ".subpel_conv.0", co * 4, ci, 1)
            d.declare_conv(pre + ".conv", co, co, 3)
            d.declare_conv(pre + ".upsample.0", co * 4, ci, 1)
        return (pre, kind, ci, co)

    # ------------------------------------------------------------------ tables
    def update(self, scale_table=None, force: bool = False):
        """GaussianConditional.update_scale_table(get_scale_table()) (compression.py:275-280)."""
        if self.tables is None or force or scale_table is not None:
            self.tables = coders.GaussianTables(scale_table)
            self._plans.clear()  # recorded plans hold the previous device scale table
        return True

    # ------------------------------------------------------------------ nets
    def _block(self, blk, x):
        pre, kind, ci, co = blk
        s = self.store
        if kind == "conv":
            return ops.conv2d(x, s.conv(pre))
        if kind == "rb":
            identity = x if ci == co else ops.conv2d(x, s.conv(pre + ".adaptor"))
            out = ops.conv2d(x, s.conv(pre + ".conv1"), act=ops.LEAKY, slope=LEAK)
            return ops.conv2d(out, s.conv(pre + ".conv2"), act=ops.LEAKY, slope=LEAK, res=identity)
        if kind == "rbs":
            out = ops.conv2d(x, s.conv(pre + ".conv1", stride=2, pad=1), act=ops.LEAKY, slope=LEAK)
            identity = ops.conv2d(x, s.conv(pre + ".downsample", stride=2, pad=0))
            return ops.conv2d(out, s.conv(pre + ".conv2"), act=ops.LEAKY, slope=0.1, res=identity)
        if kind == "rbu":
            out = ops.conv2d(x, s.conv(pre + ".subpel_conv.0"), pixel_shuffle=True, act=ops.LEAKY, slope=LEAK)
            identity = ops.conv2d(x, s.conv(pre + ".upsample.0"), pixel_shuffle=True)
            return ops.conv2d(out, s.conv(pre + ".conv"), act=ops.LEAKY, slope=0.1, res=identity)
        raise ValueError(kind)

    def _seq(self, blocks, x):
        for b in blocks:
            x = self._block(b, x)
        return x

    def _pad_width(self, c: int):
        """bf16: zero-pad the odd hidden widths of the entropy nets (5/3 and 4/3 of 2c, 224) to 64-channel
        blocks (16 below 32) so their convs gather 16-byte vectors / run on the LDS-DMA kernel. Encoder and
        decoder pad identically (the padded channels are exactly 0), so mu / sigma stay identical
        between them; the fp32 parity mode keeps the reference widths."""
        if self.store.compute_dtype != torch.bfloat16:
            return None
        return -(-c // 64) * 64 if c > 32 else -(-c // 16) * 16

    def _ep(self, name: str, i: int, x: torch.Tensor, x2: torch.Tensor) -> torch.Tensor:
        s, p = self.store, self.p
        f0, f2, f4 = (f"{p}{name}.{i}.fusion.{j}" for j in (0, 2, 4))
        w0, w2 = s.shapes[f0 + ".weight"][0], s.shapes[f2 + ".weight"][0]
        p0, p2 = self._pad_width(w0), self._pad_width(w2)
        h = ops.conv2d(x, s.conv(f0, cout_pad=p0), x2=x2, act=ops.GELU)
        h = ops.conv2d(h, s.conv(f2, cin_pad=p0, cout_pad=p2), act=ops.GELU)
        return ops.conv2d(h, s.conv(f4, cin_pad=p2))

    def _channel_ctx(self, i: int, yhat_prefix: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        s, p = self.store, self.p
        f0, f2, f4 = (f"{p}channel_context.{i}.fushion.{j}" for j in (0, 2, 4))
        p0 = self._pad_width(s.shapes[f0 + ".weight"][0])
        h = ops.conv2d(yhat_prefix, s.conv(f0, cout_pad=p0), act=ops.GELU)
        h = ops.conv2d(h, s.conv(f2, cin_pad=p0), act=ops.GELU)
        return ops.conv2d(h, s.conv(f4), out=out)

    # ------------------------------------------------------------------ VQ
    def _codebook(self) -> torch.Tensor:
        return self.store.get(self.p + "quantize.embedding.weight")

    def vq_quant(self, z: torch.Tensor):
        """VectorQuantiser.quant: first-argmin over (|z|^2 + |e|^2) - 2 z.e in fp32."""
        B, hz, wz, N = z.shape
        rows = B * hz * wz
        E = self._codebook()
        zf = ops.cast(z.contiguous(), torch.float32).view(rows, N)
        zn = torch.empty(rows, dtype=torch.float32, device=z.device)
        ops.call("rdeic_row_sqnorm", zf.data_ptr(), rows, N, N, zn.data_ptr(), 0, ops.stream_ptr())
        if self._en is None or self._en.device != z.device:
            self._en = torch.empty(E.shape[0], dtype=torch.float32, device=z.device)
            ops.call("rdeic_row_sqnorm", E.data_ptr(), E.shape[0], N, N, self._en.data_ptr(), 0, ops.stream_ptr())
        dot = ops.linear(zf, self.store.conv(self.p + "quantize.embedding", dtype=torch.float32), images=B)
        idx = torch.empty(rows, dtype=torch.int32, device=z.device)
        ops.call("rdeic_vq_argmin", dot.data_ptr(), zn.data_ptr(), self._en.data_ptr(), rows, E.shape[0],
                 idx.data_ptr(), ops.stream_ptr())
        return self.codebook_entry(idx, B, hz, wz), idx.view(B, hz, wz)

    def codebook_entry(self, idx: torch.Tensor, B: int, hz: int, wz: int) -> torch.Tensor:
        E = self._codebook()
        N = E.shape[1]
        zq = torch.empty((B, hz, wz, N), dtype=self.store.compute_dtype, device=E.device)
        ops.call("rdeic_gather_rows", E.data_ptr(), N, idx.contiguous().data_ptr(), B * hz * wz, N, zq.data_ptr(), N,
                 ops.dt_code(zq), ops.stream_ptr())
        return zq

    # ------------------------------------------------------------------ entropy stages
    def _pinned(self, key: str, n: int, dtype=torch.int32) -> torch.Tensor:
        """Reusable page-locked host staging buffer (>= n elements) for the coder round trips."""
        cache = self.__dict__.setdefault("_pin_cache", {})
        buf = cache.get(key)
        if buf is None or buf.numel() < n or buf.dtype != dtype:
            buf = torch.empty(max(n, 1), dtype=dtype, pin_memory=True)
            cache[key] = buf
        return buf[:n]

    def stage_sizes(self, hy: int, wy: int) -> List[int]:
        sizes = []
        for c in self.slice_ch:
            sizes += [c * hy * (wy // 2)] * 2
        return sizes

    def _stage_common(self, hy, wy, B, device, dt):
        yhat = torch.empty((B, hy, wy, self.M), dtype=dt, device=device)
        cmax = max(self.slice_ch)
        ctx = torch.empty((B, hy, wy, 4 * cmax), dtype=dt, device=device)
        anchor = torch.empty((B, hy, wy, cmax), dtype=dt, device=device)
        return yhat, ctx, anchor

    def _stage_gen(self, hyper, hy, wy, emit, bufs):
        """Generator over the 20 checkerboard stages of one image group (hyper and bufs are that
        group's batch slices). emit(i, phase, params, c, off, yhat_slice, anchor_buf) produces the
        dequantised slice values (encode: from y; decode: from the bitstream). It may return a
        generator, whose yields mark the host round trips other groups can overlap."""
        yhat, ctxbuf, anchor_full = bufs
        off = 0
        for i, c in enumerate(self.slice_ch):
            s0 = self.slice_off[i]
            ctx = ctxbuf[..., :4 * c]
            anchor = anchor_full[..., :c]
            if i == 0:
                pa = self._ep("entropy_parameters_anchor", 0, hyper, None)
            else:
                self._channel_ctx(i, yhat[..., :s0], out=ctx[..., 2 * c:4 * c])
                pa = self._ep("entropy_parameters_anchor", i, ctx[..., 2 * c:4 * c], hyper)
            r = emit(i, 0, pa, c, off, yhat[..., s0:s0 + c], anchor)
            if r is not None:
                yield from r
            off += c * hy * (wy // 2)
            ops.conv2d(anchor, self.store.conv(f"{self.p}local_context.{i}"), out=ctx[..., :2 * c])
            pn = self._ep("entropy_parameters_nonanchor", i, ctx[..., :(4 * c if i else 2 * c)], hyper)
            r = emit(i, 1, pn, c, off, yhat[..., s0:s0 + c], None)
            if r is not None:
                yield from r
            off += c * hy * (wy // 2)

    def _run_stages(self, hyper, B, hy, wy, emit):
        """The 20 stages for the whole batch as one group."""
        bufs = self._stage_common(hy, wy, B, hyper.device, hyper.dtype)
        for _ in self._stage_gen(hyper, hy, wy, emit, bufs):
            pass
        return bufs[0]

    def _groups(self, B: int) -> List[Tuple[int, int]]:
        g = max(1, min(int(self.coder_groups), B))
        cut = [B * k // g for k in range(g + 1)]
        return [(cut[k], cut[k + 1]) for k in range(g)]

    @staticmethod
    def _interleave(gens) -> None:
        """Round-robin over the groups' stage generators (one stream; host waits are per-event,
        so a group's host step never waits for GPU work queued after it)."""
        live = list(gens)
        while live:
            for g in list(live):
                try:
                    next(g)
                except StopIteration:
                    live.remove(g)

    def _run_region(self, name, fn, inputs, before=None):
        """fn(*inputs) eagerly, or recorded once per shape and replayed (launch plan)."""
        if not self.use_plans:
            if before is not None:
                before()
            return fn(*inputs)
        key = (name, self.coder_groups) + tuple((tuple(t.shape), t.dtype) for t in inputs)
        return self._plans.run(key, fn, inputs, before=before)

    # ------------------------------------------------------------------ compress / decompress
    def _splitk(self):
        """Split-K for the entropy model's small-grid convs (bf16; ops.SPLITK_ENTROPY): the k-split count
        is chosen from the per-image shape (ops.SPLITK_NOMINAL_BATCH), so the encoder and the decoder —
        whatever their batch — run every layer with the same k grouping and compute identical mu / sigma.
        The fp32 parity mode keeps the unsplit order of the oracle comparison."""
        import contextlib
        if self.store.compute_dtype == torch.bfloat16 and ops.SPLITK_ENTROPY:
            return ops.splitk_allowed()
        return contextlib.nullcontext()

    def _compress_gpu(self, h: torch.Tensor) -> torch.Tensor:
        with self._splitk():
            return self._compress_gpu_body(h)

    def _compress_gpu_body(self, h: torch.Tensor) -> torch.Tensor:
        """compress() up to the bytes of the z indexes: nets, VQ, the 20 stages, and (host steps)
        the rANS coding of each image group into self._io["y_strings"]. Returns the pinned host
        copy of the VQ indexes [B, hz, wz], complete once the region has run."""
        B = h.shape[0]
        y = self._seq(self.g_a, h)
        z = self._seq(self.hyper_enc, y)
        z_q, z_idx = self.vq_quant(z)
        hyper = self._seq(self.hyper_dec, z_q)
        _, hy, wy, _ = y.shape
        total = sum(self.stage_sizes(hy, wy))
        table = self.tables.device_scale_table(h.device)
        dtc = ops.dt_code(h)
        bufs = self._stage_common(hy, wy, B, h.device, hyper.dtype)
        zi_p = self._pinned("enc_zidx", z_idx.numel()).view(z_idx.shape)
        host_step(lambda: zi_p.copy_(z_idx, non_blocking=True))

        def group(gi: int, b0: int, b1: int):
            nb = b1 - b0
            yg = y[b0:b1]
            # the symbols and indexes go straight from the stage kernels into pinned host memory
            # (device-addressable; ordered for the host by the event after the last stage): no copy
            # launches on the stream
            sym_p = self._pinned(f"enc_sym{gi}", nb * total).view(nb, total)
            idx_p = self._pinned(f"enc_idx{gi}", nb * total).view(nb, total)
            done = torch.cuda.Event()

            def emit(i, phase, params, c, off, yhat_slice, anchor):
                s0 = self.slice_off[i]
                ys = yg[..., s0:s0 + c]
                ops.call("rdeic_ckbd_encode", ys.data_ptr(), ops.pix_ld(ys), params.data_ptr(), ops.pix_ld(params), nb,
                         hy, wy, c, phase, table.data_ptr(), table.numel(), float(coders.SCALE_BOUND), sym_p.data_ptr(),
                         idx_p.data_ptr(), total, off, yhat_slice.data_ptr(), ops.pix_ld(yhat_slice),
                         None if anchor is None else anchor.data_ptr(), 0 if anchor is None else ops.pix_ld(anchor),
                         dtc, ops.stream_ptr())

            yield from self._stage_gen(hyper[b0:b1], hy, wy, emit, [t[b0:b1] for t in bufs])

            def to_host():
                done.record()

            host_step(to_host)
            yield  # the next group's stages are queued before this group is coded

            def code():
                done.synchronize()
                self._io["y_strings"][b0:b1] = coders.rans_encode_batch(sym_p.numpy(), idx_p.numpy(), self.tables)

            host_step(code)

        self._interleave([group(gi, b0, b1) for gi, (b0, b1) in enumerate(self._groups(B))])
        return zi_p

    def compress_with(self, front, x: torch.Tensor) -> List[dict]:
        """compress(front(x)), with front's launches (e.g. the VAE encoder; launch-only) inside the
        same recorded region."""
        self.update()
        B = x.shape[0]
        self._io = {"y_strings": [b""] * B}
        try:
            zi = self._run_region("compress", lambda t: self._compress_gpu(front(t)), [x]).numpy()
            y_strings = self._io["y_strings"]
        finally:
            self._io = {}
        hz, wz = zi.shape[1], zi.shape[2]
        out = []
        for b in range(B):
            z_str = coders.ac_encode_uniform(zi[b], self.codebook_size)
            out.append({"strings": [[y_strings[b]], [z_str]], "shape": (hz, wz)})
        return out

    @torch.no_grad()
    def compress(self, h: torch.Tensor) -> List[dict]:
        """h: NHWC [B, H/8, W/8, 512] (compute dtype). Returns one reference-format dict per image:
        {"strings": [[y_string], [z_string]], "shape": (zh, zw)} (compression.py:151-213)."""
        return self.compress_with(lambda t: t, h)

    def _decompress_gpu(self, z_idx: torch.Tensor):
        with self._splitk():
            return self._decompress_gpu_body(z_idx)

    def _decompress_gpu_body(self, z_idx: torch.Tensor):
        """decompress() from the device VQ indexes on: codebook, hyper decoder, the 20 stages with
        their rANS round trips (host steps, decoders in self._io["decs"]), g_s and the out conv."""
        B, hz, wz = z_idx.shape
        z_q = self.codebook_entry(z_idx, B, hz, wz)
        hyper = self._seq(self.hyper_dec, z_q)
        _, hy, wy, _ = hyper.shape
        dev = hyper.device
        table = self.tables.device_scale_table(dev)
        dtc = ops.dt_code(hyper)
        nmax = max(self.stage_sizes(hy, wy))
        bufs = self._stage_common(hy, wy, B, dev, hyper.dtype)

        def group(gi: int, b0: int, b1: int):
            nb = b1 - b0
            idx_pin = self._pinned(f"dec_idx{gi}", nb * nmax)  # sized once: no regrowth mid-loop
            sym_pin = self._pinned(f"dec_sym{gi}", nb * nmax)

            def emit(i, phase, params, c, off, yhat_slice, anchor):
                # the indexes kernel writes pinned host memory and the dequant kernel reads the decoded
                # symbols from it (device-addressable): the round trip has no copy launches. The host
                # reads after the event; it rewrites the symbols only after the next stage's event,
                # which the stream orders after this stage's dequant.
                n = c * hy * (wy // 2)
                idx_p = idx_pin[:nb * n].view(nb, n)
                sym_p = sym_pin[:nb * n].view(nb, n)
                ops.call("rdeic_ckbd_indexes", params.data_ptr(), ops.pix_ld(params), nb, hy, wy, c, phase,
                         table.data_ptr(), table.numel(), float(coders.SCALE_BOUND), idx_p.data_ptr(), n, 0, dtc,
                         ops.stream_ptr())
                ready = torch.cuda.Event()

                def to_host():
                    ready.record()

                host_step(to_host)
                yield  # other groups queue their stages while these indexes come back

                def decode():
                    ready.synchronize()
                    # isolate=True: a per-stream status instead of one exception for the batch; the failed and
                    # the absent streams' symbols are written as 0, so the dequant below reads host-written rows
                    st = self._io.get("status")
                    coders.rans_decode_batch(self._io["decs"][b0:b1], idx_p.numpy(), self.tables, out=sym_p.numpy(),
                                             status=None if st is None else st[b0:b1])

                host_step(decode)
                ops.call("rdeic_ckbd_dequant", sym_p.data_ptr(), params.data_ptr(), ops.pix_ld(params), nb, hy, wy, c,
                         phase, n, 0, yhat_slice.data_ptr(), ops.pix_ld(yhat_slice),
                         None if anchor is None else anchor.data_ptr(), 0 if anchor is None else ops.pix_ld(anchor),
                         dtc, ops.stream_ptr())

            return self._stage_gen(hyper[b0:b1], hy, wy, emit, [t[b0:b1] for t in bufs])

        self._interleave([group(gi, b0, b1) for gi, (b0, b1) in enumerate(self._groups(B))])
        guide_hint = self._seq(self.g_s, bufs[0])
        c_latent = ops.conv2d(guide_hint, self.store.conv(self.p + "out"), out_f32=True)
        return c_latent, guide_hint

    @staticmethod
    def check_z_shape(shape) -> Tuple[int, int]:
        """The header's hyper-latent shape as ints; ValueError when no image can have it."""
        hz, wz = int(shape[0]), int(shape[1])
        if not (0 < hz <= 1024 and 0 < wz <= 1024 and hz * wz <= 65536):  # a 16384^2 image has a 256^2 z
            raise ValueError(f"implausible hyper-latent shape {(hz, wz)} (corrupted header?)")
        return hz, wz

    @torch.no_grad()
    def decompress(self, strings_list: Sequence[Sequence[Sequence[bytes]]], shape: Tuple[int, int],
                   device="cuda", isolate: bool = False):
        """strings_list[b] = [[y_string], [z_string]] for image b (all of one latent shape).
        Returns (c_latent fp32 NHWC [B,h,w,4], guide_hint NHWC [B,h,w,M]) (compression.py:215-273).

        isolate=True returns (c_latent, guide_hint, errors): a stream fails on its own and the batch goes on.
        errors[b] is None, or the exception image b would have raised alone: a z string that does not decode, or a
        rANS status other than 0 in any of the 20 stages. strings_list[b] may itself be an exception (a body that
        did not parse): it is carried into errors[b]. An image that fails before the device work runs with zero z
        indexes and no decoder; one that fails in a stage decodes zeros from there on. The launches are the ones of
        isolate=False (one recorded plan serves both), the survivors' rows are what they decode to alone, and the
        failed rows are returned as zeros."""
        self.update()
        B = len(strings_list)
        hz, wz = self.check_z_shape(shape)
        errors: List[Optional[Exception]] = [None] * B
        if not isolate:
            zi = np.stack([coders.ac_decode_uniform(st[1][0], hz * wz, self.codebook_size) for st in strings_list])
        else:
            zi = np.zeros((B, hz * wz), dtype=np.int16)
            for b, st in enumerate(strings_list):
                try:
                    if isinstance(st, Exception):
                        raise st
                    zi[b] = coders.ac_decode_uniform(st[1][0], hz * wz, self.codebook_size)
                    st[0][0]  # a header that announces fewer strings than two
                except Exception as e:  # noqa: BLE001 — the reference's convention: any exception is a decode failure
                    errors[b] = e
        self.last_z_idx = zi  # [B, hz * wz] VQ indices of this call (the validation epoch's codebook usage)
        z_idx = torch.from_numpy(zi.astype(np.int32).reshape(B, hz, wz)).to(device)

        def close_decoders():
            for d in self._io.get("decs", []):
                if d is not None:
                    d.close()

        def fresh_decoders():  # the decoders are stateful: one fresh set per execution of the region
            close_decoders()
            self._io["decs"] = [None if errors[b] is not None else coders.RansDecoder(st[0][0])
                                for b, st in enumerate(strings_list)]
            if isolate:
                self._io["status"] = np.zeros(B, dtype=np.int32)

        self._io = {}
        try:
            c_latent, guide_hint = self._run_region("decompress", self._decompress_gpu, [z_idx], before=fresh_decoders)
            if self.use_plans:  # the plan's outputs are its static buffers
                c_latent, guide_hint = c_latent.clone(), guide_hint.clone()
            status = self._io.get("status")
        finally:
            close_decoders()
            self._io = {}
        if not isolate:
            return c_latent, guide_hint
        for b in range(B):
            if errors[b] is None and status[b] != 0:
                errors[b] = (_lib.BitstreamError if status[b] == _lib.EBADMSG else _lib.RdeicError)(
                    "rdeic_rans_decode_batch", int(status[b]))
        bad = [b for b in range(B) if errors[b] is not None]
        if bad:
            c_latent[bad] = 0
            guide_hint[bad] = 0
        return c_latent, guide_hint, errors
