"""Time the DISTS metric (rdeic_amd/dists.py) on the device: the whole call, its split between the fp32 backbone
convs, the prep, the four L2 pools and the six moment reductions with their finalizes, each dists.hip kernel's
achieved bytes/s (the bytes the algorithm needs, from shapes, over the event-timed launch), and LPIPS("vgg") on
the same pairs in the same process as the yardstick for the shared backbone. Seeded backbone, seeded weights,
synthetic images.

    python tools/dists_bench.py [--pairs 16] [--size 512] [--reps 20] [--out profiles/FILE.jsonl]

With --loss it times the training loss instead (DISTS.loss): forward and forward + backward for 1 and 16
pairs, LPIPS("vgg").loss on the same inputs in the same process, the conv share of the DISTS loss, every new kernel
of the backward with its algorithmic bytes/s, and (unless --no-refine) the eager refine step at B = 1 with and without
the DISTS term, measured alternately in one process.

    python tools/dists_bench.py --loss [--size 512] [--reps 20] [--no-refine] [--out profiles/FILE.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12  # bytes/s, float4 copy on this part


def timed(fn, reps):
    """Median milliseconds of fn() by device events, after 3 warm-up calls."""
    for _ in range(3):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def wall(fn, reps):
    """(median, min) milliseconds of fn() on the host clock; fn ends in a device-to-host copy."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms)


def loss_bench(a):
    from rdeic_amd import dists as D, lpips as L, ops
    from rdeic_amd.synthetic import synth_image
    backbone = L.seeded_backbone("vgg")
    m = D.DISTS(D.seeded_weights(), backbone=backbone)
    g = torch.Generator().manual_seed(1)
    lp = L.LPIPS("vgg", backbone=backbone,
                 lin={f"lin{k}": torch.rand(c, generator=g) * 0.1 for k, c in enumerate(L.CHANNELS["vgg"])})
    s, heads, lines = a.size, [], []
    for n in (1, 16):
        tgt = torch.from_numpy(np.stack([synth_image(s, s, 100 + i) for i in range(n)])).float() / 127.5 - 1.0
        t = tgt.cuda()
        p = (t + torch.randn(t.shape, generator=torch.Generator().manual_seed(n)).cuda() * (12.0 / 127.5))
        p.requires_grad_(True)

        def fwd(model):
            with torch.no_grad():
                return model.loss(p, t)

        def fwd_bwd(model):
            p.grad = None
            model.loss(p, t).backward()

        head = {"mode": "loss", "pairs": n, "size": s}
        for name, model in (("dists", m), ("lpips_vgg", lp)):
            head[f"{name}_fwd_ms"] = timed(lambda: fwd(model), a.reps)
            head[f"{name}_fwd_bwd_ms"] = timed(lambda: fwd_bwd(model), a.reps)
        head["dists_over_lpips_vgg_fwd_bwd"] = head["dists_fwd_bwd_ms"] / head["lpips_vgg_fwd_bwd_ms"]

        # launch by launch on the prediction side's activations
        groups = {"conv_fwd": 0.0, "conv_bwd": 0.0, "prep": 0.0, "l2pool": 0.0, "l2pool_bwd": 0.0, "moments": 0.0,
                  "tap_bwd": 0.0}

        def add(kind, name, ms, nbytes, times=1):
            groups[kind] += ms * times
            lines.append({"pairs": n, "kind": kind, "name": name, "ms": ms, "bytes": nbytes,
                          "TBps": nbytes / (ms * 1e-3) / 1e12, "of_hbm": nbytes / (ms * 1e-3) / HBM_ACHIEVABLE})

        pd = p.detach()
        raw, x = D.prep_float(pd)
        traw, _ = D.prep_float(t)
        add("prep", f"prep_float {n}x{s}x{s}", timed(lambda: D.prep_float(pd), a.reps), n * s * s * (12 + 32), 2)
        dn, dr = torch.randn_like(x), torch.randn_like(raw)
        add("prep", f"prep_bwd {n}x{s}x{s}", timed(lambda: D.prep_bwd(dn, dr), a.reps), n * s * s * (32 + 12))
        gs = torch.full((n,), -1.0 / n, dtype=torch.float64, device="cuda")
        w0, packs = m._bwd_weights()

        def tap(k, f0, f1):
            mom = D.moments(f0, f1)
            add("moments", f"moments{k} {tuple(f0.shape)}", timed(lambda: D.moments(f0, f1), a.reps),
                4 * 2 * 2 * f0.numel())
            d = torch.zeros_like(f0)
            add("tap_bwd", f"tap_bwd{k} {tuple(f0.shape)} write (coefficients + apply)",
                timed(lambda: D.tap_bwd(f0, f1, mom, m.alpha[k], m.beta[k], gs), a.reps), 4 * 3 * f0.numel(),
                1 if k in (0, 5) else 0)
            if k not in (0, 5):  # the pool / conv chain's gradient is already in the buffer at taps 1..4
                add("tap_bwd", f"tap_bwd{k} {tuple(f0.shape)} add (coefficients + apply)",
                    timed(lambda: D.tap_bwd(f0, f1, mom, m.alpha[k], m.beta[k], gs, out=d), a.reps),
                    4 * 4 * f0.numel())

        tap(0, raw, traw)
        ci, k = 0, 1
        with ops.splitk_as((False, False)):
            for op in L.NETS["vgg"]:
                if op[0] == "conv":
                    cv, xin = m.convs[ci], x
                    y = ops.conv2d(xin, cv, act=ops.LEAKY, slope=0.0)
                    add("conv_fwd", f"conv{ci} {tuple(xin.shape)}->{tuple(y.shape)}",
                        timed(lambda: ops.conv2d(xin, cv, act=ops.LEAKY, slope=0.0), a.reps),
                        4 * (xin.numel() + y.numel() + cv.weight.numel()), 2)
                    dy = torch.randn_like(y)
                    if ci == 0:
                        add("conv_bwd", f"dgrad_small0 {tuple(y.shape)}->{tuple(xin.shape)}",
                            timed(lambda: L.conv_dgrad_small(dy, y, w0, (s, s), 4, 3, 1, 1), a.reps),
                            4 * (2 * y.numel() + xin.numel()))
                    else:
                        hw = tuple(xin.shape[1:3])
                        add("conv_bwd", f"dgrad{ci} {tuple(y.shape)}->{tuple(xin.shape)}",
                            timed(lambda: ops.conv2d(dy, packs[ci], out_hw=hw), a.reps),
                            4 * (xin.numel() + y.numel() + cv.weight.numel()))
                    x, ci = y, ci + 1
                elif op[0] == "pool":
                    xin = x
                    y = D.l2_pool(xin)
                    add("l2pool", f"l2pool {tuple(xin.shape)}", timed(lambda: D.l2_pool(xin), a.reps),
                        4 * (xin.numel() + y.numel()), 2)
                    dy = torch.randn_like(y)
                    add("l2pool_bwd", f"l2pool_bwd {tuple(xin.shape)}",
                        timed(lambda: D.l2_pool_bwd(xin, y, dy), a.reps), 4 * (2 * xin.numel() + 2 * y.numel()))
                    x = y
                else:
                    with torch.no_grad():
                        f1 = torch.randn_like(x).relu_()
                    tap(k, x, f1)
                    k += 1
        head["launch_sum_ms"] = dict(groups)
        head["launch_sum_ms"]["sum"] = sum(groups.values())
        head["conv_share_of_fwd_bwd"] = (groups["conv_fwd"] + groups["conv_bwd"]) / head["dists_fwd_bwd_ms"]
        heads.append(head)
        del p, t, x, raw, traw
        torch.cuda.empty_cache()
    if not a.no_refine:
        heads.append(refine_bench(a, m))
    for r in lines:
        print(f"n={r['pairs']:<2d} {r['kind']:10s} {r['name']:66s} {r['ms']:8.4f} ms  {r['TBps']:.3f} TB/s "
              f"({100 * r['of_hbm']:.0f}% of achievable HBM)")
    for h in heads:
        print(json.dumps(h))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in heads + lines:
                f.write(json.dumps(r) + "\n")


def refine_bench(a, dists_model):
    """The eager refine step at B = 1 with and without the DISTS term, alternately, host clock around a step that
    ends in a synchronize."""
    from rdeic_amd import lpips as L
    from rdeic_amd.finetune import FineTuneConfig, FineTuner, nchw_draws_to_nhwc
    from rdeic_amd.rdeic import RDEIC
    from rdeic_amd.synthetic import refine_draws, synth_context, synth_image
    s = a.size
    g = torch.Generator().manual_seed(2)
    lin = {f"lin{k}": torch.rand(c, generator=g) * 0.1 for k, c in enumerate(L.CHANNELS["alex"])}
    fts = {}
    for name, w in (("without", 0.0), ("with", 0.5)):
        model = RDEIC(compute_dtype=torch.float32).init_synthetic()
        fts[name] = FineTuner(model, FineTuneConfig(used_timesteps=model.used_timesteps, is_refine=True, fixed_step=2,
                                                    l_dists_weight=w),
                              lpips=L.LPIPS("alex", backbone=L.seeded_backbone("alex"), lin=lin),
                              dists=dists_model if w else None)
    ctx = synth_context().cuda()
    img = torch.from_numpy(synth_image(s, s, 231)).cuda()[None]
    slice_ch = fts["with"].m.cfg["compression"]["slice_ch"]
    draws = [nchw_draws_to_nhwc(refine_draws(1, s // 8, s // 8, slice_ch, 7919 + i, 2), "cuda") for i in range(4)]
    ms = {"without": [], "with": []}
    reps = max(3, a.reps // 4)
    for i in range(2 + reps):
        for name in ("without", "with"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fts[name].training_step(img, ctx, draws[i % len(draws)])
            torch.cuda.synchronize()
            if i >= 2:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    out = {"mode": "refine_step", "size": s, "batch": 1, "dtype": "fp32", "reps": reps,
           "without_ms": statistics.median(ms["without"]), "with_ms": statistics.median(ms["with"]),
           "without_ms_all": ms["without"], "with_ms_all": ms["with"]}
    out["added_ms"] = out["with_ms"] - out["without_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loss", action="store_true", help="time DISTS.loss (forward, backward, its kernels) instead")
    ap.add_argument("--no-refine", action="store_true", help="with --loss: skip the refine-step comparison")
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dists_bench needs the GPU")
    if a.loss:
        return loss_bench(a)
    from rdeic_amd import dists as D, lpips as L, ops
    from rdeic_amd.synthetic import synth_image
    backbone = L.seeded_backbone("vgg")
    m = D.DISTS(D.seeded_weights(), backbone=backbone)
    g = torch.Generator().manual_seed(1)
    lp = L.LPIPS("vgg", backbone=backbone,
                 lin={f"lin{k}": torch.rand(c, generator=g) * 0.1 for k, c in enumerate(L.CHANNELS["vgg"])})
    n, s = a.pairs, a.size
    tgt = np.stack([synth_image(s, s, 100 + i) for i in range(n)])
    rng = np.random.default_rng(0)
    pred = np.clip(tgt + rng.normal(0, 12.0, tgt.shape), 0, 255).astype(np.uint8)
    p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(tgt).cuda()

    # the whole calls, host clock around work that ends in a device-to-host copy
    d_ms, d_min = wall(lambda: m(p, t), a.reps)
    l_ms, l_min = wall(lambda: lp(p, t), a.reps)
    head = {"pairs": n, "size": s, "chunk_pairs": D.chunk_pairs(s, s), "dists_call_ms": d_ms,
            "dists_call_ms_min": d_min, "lpips_vgg_call_ms": l_ms, "lpips_vgg_call_ms_min": l_min,
            "dists_over_lpips_vgg": d_ms / l_ms}
    lines = []

    # launch by launch, on one chunk-sized batch as __call__ runs it
    cp = min(n, D.chunk_pairs(s, s))
    both = torch.cat([p[:cp], t[:cp]])
    nb = both.shape[0]
    groups = {"prep": 0.0, "conv": 0.0, "l2pool": 0.0, "moments": 0.0, "score": 0.0}

    def add(kind, name, ms, nbytes, flops=0.0):
        groups[kind] += ms
        rec = {"kind": kind, "name": name, "ms": ms, "bytes": nbytes, "TBps": nbytes / (ms * 1e-3) / 1e12,
               "of_hbm": nbytes / (ms * 1e-3) / HBM_ACHIEVABLE}
        if flops:
            rec["TFLOPs"] = flops / (ms * 1e-3) / 1e12
        lines.append(rec)

    def add_tap(k, f):
        f0, f1 = f[:cp], f[cp:]
        mom = D.moments(f0, f1)
        out = torch.empty(cp, dtype=torch.float64, device="cuda")
        # two passes over both maps; the fp64 partials are 5 / (8 * rows per block) of that and are left out
        add("moments", f"moments{k} {tuple(f0.shape)} (2 passes + 2 finalizes)",
            timed(lambda: D.moments(f0, f1), a.reps), 4 * 2 * 2 * f0.numel())
        add("score", f"score{k} [{cp}, 5, {f0.shape[3]}]",
            timed(lambda: D.tap_score(mom, m.alpha[k], m.beta[k], out=out), a.reps),
            8 * (mom.numel() + 2 * f0.shape[3]))

    raw, x = D.prep(both)
    add("prep", f"prep {nb}x{s}x{s}", timed(lambda: D.prep(both), a.reps), nb * s * s * (3 + 32))
    add_tap(0, raw)
    ci, k = 0, 1
    with ops.splitk_as((False, False)):
        for op in L.NETS["vgg"]:
            if op[0] == "conv":
                cv, xin = m.convs[ci], x
                y = ops.conv2d(xin, cv, act=ops.LEAKY, slope=0.0)
                fl = 2.0 * y.numel() * cv.kh * cv.kw * cv.cin
                add("conv", f"conv{ci} {tuple(xin.shape)}->{tuple(y.shape)} k{cv.kh}",
                    timed(lambda: ops.conv2d(xin, cv, act=ops.LEAKY, slope=0.0), a.reps),
                    4 * (xin.numel() + y.numel() + cv.weight.numel()), fl)
                x, ci = y, ci + 1
            elif op[0] == "pool":
                xin = x
                y = D.l2_pool(xin)
                add("l2pool", f"l2pool {tuple(xin.shape)}", timed(lambda: D.l2_pool(xin), a.reps),
                    4 * (xin.numel() + y.numel()))
                x = y
            else:
                add_tap(k, x)
                k += 1
    head["chunk_images"] = nb
    head["chunk_ms"] = dict(groups)
    head["chunk_ms"]["sum"] = sum(groups.values())
    for r in lines:
        extra = f"  {r['TFLOPs']:.1f} TF" if "TFLOPs" in r else ""
        print(f"{r['kind']:7s} {r['name']:62s} {r['ms']:8.4f} ms  {r['TBps']:.3f} TB/s ({100 * r['of_hbm']:.0f}% of "
              f"achievable HBM){extra}")
    print(json.dumps(head))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(head) + "\n")
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
