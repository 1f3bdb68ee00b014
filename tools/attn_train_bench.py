"""Training attention, flash against materialised, on config 5's shapes (bf16, batch 1): time of one
forward + backward (captured as a graph and replayed, as the fine-tune step runs it), library entry calls,
kernel launches and peak memory above the inputs. One JSON line per shape.

  python tools/attn_train_bench.py [--size 512] [--batch 1] [--reps 20] [--only base|control]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CTX = 77
# (branch, head dim, [(heads, latent side divisor)]) of the UNet / control model at each attention level
LEVELS = (("base", 64, ((5, 1), (10, 2), (20, 4), (20, 8))), ("control", 16, ((4, 1), (8, 2), (16, 4), (16, 8))))


def run(impl, batch, heads, lq, lk, dh, grads, reps):
    from rdeic_amd import _lib, autograd as AG
    AG.set_attention_impl(impl)
    g = torch.Generator(device="cuda").manual_seed(1)
    c = heads * dh
    q, do = (torch.randn(batch * lq, c, generator=g, device="cuda").bfloat16() for _ in range(2))
    k, v = (torch.randn(batch * lk, c, generator=g, device="cuda").bfloat16() for _ in range(2))
    q.requires_grad_()
    if grads == "qkv":
        k.requires_grad_()
        v.requires_grad_()
    wrt = (q, k, v) if grads == "qkv" else (q,)

    def body():
        return torch.autograd.grad(AG.attention(q, k, v, batch, heads, dh ** -0.5), wrt, do)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        _lib.RECORDER = []
        body()
        calls = [name for name, *_ in _lib.RECORDER]
        _lib.RECORDER = None
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = body()
    for _ in range(3):
        graph.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    del out
    # kernels: every materialised entry is one kernel; the flash backward entry is delta + dK/dV (+ slab sum
    # when the query sweep is chunked: the workspace then holds slabs) + dQ
    kernels = len(calls)
    if "rdeic_attention_bwd" in calls:
        ws = int(_lib.load().rdeic_attention_bwd_workspace(batch, heads, lq, lk, dh))
        delta = (batch * heads * lq + 3) // 4 * 16
        kernels += 1 + (2 if grads == "qkv" and ws > delta else 1 if grads == "qkv" else 0)
    return {"us": round(1000.0 * e0.elapsed_time(e1) / reps, 1), "calls": len(calls), "kernels": kernels,
            "peak_mib": round(peak / 2**20, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    side = args.size // 8
    for branch, dh, levels in LEVELS:
        if args.only and args.only != branch:
            continue
        for heads, div in levels:
            L = (side // div) ** 2
            # self-attention: all three gradients; cross-attention: K / V come from the text context through
            # frozen (base) or trained (control) projections; the base UNet is frozen, so dQ only there
            for kind, lk, grads in (("self", L, "qkv"), ("cross", CTX, "qkv" if branch == "control" else "q")):
                row = {"branch": branch, "dh": dh, "heads": heads, "lq": L, "lk": lk, "kind": kind, "grads": grads,
                       "batch": args.batch}
                for impl in ("materialized", "flash"):
                    row[impl] = run(impl, args.batch, heads, L, lk, dh, grads, args.reps)
                row["speedup"] = round(row["materialized"]["us"] / row["flash"]["us"], 2)
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
