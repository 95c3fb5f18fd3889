"""Packed-sequence flash attention: segmented kernels vs the dense kernels,
forward + backward, at the 8k SFT shape.

Run on a GPU box:
    python tools/bench_packed_attn.py [--rounds 7] [--iters 30] [--docs 8]

Three variants are timed with device events on the same seeded inputs:
    seg-N     segmented kernels, N equal documents per row
    seg-1     segmented kernels, one document per row (= the dense mask;
              its gap to `dense` is the overhead of the segment bounds)
    dense     the dense causal kernels (unchanged by the segmented mode)
The variants alternate inside every round, so drift of a shared machine
hits all of them alike; the median over rounds and the min..max spread are
printed, then one JSON line. By tile count seg-N does roughly 1/N of the
dense work; if it is not faster than dense, tile skipping is broken.
"""

import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--docs", type=int, default=8)
    ap.add_argument("--seq", type=int, default=8192)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--hq", type=int, default=32)
    ap.add_argument("--hkv", type=int, default=8)
    ap.add_argument("--d", type=int, default=128)
    args = ap.parse_args()

    from neuronx_distributed_training_amd.ops import (
        require_extension, segment_bounds,
    )

    ext = require_extension()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    dev, bf = "cuda:0", torch.bfloat16
    torch.manual_seed(0)
    b, hq, hkv, s, d = args.batch, args.hq, args.hkv, args.seq, args.d
    assert s % args.docs == 0
    q = torch.randn(b, hq, s, d, device=dev, dtype=bf)
    k = torch.randn(b, hkv, s, d, device=dev, dtype=bf)
    v = torch.randn(b, hkv, s, d, device=dev, dtype=bf)
    do = torch.randn(b, hq, s, d, device=dev, dtype=bf)
    scale = 1.0 / math.sqrt(d)

    def bounds(n_docs):
        ids = (torch.arange(s, device=dev) // (s // n_docs)).expand(b, s)
        return segment_bounds(ids.contiguous())

    def seg_fn(n_docs):
        qs, ke = bounds(n_docs)

        def step():
            o, lse = ext.flash_attn_fwd_seg(q, k, v, qs, ke, scale, 0)
            return o, ext.flash_attn_bwd_seg(do, q, k, v, o, lse, qs, ke,
                                             scale, 0)
        return step

    def dense_fn():
        o, lse = ext.flash_attn_fwd(q, k, v, True, scale, 0)
        return o, ext.flash_attn_bwd(do, q, k, v, o, lse, True, scale, 0)

    variants = {
        f"seg-{args.docs}": seg_fn(args.docs),
        "seg-1": seg_fn(1),
        "dense": dense_fn,
    }

    # same numbers first: one document is the dense mask
    o1, g1 = variants["seg-1"]()
    od, gd = variants["dense"]()
    drift = max(float((a.float() - c.float()).abs().max())
                for a, c in zip((o1,) + tuple(g1), (od,) + tuple(gd)))
    print(f"seg-1 vs dense max abs diff (o, dq, dk, dv): {drift:.3e}")

    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()

    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.iters):
                fn()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / args.iters)

    med = {n: statistics.median(t) for n, t in times.items()}
    for n, t in times.items():
        print(f"{n:>8}: fwd+bwd median {med[n]:8.3f} ms   "
              f"min {min(t):8.3f}  max {max(t):8.3f}   ({args.rounds} rounds "
              f"x {args.iters} iters)")
    packed = f"seg-{args.docs}"
    print(f"{packed} is {med['dense'] / med[packed]:.2f}x faster than dense; "
          f"seg-1 overhead over dense {100 * (med['seg-1'] / med['dense'] - 1):+.1f}%")
    print(json.dumps({
        "shape": dict(b=b, hq=hq, hkv=hkv, s=s, d=d, docs=args.docs),
        "median_ms": med,
        "min_ms": {n: min(t) for n, t in times.items()},
        "max_ms": {n: max(t) for n, t in times.items()},
        "seg1_vs_dense_max_abs_diff": drift,
    }))


if __name__ == "__main__":
    main()
