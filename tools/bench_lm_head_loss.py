"""A/B the LM-head loss, forward plus backward: the fused kernels
(parallel_linear_cross_entropy: no logits tensor) against the unfused path
(F.linear with lm_head.weight, then parallel_cross_entropy), at the bench
batch of the 8B recipe and at its TP=8 vocab shard.

    python tools/bench_lm_head_loss.py [--rounds 5] [--window 0.5]
                                       [--out samples.json]

Per shape (N, H, V): both arms are warmed up, then alternate over --rounds
rounds; each timed window runs enough steps to last at least --window seconds
and has a device synchronisation on both sides. Peak memory is
torch.cuda.max_memory_allocated above the level before the call, from one
step per arm with the gradients of the previous step freed. The forward
binding alone is timed too, for the rate of the hand-written GEMM
(2 N H V operations over its time). Prints one JSON line.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(16384, 4096, 128256), (16384, 4096, 16032)]  # TP=1, TP=8 shard


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5,
                    help="minimum seconds per timed window")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lm_head_loss needs a GPU"

    from neuronx_distributed_training_amd import ops
    from neuronx_distributed_training_amd.parallel.loss import (
        parallel_cross_entropy, parallel_linear_cross_entropy,
    )

    ext = ops.require_extension()
    result = {"rounds": args.rounds, "shapes": []}
    for N, H, V in SHAPES:
        torch.manual_seed(N + V)
        bf = torch.bfloat16
        h = torch.randn(N, H, device="cuda", dtype=bf, requires_grad=True)
        w = (torch.randn(V, H, device="cuda", dtype=bf) / H ** 0.5
             ).requires_grad_(True)
        target = torch.randint(0, V, (N,), device="cuda")

        def step(fused):
            h.grad = w.grad = None
            if fused:
                loss = parallel_linear_cross_entropy(h, w, target)
            else:
                loss = parallel_cross_entropy(F.linear(h, w), target)
            loss.mean().backward()

        def window(fn, n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n

        arms = {"fused": lambda: step(True), "unfused": lambda: step(False)}
        peak = {}
        for arm, fn in arms.items():  # warm-up, then one measured step
            window(fn, 2)
            h.grad = w.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            window(fn, 1)
            peak[arm] = torch.cuda.max_memory_allocated() - base
        n = 1
        while True:  # steps per window, from the faster arm
            per = min(window(fn, n) for fn in arms.values())
            if per * n >= args.window:
                break
            n = max(n + 1, int(1.1 * args.window / per) + 1)
        samples = {arm: [] for arm in arms}
        for r in range(args.rounds):
            order = list(arms) if r % 2 == 0 else list(arms)[::-1]
            for arm in order:
                samples[arm].append(window(arms[arm], n) * 1e3)
        with torch.no_grad():
            hd, wd = h.detach(), w.detach()
            kern = lambda: ext.lmhead_ce_fwd(hd, wd, target, 0)  # noqa: E731
            window(kern, 2)
            kn = max(1, int(args.window / window(kern, 2)) + 1)
            kms = statistics.median(window(kern, kn) for _ in range(3)) * 1e3
        entry = {"N": N, "H": H, "V": V, "steps_per_window": n,
                 "logits_bytes": N * V * 2,
                 "fwd_kernels_ms": kms,
                 "fwd_kernels_tflops": 2.0 * N * H * V / kms / 1e9}
        for arm, xs in samples.items():
            entry[arm] = {"median_ms": statistics.median(xs), "min_ms": min(xs),
                          "max_ms": max(xs), "samples_ms": xs,
                          "peak_bytes": peak[arm]}
            print(f"N {N} H {H} V {V} {arm}: median "
                  f"{entry[arm]['median_ms']:.2f} ms (min {min(xs):.2f}, max "
                  f"{max(xs):.2f}), peak {peak[arm] / 2**20:.0f} MiB",
                  flush=True)
        print(f"N {N} H {H} V {V} lmhead_ce_fwd alone: {kms:.2f} ms, "
              f"{entry['fwd_kernels_tflops']:.0f} TFLOP/s", flush=True)
        result["shapes"].append(entry)
        del h, w
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
