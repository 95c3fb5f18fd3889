"""A/B one LoRA linear (base GEMM + adapter delta), forward plus backward:
the fused HIP kernels against NXDT_LORA_FUSED=0 (the eager expression), at
the TP=8 shapes of the Llama-3 8B LoRA recipe.

    python tools/bench_lora.py [--tokens 4096] [--rank 16] [--runs 5]
                               [--iters 50] [--out samples.json]

The arms alternate run by run; each run is `iters` steps between two device
synchronisations after a warm-up of both arms. --parts also times the adapter
delta alone (lora_delta_add on a fixed base output), which is what the
kernels replace.
"""

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

SHAPES = [(4096, 512), (4096, 256), (512, 4096)]  # (K, N): q, kv, o at TP=8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=4096)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--parts", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lora needs a GPU"

    from neuronx_distributed_training_amd.ops import lora_delta_add

    T, r, bf = args.tokens, args.rank, torch.bfloat16
    scaling = 32.0 / r
    result = {"tokens": T, "rank": r, "iters": args.iters, "shapes": []}
    for K, N in SHAPES:
        torch.manual_seed(K + N)
        x = torch.randn(T, K, device="cuda", dtype=bf, requires_grad=True)
        W = torch.randn(N, K, device="cuda", dtype=bf) / K ** 0.5
        A = (torch.randn(r, K, device="cuda", dtype=bf) / K ** 0.5
             ).requires_grad_(True)
        B = (torch.randn(N, r, device="cuda", dtype=bf) / r ** 0.5
             ).requires_grad_(True)
        dout = torch.randn(T, N, device="cuda", dtype=bf)
        base_fixed = F.linear(x.detach(), W).requires_grad_(True)

        def linear_step():
            out = lora_delta_add(F.linear(x, W), x, A, B, scaling)
            out.backward(dout)
            x.grad = A.grad = B.grad = None

        def delta_step():
            out = lora_delta_add(base_fixed, x, A, B, scaling)
            out.backward(dout)
            x.grad = A.grad = B.grad = base_fixed.grad = None

        def timed(step, fused):
            os.environ["NXDT_LORA_FUSED"] = "1" if fused else "0"
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                step()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.iters * 1e6  # us / step

        entry = {"K": K, "N": N}
        steps = {"linear": linear_step}
        if args.parts:
            steps["delta"] = delta_step
        for name, step in steps.items():
            for fused in (True, False):  # warm-up of both arms
                timed(step, fused)
            samples = {"fused": [], "eager": []}
            for _ in range(args.runs):
                samples["fused"].append(timed(step, True))
                samples["eager"].append(timed(step, False))
            med = {a: statistics.median(v) for a, v in samples.items()}
            entry[name] = {"samples_us": samples, "median_us": med}
            print(f"K {K} N {N} {name}: fused {med['fused']:.1f} us, eager "
                  f"{med['eager']:.1f} us, eager / fused "
                  f"{med['eager'] / med['fused']:.3f}", flush=True)
        result["shapes"].append(entry)
    os.environ.pop("NXDT_LORA_FUSED", None)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
