"""Kernel A/B at decode shapes: the split-KV decode kernel
(flash_attn_decode) against the training forward that decode ran through
before (flash_attn_fwd), on identical inputs in one process, arms
alternating.

    python tools/bench_flash_decode.py [--iters 200] [--rounds 5]

Per shape: median time per call of each arm (device events around `iters`
back-to-back calls, median over `rounds` alternating rounds), the max abs
difference of the two outputs, and the achieved K/V bytes per second =
2 * B * HKV * S_kv * D * 2 bytes (what the algorithm must read) over that
time. A call of the decode arm is its two kernels plus the allocation of
their outputs, as the model issues it.
"""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def _time(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters * 1e3   # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--splits", type=int, default=0,
                    help="num_splits override (0 = heuristic)")
    args = ap.parse_args()

    from neuronx_distributed_training_amd import ops

    if not torch.cuda.is_available():
        raise SystemExit("bench_flash_decode needs a GPU")
    ext = ops.require_extension()
    hq, hkv, d, sq = 32, 8, 128, 1
    scale = d ** -0.5
    bf = torch.bfloat16
    for b in (1, 8):
        for skv in (512, 4096, 8192):
            torch.manual_seed(0)
            q = torch.randn(b, hq, sq, d, device="cuda", dtype=bf)
            k = torch.randn(b, hkv, skv, d, device="cuda", dtype=bf)
            v = torch.randn(b, hkv, skv, d, device="cuda", dtype=bf)
            lo = torch.zeros(b, device="cuda", dtype=torch.int32)
            hi = torch.full((b,), skv, device="cuda", dtype=torch.int32)

            def new():
                return ext.flash_attn_decode(q, k, v, lo, hi, skv, scale, 0,
                                             args.splits)

            def old():
                return ext.flash_attn_fwd(q, k, v, True, scale, 0)

            diff = float((new()[0].float() - old()[0].float()).abs().max())
            for fn in (new, old):       # warm-up of both arms at this shape
                _time(fn, 20)
            t_new, t_old = [], []
            for _ in range(args.rounds):
                t_new.append(_time(new, args.iters))
                t_old.append(_time(old, args.iters))
            tn, to = statistics.median(t_new), statistics.median(t_old)
            kv_bytes = 2 * b * hkv * skv * d * 2
            print(f"B={b} S_kv={skv}: decode {tn:7.1f} us "
                  f"[{min(t_new):.1f}..{max(t_new):.1f}] "
                  f"({kv_bytes / tn / 1e6:6.2f} TB/s K/V)  "
                  f"fwd_v2 {to:7.1f} us [{min(t_old):.1f}..{max(t_old):.1f}] "
                  f"({kv_bytes / to / 1e6:6.2f} TB/s K/V)  "
                  f"speedup {to / tn:5.2f}x  max|dO| {diff:.4f}", flush=True)


if __name__ == "__main__":
    main()
