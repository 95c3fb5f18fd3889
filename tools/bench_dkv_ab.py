"""A/B of the two dK/dV backward kernels at the flagship attention shape.

    python tools/bench_dkv_ab.py [--rounds 5] [--window 0.5]

Shape: B 2, HQ 32, HKV 8, S 8192, D 128, causal, the fused-QKV strides of
models/llama.py, random data. First asserts that dQ / dK / dV of the default
(pipelined) binding and of its ``_sbuf`` twin are bit-equal at this shape,
then times the whole backward call of each arm: arms alternate over
``--rounds`` rounds, each timed window runs enough calls to last at least
``--window`` seconds and has a device sync on both sides. Prints the per-call
time of every window and median / min / max per arm, then one JSON line.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from neuronx_distributed_training_amd import ops  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5,
                    help="minimum seconds per timed window")
    ap.add_argument("--seq", type=int, default=8192)
    args = ap.parse_args()
    assert args.rounds >= 5, "at least five rounds"

    ext = ops.require_extension()
    torch.manual_seed(0)
    b, hq, hkv, s, d = 2, 32, 8, args.seq, 128
    scale = d ** -0.5
    nq, nkv = hq * d, hkv * d
    qkv = torch.randn(s, b, nq + 2 * nkv, device="cuda", dtype=torch.bfloat16)
    qs, ks, vs = qkv.split([nq, nkv, nkv], dim=-1)
    q = qs.view(s, b, hq, d).permute(1, 2, 0, 3)
    k = ks.view(s, b, hkv, d).permute(1, 2, 0, 3)
    v = vs.view(s, b, hkv, d).permute(1, 2, 0, 3)
    do = torch.randn(s, b, hq, d, device="cuda",
                     dtype=torch.bfloat16).permute(1, 2, 0, 3)
    o, lse = ext.flash_attn_fwd(q, k, v, True, scale)
    call = {
        "pipe": lambda: ext.flash_attn_bwd(do, q, k, v, o, lse, True, scale),
        "sbuf": lambda: ext.flash_attn_bwd_sbuf(do, q, k, v, o, lse, True,
                                                scale),
    }

    got, want = call["pipe"](), call["sbuf"]()
    for name, a, w in zip(("dq", "dk", "dv"), got, want):
        assert torch.isfinite(w.float()).all(), name
        assert torch.equal(a, w), f"{name}: pipe and sbuf differ"
    del got, want
    print(f"bit-equal at B{b} HQ{hq} HKV{hkv} S{s} D{d} causal")

    def window(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    for fn in call.values():  # warm-up
        window(fn, 3)
    # calls per window from the slower of the two arms' first estimate
    per = min(window(fn, 5) for fn in call.values())
    n = max(5, int(args.window / per) + 1)

    samples = {"pipe": [], "sbuf": []}
    for r in range(args.rounds):
        for arm in (("sbuf", "pipe") if r % 2 == 0 else ("pipe", "sbuf")):
            ms = window(call[arm], n) * 1e3
            samples[arm].append(ms)
            print(f"round {r} {arm}: {ms:.3f} ms/call ({n} calls)")
    out = {"shape": [b, hq, hkv, s, d], "calls_per_window": n}
    for arm, xs in samples.items():
        out[arm] = {"median_ms": statistics.median(xs), "min_ms": min(xs),
                    "max_ms": max(xs), "samples_ms": xs}
        print(f"{arm}: median {out[arm]['median_ms']:.3f}  "
              f"min {out[arm]['min_ms']:.3f}  max {out[arm]['max_ms']:.3f} ms")
    out["separated"] = max(samples["pipe"]) < min(samples["sbuf"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
