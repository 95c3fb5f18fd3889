"""Decode (serving) throughput: Llama-3 8B incremental KV-cache decode
on one MI355X — tokens/s at batch 1 and 8.

    python tools/bench_decode.py [--layers 32] [--prompt 512] [--new 64]
                                 [--cache {dynamic,static}] [--ragged]

--cache static decodes from a preallocated StaticKVCache through the
split-KV flash-decode kernel. --ragged measures one batch of 8 prompts of
unequal length (prompt/8 .. prompt tokens), left-padded with an attention
mask: the dynamic arm then recomputes the whole sequence every step, the
static arm keeps its cache.
"""

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--cache", choices=("dynamic", "static"),
                    default="dynamic")
    ap.add_argument("--ragged", action="store_true")
    args = ap.parse_args()

    from neuronx_distributed_training_amd.parallel import state as ps
    from neuronx_distributed_training_amd.models.llama import (
        LlamaConfig, LlamaForCausalLM,
    )
    from neuronx_distributed_training_amd.utils.generation import generate

    ps.initialize_model_parallel()
    torch.manual_seed(0)
    cfg = LlamaConfig(
        vocab_size=128256, hidden_size=4096, intermediate_size=14336,
        num_hidden_layers=args.layers, num_attention_heads=32,
        num_key_value_heads=8, max_position_embeddings=args.prompt + args.new,
        rope_theta=500000.0, dtype="bfloat16",
    )
    model = LlamaForCausalLM(cfg).to("cuda:0").eval()
    kw = {} if args.cache == "dynamic" else {"cache_impl": args.cache}
    tag = "" if args.cache == "dynamic" else f" [{args.cache} cache]"
    for bs in ((8,) if args.ragged else (1, 8)):
        prompt = torch.randint(0, cfg.vocab_size, (bs, args.prompt),
                               device="cuda:0")
        if args.ragged:
            lens = torch.linspace(args.prompt // 8, args.prompt, bs,
                                  device="cuda:0").long()
            pos = torch.arange(args.prompt, device="cuda:0")
            mask = (pos[None] >= args.prompt - lens[:, None]).long()
            kw["attention_mask"] = mask
            prompt = prompt * mask
            tag = f" [{args.cache} cache, ragged]"
        generate(model, prompt, max_new_tokens=4, use_cache=True, **kw)  # warmup
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = generate(model, prompt, max_new_tokens=args.new, use_cache=True,
                       **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert out.shape == (bs, args.prompt + args.new)
        toks = bs * args.new
        print(f"bs={bs}: {toks / dt:8.1f} decode tokens/s  "
              f"({dt / args.new * 1000:.2f} ms/step, prompt {args.prompt})"
              f"{tag}", flush=True)


if __name__ == "__main__":
    main()
