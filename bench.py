"""Flagship benchmark: Llama-3 8B training step, tokens/sec whole-job.

Driver contract (BASELINE.json): tokens/sec (whole node), Llama-3-8B,
TP=N, ZeRO-1, bf16, synthetic data, random-init weights. Strong scaling:
the global batch is fixed as N grows (TP shards the model across the xGMI
clique).

    python bench.py --gpus N --steps K --warmup W
    (N>1 launched by the driver via torch.distributed.run, one rank/GPU)

A plain run sets up, warms up, times the K steps and prints one JSON line.
``--dump-outputs DIR`` additionally writes what the last timed step
returned (loss, grad norm, a seeded sample of the updated weights) as
``DIR/<name>.npy``. ``--full`` is reserved for
measurements beyond the headline figure; there are none today.
"""

from __future__ import annotations

import argparse
import json
import os
import shutil
import tempfile
import time

# hipBLASLt/rocBLAS algorithm selections pre-tuned on MI355X (TunableOp):
# must be configured BEFORE torch import. Each rank copies the canonical
# CSV to its device-ordinal filename.
_REPO = os.path.dirname(os.path.abspath(__file__))
_TUNE = os.path.join(_REPO, "tunableop", "tunableop_gfx950.csv")
if os.path.exists(_TUNE) and os.environ.get("NXDT_DISABLE_TUNABLEOP") != "1":
    _lr = os.environ.get("LOCAL_RANK", "0")
    _td = tempfile.mkdtemp(prefix="tunableop_")
    shutil.copy(_TUNE, os.path.join(_td, f"tunableop_gfx950{_lr}.csv"))
    os.environ.setdefault("PYTORCH_TUNABLEOP_ENABLED", "1")
    os.environ.setdefault("PYTORCH_TUNABLEOP_TUNING", "0")
    os.environ.setdefault(
        "PYTORCH_TUNABLEOP_FILENAME", os.path.join(_td, "tunableop_gfx950.csv")
    )

os.environ.setdefault("PYTORCH_ALLOC_CONF", "expandable_segments:True")

import torch
import torch.distributed as dist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gbs", type=int, default=None, help="global batch (sequences)")
    ap.add_argument("--mbs", type=int, default=2, help="micro batch size")
    ap.add_argument("--seq", type=int, default=8192)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument(
        "--hipgraph", type=int, default=0,
        help="capture the microbatch fwd+bwd into a hipGraph (single-GPU "
        "steady state; measured ~3%% slower than eager on MI355X r01 — "
        "launch gaps are already hidden — so default off)",
    )
    ap.add_argument(
        "--dump-outputs", metavar="DIR", default=None,
        help="after the timed steps, write the last step's outputs "
        "(loss, grad norm, a seeded sample of the weights) to DIR/*.npy",
    )
    ap.add_argument(
        "--full", action="store_true",
        help="also run the measurements beyond the headline figure "
        "(none today: the plain run is the whole benchmark)",
    )
    args = ap.parse_args()
    assert args.steps >= 1, "--steps must be at least 1"

    n = args.gpus
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    use_gpu = torch.cuda.is_available()
    if world > 1:
        assert world == n, f"WORLD_SIZE {world} != --gpus {n}"
        if use_gpu:
            torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl" if use_gpu else "gloo")

    from neuronx_distributed_training_amd.parallel import state as ps
    from neuronx_distributed_training_amd.trainer.module import LlamaModule

    tp = world if world > 1 else 1
    ps.initialize_model_parallel(tensor_model_parallel_size=tp)
    torch.manual_seed(1234)

    gbs = args.gbs if args.gbs is not None else 4
    mbs = args.mbs
    seq = args.seq
    cfg = {
        "data": {"global_batch_size": gbs, "micro_batch_size": mbs, "seq_length": seq},
        "distributed_strategy": {
            "tensor_model_parallel_size": tp,
            "sequence_parallel": tp > 1,
            "zero1": True,
        },
        "model": {
            "vocab_size": 128256,
            "hidden_size": 4096,
            "intermediate_size": 14336,
            "num_layers": args.layers,
            "num_attention_heads": 32,
            "num_kv_heads": 8,
            "rope_theta": 500000.0,
            "grad_clip": 1.0,
            "optim": {"lr": 3.0e-4, "sched": {"warmup_steps": 10}},
        },
        "precision": {"type": "mixed_precision"},
        "exp_manager": {"log_gradient_norm": False, "log_parameter_norm": False},
    }

    module = LlamaModule(cfg)
    if use_gpu:
        # random-init the 8B weights on the device: filling them on the
        # host and copying them over took ~30 s of every run. Each weight
        # is still seeded individually, so runs stay identical.
        with torch.device("cuda"):
            module.setup()
        torch.cuda.empty_cache()
    else:
        module.setup()
    module.configure_optimizers(max_steps=args.steps + args.warmup)

    vocab = cfg["model"]["vocab_size"]
    n_micro = module.num_microbatches

    def make_micro():
        ids = torch.randint(0, vocab, (mbs, seq))
        return {"input_ids": ids, "labels": ids.clone()}

    micros = [make_micro() for _ in range(n_micro)]

    # hipGraph capture of the steady-state microbatch fwd+bwd (the XLA
    # graph-compile analog the MI355X way — BASELINE north star). Works at
    # world=1 (no collectives inside the captured region); the optimizer
    # step stays eager (ZeRO collectives at N>1).
    graphed = None
    if args.hipgraph and use_gpu and world == 1:
        try:
            static_ids = micros[0]["input_ids"].to("cuda")
            static_lab = micros[0]["labels"].to("cuda")
            # warmup on a side stream, then materialize stable .grad tensors
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(2):
                    module.optimizer.zero_grad(set_to_none=False)
                    loss = module.model(static_ids, labels=static_lab)
                    (loss / n_micro).backward()
            torch.cuda.current_stream().wait_stream(s)
            module.optimizer.zero_grad(set_to_none=False)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                static_loss = module.model(static_ids, labels=static_lab)
                (static_loss / n_micro).backward()
            graphed = (g, static_ids, static_lab, static_loss)
            if rank == 0:
                print("# hipGraph capture OK", flush=True)
        except Exception as e:  # pragma: no cover
            graphed = None
            if rank == 0:
                print(f"# hipGraph capture failed ({e}); eager path", flush=True)

    def one_step():
        if graphed is not None:
            g, sid, slab, sloss = graphed
            module.optimizer.zero_grad(set_to_none=False)
            for mb in micros:
                sid.copy_(mb["input_ids"], non_blocking=True)
                slab.copy_(mb["labels"], non_blocking=True)
                g.replay()
            gnorm = module.optimizer.step()
            module.scheduler.step()
            return sloss, gnorm
        module.optimizer.zero_grad()
        loss = module.forward_backward_step(iter(micros))
        gnorm = module.optimizer.step()
        module.scheduler.step()
        return loss, gnorm

    last = None
    for _ in range(args.warmup):
        one_step()

    if world > 1:
        dist.barrier()
    if use_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = one_step()
    if use_gpu:
        torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t1 = time.perf_counter()

    elapsed = torch.tensor([t1 - t0], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)
    ms_per_step = float(elapsed[0]) / args.steps * 1000.0
    tokens_per_step = gbs * seq
    tok_s = tokens_per_step / (ms_per_step / 1000.0)

    if rank == 0:
        print(
            json.dumps(
                {
                    "metric": "tokens_per_sec",
                    "value": tok_s,
                    "unit": "tokens/s",
                    "n_gpus": n,
                    "steps": args.steps,
                    "warmup": args.warmup,
                    "ms_per_step": ms_per_step,
                    "higher_is_better": True,
                    "scaling": "strong",
                    "vs_baseline": None,
                    "dtype": "bf16" if use_gpu else "float32",
                    "data": "synthetic",
                    "config": {
                        "model": "llama3-8B",
                        "global_batch": gbs,
                        "seq_len": seq,
                        "parallelism": f"tp{tp}_zero1" + ("_sp" if tp > 1 else ""),
                    },
                }
            ),
            flush=True,
        )
    if args.dump_outputs and rank == 0:
        _dump_outputs(args.dump_outputs, module, *last)
    if world > 1:
        dist.destroy_process_group()


_SAMPLE_PER_TENSOR = 8192


def _dump_outputs(out_dir, module, loss, gnorm):
    """Write what the last timed step handed back: its loss, its global
    grad norm, and the weights it left behind. The weights are a fixed,
    seeded sample (<= 8192 elements per parameter, in named_parameters
    order; rank 0's shard at TP>1), ~6 MB for the 8B model."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "loss.npy"),
            loss.detach().double().cpu().numpy())
    np.save(os.path.join(out_dir, "grad_norm.npy"),
            gnorm.detach().double().cpu().numpy())
    gen = torch.Generator().manual_seed(20240531)
    parts = []
    for _, p in module.model.named_parameters():
        flat = p.detach().reshape(-1)
        if flat.numel() > _SAMPLE_PER_TENSOR:
            idx = torch.randint(0, flat.numel(), (_SAMPLE_PER_TENSOR,), generator=gen)
            flat = flat[idx.to(flat.device)]
        parts.append(flat.float().cpu())
    np.save(os.path.join(out_dir, "weights_sample.npy"), torch.cat(parts).numpy())


if __name__ == "__main__":
    main()
