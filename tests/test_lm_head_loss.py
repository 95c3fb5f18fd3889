"""parallel_linear_cross_entropy and model.fused_lm_head_loss off the GPU:
today's lm_head + parallel_cross_entropy path, bit for bit."""

import os

import pytest
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# bf16 on the CPU, and fp32 with an H (40) and a V (12) no kernel would take
@pytest.mark.parametrize("dtype,H,V", [(torch.bfloat16, 64, 24),
                                       (torch.float32, 40, 12)])
def test_cpu_and_ineligible_inputs_take_the_unfused_path(dtype, H, V):
    from neuronx_distributed_training_amd.ops import linear_cross_entropy
    from neuronx_distributed_training_amd.parallel.loss import (
        parallel_cross_entropy, parallel_linear_cross_entropy,
    )

    g = torch.Generator().manual_seed(0)
    target = torch.randint(0, V, (2, 5), generator=g)
    gout = torch.randn(2, 5, generator=g)
    runs = []
    for fn in (parallel_linear_cross_entropy,
               lambda h, w, t: parallel_cross_entropy(F.linear(h, w), t)):
        g.manual_seed(1)
        h = torch.randn(2, 5, H, generator=g).to(dtype).requires_grad_(True)
        w = torch.randn(V, H, generator=g).to(dtype).requires_grad_(True)
        loss = fn(h, w, target)
        loss.backward(gout)
        runs.append((loss.detach(), h.grad, w.grad))
    assert runs[0][0].shape == target.shape
    for got, want in zip(*runs):
        assert torch.equal(got, want)
    with pytest.raises(ValueError):  # the kernel-only op has no fallback
        linear_cross_entropy(h.detach().view(-1, H), w.detach(),
                             target.view(-1))


def test_config_key_parses_and_cpu_model_is_unchanged():
    from neuronx_distributed_training_amd.models.llama import LlamaConfig
    from neuronx_distributed_training_amd.parallel import state as ps
    from neuronx_distributed_training_amd.trainer.module import LlamaModule
    from neuronx_distributed_training_amd.utils.config import (
        load_config, validate_config,
    )

    assert LlamaConfig().fused_lm_head_loss is False
    with pytest.raises(ValueError, match="fused_lm_head_loss"):
        validate_config({"model": {"fused_lm_head_loss": "false"}})
    small = ["hidden_size=64", "intermediate_size=128", "num_layers=2",
             "num_attention_heads=4", "num_kv_heads=2", "vocab_size=128"]
    overrides = ["model." + s for s in small] + [
        "data.seq_length=32", "data.global_batch_size=2",
        "data.micro_batch_size=2", "precision.type=fp32",
        "distributed_strategy.tensor_model_parallel_size=1",
        "distributed_strategy.sequence_parallel=false"]
    recipe = os.path.join(REPO, "examples", "conf", "hf_llama3_8B_config.yaml")
    ids = torch.arange(64).view(2, 32) * 7 % 128
    runs = []
    for extra in ([], ["model.fused_lm_head_loss=true"]):
        ps.destroy_model_parallel()
        mod = LlamaModule(load_config(recipe, overrides + extra))
        mod.setup()
        assert mod.model.cfg.fused_lm_head_loss is bool(extra)
        loss = mod.model(ids, labels=ids, loss_mask=(ids % 3 != 0).float())
        loss.backward()
        runs.append([loss.detach()] + [p.grad for p in mod.model.parameters()])
    for got, want in zip(*runs, strict=True):
        assert torch.equal(got, want)
