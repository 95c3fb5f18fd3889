"""NXDT_MOE_FUSED off the GPU: the switch changes nothing where the fused
token path does not apply, and rejects values other than 0 and 1."""

import pytest
import torch

from neuronx_distributed_training_amd.modules.moe import (
    ExpertMLPs, MoE, RouterTopK)
from neuronx_distributed_training_amd.ops import moe_dispatch


def _layer(capacity):
    return MoE(RouterTopK(16, 4, 2, init_seed=11),
               ExpertMLPs(4, 16, 32, init_seed=12), capacity_factor=capacity)


def _run(moe, x):
    moe.zero_grad(set_to_none=True)
    xd = x.clone().requires_grad_(True)
    y, logits = moe(xd)
    (y.sum() + logits.sum()).backward()
    return [y.detach(), xd.grad] + [p.grad for p in moe.parameters()]


@pytest.mark.parametrize("capacity", [None, 1.0], ids=["dropless", "cap1"])
def test_cpu_layer_is_bit_equal_with_the_switch_on(monkeypatch, capacity):
    def never(*a, **kw):
        raise AssertionError("fused path taken on the CPU")

    monkeypatch.setattr(moe_dispatch, "fused_moe_experts", never)
    moe = _layer(capacity)
    x = torch.randn(24, 16, generator=torch.Generator().manual_seed(3))
    monkeypatch.delenv("NXDT_MOE_FUSED", raising=False)
    want = _run(moe, x)
    for value in ("1", "0", ""):
        monkeypatch.setenv("NXDT_MOE_FUSED", value)
        for a, b in zip(_run(moe, x), want):
            assert torch.equal(a, b), value


def test_expert_parallel_layer_keeps_the_eager_path(monkeypatch):
    """With every other condition granted (the grouped kernel would be
    chosen), EP = 2 alone keeps the layer off the fused path; its eager
    branch needs a process group, so the choice itself is what is checked."""
    monkeypatch.setattr(ExpertMLPs, "grouped_chosen", lambda *a: True)
    monkeypatch.setenv("NXDT_MOE_FUSED", "1")
    moe = _layer(None)
    x = torch.zeros(8, 16)
    assert moe._fused_path(x, 2, 4) and moe._fused_path(x, 8, 64)
    assert not moe._fused_path(x, 9, 4) and not moe._fused_path(x, 2, 65)
    monkeypatch.setattr(moe, "ep", 2)
    assert not moe._fused_path(x, 2, 4)


def test_switch_rejects_other_values(monkeypatch):
    monkeypatch.setenv("NXDT_MOE_FUSED", "2")
    with pytest.raises(ValueError, match="NXDT_MOE_FUSED"):
        _layer(None)(torch.zeros(8, 16))
