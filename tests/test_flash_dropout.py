"""Attention dropout of flash_attn_func on the CPU path, and the Megatron
model that passes it: argument contract, an independent fp32 autograd
reference built from dropout_keep_mask, the default random stream, and the
(seed, offset) draw outside the activation-checkpoint wrapper."""

import math

import pytest
import torch

from neuronx_distributed_training_amd.ops import flash_attn as fa
from neuronx_distributed_training_amd.ops.flash_attn import (
    dropout_keep_mask,
    dropout_keep_scale,
    flash_attn_func,
)

RNG = (1234, 8)


def _qkv(b, hq, hkv, sq, skv, d, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(b, hq, sq, d, generator=g, requires_grad=True)
    k = torch.randn(b, hkv, skv, d, generator=g, requires_grad=True)
    v = torch.randn(b, hkv, skv, d, generator=g, requires_grad=True)
    do = torch.randn(b, hq, sq, d, generator=g)
    return q, k, v, do


def _grads(o, do, *ts):
    return torch.autograd.grad(o, ts, do)


def _reference(q, k, v, causal, window, p, rng):
    """softmax, multiply by keep mask * keep scale, matmul: plain autograd."""
    b, hq, sq, d = q.shape
    hkv, skv = k.size(1), k.size(2)
    kx = k.repeat_interleave(hq // hkv, dim=1)
    vx = v.repeat_interleave(hq // hkv, dim=1)
    s = q @ kx.transpose(-1, -2) / math.sqrt(d)
    i = torch.arange(sq)[:, None]
    j = torch.arange(skv)[None, :]
    dead = torch.zeros(sq, skv, dtype=torch.bool)
    if causal:
        dead |= j > i + (skv - sq)
        if window:
            dead |= j <= i + (skv - sq) - window
    pr = torch.softmax(s.masked_fill(dead, float("-inf")), dim=-1)
    keep = dropout_keep_mask(b, hq, sq, skv, p, rng, "cpu")
    return (pr * keep * dropout_keep_scale(p)) @ vx


def test_keep_scale_and_threshold():
    assert fa.dropout_threshold(0.1) == 26
    assert fa.dropout_threshold(0.5) == 128
    assert fa.dropout_threshold(0.0) == 0
    assert dropout_keep_scale(0.1) == 256.0 / 230.0
    assert dropout_keep_scale(0.5) == 2.0
    keep = dropout_keep_mask(2, 3, 64, 80, 0.5, RNG, "cpu")
    assert keep.dtype == torch.bool and keep.shape == (2, 3, 64, 80)
    assert torch.equal(keep, dropout_keep_mask(2, 3, 64, 80, 0.5, RNG, "cpu"))
    assert not torch.equal(
        keep, dropout_keep_mask(2, 3, 64, 80, 0.5, (1234, 12), "cpu"))
    assert not torch.equal(
        keep, dropout_keep_mask(2, 3, 64, 80, 0.5, (1235, 8), "cpu"))
    # 6 sigma of a binomial with N = 30720
    n = keep.numel()
    assert abs(keep.float().mean().item() - 0.5) < 6 * math.sqrt(0.25 / n)


def test_dropout_zero_is_todays_path():
    q, k, v, do = _qkv(2, 4, 2, 33, 33, 16)
    o0 = flash_attn_func(q, k, v, causal=True)
    g0 = _grads(o0, do, q, k, v)
    state = torch.get_rng_state()
    o1 = flash_attn_func(q, k, v, causal=True, dropout_p=0.0)
    g1 = _grads(o1, do, q, k, v)
    assert torch.equal(o0, o1)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    # t == 0 as well, and neither call touches the generator
    o2 = flash_attn_func(q, k, v, causal=True, dropout_p=1e-4)
    assert torch.equal(o0, o2)
    assert torch.equal(state, torch.get_rng_state())


@pytest.mark.parametrize(
    "hq,hkv,sq,skv,causal,window,p",
    [
        (4, 2, 37, 37, True, 0, 0.1),     # causal with GQA
        (2, 2, 20, 45, False, 0, 0.2),    # non-causal, S_q != S_kv
        (2, 1, 40, 40, True, 9, 0.5),     # sliding window
        (2, 2, 16, 48, True, 0, 0.1),     # causal, bottom-right aligned
    ],
)
def test_matches_autograd_reference(hq, hkv, sq, skv, causal, window, p):
    q, k, v, do = _qkv(2, hq, hkv, sq, skv, 16)
    o = flash_attn_func(q, k, v, causal=causal, window=window, dropout_p=p,
                        dropout_rng=RNG)
    got = _grads(o, do, q, k, v)
    ref = _reference(q, k, v, causal, window, p, RNG)
    want = _grads(ref, do, q, k, v)
    # dropout did something
    assert not torch.allclose(o, flash_attn_func(q, k, v, causal=causal,
                                                 window=window))
    assert torch.allclose(o, ref, atol=2e-5, rtol=1e-5), \
        (o - ref).abs().max()
    for a, b, n in zip(got, want, "qkv"):
        assert torch.allclose(a, b, atol=2e-5, rtol=1e-5), \
            (n, (a - b).abs().max())


def test_default_stream():
    q, k, v, _ = _qkv(1, 2, 2, 24, 24, 16)
    torch.manual_seed(7)
    before = torch.get_rng_state()
    a = flash_attn_func(q, k, v, dropout_p=0.3)
    assert not torch.equal(before, torch.get_rng_state())   # advanced
    b = flash_attn_func(q, k, v, dropout_p=0.3)
    assert not torch.equal(a, b)                            # successive differ
    torch.manual_seed(7)
    c = flash_attn_func(q, k, v, dropout_p=0.3)
    assert torch.equal(a, c)                                # seed governs
    # the drawn pair is what dropout_rng takes
    torch.manual_seed(7)
    rng = fa.draw_dropout_rng(q.device)
    d = flash_attn_func(q, k, v, dropout_p=0.3, dropout_rng=rng)
    assert torch.equal(a, d)


def test_value_errors():
    q, k, v, _ = _qkv(2, 2, 2, 16, 16, 16)
    lo = torch.zeros(2, dtype=torch.int32)
    hi = torch.full((2,), 16, dtype=torch.int32)
    ids = torch.zeros(2, 16, dtype=torch.int32)
    with pytest.raises(ValueError):
        flash_attn_func(q, k, v, dropout_p=0.1, kv_range=(lo, hi))
    with pytest.raises(ValueError):
        flash_attn_func(q, k, v, dropout_p=0.1, segment_ids=ids)
    with pytest.raises(ValueError):
        flash_attn_func(q, k, v, dropout_p=0.1,
                        seg_bounds=fa.segment_bounds(ids))
    with pytest.raises(ValueError):
        flash_attn_func(q, k, v, dropout_p=1.0)
    with pytest.raises(ValueError):
        flash_attn_func(q, k, v, dropout_p=1.5)
    with pytest.raises(ValueError):
        flash_attn_func(q, k, v, dropout_p=0.999)   # t would be 256
    with pytest.raises(ValueError):
        flash_attn_func(q, k, v, dropout_p=-0.1)
    # the same masks without dropout stay legal
    flash_attn_func(q, k, v, dropout_p=0.0, kv_range=(lo, hi))
    flash_attn_func(q, k, v, dropout_p=0.0, segment_ids=ids)


# ------------------------------ Megatron ------------------------------

def _gpt(attention_dropout, activation_checkpoint=None):
    from neuronx_distributed_training_amd.models.megatron_gpt import (
        GPTConfig, GPTModel,
    )
    from neuronx_distributed_training_amd.parallel import state as ps

    ps.destroy_model_parallel()
    torch.manual_seed(0)
    cfg = GPTConfig(
        vocab_size=64, hidden_size=32, ffn_hidden_size=64, num_layers=2,
        num_attention_heads=4, max_position_embeddings=32,
        hidden_dropout=0.0, attention_dropout=attention_dropout,
        activation_checkpoint=activation_checkpoint,
    )
    return GPTModel(cfg)


def _ids():
    return torch.randint(0, 64, (2, 16),
                         generator=torch.Generator().manual_seed(1))


def test_megatron_train_mode_applies_dropout():
    """Fails without the feature: attention_dropout was parsed and dropped."""
    model = _gpt(0.1)
    ids = _ids()
    model.eval()
    with torch.no_grad():
        ev = model(ids)
    model.train()
    with torch.no_grad():
        tr = model(ids)
    assert not torch.allclose(tr, ev)


def test_megatron_eval_mode_has_no_dropout():
    ids = _ids()
    with_p = _gpt(0.1).eval()
    without = _gpt(0.0).eval()
    without.load_state_dict(with_p.state_dict())
    with torch.no_grad():
        assert torch.equal(with_p(ids), without(ids))


def test_megatron_draws_under_the_tracker_fork():
    from neuronx_distributed_training_amd.parallel.random import (
        get_rng_tracker, model_parallel_manual_seed,
    )

    model = _gpt(0.1).train()
    ids = _ids()
    try:
        model_parallel_manual_seed(11)
        before = torch.get_rng_state()
        with torch.no_grad():
            a = model(ids)
        assert torch.equal(before, torch.get_rng_state())
        with torch.no_grad():
            b = model(ids)
        assert not torch.equal(a, b)         # the tracked state advanced
        model_parallel_manual_seed(11)
        with torch.no_grad():
            assert torch.equal(a, model(ids))
    finally:
        get_rng_tracker().reset()


@pytest.mark.parametrize("ckpt", ["selective", "full"])
def test_megatron_checkpoint_regenerates_the_mask(ckpt):
    from neuronx_distributed_training_amd.parallel.random import (
        get_rng_tracker, model_parallel_manual_seed,
    )

    ids = _ids()
    out = []
    try:
        for mode in (None, ckpt):
            model = _gpt(0.1, mode).train()
            model_parallel_manual_seed(5)
            loss = model(ids, labels=ids.clone())
            loss.backward()
            out.append((loss.detach(),
                        {n: p.grad for n, p in model.named_parameters()}))
    finally:
        get_rng_tracker().reset()
    (l0, g0), (l1, g1) = out
    assert torch.equal(l0, l1)
    assert g0.keys() == g1.keys()
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


def test_megatron_context_parallel_with_dropout_raises(monkeypatch):
    from neuronx_distributed_training_amd.parallel import state as ps

    _gpt(0.1)   # fine without CP
    monkeypatch.setattr(ps, "get_context_model_parallel_world_size",
                        lambda: 2)
    with pytest.raises(ValueError, match="attention_dropout"):
        _gpt(0.1)
