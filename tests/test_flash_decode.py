"""CPU: the fp32 reference path of ops.flash_attn_decode against
flash_attn_func on the row's own slice, and generate(cache_impl="static") on
a left-padded batch against each row generated alone without padding."""

import pytest
import torch

from neuronx_distributed_training_amd.ops import (
    flash_attn_decode, flash_attn_func,
)


@pytest.mark.parametrize("sq,hq,hkv,window", [(1, 4, 2, 0), (3, 4, 4, 0),
                                              (3, 8, 2, 7)])
def test_cpu_path_equals_flash_attn_func_on_the_slice(sq, hq, hkv, window):
    torch.manual_seed(sq + hq)
    ranges = [(0, 5), (3, 40), (11, 29), (6, 6)]   # last row: empty
    b, cap, d = len(ranges), 40, 16
    q = torch.randn(b, hq, sq, d)
    k = torch.full((b, hkv, cap, d), float("nan"))
    v = torch.full((b, hkv, cap, d), float("nan"))
    for r, (lo, hi) in enumerate(ranges):
        k[r, :, lo:hi] = torch.randn(hkv, hi - lo, d)
        v[r, :, lo:hi] = torch.randn(hkv, hi - lo, d)
    lo_t = torch.tensor([r[0] for r in ranges])
    hi_t = torch.tensor([r[1] for r in ranges])
    o, lse = flash_attn_decode(q, k, v, hi_t, lo_t, window=window,
                               return_lse=True)
    assert o.shape == q.shape and lse.shape == (b, hq, sq)
    assert torch.isfinite(o).all()
    for r, (lo, hi) in enumerate(ranges):
        if lo == hi:
            assert (o[r] == 0).all() and (lse[r] == -1e30).all()
            continue
        ref = flash_attn_func(q[r:r + 1], k[r:r + 1, :, lo:hi],
                              v[r:r + 1, :, lo:hi], causal=True,
                              window=window)
        assert torch.allclose(o[r:r + 1], ref, atol=1e-6, rtol=1e-5), r


def test_forward_only_and_argument_errors():
    q = torch.randn(1, 2, 1, 8, requires_grad=True)
    kv = torch.randn(1, 2, 4, 8)
    hi = torch.tensor([4])
    with pytest.raises(RuntimeError, match="forward only"):
        flash_attn_decode(q, kv, kv, hi)
    with torch.no_grad():
        flash_attn_decode(q, kv, kv, hi)
        with pytest.raises(ValueError, match="max_kv"):
            flash_attn_decode(q, kv, kv, hi, max_kv=5)


def test_static_cache_generate_left_padded_matches_rows_alone():
    from neuronx_distributed_training_amd.parallel import state as ps
    from neuronx_distributed_training_amd.models.llama import (
        LlamaConfig, LlamaForCausalLM, StaticKVCache,
    )
    from neuronx_distributed_training_amd.utils.generation import generate

    ps.destroy_model_parallel()
    torch.manual_seed(0)
    model = LlamaForCausalLM(
        LlamaConfig(vocab_size=64, hidden_size=32, intermediate_size=64,
                    num_hidden_layers=2, num_attention_heads=4,
                    num_key_value_heads=2, max_position_embeddings=64)
    ).eval()
    lens, s, new = [5, 8, 3], 8, 4
    rows = [torch.randint(1, 64, (1, n)) for n in lens]
    ids = torch.zeros(len(lens), s, dtype=torch.long)
    mask = torch.zeros(len(lens), s, dtype=torch.long)
    for r, row in enumerate(rows):
        ids[r, s - lens[r]:] = row[0]
        mask[r, s - lens[r]:] = 1
    alone = [generate(model, row, max_new_tokens=new) for row in rows]

    fed = []
    hook = model.register_forward_pre_hook(
        lambda mod, args: fed.append(tuple(args[0].shape)))
    out = generate(model, ids, max_new_tokens=new, attention_mask=mask,
                   cache_impl="static")
    hook.remove()
    # the cache was kept: one prefill, then one token per step
    assert fed == [(3, s)] + [(3, 1)] * (new - 1)
    for r, n in enumerate(lens):
        assert torch.equal(out[r, s:], alone[r][0, n:]), r

    # logits of the prefill and of every decode step (teacher-forced with
    # the tokens above) against the row's own unpadded full forward
    with torch.no_grad():
        cache = StaticKVCache(2, len(lens), s + new)
        got = [model(ids, kv_cache=cache, attention_mask=mask)[:, -1]]
        for t in range(new - 1):
            got.append(model(out[:, s + t:s + t + 1], kv_cache=cache)[:, -1])
        for r, n in enumerate(lens):
            full = model(alone[r][:, :-1])[0]
            for t, g in enumerate(got):
                assert torch.allclose(g[r], full[n - 1 + t], atol=1e-5), (r, t)
        with pytest.raises(ValueError, match="capacity"):
            model(out[:, -2:], kv_cache=cache)
    assert cache.seq_len == s + new - 1
