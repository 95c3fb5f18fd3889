"""Dense fp32 reference for attention with a per-batch-row key range, shared
by tests/test_flash_kv_range.py (CPU) and tests/test_gpu_flash_kv_range.py.

Built from an explicit boolean mask and plain autograd, independent of the
op's own reference path. Pair (query i, key j) of batch row b is alive iff
lo[b] <= j < hi[b], and (causal) j <= i + coff, and (causal, window > 0)
j > i + coff - window, with coff = S_kv - S_q. Query rows with no alive key
are replaced by zeros (output and every gradient they would contribute)."""

import torch


def alive_mask(b, sq, skv, lo, hi, causal, window, device):
    """[b, 1, sq, skv] bool, True = alive."""
    lo = torch.as_tensor(lo, device=device).long()
    hi = torch.as_tensor(hi, device=device).long()
    i = torch.arange(sq, device=device)[:, None]
    j = torch.arange(skv, device=device)[None, :]
    coff = skv - sq
    alive = torch.ones(sq, skv, dtype=torch.bool, device=device)
    if causal:
        alive &= j <= i + coff
        if window and window > 0:
            alive &= j > i + coff - window
    rng = (j[None] >= lo[:, None, None]) & (j[None] < hi[:, None, None])
    return (alive[None] & rng)[:, None]


def dense_attention(q, k, v, lo, hi, causal=True, scale=None, window=0,
                    dout=None):
    """fp32 forward (and backward when `dout` is given) on q's device.
    Returns (o, dq, dk, dv, alive); the grads are None without `dout`."""
    b, hq, sq, d = q.shape
    hkv, skv = k.size(1), k.size(2)
    g = hq // hkv
    if scale is None:
        scale = d ** -0.5
    qr = q.detach().float().clone().requires_grad_(True)
    kr = k.detach().float().clone().requires_grad_(True)
    vr = v.detach().float().clone().requires_grad_(True)
    kx = kr.repeat_interleave(g, 1)
    vx = vr.repeat_interleave(g, 1)
    alive = alive_mask(b, sq, skv, lo, hi, causal, window, q.device)
    empty = ~alive.any(-1, keepdim=True)
    s = torch.matmul(qr, kx.transpose(-1, -2)) * scale
    s = s.masked_fill(~alive, float("-inf"))
    s = torch.where(empty, torch.zeros_like(s), s)   # no all -inf row
    p = torch.softmax(s, dim=-1).masked_fill(empty, 0.0)
    o = torch.matmul(p, vx)
    if dout is None:
        return o.detach(), None, None, None, alive
    o.backward(dout.float())
    return o.detach(), qr.grad, kr.grad, vr.grad, alive


def llama_fp32_logits(params, cfg, ids, attention_mask):
    """Plain-PyTorch fp32 forward of LlamaForCausalLM at TP=1 (separate
    q_proj / kv_proj, i.e. GQA configs) on the device of `params`, with the
    padding mask applied key-side as an explicit boolean mask. `params`
    maps parameter names to fp32 tensors (autograd leaves if gradients are
    wanted). Returns logits [b, s, vocab]."""
    import torch.nn.functional as F
    from neuronx_distributed_training_amd.ops.rope import build_rope_cache

    b, s = ids.shape
    dev = ids.device
    hq, hkv, d = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
    cos, sin = build_rope_cache(s, d, cfg.rope_theta, device=dev)

    def norm(x, w):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True)
                               + cfg.rms_norm_eps) * w

    def rope(x):
        x1, x2 = x.chunk(2, dim=-1)
        return x * cos[:s] + torch.cat((-x2, x1), dim=-1) * sin[:s]

    m = attention_mask != 0
    j = torch.arange(s, device=dev)
    alive = (j[None, :] <= j[:, None])[None, None] & m[:, None, None, :]
    empty = ~alive.any(-1, keepdim=True)
    x = params["model.embed_tokens.weight"][ids]            # [b, s, h]
    for li in range(cfg.num_hidden_layers):
        pre = f"model.layers.{li}."
        h = norm(x, params[pre + "input_layernorm.weight"])
        q = F.linear(h, params[pre + "self_attn.q_proj.weight"])
        k, v = F.linear(h, params[pre + "self_attn.kv_proj.weight"]).chunk(
            2, dim=-1)
        q = rope(q.view(b, s, hq, d).transpose(1, 2))
        k = rope(k.view(b, s, hkv, d).transpose(1, 2))
        v = v.view(b, s, hkv, d).transpose(1, 2)
        k = k.repeat_interleave(hq // hkv, 1)
        v = v.repeat_interleave(hq // hkv, 1)
        sc = torch.matmul(q, k.transpose(-1, -2)) * d ** -0.5
        sc = sc.masked_fill(~alive, float("-inf"))
        sc = torch.where(empty, torch.zeros_like(sc), sc)
        p = torch.softmax(sc, dim=-1).masked_fill(empty, 0.0)
        o = torch.matmul(p, v).transpose(1, 2).reshape(b, s, hq * d)
        x = x + F.linear(o, params[pre + "self_attn.o_proj.weight"])
        h = norm(x, params[pre + "post_attention_layernorm.weight"])
        gate, up = F.linear(
            h, params[pre + "mlp.gate_up_proj.weight"]).chunk(2, dim=-1)
        x = x + F.linear(F.silu(gate) * up,
                         params[pre + "mlp.down_proj.weight"])
    x = norm(x, params["model.norm.weight"])
    return F.linear(x, params["lm_head.weight"])


def masked_lm_loss(logits, ids, loss_mask):
    """Next-token CE averaged over loss_mask[:, 1:] (LlamaForCausalLM's
    loss with labels = ids)."""
    import torch.nn.functional as F

    per_tok = F.cross_entropy(
        logits[:, :-1].reshape(-1, logits.size(-1)).float(),
        ids[:, 1:].reshape(-1), reduction="none").view(ids.size(0), -1)
    m = loss_mask[:, 1:].to(per_tok.dtype)
    return (per_tok * m).sum() / m.sum().clamp(min=1)
