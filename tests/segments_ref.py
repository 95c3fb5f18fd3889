"""Dense fp32 reference for packed-sequence (segmented) causal attention,
shared by tests/test_flash_segments.py (CPU) and
tests/test_gpu_flash_segments.py.

Built from an explicit block-diagonal boolean mask and plain autograd,
independent of the op's own reference path and of segment_bounds. Pair
(query i, key j) of batch row b is alive iff seg[b, i] == seg[b, j],
j <= i, and (window > 0) j > i - window. Every query sees itself, so no row
is empty."""

import torch


def ids_from_lengths(layouts, s, device="cpu"):
    """[[len, len, ...], ...] (each summing to s) -> int64 [B, s] ids."""
    rows = []
    for lens in layouts:
        assert sum(lens) == s, (lens, s)
        rows.append(torch.repeat_interleave(
            torch.arange(len(lens)), torch.tensor(lens)))
    return torch.stack(rows).to(device)


def segment_alive(seg, window=0):
    """[b, 1, s, s] bool, True = alive."""
    s = seg.size(1)
    i = torch.arange(s, device=seg.device)[:, None]
    j = torch.arange(s, device=seg.device)[None, :]
    alive = j <= i
    if window and window > 0:
        alive = alive & (j > i - window)
    same = seg[:, :, None] == seg[:, None, :]
    return (alive[None] & same)[:, None]


def dense_attention_seg(q, k, v, seg, scale=None, window=0, dout=None):
    """fp32 forward (and backward when `dout` is given) on q's device.
    Returns (o, dq, dk, dv); the grads are None without `dout`."""
    hq, d = q.size(1), q.size(3)
    g = hq // k.size(1)
    if scale is None:
        scale = d ** -0.5
    qr = q.detach().float().clone().requires_grad_(True)
    kr = k.detach().float().clone().requires_grad_(True)
    vr = v.detach().float().clone().requires_grad_(True)
    kx = kr.repeat_interleave(g, 1)
    vx = vr.repeat_interleave(g, 1)
    alive = segment_alive(seg, window)
    s = torch.matmul(qr, kx.transpose(-1, -2)) * scale
    s = s.masked_fill(~alive, float("-inf"))
    o = torch.matmul(torch.softmax(s, dim=-1), vx)
    if dout is None:
        return o.detach(), None, None, None
    o.backward(dout.float())
    return o.detach(), qr.grad, kr.grad, vr.grad


def llama_fp32_logits_seg(params, cfg, ids, seg):
    """Plain-PyTorch fp32 forward of LlamaForCausalLM at TP=1 (separate
    q_proj / kv_proj, i.e. GQA configs) on the device of `params`, with the
    block-diagonal causal mask of `seg` [b, s] as an explicit boolean mask.
    RoPE positions run over the whole row (not reset per segment), like the
    model's. `params` maps parameter names to fp32 tensors (autograd leaves
    if gradients are wanted). Returns logits [b, s, vocab]."""
    import torch.nn.functional as F
    from neuronx_distributed_training_amd.ops.rope import build_rope_cache

    b, s = ids.shape
    hq, hkv, d = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
    cos, sin = build_rope_cache(s, d, cfg.rope_theta, device=ids.device)

    def norm(x, w):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True)
                               + cfg.rms_norm_eps) * w

    def rope(x):
        x1, x2 = x.chunk(2, dim=-1)
        return x * cos[:s] + torch.cat((-x2, x1), dim=-1) * sin[:s]

    alive = segment_alive(seg)
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
        o = torch.matmul(torch.softmax(sc, dim=-1), v)
        o = o.transpose(1, 2).reshape(b, s, hq * d)
        x = x + F.linear(o, params[pre + "self_attn.o_proj.weight"])
        h = norm(x, params[pre + "post_attention_layernorm.weight"])
        gate, up = F.linear(
            h, params[pre + "mlp.gate_up_proj.weight"]).chunk(2, dim=-1)
        x = x + F.linear(F.silu(gate) * up,
                         params[pre + "mlp.down_proj.weight"])
    x = norm(x, params["model.norm.weight"])
    return F.linear(x, params["lm_head.weight"])
