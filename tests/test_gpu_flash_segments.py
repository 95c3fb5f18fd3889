"""Segmented (packed-sequence, block-diagonal causal) flash attention kernels
on MI355X vs fp32 dense attention with an explicit mask, computed on the GPU
(tests/segments_ref.py). Tolerances are test_gpu_flash_kv_range.py's:
forward max abs error < 0.02, backward err / max(1, |ref|.max()) < 0.05,
all outputs finite."""

import pytest
import torch

from tests.kv_range_ref import masked_lm_loss
from tests.segments_ref import (
    dense_attention_seg, ids_from_lengths, llama_fp32_logits_seg,
)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from neuronx_distributed_training_amd import ops

    return ops.require_extension()  # fail loudly if the .so is missing


def _poison(*shapes_dtypes):
    """Fill-and-free NaN buffers of the kernels' output sizes, so a block
    the caching allocator hands back to torch::empty is visibly garbage
    unless the kernel writes all of it."""
    junk = [torch.full(shape, float("nan"), device="cuda", dtype=dt)
            for shape, dt in shapes_dtypes]
    del junk


def _inputs(b, hq, hkv, s, d, seed):
    torch.manual_seed(seed)
    dev, bf = "cuda", torch.bfloat16
    q = torch.randn(b, hq, s, d, device=dev, dtype=bf)
    k = torch.randn(b, hkv, s, d, device=dev, dtype=bf)
    v = torch.randn(b, hkv, s, d, device=dev, dtype=bf)
    do = (torch.randn(b, hq, s, d, device=dev) + 2.0).to(bf)  # no zero row
    return q, k, v, do


def _op(q, k, v, do, seg, window=0):
    """One NaN-poisoned fwd + bwd through the public op; returns detached
    (o, dq, dk, dv)."""
    from neuronx_distributed_training_amd.ops import flash_attn_func

    b, hq, s, d = q.shape
    hkv = k.size(1)
    g = hq // hkv
    bf, f32 = torch.bfloat16, torch.float32
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    _poison(((s, b, hq, d), bf), ((b, hq, s), f32))
    o = flash_attn_func(q, k, v, causal=True, window=window, segment_ids=seg)
    _poison(((s, b, hq, d), bf), ((g, s, b, hkv, d), f32),
            ((g, s, b, hkv, d), f32), ((b, hq, s), f32))
    o.backward(do)
    return o.detach(), q.grad, k.grad, v.grad


def _run(layouts, hq, hkv, s, d, window=0, seed=0):
    """Segmented op fwd + bwd vs the dense reference; asserts the
    tolerances and finiteness; returns the tensors."""
    seg = ids_from_lengths(layouts, s, device="cuda")
    q, k, v, do = _inputs(len(layouts), hq, hkv, s, d, seed)
    ro, rdq, rdk, rdv = dense_attention_seg(q, k, v, seg, window=window,
                                            dout=do)
    o, dq, dk, dv = _op(q, k, v, do, seg, window)
    assert torch.isfinite(o.float()).all()
    err = (o.float() - ro).abs().max()
    print(f"fwd max err {float(err):.5f}")
    assert err < 0.02, f"fwd max err {err}"
    for got, want, name in ((dq, rdq, "dq"), (dk, rdk, "dk"),
                            (dv, rdv, "dv")):
        assert torch.isfinite(got.float()).all(), name
        e = (got.float() - want).abs().max()
        sc = want.abs().max().clamp(min=1)
        print(f"{name} rel err {float(e / sc):.5f}")
        assert e / sc < 0.05, f"{name} rel err {e / sc}"
    return dict(q=q, k=k, v=v, do=do, seg=seg, o=o, dq=dq, dk=dk, dv=dv)


LAYOUT1 = [[333], [70, 1, 63, 130, 69], [64, 64, 128, 77]]


def test_ragged_segments(ext):
    """Case 1: mid-sub-block boundaries, a length-1 segment, rows whose
    first visited KV tile is entirely dead (the forward p = exp(0) = 1
    trap), and a tile-aligned row."""
    from neuronx_distributed_training_amd.ops import flash_attn_func

    r = _run(LAYOUT1, 4, 2, 333, 128)
    # batch row 0 is one segment: must agree with the dense kernel
    dense = flash_attn_func(r["q"][:1], r["k"][:1], r["v"][:1], causal=True)
    diff = (dense.float() - r["o"][:1].float()).abs().max()
    print(f"row 0 segmented vs dense: max diff {float(diff)}, "
          f"bit-equal {torch.equal(dense, r['o'][:1])}")
    assert diff < 0.02


def test_bm256_instantiation(ext):
    """Case 2: ceil(S / 256) * B * HQ = 512 is not < 512, so the launchers
    pick the BM = 256 forward / dq variants; segments cross and end on the
    q-tile boundary."""
    _run([[100, 412], [256, 256], [300, 212], [512]], 64, 8, 512, 64, seed=2)


def test_sliding_window_plus_segments(ext):
    """Case 3."""
    _run([[150, 234]], 4, 2, 384, 128, window=100, seed=3)


def test_every_token_its_own_segment(ext):
    """Case 4: softmax over one key, so O is exactly V of the kv head."""
    s = 128
    r = _run([[1] * s, [1] * s], 4, 2, s, 128, seed=4)
    want = r["v"].repeat_interleave(2, dim=1)
    assert torch.equal(r["o"], want)


def test_isolation_is_bit_exact(ext):
    """Case 5: replacing the first segment's q/k/v/dO leaves O, dQ, dK, dV
    of every other segment bit-identical (dead entries give p = 0 exactly
    and the kernels use no atomics)."""
    s = 333
    seg = ids_from_lengths(LAYOUT1, s, device="cuda")
    q, k, v, do = _inputs(3, 4, 2, s, 128, seed=5)
    base = _op(q, k, v, do, seg)
    q2, k2, v2, do2 = (t.clone() for t in (q, k, v, do))
    first = {1: LAYOUT1[1][0], 2: LAYOUT1[2][0]}   # rows with > 1 segment
    torch.manual_seed(55)
    for row, n in first.items():
        for t in (q2, k2, v2, do2):
            t[row, :, :n] = (torch.randn_like(t[row, :, :n].float()) * 1.5
                             + 0.5).to(t.dtype)
    moved = _op(q2, k2, v2, do2, seg)
    for name, a, c in zip(("o", "dq", "dk", "dv"), base, moved):
        assert torch.isfinite(c.float()).all(), name
        assert torch.equal(a[0], c[0]), name          # untouched batch row
        for row, n in first.items():
            assert torch.equal(a[row, :, n:], c[row, :, n:]), (name, row)
            assert not torch.equal(a[row, :, :n], c[row, :, :n]), (name, row)


def test_binding_checks_bound_tensors(ext):
    """Case 6."""
    b, s = 2, 64
    q = torch.randn(b, 2, s, 128, device="cuda", dtype=torch.bfloat16)
    qs = torch.zeros(b, s, device="cuda", dtype=torch.int32)
    ke = torch.full((b, s), s, device="cuda", dtype=torch.int32)
    o, lse = ext.flash_attn_fwd_seg(q, q, q, qs, ke, 0.1, 0)   # fine
    wide = torch.zeros(b, 2 * s, device="cuda", dtype=torch.int32)[:, ::2]
    bad = [
        (qs.long(), ke),                         # dtype
        (qs, ke.cpu()),                          # device
        (qs[:1], ke),                            # shape [B, S]
        (qs, ke[:, :32]),
        (qs.reshape(-1), ke),
        (wide, ke),                              # stride
    ]
    for a, c in bad:
        with pytest.raises(RuntimeError):
            ext.flash_attn_fwd_seg(q, q, q, a, c, 0.1, 0)
        with pytest.raises(RuntimeError):
            ext.flash_attn_bwd_seg(q, q, q, q, o, lse, a, c, 0.1, 0)
    kv_short = q[:, :, :32]                      # S_q != S_kv
    with pytest.raises(RuntimeError):
        ext.flash_attn_fwd_seg(q, kv_short, kv_short, qs, ke, 0.1, 0)
    with pytest.raises(RuntimeError):
        ext.flash_attn_bwd_seg(q, q, kv_short, kv_short, o, lse, qs, ke,
                               0.1, 0)


# ------------------------------------------------------------ model level
def _tiny_bf16():
    from neuronx_distributed_training_amd.parallel import state as ps
    from neuronx_distributed_training_amd.models.llama import (
        LlamaConfig, LlamaForCausalLM,
    )

    ps.destroy_model_parallel()
    ps.initialize_model_parallel()
    torch.manual_seed(21)
    cfg = LlamaConfig(
        vocab_size=512, hidden_size=256, intermediate_size=512,
        num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
        max_position_embeddings=160, dtype="bfloat16",
    )
    return LlamaForCausalLM(cfg).cuda().train()


ATTN_W = "model.layers.0.self_attn.kv_proj.weight"
NORM_W = "model.layers.1.input_layernorm.weight"


def test_model_packed_vs_unpacked_vs_fp32(ext, monkeypatch):
    """Case 7: one row of three packed documents plus a pad tail through
    the segmented kernels is as close to an fp32 reference (same weights,
    plain PyTorch with the block-diagonal mask) as the same model run on
    each document alone through the dense kernels:
    err_packed <= 2 * err_unpacked + 1e-3 for logits at real positions, the
    masked loss, one attention and one norm weight grad."""
    calls = {"fwd": 0, "bwd": 0}
    real_f, real_b = ext.flash_attn_fwd_seg, ext.flash_attn_bwd_seg

    def spy_f(*a, **kw):
        calls["fwd"] += 1
        return real_f(*a, **kw)

    def spy_b(*a, **kw):
        calls["bwd"] += 1
        return real_b(*a, **kw)

    monkeypatch.setattr(ext, "flash_attn_fwd_seg", spy_f)
    monkeypatch.setattr(ext, "flash_attn_bwd_seg", spy_b)

    s, docs = 160, [47, 38, 60]                  # + a pad tail of 15
    seg = ids_from_lengths([docs + [s - sum(docs)]], s, device="cuda")
    g = torch.Generator().manual_seed(23)
    ids = torch.randint(1, 512, (1, s), generator=g).cuda()
    real = seg < len(docs)
    ids = ids * real                             # pad token 0
    # scored: real tokens that are not the first of their document
    lm = real.clone()
    lm[:, 1:] &= seg[:, 1:] == seg[:, :-1]
    lm[:, 0] = False
    n_scored = int(lm.sum())
    assert n_scored == sum(docs) - len(docs)

    def grads_of(model):
        p = dict(model.named_parameters())
        return p[ATTN_W].grad.float(), p[NORM_W].grad.float()

    packed = _tiny_bf16()
    with torch.no_grad():
        logits_p = packed(ids, segment_ids=seg).float()[real]
    loss_p = packed(ids, labels=ids, loss_mask=lm, segment_ids=seg)
    loss_p.backward()
    assert calls == {"fwd": 4, "bwd": 2}, calls   # 2 layers x (2 fwd, 1 bwd)
    got_p = (logits_p, loss_p.detach().float()) + grads_of(packed)

    # the yardstick: each document alone, dense kernels
    calls.update(fwd=0, bwd=0)
    alone = _tiny_bf16()
    logits_u, loss_u, at = [], 0.0, 0
    for n in docs:
        d_ids = ids[:, at:at + n]
        with torch.no_grad():
            logits_u.append(alone(d_ids).float()[0])
        part = alone(d_ids, labels=d_ids) * ((n - 1) / n_scored)
        part.backward()                           # grads accumulate
        loss_u = loss_u + part.detach().float()
        at += n
    assert calls == {"fwd": 0, "bwd": 0}, calls
    got_u = (torch.cat(logits_u), loss_u) + grads_of(alone)

    # fp32 reference: the same (bf16-valued) weights, plain PyTorch
    params = {n: p.detach().float().requires_grad_(True)
              for n, p in alone.named_parameters()}
    for n, p in packed.named_parameters():
        assert torch.equal(p.detach().float(), params[n].detach()), n
    ref_logits = llama_fp32_logits_seg(params, alone.cfg, ids, seg)
    ref_loss = masked_lm_loss(ref_logits, ids, lm)
    ref_loss.backward()
    ref = (ref_logits.detach()[real], ref_loss.detach(),
           params[ATTN_W].grad, params[NORM_W].grad)

    for name, a, u, r in zip(("logits", "loss", "attn grad", "norm grad"),
                             got_p, got_u, ref):
        assert torch.isfinite(a).all(), name
        err_p = float((a - r).abs().max())
        err_u = float((u - r).abs().max())
        print(f"{name}: packed err {err_p:.3e}  unpacked err {err_u:.3e}  "
              f"|ref| max {float(r.abs().max()):.3e}")
        assert err_p <= 2 * err_u + 1e-3, (name, err_p, err_u)


def test_model_rejects_what_the_kernels_lack(ext):
    from neuronx_distributed_training_amd.parallel import state as ps
    from neuronx_distributed_training_amd.models.llama import (
        LlamaConfig, LlamaForCausalLM,
    )

    ps.destroy_model_parallel()
    ps.initialize_model_parallel()
    cfg = LlamaConfig(
        vocab_size=128, hidden_size=64, intermediate_size=128,
        num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2,
        max_position_embeddings=32, dtype="bfloat16",     # head_dim 16
    )
    model = LlamaForCausalLM(cfg).cuda()
    ids = torch.randint(1, 128, (1, 32), device="cuda")
    seg = ids_from_lengths([[13, 19]], 32, device="cuda")
    with pytest.raises(ValueError, match="head_dim"):
        model(ids, segment_ids=seg)
