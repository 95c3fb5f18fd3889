"""Ranged (per-batch-row key range) flash attention kernels on MI355X vs
fp32 dense attention with an explicit mask, computed on the GPU
(tests/kv_range_ref.py). Tolerances are test_gpu_kernels.py's: forward max
abs error < 0.02, backward err / max(1, |ref|.max()) < 0.05, over ALL rows
(padded query rows included), plus exact zeros / finiteness where the
semantics define them."""

import pytest
import torch

from tests.kv_range_ref import (
    dense_attention, llama_fp32_logits, masked_lm_loss,
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


def _run(ranges, hq, hkv, sq, skv, d, causal=True, window=0, bwd=True,
         seed=0):
    """Ranged op fwd (+bwd) vs the dense reference; asserts the tolerances
    and the exact-zero / finiteness conditions; returns the tensors."""
    from neuronx_distributed_training_amd.ops import flash_attn_func

    torch.manual_seed(seed)
    b = len(ranges)
    g = hq // hkv
    dev, bf = "cuda", torch.bfloat16
    q = torch.randn(b, hq, sq, d, device=dev, dtype=bf, requires_grad=bwd)
    k = torch.randn(b, hkv, skv, d, device=dev, dtype=bf, requires_grad=bwd)
    v = torch.randn(b, hkv, skv, d, device=dev, dtype=bf, requires_grad=bwd)
    # non-zero on every row
    do = (torch.randn(b, hq, sq, d, device=dev) + 2.0).to(bf)
    lo = torch.tensor([r[0] for r in ranges], device=dev, dtype=torch.int32)
    hi = torch.tensor([r[1] for r in ranges], device=dev, dtype=torch.int32)

    ro, rdq, rdk, rdv, alive = dense_attention(
        q, k, v, lo, hi, causal=causal, window=window,
        dout=do if bwd else None)
    empty = ~alive.any(-1).expand(b, hq, sq)
    j = torch.arange(skv, device=dev)
    dead_key = ((j[None] < lo[:, None]) | (j[None] >= hi[:, None]))
    dead_key = dead_key[:, None].expand(b, hkv, skv)

    f32 = torch.float32
    _poison(((sq, b, hq, d), bf), ((b, hq, sq), f32))
    o = flash_attn_func(q, k, v, causal=causal, window=window,
                        kv_range=(lo, hi))
    err = (o.float() - ro).abs().max()
    err = err.detach()
    print(f"fwd max err {float(err):.5f}")
    assert torch.isfinite(o.float()).all()
    assert err < 0.02, f"fwd max err {err}"
    assert (o.detach()[empty] == 0).all(), "empty rows must give O == 0"
    out = dict(q=q, k=k, v=v, o=o, lo=lo, hi=hi, empty=empty,
               dead_key=dead_key)
    if not bwd:
        return out

    _poison(((sq, b, hq, d), bf), ((g, skv, b, hkv, d), f32),
            ((g, skv, b, hkv, d), f32), ((b, hq, sq), f32))
    o.backward(do)
    for got, want, name in ((q.grad, rdq, "dq"), (k.grad, rdk, "dk"),
                            (v.grad, rdv, "dv")):
        assert torch.isfinite(got.float()).all(), name
        e = (got.float() - want).abs().max()
        sc = want.abs().max().clamp(min=1)
        print(f"{name} rel err {float(e / sc):.5f}")
        assert e / sc < 0.05, f"{name} rel err {e / sc}"
    assert (q.grad[empty] == 0).all(), "empty rows must give dQ == 0"
    assert (k.grad[dead_key] == 0).all(), "out-of-range keys: dK == 0"
    assert (v.grad[dead_key] == 0).all(), "out-of-range keys: dV == 0"
    return out


def test_lse_of_empty_rows_is_finite(ext):
    """Binding level: the stored LSE is finite on every row, empty ones
    included (block-aligned and mid-tile lo)."""
    torch.manual_seed(1)
    b, hq, hkv, s, d = 2, 4, 2, 333, 128
    q = torch.randn(b, hq, s, d, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(b, hkv, s, d, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(b, hkv, s, d, device="cuda", dtype=torch.bfloat16)
    lo = torch.tensor([70, 256], device="cuda", dtype=torch.int32)
    hi = torch.tensor([333, 300], device="cuda", dtype=torch.int32)
    _poison(((s, b, hq, d), torch.bfloat16), ((b, hq, s), torch.float32))
    o, lse = ext.flash_attn_fwd_range(q, k, v, lo, hi, True, d ** -0.5, 0)
    assert torch.isfinite(lse).all()
    assert torch.isfinite(o.float()).all()
    assert (o[0, :, :70] == 0).all() and (o[1, :, :256] == 0).all()


def test_binding_checks_range_tensors(ext):
    q = torch.randn(2, 2, 64, 128, device="cuda", dtype=torch.bfloat16)
    lo = torch.zeros(2, device="cuda", dtype=torch.int32)
    hi = torch.full((2,), 64, device="cuda", dtype=torch.int32)
    bad = [
        (lo.long(), hi),                         # dtype
        (lo, hi.cpu()),                          # device
        (lo[:1], hi),                            # shape
        (torch.zeros(4, device="cuda", dtype=torch.int32)[::2], hi),  # stride
    ]
    for l, h in bad:
        with pytest.raises(RuntimeError):
            ext.flash_attn_fwd_range(q, q, q, l, h, True, 0.1, 0)


def test_mixed_batch_ragged(ext):
    """Case 1: lo = 70 / 37 put empty rows into the same q-block and the
    same 64-key tile as valid rows (the forward p = exp(0) = 1 trap)."""
    from neuronx_distributed_training_amd.ops import flash_attn_func

    s = 333
    r = _run([(0, s), (70, s), (0, 130), (37, 200)], 4, 2, s, s, 128)
    assert r["empty"][1].any() and r["empty"][3].any()
    # batch row 0 has the full range: must agree with the dense kernel
    dense = flash_attn_func(r["q"][:1].detach(), r["k"][:1].detach(),
                            r["v"][:1].detach(), causal=True)
    diff = (dense.float() - r["o"][:1].detach().float()).abs().max()
    print(f"row 0 ranged vs unranged: max diff {float(diff)}, "
          f"bit-equal {torch.equal(dense, r['o'][:1].detach())}")
    assert diff < 0.02


def test_block_aligned_edges(ext):
    """Case 2: whole q-blocks empty, whole key blocks skipped; their O, dQ,
    dK, dV slabs must be written as zeros (the outputs are torch::empty)."""
    s = 512
    r = _run([(256, s), (0, 256), (128, 384)], 4, 2, s, s, 128, seed=2)
    assert (r["o"][0, :, :256] == 0).all()
    assert (r["q"].grad[0, :, :256] == 0).all()
    assert (r["k"].grad[0, :, :256] == 0).all()
    assert (r["v"].grad[1, :, 256:] == 0).all()
    assert (r["k"].grad[2, :, 384:] == 0).all()


def test_bm256_instantiation(ext):
    """Case 3: ceil(S / 256) * B * HQ = 512 is not < 512, so the launchers
    pick the BM = 256 forward / dq variants."""
    s = 512
    _run([(100, s), (0, 300), (64, 448), (0, s)], 64, 8, s, s, 64, seed=3)


def test_sliding_window_plus_range(ext):
    """Case 4."""
    s = 384
    _run([(50, s), (0, 300)], 4, 2, s, s, 128, window=100, seed=4)


@pytest.mark.parametrize("sq,skv,bwd", [(1, 300, False), (128, 512, True)])
def test_crosslen_plus_range(ext, sq, skv, bwd):
    """Case 5: S_q != S_kv (bottom-right aligned causal) with lo = 45."""
    _run([(45, skv), (45, skv)], 4, 2, sq, skv, 128, bwd=bwd, seed=5)


def test_degenerate_range(ext):
    """Case 6: lo == hi — the whole batch row is zeros, all finite."""
    s = 200
    r = _run([(0, s), (64, 64), (10, 150)], 4, 2, s, s, 128, seed=6)
    assert r["empty"][1].all()
    assert (r["o"][1] == 0).all()
    for t in (r["q"], r["k"], r["v"]):
        assert (t.grad[1] == 0).all()


# ------------------------------------------------------------ model level
def _tiny_bf16(padded_attention):
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
        padded_attention=padded_attention,
    )
    return LlamaForCausalLM(cfg).cuda().train()


ATTN_W = "model.layers.0.self_attn.kv_proj.weight"
NORM_W = "model.layers.1.input_layernorm.weight"


def test_model_auto_vs_eager_vs_fp32(ext, monkeypatch):
    """Case 7: "auto" takes the ranged kernel and is as close to an fp32
    reference (same weights, plain PyTorch on the GPU) as the eager bf16
    path is: err_flash <= 2 * err_eager + 1e-3 for logits at valid
    positions, the masked loss, one attention and one norm weight grad."""
    calls = {"fwd": 0, "bwd": 0}
    real_f, real_b = ext.flash_attn_fwd_range, ext.flash_attn_bwd_range

    def spy_f(*a, **kw):
        calls["fwd"] += 1
        return real_f(*a, **kw)

    def spy_b(*a, **kw):
        calls["bwd"] += 1
        return real_b(*a, **kw)

    monkeypatch.setattr(ext, "flash_attn_fwd_range", spy_f)
    monkeypatch.setattr(ext, "flash_attn_bwd_range", spy_b)

    s = 160
    g = torch.Generator().manual_seed(22)
    ids = torch.randint(1, 512, (2, s), generator=g).cuda()
    am = torch.ones(2, s, dtype=torch.long, device="cuda")
    am[0, :37] = 0                    # left-padded row
    am[1, s - 50:] = 0                # right-padded row
    ids = ids * am
    valid = am.bool()
    lm = am.clone()
    lm[:, 1:] &= am[:, :-1]           # scored token and its predictor real

    def run(model):
        model.zero_grad()
        with torch.no_grad():
            logits = model(ids, attention_mask=am).float()
        loss = model(ids, labels=ids, loss_mask=lm, attention_mask=am)
        loss.backward()
        grads = dict(model.named_parameters())
        return (logits[valid], loss.detach().float(),
                grads[ATTN_W].grad.float(), grads[NORM_W].grad.float())

    auto = _tiny_bf16("auto")
    got_auto = run(auto)
    assert calls == {"fwd": 4, "bwd": 2}, calls   # 2 layers x (2 fwd, 1 bwd)
    calls.update(fwd=0, bwd=0)
    eager = _tiny_bf16("eager")
    got_eager = run(eager)
    assert calls == {"fwd": 0, "bwd": 0}, calls

    # fp32 yardstick: the same (bf16-valued) weights, plain PyTorch
    params = {n: p.detach().float().requires_grad_(True)
              for n, p in eager.named_parameters()}
    for n, p in auto.named_parameters():
        assert torch.equal(p.detach().float(), params[n].detach()), n
    ref_logits = llama_fp32_logits(params, eager.cfg, ids, am)
    ref_loss = masked_lm_loss(ref_logits, ids, lm)
    ref_loss.backward()
    ref = (ref_logits.detach()[valid], ref_loss.detach(),
           params[ATTN_W].grad, params[NORM_W].grad)

    for name, a, e, r in zip(("logits", "loss", "attn grad", "norm grad"),
                             got_auto, got_eager, ref):
        assert torch.isfinite(a).all(), name
        err_a = float((a - r).abs().max())
        err_e = float((e - r).abs().max())
        print(f"{name}: flash err {err_a:.3e}  eager err {err_e:.3e}  "
              f"|ref| max {float(r.abs().max()):.3e}")
        assert err_a <= 2 * err_e + 1e-3, (name, err_a, err_e)

    # a mask with a hole: "auto" must take the eager path
    am_hole = am.clone()
    am_hole[1, 20] = 0
    with torch.no_grad():
        la = auto(ids, attention_mask=am_hole)
        le = eager(ids, attention_mask=am_hole)
    assert calls == {"fwd": 0, "bwd": 0}, calls
    assert torch.equal(la, le)


def test_dense_fwd_head_dim_64(ext):
    """The (unranged) double-buffered forward at head_dim 64: only the
    first BN*D/16 = 256 threads own a V row-pair slice to stage."""
    from neuronx_distributed_training_amd.ops import flash_attn_func

    torch.manual_seed(8)
    b, hq, hkv, s, d = 2, 4, 2, 333, 64
    q = torch.randn(b, hq, s, d, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(b, hkv, s, d, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(b, hkv, s, d, device="cuda", dtype=torch.bfloat16)
    o = flash_attn_func(q, k, v, causal=True)
    ref = torch.nn.functional.scaled_dot_product_attention(
        q.float(), k.float().repeat_interleave(2, 1),
        v.float().repeat_interleave(2, 1), is_causal=True)
    err = (o.float() - ref).abs().max()
    assert err < 0.02, f"max err {err}"
