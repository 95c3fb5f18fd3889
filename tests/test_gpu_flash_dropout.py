"""Attention dropout inside the flash-attention kernels on MI355X.

The reference is fp32 dense attention on the GPU with the keep mask that
flash_attn_dropout_mask writes: softmax, multiply by mask * keep_scale,
matmul. A kernel that used any other mask is off by O(1), so these cases
also prove that the forward, the dQ and the dK/dV kernel and the mask kernel
agree. Tolerances are test_gpu_flash_kv_range.py's, each multiplied by
keep_scale (dropout multiplies every kept probability, and with it its
rounding error, by that factor): forward max abs error < 0.02 * keep_scale,
backward err / max(1, |ref|.max()) < 0.05 * keep_scale, all outputs finite."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

RNG = (20240607, 12)


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


def _inputs(b, hq, hkv, sq, skv, d, seed, std=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    dev, bf = "cuda", torch.bfloat16
    q = (torch.randn(b, hq, sq, d, device=dev, generator=g) * std).to(bf)
    k = (torch.randn(b, hkv, skv, d, device=dev, generator=g) * std).to(bf)
    v = torch.randn(b, hkv, skv, d, device=dev, generator=g).to(bf)
    do = (torch.randn(b, hq, sq, d, device=dev, generator=g) + 2.0).to(bf)
    return q, k, v, do


def _op(q, k, v, do, causal, window, p, rng):
    """One NaN-poisoned fwd + bwd through the public op; returns detached
    (o, dq, dk, dv)."""
    from neuronx_distributed_training_amd.ops import flash_attn_func

    b, hq, sq, d = q.shape
    hkv, skv = k.size(1), k.size(2)
    g = hq // hkv
    bf, f32 = torch.bfloat16, torch.float32
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    _poison(((sq, b, hq, d), bf), ((b, hq, sq), f32))
    o = flash_attn_func(q, k, v, causal=causal, window=window, dropout_p=p,
                        dropout_rng=rng)
    _poison(((sq, b, hq, d), bf), ((g, skv, b, hkv, d), f32),
            ((g, skv, b, hkv, d), f32), ((b, hq, sq), f32))
    o.backward(do)
    return o.detach(), q.grad, k.grad, v.grad


def _dense_ref(q, k, v, do, causal, window, keep, keep_scale):
    """fp32 dense attention with an explicit keep mask; returns
    (o, dq, dk, dv, p) where p are the undropped probabilities."""
    b, hq, sq, d = q.shape
    hkv, skv = k.size(1), k.size(2)
    g = hq // hkv
    qf, kf, vf = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    kx = kf.repeat_interleave(g, dim=1)
    vx = vf.repeat_interleave(g, dim=1)
    s = qf @ kx.transpose(-1, -2) / math.sqrt(d)
    i = torch.arange(sq, device=q.device)[:, None]
    j = torch.arange(skv, device=q.device)[None, :]
    dead = torch.zeros(sq, skv, dtype=torch.bool, device=q.device)
    if causal:
        dead |= j > i + (skv - sq)
        if window:
            dead |= j <= i + (skv - sq) - window
    p = torch.softmax(s.masked_fill(dead, float("-inf")), dim=-1)
    o = (p * keep * keep_scale) @ vx
    o.backward(do.float())
    return o.detach(), qf.grad, kf.grad, vf.grad, p.detach()


def _run(b, hq, hkv, sq, skv, d, causal, window, p, seed=0):
    from neuronx_distributed_training_amd.ops.flash_attn import (
        dropout_keep_mask, dropout_keep_scale,
    )

    ks = dropout_keep_scale(p)
    q, k, v, do = _inputs(b, hq, hkv, sq, skv, d, seed)
    keep = dropout_keep_mask(b, hq, sq, skv, p, RNG, "cuda")
    ro, rdq, rdk, rdv, _ = _dense_ref(q, k, v, do, causal, window, keep, ks)
    o, dq, dk, dv = _op(q, k, v, do, causal, window, p, RNG)
    assert torch.isfinite(o.float()).all()
    err = (o.float() - ro).abs().max()
    print(f"fwd max err {float(err):.5f} (bound {0.02 * ks:.5f})")
    assert err < 0.02 * ks, f"fwd max err {err}"
    for got, want, name in ((dq, rdq, "dq"), (dk, rdk, "dk"),
                            (dv, rdv, "dv")):
        assert torch.isfinite(got.float()).all(), name
        e = (got.float() - want).abs().max()
        sc = want.abs().max().clamp(min=1)
        print(f"{name} rel err {float(e / sc):.5f} (bound {0.05 * ks:.5f})")
        assert e / sc < 0.05 * ks, f"{name} rel err {e / sc}"


def test_ragged_bm128(ext):
    """Case 1: BM = 128 grid, partial last KV tile, GQA, tail rows."""
    _run(2, 4, 2, 333, 333, 128, True, 0, 0.1)


def test_bm256_instantiations(ext):
    """Case 2: ceil(S / 256) * B * HQ = 512 blocks -> the 256-row kernels."""
    _run(4, 64, 8, 512, 512, 64, True, 0, 0.5)


@pytest.mark.parametrize(
    "hq,hkv,sq,skv,d,causal,window,p",
    [
        (4, 2, 100, 200, 64, False, 0, 0.2),   # non-causal, S_q != S_kv
        (4, 2, 64, 192, 128, True, 0, 0.1),    # causal, bottom-right aligned
        (4, 4, 384, 384, 128, True, 100, 0.1),  # sliding window
    ],
)
def test_further_cases(ext, hq, hkv, sq, skv, d, causal, window, p):
    """Case 3."""
    _run(2, hq, hkv, sq, skv, d, causal, window, p, seed=3)


def test_mask_read_off_the_forward(ext):
    """Case 4: V = identity makes O[i, j] = P[i, j] * M[i, j] * keep_scale,
    so (O != 0) IS the mask the forward kernel used."""
    from neuronx_distributed_training_amd.ops.flash_attn import (
        dropout_keep_mask, dropout_keep_scale,
    )

    b, hq, s, d, p = 2, 4, 64, 64, 0.5
    q, k, _, do = _inputs(b, hq, hq, s, s, d, 4, std=0.1)
    v = torch.eye(s, device="cuda", dtype=torch.bfloat16).expand(
        b, hq, s, d).contiguous()
    keep = dropout_keep_mask(b, hq, s, s, p, RNG, "cuda")
    *_, probs = _dense_ref(q, k, v, do, False, 0, keep,
                           dropout_keep_scale(p))
    # precondition: no kept probability can round to zero in bf16
    print(f"min probability {float(probs.min()):.3e}")
    assert probs.min() > 1e-3
    _poison(((s, b, hq, d), torch.bfloat16), ((b, hq, s), torch.float32))
    o, _ = ext.flash_attn_fwd_drop(q, k, v, False, 1.0 / math.sqrt(d), 0, p,
                                   *RNG)
    assert torch.isfinite(o.float()).all()
    for bi in range(b):
        for h in range(hq):
            assert torch.equal(o[bi, h] != 0, keep[bi, h]), (bi, h)
    frac = keep.float().mean().item()
    assert 0.4 < frac < 0.6, frac   # and it is not trivially all / nothing


@pytest.mark.parametrize("d,s,hq", [(128, 333, 4), (64, 512, 128)])
def test_lse_is_the_undropped_one(ext, d, s, hq):
    """Case 5: the dropout forward sums fp32 probabilities, the dense one
    bf16-rounded ones: relative error <= 2^-9 in l, hence in log l; doubled
    for margin. Both row-block sizes."""
    q, k, v, _ = _inputs(2, hq, hq // 2, s, s, d, 5)
    scale = 1.0 / math.sqrt(d)
    _poison(((s, 2, hq, d), torch.bfloat16), ((2, hq, s), torch.float32))
    _, lse_d = ext.flash_attn_fwd_drop(q, k, v, True, scale, 0, 0.5, *RNG)
    _, lse = ext.flash_attn_fwd(q, k, v, True, scale, 0)
    assert torch.isfinite(lse_d).all()
    diff = (lse_d - lse).abs().max()
    print(f"lse max abs diff {float(diff):.6f} (bound {2 ** -8:.6f})")
    assert diff <= 2 ** -8


def test_purity(ext):
    """Case 6."""
    from neuronx_distributed_training_amd.ops.flash_attn import (
        dropout_keep_mask,
    )

    big = dropout_keep_mask(2, 4, 512, 512, 0.1, RNG, "cuda")
    small = dropout_keep_mask(2, 4, 333, 333, 0.1, RNG, "cuda")
    assert torch.equal(small, big[:, :, :333, :333])
    assert torch.equal(small, dropout_keep_mask(2, 4, 333, 333, 0.1, RNG,
                                                "cuda"))
    other_off = dropout_keep_mask(2, 4, 333, 333, 0.1, (RNG[0], RNG[1] + 4),
                                  "cuda")
    other_seed = dropout_keep_mask(2, 4, 333, 333, 0.1, (RNG[0] + 1, RNG[1]),
                                   "cuda")
    assert not torch.equal(small, other_off)
    assert not torch.equal(small, other_seed)
    assert not torch.equal(other_off, other_seed)

    q, k, v, do = _inputs(2, 4, 2, 333, 333, 128, 6)
    a = _op(q, k, v, do, True, 0, 0.1, RNG)
    b = _op(q, k, v, do, True, 0, 0.1, RNG)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    c = _op(q, k, v, do, True, 0, 0.1, (RNG[0], RNG[1] + 4))
    e = _op(q, k, v, do, True, 0, 0.1, (RNG[0] + 1, RNG[1]))
    for x, y, z in zip(a, c, e):
        assert not torch.equal(x, y)
        assert not torch.equal(x, z)


@pytest.mark.parametrize("p,t", [(0.1, 26), (0.5, 128)])
def test_mask_statistics(ext, p, t):
    """Case 7: binomial bounds at 6 sigma, so a true uniform source passes."""
    from neuronx_distributed_training_amd.ops.flash_attn import (
        dropout_keep_mask,
    )

    h, s = 8, 512
    m = dropout_keep_mask(1, h, s, s, p, RNG, "cuda")[0].double()  # [h, s, s]
    keep = 1.0 - t / 256.0

    def check(frac, target, n, what):
        bound = 6.0 * math.sqrt(target * (1.0 - target) / n)
        dev = (frac - target).abs().max().item()
        print(f"{what}: max deviation {dev:.5f} (6 sigma {bound:.5f})")
        assert dev <= bound, what

    check(m.mean().reshape(1), keep, h * s * s, "overall")
    check(m.mean(dim=(1, 2)), keep, s * s, "per head")
    check(m.mean(dim=2), keep, s, "per row")
    check(m.mean(dim=1), keep, s, "per column")
    agree = keep * keep + (1.0 - keep) * (1.0 - keep)
    check((m[0] == m[1]).double().mean().reshape(1), agree, s * s,
          "heads 0 / 1")
    # rows i, i + 1 inside one 4-query group (bytes of one random word)
    i = torch.arange(s - 1, device="cuda")
    i = i[i % 4 != 3]
    rows = (m[:, i] == m[:, i + 1]).double()
    check(rows.mean().reshape(1), agree, rows.numel(), "rows i / i + 1")
    # keys j, j + 16 (words of one generator call inside a 64-key block)
    cols = (m[:, :, :-16] == m[:, :, 16:]).double()
    check(cols.mean().reshape(1), agree, cols.numel(), "keys j / j + 16")


def test_autograd_stream(ext):
    """Case 8: the default generator governs dropout_rng=None."""
    from torch.utils.checkpoint import checkpoint

    from neuronx_distributed_training_amd.ops import flash_attn_func

    q, k, v, do = _inputs(2, 4, 2, 200, 200, 64, 8)

    def run(seed, ckpt=False):
        if seed is not None:
            torch.manual_seed(seed)
        qq, kk, vv = (t.detach().clone().requires_grad_(True)
                      for t in (q, k, v))

        def fn(a, b, c):
            return flash_attn_func(a, b, c, causal=True, dropout_p=0.1)

        o = (checkpoint(fn, qq, kk, vv, use_reentrant=False) if ckpt
             else fn(qq, kk, vv))
        o.backward(do)
        return o.detach(), qq.grad, kk.grad, vv.grad

    a = run(31)
    assert torch.cuda.default_generators[0].get_offset() == 4   # advanced
    b = run(None)                       # successive calls differ
    c = run(31)                         # manual_seed reproduces
    d = run(31, ckpt=True)              # the recompute regenerates the mask
    for x, y, z, w in zip(a, b, c, d):
        assert not torch.equal(x, y)
        assert torch.equal(x, z)
        assert torch.equal(x, w)


def test_binding_checks(ext):
    """Case 9."""
    from neuronx_distributed_training_amd.ops import flash_attn_func

    q, k, v, do = _inputs(1, 2, 2, 64, 64, 64, 9)
    scale = 0.125
    o, lse = ext.flash_attn_fwd(q, k, v, True, scale, 0)
    for bad in (-0.1, 1.0, 0.999):
        with pytest.raises(RuntimeError):
            ext.flash_attn_fwd_drop(q, k, v, True, scale, 0, bad, 1, 0)
        with pytest.raises(RuntimeError):
            ext.flash_attn_bwd_drop(do, q, k, v, o, lse, True, scale, 0, bad,
                                    1, 0)
        with pytest.raises(RuntimeError):
            ext.flash_attn_dropout_mask(1, 2, 64, 64, bad, 1, 0)
    # p_drop = 0 through the drop bindings is the dense kernel, bit for bit
    o0, lse0 = ext.flash_attn_fwd_drop(q, k, v, True, scale, 0, 0.0, 1, 0)
    assert torch.equal(o0, o) and torch.equal(lse0, lse)
    assert bool(ext.flash_attn_dropout_mask(1, 2, 64, 64, 0.0, 1, 0).all())
    # and through the public op
    a = _op(q, k, v, do, True, 0, 0.0, None)
    qq, kk, vv = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    od = flash_attn_func(qq, kk, vv, causal=True)
    od.backward(do)
    for x, y in zip(a, (od.detach(), qq.grad, kk.grad, vv.grad)):
        assert torch.equal(x, y)


def test_megatron_model(ext, monkeypatch):
    """Case 10: train mode runs the dropout bindings, once per layer, eval
    mode the dense ones; same seed, same loss."""
    from neuronx_distributed_training_amd.models.megatron_gpt import (
        GPTConfig, GPTModel,
    )
    from neuronx_distributed_training_amd.parallel import state as ps
    from neuronx_distributed_training_amd.parallel.random import (
        get_rng_tracker, model_parallel_manual_seed,
    )

    calls = {}
    for name in ("flash_attn_fwd", "flash_attn_bwd", "flash_attn_fwd_drop",
                 "flash_attn_bwd_drop"):
        def spy(*a, _real=getattr(ext, name), _name=name, **kw):
            calls[_name] = calls.get(_name, 0) + 1
            return _real(*a, **kw)

        monkeypatch.setattr(ext, name, spy)

    ps.destroy_model_parallel()
    torch.manual_seed(0)
    cfg = GPTConfig(vocab_size=512, hidden_size=256, num_layers=2,
                    num_attention_heads=4, max_position_embeddings=128,
                    hidden_dropout=0.0, attention_dropout=0.1,
                    dtype="bfloat16")
    model = GPTModel(cfg).cuda()
    ids = torch.randint(0, 512, (2, 128),
                        generator=torch.Generator().manual_seed(1)).cuda()
    try:
        losses = []
        for _ in range(2):
            model.train()
            model.zero_grad(set_to_none=True)
            model_parallel_manual_seed(17)
            calls.clear()
            loss = model(ids, labels=ids.clone())
            loss.backward()
            assert calls == {"flash_attn_fwd_drop": 2,
                             "flash_attn_bwd_drop": 2}, calls
            assert torch.isfinite(loss)
            for n, p_ in model.named_parameters():
                assert p_.grad is not None and \
                    torch.isfinite(p_.grad.float()).all(), n
            losses.append(loss.detach().clone())
        assert torch.equal(losses[0], losses[1])
        model.eval()
        calls.clear()
        with torch.no_grad():
            ev = model(ids, labels=ids.clone())
        assert calls == {"flash_attn_fwd": 2}, calls
        assert torch.isfinite(ev)
    finally:
        get_rng_tracker().reset()
