"""Dense (unranged) v2 flash attention on MI355X at the call patterns
training uses: the fused-QKV strides of models/llama.py, head_dim 64
backward, the BM = 256 instantiations the benchmark shape takes, ragged
q-block / key-tile tails, sliding window with all three gradients, sub-tile
lengths and decode. O, LSE, dQ, dK, dV are compared with an fp32 reference
on the GPU (tests/kv_range_ref.dense_attention with the full key range; LSE
= logsumexp of the masked scaled scores). Tolerances are the suite's:
O max abs err < 0.02, LSE max abs err < 2e-2, grads
max|err| / max(1, max|ref|) < 0.05. Also here: the host-side argument
contracts of the backward and RMSNorm bindings."""

import pytest
import torch

from tests.kv_range_ref import alive_mask, dense_attention

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def ext():
    from neuronx_distributed_training_amd import ops

    return ops.require_extension()  # fail loudly if the .so is missing


def _poison(*shapes_dtypes):
    """Fill-and-free NaN buffers of the kernels' output sizes: every output
    is torch::empty, so a block the kernel leaves unwritten shows."""
    junk = [torch.full(shape, float("nan"), device="cuda", dtype=dt)
            for shape, dt in shapes_dtypes]
    del junk


def _inputs(b, hq, hkv, sq, skv, d, layout, bwd):
    """q, k, v, dout as logical [b, h, s, d] tensors plus a function that
    returns (dq, dk, dv) after backward."""
    dev = "cuda"
    if layout == "bhsd":
        q = torch.randn(b, hq, sq, d, device=dev, dtype=BF, requires_grad=bwd)
        k = torch.randn(b, hkv, skv, d, device=dev, dtype=BF,
                        requires_grad=bwd)
        v = torch.randn(b, hkv, skv, d, device=dev, dtype=BF,
                        requires_grad=bwd)
        dout = torch.randn(b, hq, sq, d, device=dev, dtype=BF)
        return q, k, v, dout, lambda: (q.grad, k.grad, v.grad)
    assert layout == "fused" and sq == skv
    # models/llama.py: one [s, b, (hq + 2 hkv) d] projection output, split
    # by columns, each part viewed [s, b, h, d] and permuted to [b, h, s, d]
    s = sq
    nq, nkv = hq * d, hkv * d
    leaf = torch.randn(s, b, nq + 2 * nkv, device=dev, dtype=BF,
                       requires_grad=bwd)
    qs, ks, vs = leaf.split([nq, nkv, nkv], dim=-1)
    q = qs.view(s, b, hq, d).permute(1, 2, 0, 3)
    k = ks.view(s, b, hkv, d).permute(1, 2, 0, 3)
    v = vs.view(s, b, hkv, d).permute(1, 2, 0, 3)
    assert not q.is_contiguous() and not k.is_contiguous()
    dout = torch.randn(s, b, hq, d, device=dev, dtype=BF).permute(1, 2, 0, 3)

    def grads():
        gq, gk, gv = leaf.grad.split([nq, nkv, nkv], dim=-1)
        return (gq.view(s, b, hq, d).permute(1, 2, 0, 3),
                gk.view(s, b, hkv, d).permute(1, 2, 0, 3),
                gv.view(s, b, hkv, d).permute(1, 2, 0, 3))

    return q, k, v, dout, grads


def _ref_lse(q, k, causal, window, scale):
    b, hq, sq, _ = q.shape
    hkv, skv = k.size(1), k.size(2)
    kx = k.detach().float().repeat_interleave(hq // hkv, 1)
    s = torch.matmul(q.detach().float(), kx.transpose(-1, -2)) * scale
    alive = alive_mask(b, sq, skv, [0] * b, [skv] * b, causal, window,
                       q.device)
    return torch.logsumexp(s.masked_fill(~alive, float("-inf")), dim=-1)


def _check(ext, b, hq, hkv, sq, skv, d, causal, window, layout, bwd=True,
           seed=0):
    from neuronx_distributed_training_amd.ops import flash_attn_func

    torch.manual_seed(seed)
    tag = f"{(b, hq, hkv, sq, skv, d, causal, window, layout)}"
    g = hq // hkv
    scale = d ** -0.5
    q, k, v, dout, grads = _inputs(b, hq, hkv, sq, skv, d, layout, bwd)
    ro, rdq, rdk, rdv, _ = dense_attention(
        q, k, v, [0] * b, [skv] * b, causal=causal, scale=scale,
        window=window, dout=dout if bwd else None)
    rlse = _ref_lse(q, k, causal, window, scale)

    _poison(((sq, b, hq, d), BF), ((b, hq, sq), F32))
    _, lse = ext.flash_attn_fwd(q.detach(), k.detach(), v.detach(), causal,
                                scale, window)
    lerr = float((lse - rlse).abs().max())
    _poison(((sq, b, hq, d), BF), ((b, hq, sq), F32))
    o = flash_attn_func(q, k, v, causal=causal, window=window)
    oerr = float((o.detach().float() - ro).abs().max())
    print(f"{tag}: o err {oerr:.5f}  lse err {lerr:.5f}")
    assert torch.isfinite(o.detach().float()).all(), tag
    assert torch.isfinite(lse).all(), tag
    assert oerr < 0.02, f"{tag}: o max err {oerr}"
    assert lerr < 2e-2, f"{tag}: lse max err {lerr}"
    if not bwd:
        return
    _poison(((sq, b, hq, d), BF), ((g, skv, b, hkv, d), F32),
            ((g, skv, b, hkv, d), F32), ((b, hq, sq), F32))
    o.backward(dout)
    rels = {}
    for name, got, want in zip(("dq", "dk", "dv"), grads(), (rdq, rdk, rdv)):
        assert got.shape == want.shape, (tag, name)
        assert torch.isfinite(got.float()).all(), (tag, name)
        e = (got.float() - want).abs().max()
        rels[name] = float(e / want.abs().max().clamp(min=1))
    print(f"{tag}: " + "  ".join(f"{n} rel {r:.5f}" for n, r in rels.items()))
    for name, rel in rels.items():
        assert rel < 0.05, f"{tag}: {name} rel err {rel}"


# (b, hq, hkv, sq, skv, d, causal, window, layout)
CASES = [
    # production strides
    (2, 4, 2, 333, 333, 128, True, 0, "fused"),
    # head_dim 64 backward
    (2, 8, 2, 333, 333, 64, True, 0, "fused"),
    (1, 4, 1, 256, 384, 64, False, 0, "bhsd"),
    # BM = 256 branch: ceil(300 / 256) * 4 * 64 = 512, ragged tails
    (4, 64, 8, 300, 300, 128, True, 0, "bhsd"),
    (4, 64, 8, 300, 300, 64, True, 0, "fused"),
    (4, 64, 8, 300, 400, 128, False, 0, "bhsd"),
    # sliding window, all three gradients
    (1, 4, 2, 384, 384, 128, True, 100, "bhsd"),
    (1, 4, 2, 128, 512, 128, True, 160, "bhsd"),
] + [
    # sub-tile and tile-edge lengths
    (1, 2, 1, s, s, 128, True, 0, "bhsd") for s in (1, 63, 64, 65, 129)
]


@pytest.mark.parametrize(
    "case", CASES, ids=["-".join(str(x) for x in c) for c in CASES])
def test_dense_fwd_bwd(ext, case):
    _check(ext, *case, seed=CASES.index(case))


@pytest.mark.parametrize("skv", [1, 65])
def test_decode_fwd(ext, skv):
    """sq = 1 against a cache of skv keys: forward and LSE only."""
    _check(ext, 2, 4, 2, 1, skv, 128, True, 0, "bhsd", bwd=False, seed=30)


def test_bwd_strided_lse_equals_contiguous(ext):
    """The ring's j > r hop passes lse[:, :, half:], a strided view. The
    binding must hand the kernels the same values as for a contiguous copy:
    results bit-equal (the kernels use no atomics)."""
    torch.manual_seed(31)
    b, hq, hkv, half, d = 2, 4, 2, 80, 128
    scale = d ** -0.5
    q = torch.randn(b, hq, 2 * half, d, device="cuda", dtype=BF)
    k = torch.randn(b, hkv, 2 * half, d, device="cuda", dtype=BF)
    v = torch.randn(b, hkv, 2 * half, d, device="cuda", dtype=BF)
    do = torch.randn(b, hq, 2 * half, d, device="cuda", dtype=BF)
    o, full = ext.flash_attn_fwd(q, k, v, False, scale)
    view = full[:, :, half:]
    assert not view.is_contiguous()
    args = (do[:, :, half:].contiguous(), q[:, :, half:], k, v,
            o[:, :, half:])
    got = ext.flash_attn_bwd(*args, view, False, scale)
    want = ext.flash_attn_bwd(*args, view.contiguous(), False, scale)
    for name, a, w in zip(("dq", "dk", "dv"), got, want):
        assert torch.isfinite(w.float()).all(), name
        assert torch.equal(a, w), name


def test_flash_fwd_dbuf_matches_sbuf_d64(ext):
    """head_dim 64 A/B of the two forward kernels (only the first
    BN*D/16 = 256 threads own a V row-pair slice to stage), BM = 128 and
    BM = 256 grids: bit-identical like the head_dim 128 A/B."""
    torch.manual_seed(32)
    d = 64
    for b, hq, hkv, s in ((2, 4, 2, 333), (4, 64, 8, 300)):
        q = torch.randn(b, hq, s, d, device="cuda", dtype=BF)
        k = torch.randn(b, hkv, s, d, device="cuda", dtype=BF)
        v = torch.randn(b, hkv, s, d, device="cuda", dtype=BF)
        o1, l1 = ext.flash_attn_fwd(q, k, v, True, d ** -0.5)
        o2, l2 = ext.flash_attn_fwd_sbuf(q, k, v, True, d ** -0.5)
        assert torch.equal(o1, o2) and torch.equal(l1, l2), (b, hq, s)


# ------------------------------------------------- binding contracts (host)
def _bwd_call(ext, which, do, q, k, v, o, lse):
    if which == "range":
        lo = torch.zeros(q.size(0), device="cuda", dtype=torch.int32)
        hi = torch.full((q.size(0),), k.size(2), device="cuda",
                        dtype=torch.int32)
        return ext.flash_attn_bwd_range(do, q, k, v, o, lse, lo, hi, True,
                                        0.1, 0)
    fn = ext.flash_attn_bwd if which == "v2" else ext.flash_attn_bwd_v3
    return fn(do, q, k, v, o, lse, True, 0.1, 0)


@pytest.mark.parametrize("which", ["v2", "range", "v3"])
def test_bwd_bindings_reject_bad_arguments(ext, which):
    """Each of these raises on the host before any kernel launch."""
    def t(*shape, dtype=BF):
        return torch.zeros(*shape, device="cuda", dtype=dtype)

    b, hq, hkv, s, d = 1, 4, 2, 64, 128
    q, kv, lse = t(b, hq, s, d), t(b, hkv, s, d), t(b, hq, s, dtype=F32)
    strided = t(b, hkv, s, 2 * d)[..., ::2]          # stride(3) == 2
    assert strided.shape == kv.shape and strided.stride(3) == 2
    bad = {
        "head_dim 32": (t(b, hq, s, 32), t(b, hq, s, 32), t(b, hkv, s, 32),
                        t(b, hkv, s, 32), t(b, hq, s, 32), lse),
        "hq % hkv": (q, q, t(b, 3, s, d), t(b, 3, s, d), q, lse),
        "k stride": (q, q, strided, kv, q, lse),
        "v stride": (q, q, kv, strided, q, lse),
        "lse dtype": (q, q, kv, kv, q, lse.to(BF)),
        "lse double": (q, q, kv, kv, q, lse.double()),
        "lse shape": (q, q, kv, kv, q, lse[:, :, : s // 2]),
        "lse rank": (q, q, kv, kv, q, lse.reshape(b, hq * s)),
        "lse device": (q, q, kv, kv, q, lse.cpu()),
    }
    for name, args in bad.items():
        with pytest.raises(RuntimeError):
            _bwd_call(ext, which, *args)
            pytest.fail(f"{which}: {name} was accepted")


def test_sbuf_binding_rejects_gqa_mismatch(ext):
    q = torch.zeros(1, 4, 64, 128, device="cuda", dtype=BF)
    kv = torch.zeros(1, 3, 64, 128, device="cuda", dtype=BF)
    with pytest.raises(RuntimeError):
        ext.flash_attn_fwd_sbuf(q, kv, kv, True, 0.1)


def test_rmsnorm_bindings_reject_non_bf16_weight(ext):
    x = torch.randn(4, 64, device="cuda", dtype=BF)
    w32 = torch.ones(64, device="cuda", dtype=F32)
    inv = torch.ones(4, device="cuda", dtype=F32)
    with pytest.raises(RuntimeError):
        ext.rmsnorm_fwd(x, w32, 1e-5)
    with pytest.raises(RuntimeError):
        ext.rmsnorm_bwd(x, x, w32, inv)
    with pytest.raises(RuntimeError):
        ext.rmsnorm_fwd(x, w32.half(), 1e-5)
