"""Elementwise HIP kernels on MI355X at the sizes and call patterns
production uses and the small friendly shapes of test_gpu_kernels.py never
reach: second grid-stride passes, scalar tails, optional AdamW arguments,
strided inputs, odd vocab shards. References are plain torch in fp32 / fp64
computed from the same bf16 (fp32 for AdamW) inputs.

Tolerances are test_gpu_kernels.py's (outputs and dx: atol 0.05, rtol 0.05;
CE loss atol 2e-2, rtol 1e-3; CE dlogits < 1.5e-2; AdamW atol 1e-6) with
two additions:
- AdamW gets rtol 1e-5 on top (about ten fp32 roundings of 1.2e-7), needed
  once values exceed 1;
- RMSNorm dw: max|err| / max|ref| < 0.01. dw is ONE bf16 rounding of an
  fp32 sum, half-ulp 2^-9 ~ 0.002; the bound is that with a 5x margin (an
  absolute 0.8 would hide skipped rows)."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def ext():
    from neuronx_distributed_training_amd import ops

    return ops.require_extension()  # fail loudly if the .so is missing


def _close(got, want, what, atol=0.05, rtol=0.05):
    got, want = got.detach().float(), want.detach().float()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), what
    diff = (got - want).abs()
    excess = float((diff - (atol + rtol * want.abs())).max())
    print(f"{what}: max abs err {float(diff.max()):.3e}  "
          f"max (err - tol) {excess:.3e}")
    assert excess <= 0, f"{what}: exceeds atol {atol} rtol {rtol} by {excess}"


# ------------------------------------------------------------------ AdamW
@pytest.mark.parametrize("n", [1, 3, 10003, 8192 * 256 * 4 + 1027])
def test_adamw_tail_scale_and_bf16_copy(ext, n):
    """n % 4 scalar tail (the largest n also takes a second grid-stride
    pass: the grid caps at 8192 * 256 threads of 4 elements), grad_scale as
    a device scalar, and p_bf16 as a slice of a larger guarded buffer — the
    three things ZeRO-1 uses on every step."""
    torch.manual_seed(40)
    dev = "cuda"
    p = torch.randn(n, device=dev)
    g = torch.randn(n, device=dev)
    m = torch.randn(n, device=dev) * 0.1
    v = torch.rand(n, device=dev) * 0.1
    wd_mask = torch.rand(n, device=dev) > 0.5
    gs = torch.tensor(0.37, device=dev, dtype=F32)
    guard = 7.0
    buf = torch.full((n + 256,), guard, device=dev, dtype=BF)
    p16 = buf[128:128 + n]
    lr, b1, b2, eps, wd, t = 1e-3, 0.9, 0.95, 1e-8, 0.01, 3

    # fp64 reference of the same math
    pd, gd, md, vd = (x.double() for x in (p, g, m, v))
    gd = gd * gs.double()
    mr = b1 * md + (1 - b1) * gd
    vr = b2 * vd + (1 - b2) * gd * gd
    denom = (vr / (1 - b2 ** t)).sqrt() + eps
    one = torch.ones((), device=dev, dtype=torch.float64)
    decay = torch.where(wd_mask, one * (1 - lr * wd), one)
    pr = pd * decay - (lr / (1 - b1 ** t)) * mr / denom

    ext.adamw_step(p, g, m, v, wd_mask, lr, b1, b2, eps, wd, t,
                   grad_scale=gs, p_bf16=p16)
    for name, got, want in (("p", p, pr), ("m", m, mr), ("v", v, vr)):
        assert torch.isfinite(got).all(), name
        diff = (got.double() - want).abs()
        excess = float((diff - (1e-6 + 1e-5 * want.abs())).max())
        print(f"adamw n={n} {name}: max abs err {float(diff.max()):.3e}  "
              f"max (err - tol) {excess:.3e}")
        assert excess <= 0, (name, excess)
    # __float2bfloat16 rounds to nearest even, like torch
    assert torch.equal(p16, p.to(BF))
    assert (buf[:128] == guard).all() and (buf[128 + n:] == guard).all()


# ---------------------------------------------------------------- RMSNorm
def _rmsnorm_case(x, w, what, eps=1e-5):
    """Forward check, then backward of both the op and the fp32 formula
    with one random dy; returns the reference (dx, dw)."""
    from neuronx_distributed_training_amd.ops import rmsnorm

    y = rmsnorm(x, w, eps)
    xr = x.detach().float().clone().requires_grad_(True)
    wr = w.detach().float().clone().requires_grad_(True)
    ref = xr * torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + eps) * wr
    _close(y, ref, f"rmsnorm {what} y")
    g = torch.randn(y.shape, device="cuda", dtype=BF)
    y.backward(g)
    ref.backward(g.float())
    return xr.grad, wr.grad


def _dw_check(got, want, what):
    assert torch.isfinite(got.float()).all(), what
    rel = float((got.float() - want).abs().max() / want.abs().max())
    print(f"rmsnorm {what} dw: max|err|/max|ref| {rel:.5f}")
    assert rel < 0.01, f"{what}: dw rel err {rel}"


@pytest.mark.parametrize("n,h", [(1500, 4096), (5, 8), (3, 1032)])
def test_rmsnorm_row_stride_and_narrow_rows(ext, n, h):
    """N = 1500 > 1024 blocks: the backward strides over rows and flushes
    dw with atomics from every block. H = 8 / 1032: fewer vectors than
    threads, and H no multiple of 256 * 8."""
    torch.manual_seed(41)
    x = torch.randn(n, h, device="cuda", dtype=BF, requires_grad=True)
    w = torch.randn(h, device="cuda", dtype=BF, requires_grad=True)
    dx, dw = _rmsnorm_case(x, w, f"{n}x{h}")
    _close(x.grad, dx, f"rmsnorm {n}x{h} dx")
    _dw_check(w.grad, dw, f"{n}x{h}")


def test_rmsnorm_noncontiguous_3d_input(ext):
    """[s, b, h] made by a transpose, as the sequence-first model passes."""
    torch.manual_seed(42)
    b, s, h = 3, 37, 1032
    leaf = torch.randn(b, s, h, device="cuda", dtype=BF, requires_grad=True)
    w = torch.randn(h, device="cuda", dtype=BF, requires_grad=True)
    x = leaf.transpose(0, 1)
    assert not x.is_contiguous()
    dx, dw = _rmsnorm_case(x, w, "3-D transposed")
    _close(leaf.grad.transpose(0, 1), dx, "rmsnorm 3-D transposed dx")
    _dw_check(w.grad, dw, "3-D transposed")


def test_rmsnorm_fp32_weight_with_bf16_activations(ext):
    """RMSNorm's default weight dtype is fp32; the kernels read bf16. The op
    casts the weight for the kernel and returns its gradient in fp32."""
    from neuronx_distributed_training_amd.ops.rmsnorm import RMSNorm

    torch.manual_seed(43)
    n, h = 70, 1032
    mod = RMSNorm(h).cuda()
    assert mod.weight.dtype == F32
    with torch.no_grad():
        # bf16-representable values: the cast itself adds no error here
        mod.weight.copy_(torch.randn(h, device="cuda").to(BF).float())
    x = torch.randn(n, h, device="cuda", dtype=BF, requires_grad=True)
    y = mod(x)
    assert y.dtype == BF
    xr = x.detach().float().requires_grad_(True)
    wr = mod.weight.detach().clone().requires_grad_(True)
    ref = xr * torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + 1e-5) * wr
    _close(y, ref, "rmsnorm fp32-w y")
    g = torch.randn_like(y)
    y.backward(g)
    ref.backward(g.float())
    assert mod.weight.grad.dtype == F32
    _close(x.grad, xr.grad, "rmsnorm fp32-w dx")
    _dw_check(mod.weight.grad, wr.grad, "fp32-w")


# ----------------------------------------------------------------- SwiGLU
@pytest.mark.parametrize("n,i", [(2100, 8192), (1, 8)])
def test_swiglu_second_pass_and_saturation(ext, n, i):
    """2100 * 8192 / 8 = 2,150,400 vectors > 8192 * 256: the second
    grid-stride pass runs. Gates spread over +-60 saturate the sigmoid."""
    from neuronx_distributed_training_amd.ops import swiglu

    torch.manual_seed(44)
    gate = (torch.rand(n, i, device="cuda") * 120 - 60).to(BF)
    up = torch.randn(n, i, device="cuda").to(BF)
    gu = torch.cat([gate, up], dim=-1).requires_grad_(True)
    y = swiglu(gu)
    gur = gu.detach().float().requires_grad_(True)
    gr, ur = gur.chunk(2, dim=-1)
    ref = F.silu(gr) * ur
    _close(y, ref, f"swiglu {n}x{i} y")
    g = torch.randn_like(y)
    y.backward(g)
    ref.backward(g.float())
    _close(gu.grad, gur.grad, f"swiglu {n}x{i} dgu")


# ------------------------------------------------------------------- RoPE
def _rotate_half(t):
    t1, t2 = t.chunk(2, dim=-1)
    return torch.cat((-t2, t1), dim=-1)


@pytest.mark.parametrize("b,h,s,d,off,rows", [
    (2, 4, 96, 128, 0, 128),
    (2, 4, 96, 64, 0, 128),       # head_dim 64
    (2, 4, 96, 128, 37, 160),     # integer offset > 0
    (2, 8, 4200, 128, 0, 4224),   # 4,300,800 half-elements > 16384 * 256
])
def test_rope_fwd_bwd_strided_input(ext, b, h, s, d, off, rows):
    """Forward AND backward vs fp32 autograd of the table formula, input a
    permuted view of an [s, b, h*d] buffer (the fused QKV output); the
    largest case takes a second grid-stride pass. The result's storage must
    be [s, b, h, d]-contiguous: the attention path's zero-copy claim."""
    from neuronx_distributed_training_amd.ops.rope import (
        apply_rotary_pos_emb, build_rope_cache,
    )

    torch.manual_seed(45)
    cos, sin = build_rope_cache(rows, d, base=500000.0, device="cuda")
    leaf = torch.randn(s, b, h * d, device="cuda", dtype=BF,
                       requires_grad=True)
    x = leaf.view(s, b, h, d).permute(1, 2, 0, 3)
    assert not x.is_contiguous()
    y = apply_rotary_pos_emb(x, cos, sin, off)
    assert y.shape == (b, h, s, d)
    assert y.permute(2, 0, 1, 3).is_contiguous()

    xr = x.detach().float().requires_grad_(True)
    ref = xr * cos[off:off + s] + _rotate_half(xr) * sin[off:off + s]
    what = f"rope {(b, h, s, d)} off {off}"
    _close(y, ref, what + " y")
    g = torch.randn(b, h, s, d, device="cuda", dtype=BF)
    y.backward(g)
    ref.backward(g.float())
    got = leaf.grad.view(s, b, h, d).permute(1, 2, 0, 3)
    _close(got, xr.grad, what + " dx")


# ---------------------------------------------------------- cross-entropy
@pytest.mark.parametrize("n", [1, 37])
@pytest.mark.parametrize("v", [1001, 1004])
def test_ce_odd_vocab_shards(ext, v, n):
    """V % 8 != 0: rows are not 16-byte aligned, so the kernels must take
    the scalar path for the whole row. Three vocab shards of V columns each
    are combined as parallel/loss.py does over the TP group and compared
    with F.cross_entropy on the full fp32 row. Logits are scaled x30 with a
    large outlier in the last column; the targets include the four edges of
    the middle shard (vocab_start - 1, vocab_start, vocab_start + V - 1,
    vocab_start + V)."""
    torch.manual_seed(46)
    dev = "cuda"
    full = (torch.randn(n, 3 * v, device=dev) * 30).to(BF)
    full[::2, 2 * v - 1] = 250.0      # last column of the middle shard
    full[-1, 3 * v - 1] = 300.0       # last column of the row
    target = torch.randint(0, 3 * v, (n,), device=dev)
    edges = torch.tensor([v - 1, v, 2 * v - 1, 2 * v], device=dev)
    if n >= 4:
        target[:4] = edges
    else:
        target[0] = 2 * v - 1
    parts = [full[:, i * v:(i + 1) * v].contiguous() for i in range(3)]
    stats = [ext.ce_fwd(p, target, i * v) for i, p in enumerate(parts)]
    gmax = torch.stack([s[0] for s in stats]).max(0).values
    gsum = sum(s[1] * torch.exp(s[0] - gmax) for s in stats)
    tgt = sum(s[2] for s in stats)
    loss = gsum.log() + gmax - tgt

    ref_in = full.float().requires_grad_(True)
    ref = F.cross_entropy(ref_in, target, reduction="none")
    _close(loss, ref.detach(), f"ce V={v} N={n} loss", atol=2e-2, rtol=1e-3)
    # the middle shard's own statistics at its edges
    own = (target >= v) & (target < 2 * v)
    want_t = torch.where(own, full.float().gather(
        1, target[:, None]).squeeze(1), torch.zeros(n, device=dev))
    assert torch.equal(stats[1][2], want_t)

    go = torch.rand(n, device=dev) * 4 - 2
    dls = [ext.ce_bwd(p, target, gmax, gsum, go, i * v)
           for i, p in enumerate(parts)]
    ref.backward(go)
    got = torch.cat(dls, dim=1).float()
    assert torch.isfinite(got).all()
    err = float((got - ref_in.grad).abs().max())
    print(f"ce V={v} N={n} dlogits: max abs err {err:.3e}")
    assert err < 1.5e-2, err


def test_ce_edges_single_row_middle_shard(ext):
    """N = 1 rows for each of the four shard-edge targets (the N = 1 case
    above can hold only one of them)."""
    torch.manual_seed(47)
    v = 1001
    full = (torch.randn(4, 3 * v, device="cuda") * 30).to(BF)
    mid = full[:, v:2 * v]
    for row, t in enumerate((v - 1, v, 2 * v - 1, 2 * v)):
        part = mid[row:row + 1].contiguous()
        target = torch.tensor([t], device="cuda")
        lmax, lsum, tgt = ext.ce_fwd(part, target, v)
        pf = part.float()
        assert torch.equal(lmax, pf.max(1).values)
        _close(lmax + lsum.log(), torch.logsumexp(pf, dim=1),
               f"ce edge target {t} logsumexp", atol=2e-2, rtol=1e-3)
        inside = v <= t < 2 * v
        want = pf[0, t - v] if inside else torch.zeros((), device="cuda")
        assert float(tgt) == float(want), (t, float(tgt), float(want))
