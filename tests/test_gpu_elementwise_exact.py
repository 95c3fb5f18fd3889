"""RMSNorm, SwiGLU, RoPE and vocab-parallel cross-entropy HIP kernels on
MI355X against the fp64 references of elementwise_ref.py, to rounding-level
bounds: every bf16 output within half a bf16 ulp of the reference plus a
counted number of fp32 roundings, every fp32 output within those roundings
alone (the bounds, and why, are in elementwise_ref.py's docstring; their CPU
checks in test_elementwise_ref.py). Every case prints its worst err / tol
before asserting, asserts that the bound is sharp for its inputs and that
every output element is finite, and runs each kernel twice: apart from
RMSNorm's dw (cross-block atomics) the two runs must be bit-equal.

The references are computed in fp64 on the device from the same bf16 inputs;
the inputs come from elementwise_ref.py's seeded CPU generators.

Also here: the host-side argument contracts of the eleven bindings of these
kernels (each violation a RuntimeError before any launch, the inputs
unchanged), the torch path the Python wrappers take for GPU tensors that are
not bf16, and N = 0 calls."""

import pytest
import torch

from tests import elementwise_ref as R
from tests.elementwise_ref import BF, F32, F64

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ext():
    from neuronx_distributed_training_amd import ops

    return ops.require_extension()  # fail loudly if the .so is missing


def _same(a, b, what):
    """Bit-equality of two runs (NaN-free by the comparator's own check)."""
    for i, (s, t) in enumerate(zip(a, b)):
        assert torch.equal(s, t), f"{what}: output {i} differs between runs"


# ------------------------------------------------------------------ RMSNorm
_RMS = {}


def _rms_case(n, h, eps):
    """Inputs and fp64 reference, once per (shape, eps)."""
    if (n, h, eps) not in _RMS:
        x, w, dy = R.rmsnorm_inputs(n, h, 100 + n, DEV)
        _RMS[(n, h, eps)] = (x, w, dy, R.rmsnorm_ref(x, w, dy, eps))
    return _RMS[(n, h, eps)]


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("n,h", [(5, 8), (3, 1032), (37, 4096), (1500, 256),
                                 (2, 16384)])
def test_rmsnorm_kernels(ext, n, h, eps):
    """The two kernels through their bindings. (1500, 256): the backward's
    row loop and atomic flush run past 1024 blocks; (2, 16384), the 405B
    hidden size: (H + 4) * 4 = 65552 bytes of dynamic LDS, just past 64 KiB.
    dw comes back in fp32 and is held to the fp32 bound."""
    x, w, dy, ref = _rms_case(n, h, eps)
    what = f"rmsnorm {n}x{h} eps {eps:g}"
    y, inv = ext.rmsnorm_fwd(x, w, eps)
    dx, dw = ext.rmsnorm_bwd(dy, x, w, inv)
    assert y.dtype == BF and dx.dtype == BF
    assert inv.dtype == F32 and dw.dtype == F32
    R.check_rmsnorm(ref, what, y=y, invrms=inv, dx=dx, dw=dw)
    y2, inv2 = ext.rmsnorm_fwd(x, w, eps)
    dx2, dw2 = ext.rmsnorm_bwd(dy, x, w, inv2)
    _same((y, inv, dx), (y2, inv2, dx2), what)
    R.check_rmsnorm(ref, what + " run 2", dw=dw2)


@pytest.mark.parametrize("wdtype", [BF, F32], ids=["w_bf16", "w_fp32"])
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("n,h", [(5, 8), (3, 1032), (37, 4096), (1500, 256),
                                 (2, 16384)])
def test_rmsnorm_op(ext, n, h, eps, wdtype):
    """ops.rmsnorm with a bf16 and with an fp32 weight (RMSNorm's default;
    the values are bf16-representable, so the cast for the kernel is exact).
    The weight's gradient comes back in the weight's dtype: rounded once to
    bf16 for a bf16 weight, the kernel's fp32 sum itself for an fp32 one."""
    from neuronx_distributed_training_amd.ops import rmsnorm

    x, w, dy, ref = _rms_case(n, h, eps)
    what = f"rmsnorm op {n}x{h} eps {eps:g} w {wdtype}"
    xl = x.clone().requires_grad_(True)
    wl = w.clone().to(wdtype).requires_grad_(True)
    y = rmsnorm(xl, wl, eps)
    y.backward(dy)
    assert y.dtype == BF and xl.grad.dtype == BF and wl.grad.dtype == wdtype
    R.check_rmsnorm(ref, what, y=y, dx=xl.grad, dw=wl.grad)
    yk, inv = ext.rmsnorm_fwd(x, w, eps)
    _same((y, xl.grad), (yk, ext.rmsnorm_bwd(dy, x, w, inv)[0]), what)


# ------------------------------------------------------------------- SwiGLU
@pytest.mark.parametrize("n,i", [(4, 8), (3, 1032), (2100, 8192)])
def test_swiglu_kernels(ext, n, i):
    """(2100, 8192): 2,150,400 vectors > 8192 * 256, the second grid-stride
    pass. Gates: 3 randn, a linspace(-90, 90) row, +-1e4, +-0, and the bf16
    neighbours of the zero of dsilu near -1.278."""
    from neuronx_distributed_training_amd.ops import swiglu

    gu, dy = R.swiglu_inputs(n, i, 200 + n, DEV)
    ref = R.swiglu_ref(gu, dy)
    what = f"swiglu {n}x{i}"
    y = ext.swiglu_fwd(gu)
    dgu = ext.swiglu_bwd(dy, gu)
    assert y.shape == (n, i) and dgu.shape == (n, 2 * i)
    R.check_swiglu(ref, what, y=y, dgate=dgu[:, :i], dup=dgu[:, i:])
    _same((y, dgu), (ext.swiglu_fwd(gu), ext.swiglu_bwd(dy, gu)), what)
    if n * i < 10000:   # the op is the same two calls
        gl = gu.clone().requires_grad_(True)
        yo = swiglu(gl)
        yo.backward(dy)
        _same((y, dgu), (yo, gl.grad), what + " op")


# --------------------------------------------------------------------- RoPE
def _qkv_view(s, b, h, d, seed):
    """q of a fused [s, b, 3 * h * d] QKV buffer as a [b, h, s, d] view."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.randn(s, b, 3 * h * d, generator=g).to(BF).to(DEV)
    x = buf[:, :, :h * d].view(s, b, h, d).permute(1, 2, 0, 3)
    assert not x.is_contiguous() and x.stride(3) == 1
    return x


@pytest.mark.parametrize("d,off,off2", [
    (128, 0, -1), (64, 0, -1), (128, 37, -1), (128, 96, 896), (64, 96, 896)])
def test_rope_fwd_random_tables(ext, d, off, off2):
    """The elementwise contract with independent values in all D columns of
    both tables (the real tables' two halves are equal and hide a read from
    the wrong half), on a strided fused-QKV view; single offset and zigzag."""
    b, h, s = 2, 4, 96
    x = _qkv_view(s, b, h, d, 300 + d)
    cos, sin = R.rope_random_tables(1024, d, 301, DEV)
    what = f"rope D={d} off {off}/{off2} random tables"
    y = ext.rope_fwd(x, cos, sin, off, off2)
    assert y.shape == (b, h, s, d) and y.permute(2, 0, 1, 3).is_contiguous()
    R.check_rope(R.rope_fwd_ref(x, cos, sin, off, off2), y, what)
    _same((y,), (ext.rope_fwd(x, cos, sin, off, off2),), what)


@pytest.mark.parametrize("b,h,s,d,off,rows", [
    (2, 4, 96, 128, 0, 128),
    (2, 4, 96, 64, 0, 128),
    (2, 4, 96, 128, 37, 160),
    (2, 8, 4200, 128, 0, 4224),      # second grid-stride pass
    (2, 4, 96, 128, (96, 896), 1024),  # zigzag, backward included
    (2, 4, 96, 64, (96, 896), 1024),
])
def test_rope_op_real_tables(ext, b, h, s, d, off, rows):
    """Forward and backward of apply_rotary_pos_emb with the model's tables
    at the shapes of test_rope_fwd_bwd_strided_input, plus the zigzag
    backward. The backward is the kernel run with -sin, the transpose of the
    forward map for tables whose halves agree."""
    from neuronx_distributed_training_amd.ops.rope import apply_rotary_pos_emb

    cos, sin = R.rope_real_tables(rows, d, device=DEV)
    g = torch.Generator().manual_seed(310)
    leaf = torch.randn(s, b, h * d, generator=g).to(BF).to(DEV)
    leaf.requires_grad_(True)
    dy = torch.randn(b, h, s, d, generator=g).to(BF).to(DEV)
    x = leaf.view(s, b, h, d).permute(1, 2, 0, 3)
    o, o2 = off if isinstance(off, tuple) else (off, -1)
    what = f"rope op {(b, h, s, d)} off {off}"
    y = apply_rotary_pos_emb(x, cos, sin, off)
    assert y.permute(2, 0, 1, 3).is_contiguous()
    R.check_rope(R.rope_fwd_ref(x, cos, sin, o, o2), y, what + " y")
    y.backward(dy)
    dx = leaf.grad.view(s, b, h, d).permute(1, 2, 0, 3)
    R.check_rope(R.rope_bwd_ref(dy, cos, sin, o, o2), dx, what + " dx")
    _same((y.detach(),), (ext.rope_fwd(x.detach(), cos, sin, o, o2),), what)
    _same((dx,), (ext.rope_fwd(dy, cos, -sin, o, o2),), what + " bwd")


# ------------------------------------------------------------ cross-entropy
def _ce_run(ext, full, target, gout, shards):
    """Per-shard forward, the combination parallel/loss.py makes over the TP
    group, per-shard backward."""
    v = full.size(1) // shards
    parts = [full[:, i * v:(i + 1) * v].contiguous() for i in range(shards)]
    stats = [ext.ce_fwd(p, target, i * v) for i, p in enumerate(parts)]
    gmax = torch.stack([s[0] for s in stats]).max(0).values
    gsum = sum(s[1] * torch.exp(s[0] - gmax) for s in stats)
    loss = gsum.log() + gmax - sum(s[2] for s in stats)
    dl = torch.cat([ext.ce_bwd(p, target, gmax, gsum, gout, i * v)
                    for i, p in enumerate(parts)], dim=1)
    return stats, loss, dl


@pytest.mark.parametrize("shards", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("v", [8, 255, 1001, 2056, 16032])
def test_ce_kernels(ext, v, n, shards):
    """V % 8 != 0 takes the scalar loop for the whole row, V = 8 leaves 255
    threads without a column, V = 16032 is the TP = 8 Llama-3 shard. Logits
    4 randn with a 60.0 outlier in a shard's last column and four -inf
    padding columns; targets on the shard edges and one -100, for which the
    loss is the lse and dlogits softmax times gout."""
    full, target, gout = R.ce_inputs(n, v, shards, 400 + v, DEV)
    ref = R.ce_ref(full, target, gout, shards)
    what = f"ce V={v} N={n} x{shards}"
    stats, loss, dl = _ce_run(ext, full, target, gout, shards)
    for i, s in enumerate(stats):
        R.check_ce_stats(ref, i, what, *s)
    R.check_ce_loss(ref, loss, what)
    R.check_ce_dlogits(ref, dl, what)
    stats2, loss2, dl2 = _ce_run(ext, full, target, gout, shards)
    _same([t for s in stats for t in s] + [loss, dl],
          [t for s in stats2 for t in s] + [loss2, dl2], what)


@pytest.mark.parametrize("sliced", [False, True], ids=["dense", "sliced"])
@pytest.mark.parametrize("v", [1001, 2056])
def test_parallel_cross_entropy_tp1(ext, v, sliced):
    """The same through parallel_cross_entropy at tp = 1. `sliced`: the
    logits are buf[..., :V] of a wider buffer, whose reshape(-1, V) is a
    strided view; forward and backward must both see the contiguous copy."""
    from neuronx_distributed_training_amd.parallel.loss import (
        parallel_cross_entropy,
    )

    n = 5
    full, target, gout = R.ce_inputs(n, v, 1, 410 + v, DEV)
    ref = R.ce_ref(full, target, gout, 1)
    what = f"parallel_cross_entropy V={v} {'sliced' if sliced else 'dense'}"
    if sliced:
        leaf = torch.zeros(n, v + 24, device=DEV, dtype=BF)
        leaf[:, :v] = full
        leaf[:, v:] = 7.0
        leaf.requires_grad_(True)
        logits = leaf[..., :v]
        assert not logits.reshape(-1, v).is_contiguous()
    else:
        leaf = full.clone().requires_grad_(True)
        logits = leaf
    loss = parallel_cross_entropy(logits, target)
    R.check_ce_loss(ref, loss, what)
    loss.backward(gout)
    R.check_ce_dlogits(ref, leaf.grad[:, :v], what)
    assert not leaf.grad[:, v:].any()


def test_logprobs_from_parallel_logits(ext):
    """from_parallel_logits_to_logprobs at b = 2, s = 9: logprobs of
    target[:, 1:] under logits[:, :-1], a strided slice."""
    from neuronx_distributed_training_amd.parallel.loss import (
        from_parallel_logits_to_logprobs,
    )

    b, s, v = 2, 9, 1001
    full, target, gout = R.ce_inputs(b * (s - 1), v, 1, 420, DEV)
    ref = R.ce_ref(full, target, gout, 1)
    logits = torch.randn(b, s, v, device=DEV).to(BF)
    logits[:, :-1] = full.view(b, s - 1, v)
    tgt = torch.zeros(b, s, dtype=torch.long, device=DEV)
    tgt[:, 1:] = target.view(b, s - 1)
    logits.requires_grad_(True)
    lp = from_parallel_logits_to_logprobs(logits, tgt)
    assert lp.shape == (b, s - 1)
    R.check_ce_loss(ref, -lp.reshape(-1), "logprobs")
    lp.backward(-gout.view(b, s - 1))
    R.check_ce_dlogits(ref, logits.grad[:, :-1].reshape(-1, v), "logprobs")
    assert not logits.grad[:, -1].any()


# ---------------------------------------------------------------- contracts
def _rejects(fn, args, what):
    """fn(*args) raises RuntimeError before any launch: every tensor
    argument is bit-identical afterwards and the device is healthy."""
    before = [a.clone() if torch.is_tensor(a) else None for a in args]
    with pytest.raises(RuntimeError):
        fn(*args)
        pytest.fail(f"{what} was accepted")
    torch.cuda.synchronize()
    for a, c in zip(args, before):
        if c is not None:
            assert torch.equal(a, c), what


def test_swiglu_binding_contracts(ext):
    gu = torch.randn(4, 32, device=DEV).to(BF)
    dy = torch.randn(4, 16, device=DEV).to(BF)
    ext.swiglu_fwd(gu), ext.swiglu_bwd(dy, gu)
    wide = torch.randn(4, 64, device=DEV).to(BF)
    fwd = {
        "fp32": gu.float(), "fp16": gu.half(), "cpu": gu.cpu(),
        "strided": wide[:, ::2], "I % 8": gu[:, :24].contiguous(),
        "odd columns": wide[:, :17].contiguous(), "1-D": gu.reshape(-1),
        "3-D": gu.reshape(2, 2, 32),
    }
    for name, t in fwd.items():
        _rejects(ext.swiglu_fwd, (t,), f"swiglu_fwd gate_up {name}")
        if name not in ("1-D", "3-D"):
            _rejects(ext.swiglu_bwd, (dy, t), f"swiglu_bwd gate_up {name}")
    bwd = {
        "fp32": dy.float(), "fp16": dy.half(), "cpu": dy.cpu(),
        "strided": gu[:, ::2], "wide": gu[:, :24].contiguous(),
        "short": dy[:3].contiguous(), "1-D": dy.reshape(-1),
    }
    for name, t in bwd.items():
        _rejects(ext.swiglu_bwd, (t, gu), f"swiglu_bwd dy {name}")


def test_rmsnorm_binding_contracts(ext):
    x = torch.randn(4, 64, device=DEV).to(BF)
    w = torch.ones(64, device=DEV, dtype=BF)
    _, inv = ext.rmsnorm_fwd(x, w, 1e-5)
    ext.rmsnorm_bwd(x, x, w, inv)
    w72 = torch.ones(72, device=DEV, dtype=BF)
    for name, args in {
        "w numel": (x, w72, 1e-5), "x 3-D": (x.reshape(2, 2, 64), w, 1e-5),
        "x fp32": (x.float(), w, 1e-5), "w cpu": (x, w.cpu(), 1e-5),
        "H % 8": (x[:, :60].contiguous(), w[:60].contiguous(), 1e-5),
    }.items():
        _rejects(ext.rmsnorm_fwd, args, f"rmsnorm_fwd {name}")
    for name, args in {
        "dy fp32": (x.float(), x, w, inv), "x fp32": (x, x.float(), w, inv),
        "dy fp16": (x.half(), x, w, inv),
        "dy shape": (x[:3].contiguous(), x, w, inv),
        "dy cpu": (x.cpu(), x, w, inv),
        "dy strided": (torch.cat([x, x], 1)[:, ::2], x, w, inv),
        "w numel": (x, x, w72, inv),
        "invrms bf16": (x, x, w, inv.to(BF)),
        "invrms fp64": (x, x, w, inv.double()),
        "invrms cpu": (x, x, w, inv.cpu()),
        "invrms numel": (x, x, w, inv[:3].contiguous()),
        "invrms strided": (x, x, w, torch.cat([inv, inv])[::2]),
        "H % 8": (x[:, :60].contiguous(), x[:, :60].contiguous(),
                  w[:60].contiguous(), inv),
    }.items():
        _rejects(ext.rmsnorm_bwd, args, f"rmsnorm_bwd {name}")


def test_rope_binding_contracts(ext):
    x = torch.randn(1, 2, 8, 16, device=DEV).to(BF)
    cos, sin = R.rope_real_tables(32, 16, device=DEV)
    ext.rope_fwd(x, cos, sin, 24, -1)      # rows 24 .. 31: the last ones
    ext.rope_fwd(x, cos, sin, 0, 28)       # zigzag: rows 0 .. 3, 28 .. 31
    x7 = torch.randn(1, 2, 8, 7, device=DEV).to(BF)
    for name, args in {
        "x fp32": (x.float(), cos, sin, 0, -1),
        "x fp16": (x.half(), cos, sin, 0, -1),
        "x cpu": (x.cpu(), cos, sin, 0, -1),
        "cos fp64": (x, cos.double(), sin, 0, -1),
        "sin fp64": (x, cos, sin.double(), 0, -1),
        "sin bf16": (x, cos, sin.to(BF), 0, -1),
        "cos cpu": (x, cos.cpu(), sin, 0, -1),
        "sin cpu": (x, cos, sin.cpu(), 0, -1),
        "too few rows": (x, cos, sin, 25, -1),
        "cos too few rows": (x, cos[:31], sin, 24, -1),
        "sin too few rows": (x, cos, sin[:31], 24, -1),
        "zigzag second half too few rows": (x, cos, sin, 0, 29),
        "zigzag first half too few rows": (x, cos, sin, 29, 0),
        "negative offset": (x, cos, sin, -1, -1),
        "table width": (x, cos[:, :8], sin[:, :8], 0, -1),
        "table 1-D": (x, cos.reshape(-1), sin.reshape(-1), 0, -1),
        "odd D": (x7, cos[:, :7], sin[:, :7], 0, -1),
        "zigzag odd s": (x[:, :, :7], cos, sin, 0, 16),
    }.items():
        _rejects(ext.rope_fwd, args, f"rope_fwd {name}")


def test_ce_binding_contracts(ext):
    n, v = 4, 40
    lg = torch.randn(n, v, device=DEV).to(BF)
    t = torch.randint(0, v, (n,), device=DEV)
    lmax, lsum, _ = ext.ce_fwd(lg, t, 0)
    go = torch.ones(n, device=DEV)
    ext.ce_bwd(lg, t, lmax, lsum, go, 0)
    for name, args in {
        "targets cpu": (lg, t.cpu(), 0), "targets int32": (lg, t.int(), 0),
        "targets numel": (lg, t[:3], 0), "logits fp32": (lg.float(), t, 0),
        "logits strided": (torch.cat([lg, lg], 1)[:, ::2], t, 0),
        "logits cpu": (lg.cpu(), t, 0), "logits 1-D": (lg.reshape(-1), t, 0),
    }.items():
        _rejects(ext.ce_fwd, args, f"ce_fwd {name}")
    bad = {"logits fp32": (lg.float(), t, lmax, lsum, go, 0),
           "logits cpu": (lg.cpu(), t, lmax, lsum, go, 0),
           "targets cpu": (lg, t.cpu(), lmax, lsum, go, 0),
           "targets int32": (lg, t.int(), lmax, lsum, go, 0),
           "targets numel": (lg, t[:3], lmax, lsum, go, 0)}
    for pos, name in ((2, "gmax"), (3, "gsum"), (4, "gout")):
        for kind, f in (("fp64", lambda a: a.double()),
                        ("bf16", lambda a: a.to(BF)),
                        ("cpu", lambda a: a.cpu()),
                        ("numel", lambda a: a[:3]),
                        ("scalar", lambda a: a[0])):
            args = [lg, t, lmax, lsum, go, 0]
            args[pos] = f(args[pos])
            bad[f"{name} {kind}"] = tuple(args)
    for name, args in bad.items():
        _rejects(ext.ce_bwd, args, f"ce_bwd {name}")


# ------------------------------------------- GPU tensors that are not bf16
def test_fp32_gpu_tensors_take_the_torch_path(ext):
    """The kernels read bf16 only; the wrappers route every other GPU dtype
    to the torch formulas on the device (no kernel exists, so none is
    skipped). Checked against the fp64 reference of the fp32 inputs with the
    fp32 roundings alone: no half-ulp term."""
    from neuronx_distributed_training_amd.ops import rmsnorm, swiglu
    from neuronx_distributed_training_amd.ops.rope import apply_rotary_pos_emb

    g = torch.Generator().manual_seed(500)
    x = torch.randn(37, 1032, generator=g).to(DEV).requires_grad_(True)
    w = (1 + 0.3 * torch.randn(1032, generator=g)).to(DEV).requires_grad_(True)
    dy = torch.randn(37, 1032, generator=g).to(DEV)
    ref = R.rmsnorm_ref(x, w, dy, 1e-5)
    y = rmsnorm(x, w, 1e-5)
    y.backward(dy)
    assert y.dtype == F32 and x.grad.dtype == F32 and w.grad.dtype == F32
    R.assert_close(y, ref.y, "fp32 rmsnorm y", k=ref.k, half_ulp=False)
    R.assert_close(x.grad, ref.dx, "fp32 rmsnorm dx", A=ref.A_dx, k=ref.k,
                   half_ulp=False)
    R.assert_close(w.grad, ref.dw, "fp32 rmsnorm dw", A=ref.A_dw,
                   k=ref.n + ref.k, half_ulp=False)

    gu = (3 * torch.randn(3, 2064, generator=g)).to(DEV).requires_grad_(True)
    dyu = torch.randn(3, 1032, generator=g).to(DEV)
    sref = R.swiglu_ref(gu, dyu)
    ys = swiglu(gu)
    ys.backward(dyu)
    assert ys.dtype == F32
    R.assert_close(ys, sref.y, "fp32 swiglu y", k=sref.k, half_ulp=False)
    R.assert_close(gu.grad[:, :1032], sref.dgate, "fp32 swiglu dgate",
                   A=sref.A_dgate, k=sref.k, half_ulp=False)
    R.assert_close(gu.grad[:, 1032:], sref.dup, "fp32 swiglu dup", k=sref.k,
                   half_ulp=False)
    # fp16 has no kernel either and must not be read as bf16
    yh = swiglu(gu.detach().half())
    assert yh.dtype == torch.float16
    yd = ys.detach()
    assert bool(((yh.float() - yd).abs() <= 4e-3 * yd.abs() + 1e-3).all())

    cos, sin = R.rope_real_tables(160, 64, device=DEV)
    xr = torch.randn(2, 4, 96, 64, generator=g).to(DEV).requires_grad_(True)
    dyr = torch.randn(2, 4, 96, 64, generator=g).to(DEV)
    yr = apply_rotary_pos_emb(xr, cos, sin, 37)
    yr.backward(dyr)
    assert yr.dtype == F32
    rf = R.rope_fwd_ref(xr, cos, sin, 37)
    rb = R.rope_bwd_ref(dyr, cos, sin, 37)
    R.assert_close(yr, rf.y, "fp32 rope y", A=rf.A, k=4, half_ulp=False)
    R.assert_close(xr.grad, rb.y, "fp32 rope dx", A=rb.A, k=4, half_ulp=False)


# -------------------------------------------------------------------- N = 0
def test_empty_inputs_launch_nothing(ext):
    """N = 0 would be a grid of zero blocks, an invalid launch: the bindings
    return empty outputs without launching, and the device is healthy
    afterwards."""
    e = lambda *shape: torch.empty(*shape, device=DEV, dtype=BF)
    w = torch.ones(64, device=DEV, dtype=BF)
    y, inv = ext.rmsnorm_fwd(e(0, 64), w, 1e-5)
    assert y.shape == (0, 64) and inv.shape == (0,)
    dx, dw = ext.rmsnorm_bwd(e(0, 64), e(0, 64), w, inv)
    assert dx.shape == (0, 64) and dw.shape == (64,) and not dw.any()
    assert ext.swiglu_fwd(e(0, 32)).shape == (0, 16)
    assert ext.swiglu_bwd(e(0, 16), e(0, 32)).shape == (0, 32)
    cos, sin = R.rope_real_tables(8, 16, device=DEV)
    assert ext.rope_fwd(e(1, 2, 0, 16), cos, sin, 0, -1).shape == (1, 2, 0, 16)
    assert ext.rope_fwd(e(0, 2, 4, 16), cos, sin, 0, -1).shape == (0, 2, 4, 16)
    t = torch.empty(0, dtype=torch.long, device=DEV)
    stats = ext.ce_fwd(e(0, 40), t, 0)
    assert all(s.shape == (0,) for s in stats)
    f = torch.empty(0, device=DEV)
    assert ext.ce_bwd(e(0, 40), t, f, f, f, 0).shape == (0, 40)
    torch.cuda.synchronize()
    gu, dy = R.swiglu_inputs(4, 8, 600, DEV)
    R.check_swiglu(R.swiglu_ref(gu, dy), "after N = 0", y=ext.swiglu_fwd(gu))
    torch.cuda.synchronize()
