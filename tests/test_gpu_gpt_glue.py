"""The Megatron GPT family's glue kernels on MI355X: LayerNorm (layernorm.hip)
and exact GELU / GEGLU (gelu.hip), against fp64 references evaluated on the
device from the same bf16 inputs.

Bounds (not measured; profiles/README_gpt_glue.md has the observed ratios).
The yardstick is torch's own fp32 evaluation of the same inputs before any
rounding to bf16, and E = max |yardstick - ref64| over the tensor, floored at
2^-24 max |ref64|:
  bf16 outputs       |out - ref| <= 2^-8 |ref| + 2 E   (half a bf16 ulp for the
                     one rounding, 2 E for another, equally good fp32 order;
                     GEGLU's y rounds twice: 2^-7)
  mean, rstd (fp32)  |out - ref| <= 2 E
  dw, db (fp32)      |out - ref| <= 4 E   (another summation order over rows)
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64


@pytest.fixture(scope="module")
def ext():
    from neuronx_distributed_training_amd import ops

    return ops.require_extension()  # fail loudly if the .so is missing


def _randn(seed, *shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _check(out, ref, yard, rel, k, what):
    """|out - ref| <= rel |ref| + k E, elementwise; prints err / bound."""
    assert out.shape == ref.shape and torch.isfinite(out).all(), what
    e = max((yard.double() - ref).abs().max(), 2.0 ** -24 * ref.abs().max())
    ratio = ((out.double() - ref).abs() / (rel * ref.abs() + k * e)).max()
    print(f"{what}: err/bound {float(ratio):.3f}")
    assert ratio <= 1.0, f"{what}: err/bound {float(ratio):.3f}"


# ----------------------------------------------------------------- LayerNorm
_LN = {}


def _ln_eval(x, w, b, dy, eps, dt):
    xr, wr, br = (t.to(dt).requires_grad_(True) for t in (x, w, b))
    y, mean, rstd = torch.native_layer_norm(xr, (x.shape[1],), wr, br, eps)
    dx, dw, db = torch.autograd.grad(y, (xr, wr, br), dy.to(dt))
    return dict(y=y.detach(), mean=mean.detach().flatten(),
                rstd=rstd.detach().flatten(), dx=dx, dw=dw, db=db)


def _ln_case(n, h, eps):
    """Inputs, fp64 reference and fp32 yardstick, once per case."""
    if (n, h, eps) not in _LN:
        x = _randn(10 + n, n, h, scale=2.0)
        x[n // 2] += 300.0  # E[x^2] - mean^2 loses this row's variance in fp32
        x, w, b, dy = (t.to(BF).to(DEV) for t in (
            x, _randn(11 + n, h), _randn(12 + n, h), _randn(13 + n, n, h)))
        _LN[(n, h, eps)] = (x, w, b, dy, _ln_eval(x, w, b, dy, eps, F64),
                            _ln_eval(x, w, b, dy, eps, F32))
    return _LN[(n, h, eps)]


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("n,h", [
    (5, 8),          # one vector per row, 63 idle lanes
    (3, 1032),       # wave form, unequal vector counts, fewer rows than waves
    (37, 2048),      # wave form full, N no multiple of 4
    (1500, 256),     # hundreds of blocks: the partial-sum workspace at work
    (2100, 64),      # wave form: more rows than 2 blocks per CU take at once
    (9, 4096),       # block-per-row register form
    (600, 4096),     # block form: more rows than 2 blocks per CU
    (2, 16384),      # looped form
])
def test_layernorm_kernels(ext, n, h, eps):
    x, w, b, dy, ref, yard = _ln_case(n, h, eps)
    what = f"layernorm {n}x{h} eps {eps:g}"
    runs = []
    for _ in range(2):
        y, mean, rstd = ext.layernorm_fwd(x, w, b, eps)
        dx, dw, db = ext.layernorm_bwd(dy, x, w, mean, rstd)
        runs.append(dict(y=y, mean=mean, rstd=rstd, dx=dx, dw=dw, db=db))
    got = runs[0]
    for name, rel, k in (("y", 2.0 ** -8, 2), ("dx", 2.0 ** -8, 2),
                         ("mean", 0, 2), ("rstd", 0, 2), ("dw", 0, 4),
                         ("db", 0, 4)):
        assert got[name].dtype == (BF if rel else F32), name
        _check(got[name], ref[name], yard[name], rel, k, f"{what} {name}")
        assert torch.equal(got[name], runs[1][name]), f"{what} {name} rerun"


def test_layernorm_binding_contracts(ext):
    x = torch.randn(4, 64, device=DEV).to(BF)
    w = torch.ones(64, device=DEV, dtype=BF)
    y, mean, rstd = ext.layernorm_fwd(x, w, w, 1e-5)
    x60 = x[:, :60].contiguous()
    for fn, args in (
        (ext.layernorm_fwd, (x.float(), w, w, 1e-5)),
        (ext.layernorm_fwd, (x.cpu(), w, w, 1e-5)),
        (ext.layernorm_fwd, (x.t(), w, w, 1e-5)),
        (ext.layernorm_fwd, (x, w[:56], w, 1e-5)),
        (ext.layernorm_fwd, (x, w, w.float(), 1e-5)),
        (ext.layernorm_fwd, (x60, w[:60], w[:60], 1e-5)),
        (ext.layernorm_bwd, (x[:3], x, w, mean, rstd)),
        (ext.layernorm_bwd, (x, x, w, mean.to(BF), rstd)),
        (ext.layernorm_bwd, (x, x, w, mean, rstd[:3])),
        (ext.gelu_fwd, (x.float(),)), (ext.gelu_bwd, (x, x60)),
        (ext.geglu_fwd, (x[:, :24].contiguous(),)),
        (ext.geglu_bwd, (x, x)), (ext.geglu_bwd, (x[:, :32].cpu(), x)),
    ):
        with pytest.raises(RuntimeError):
            fn(*args)
    e = torch.empty(0, 64, device=DEV, dtype=BF)
    y0, m0, r0 = ext.layernorm_fwd(e, w, w, 1e-5)
    dx0, dw0, db0 = ext.layernorm_bwd(e, e, w, m0, r0)
    assert y0.shape == dx0.shape == (0, 64) and m0.shape == r0.shape == (0,)
    assert dw0.shape == db0.shape == (64,) and not dw0.any() and not db0.any()
    assert ext.gelu_fwd(e).shape == ext.gelu_bwd(e, e).shape == (0, 64)
    assert ext.geglu_fwd(e).shape == (0, 32)
    assert ext.geglu_bwd(e[:, :32], e).shape == (0, 64)
    torch.cuda.synchronize()


# -------------------------------------------------------------- GELU / GEGLU
def _act_eval(fn, x, dy, dt):
    xr = x.to(dt).requires_grad_(True)
    y = fn(xr)
    return y.detach(), torch.autograd.grad(y, xr, dy.to(dt))[0]


def _geglu_torch(gu):
    g, u = gu.chunk(2, dim=-1)
    return F.gelu(g) * u


@pytest.mark.parametrize("n,i", [(3, 8), (7, 1032), (129, 4096)])
def test_gelu_kernels(ext, n, i):
    """Inputs scaled by 3: both erf tails and the region near 0 occur."""
    x = _randn(20 + n, n, i, scale=3.0).to(BF).to(DEV)
    gu = _randn(21 + n, n, 2 * i, scale=3.0).to(BF).to(DEV)
    dy = _randn(22 + n, n, i).to(BF).to(DEV)
    for name, fn, inp, fwd, bwd, rel_y in (
            ("gelu", F.gelu, x, ext.gelu_fwd, ext.gelu_bwd, 2.0 ** -8),
            ("geglu", _geglu_torch, gu, ext.geglu_fwd, ext.geglu_bwd,
             2.0 ** -7)):
        (ry, rd), (yy, yd) = (_act_eval(fn, inp, dy, dt) for dt in (F64, F32))
        y, d = fwd(inp), bwd(dy, inp)
        assert y.dtype == BF and d.dtype == BF
        _check(y, ry, yy, rel_y, 2, f"{name} {n}x{i} y")
        _check(d, rd, yd, 2.0 ** -8, 2, f"{name} {n}x{i} dx")
        assert torch.equal(y, fwd(inp)) and torch.equal(d, bwd(dy, inp))


# ------------------------------------------------------------------ the ops
@pytest.mark.parametrize("pdtype", [BF, F32], ids=["p_bf16", "p_fp32"])
def test_ops_autograd(ext, pdtype):
    """ops.layernorm / gelu / geglu on [2, 5, H] tensors through backward():
    the bindings' results, parameter gradients in the parameters' dtypes; an
    fp32 GPU input takes the torch path bit for bit."""
    from neuronx_distributed_training_amd import ops

    n, h = 10, 264
    x, gu = (_randn(s, 2, 5, c).to(BF).to(DEV) for s, c in ((30, h), (31, 2 * h)))
    w, b = (_randn(s, h).to(BF).to(DEV) for s in (32, 33))
    dy = _randn(34, 2, 5, h).to(BF).to(DEV)
    xl = x.clone().requires_grad_(True)
    wl, bl = (t.to(pdtype).requires_grad_(True) for t in (w, b))
    y = ops.layernorm(xl, wl, bl, 1e-5)
    y.backward(dy)
    y0, mean, rstd = ext.layernorm_fwd(x.view(n, h), w, b, 1e-5)
    dx0, dw0, db0 = ext.layernorm_bwd(dy.view(n, h), x.view(n, h), w, mean, rstd)
    assert torch.equal(y, y0.view(2, 5, h)) and torch.equal(xl.grad, dx0.view(2, 5, h))
    assert wl.grad.dtype == pdtype and torch.equal(wl.grad, dw0.to(pdtype))
    assert bl.grad.dtype == pdtype and torch.equal(bl.grad, db0.to(pdtype))
    for op, inp, fwd, bwd in ((ops.gelu, x, ext.gelu_fwd, ext.gelu_bwd),
                              (ops.geglu, gu, ext.geglu_fwd, ext.geglu_bwd)):
        il = inp.clone().requires_grad_(True)
        out = op(il)
        out.backward(dy)
        flat = inp.view(n, -1)
        assert torch.equal(out, fwd(flat).view(2, 5, h))
        assert torch.equal(il.grad, bwd(dy.view(n, h), flat).view(inp.shape))
    xf, wf, bf = x.float(), w.float(), b.float()
    assert torch.equal(ops.layernorm(xf, wf, bf, 1e-5),
                       F.layer_norm(xf, (h,), wf, bf, 1e-5))
    assert torch.equal(ops.gelu(xf), F.gelu(xf))
    assert torch.equal(ops.geglu(gu.float()), _geglu_torch(gu.float()))


@pytest.mark.parametrize("block,act", [("post_ln", "gelu"),
                                       ("normformer", "geglu")])
def test_gpt_layer_uses_kernels(ext, block, act, monkeypatch):
    """A 2-layer GPTModel per arm of NXDT_GPT_GLUE. On: every norm and MLP
    activation is a kernel call; off: none is. The loss agrees within one
    bf16 ulp of the torch arm (rtol 2^-7). The final norm's weight gradient is
    a bf16-rounded sum over 128 rows whose terms differ between the arms by
    the bf16 roundings (2^-8 relative each, random in sign) of the
    activations upstream: 2^-6 relative plus 2^-7 of the largest entry."""
    from neuronx_distributed_training_amd.models.megatron_gpt import (
        GPTConfig, GPTModel,
    )
    from neuronx_distributed_training_amd.parallel import state as ps

    calls = {}
    for name in ("layernorm_fwd", "layernorm_bwd", f"{act}_fwd", f"{act}_bwd"):
        def spy(*a, _real=getattr(ext, name), _name=name, **kw):
            calls[_name] = calls.get(_name, 0) + 1
            return _real(*a, **kw)

        monkeypatch.setattr(ext, name, spy)
    ps.destroy_model_parallel()
    torch.manual_seed(0)
    cfg = GPTConfig(vocab_size=512, hidden_size=256, num_layers=2,
                    num_attention_heads=4, max_position_embeddings=64,
                    normalization="layernorm", activation=act,
                    transformer_block_type=block, dtype="bfloat16")
    model = GPTModel(cfg).to(DEV).train()
    assert isinstance(model.layers[0].input_layernorm, torch.nn.LayerNorm)
    ids = torch.randint(0, 512, (2, 64),
                        generator=torch.Generator().manual_seed(1)).to(DEV)
    out = {}
    for arm in ("0", "1"):
        monkeypatch.setenv("NXDT_GPT_GLUE", arm)
        model.zero_grad(set_to_none=True)
        calls.clear()
        loss = model(ids, labels=ids.clone())
        loss.backward()
        out[arm] = (loss.detach().float(),
                    model.final_layernorm.weight.grad.float().clone())
        norms = 2 * (3 if block == "normformer" else 2) + 1
        assert calls == ({} if arm == "0" else {
            "layernorm_fwd": norms, "layernorm_bwd": norms,
            f"{act}_fwd": 2, f"{act}_bwd": 2}), (arm, calls)
    (l0, g0), (l1, g1) = out["0"], out["1"]
    assert torch.isfinite(l1) and abs(l1 - l0) <= 2.0 ** -7 * abs(l0), (l0, l1)
    bound = 2.0 ** -6 * g0.abs() + 2.0 ** -7 * g0.abs().max()
    assert ((g1 - g0).abs() <= bound).all(), ((g1 - g0).abs() / bound).max()
