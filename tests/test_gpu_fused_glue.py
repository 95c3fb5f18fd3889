"""The fused decoder-layer glue on MI355X: residual add + RMSNorm in one
kernel each way (add_rmsnorm_fwd / add_rmsnorm_bwd) and RoPE of Q and K in one
launch (rope_fwd_pair), held bit for bit to the unfused calls they replace:
torch's bf16 add with rmsnorm_fwd / rmsnorm_bwd, and rope_fwd per tensor.

The one exception is the RMSNorm weight gradient: it comes from cross-block
atomics and is not bit-reproducible in the unfused kernel either, so it is
held to the fp32 bound of elementwise_ref.py (check_rmsnorm) instead.

rope_fwd_pair has no grid-stride loop (one thread per column pair and chunk of
eight head rows, the grid as large as that needs), so the s = 4200 case is a
grid of many blocks for the vector kernel; its misaligned twin takes the scalar
kernel past that kernel's own grid cap."""

import pytest
import torch

from tests import elementwise_ref as R
from tests.elementwise_ref import BF, F32

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ext():
    from neuronx_distributed_training_amd import ops

    return ops.require_extension()  # fail loudly if the .so is missing


def _eq(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    n = int((got != want).sum())
    assert torch.equal(got, want), f"{what}: {n} elements differ"


# ------------------------------------------------------- add + RMSNorm
_RMS = {}


def _rms_case(n, h, eps):
    """Inputs, the unfused results and the fp64 reference at h = x + delta,
    once per (shape, eps)."""
    if (n, h, eps) not in _RMS:
        x, w, dy = R.rmsnorm_inputs(n, h, 100 + n, DEV)
        g = torch.Generator().manual_seed(700 + n)
        delta = (x.cpu().float().abs().mean(1, keepdim=True)
                 * torch.randn(n, h, generator=g)).to(BF).to(DEV)
        dh = torch.randn(n, h, generator=g).to(BF).to(DEV)
        hs = torch.add(x, delta)
        _RMS[(n, h, eps)] = (x, delta, w, dy, dh, hs,
                             R.rmsnorm_ref(hs, w, dy, eps))
    return _RMS[(n, h, eps)]


@pytest.mark.parametrize("with_dh", [True, False], ids=["dh", "no_dh"])
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("n,h", [(5, 8), (3, 1032), (37, 4096), (1500, 256),
                                 (2, 16384)])
def test_add_rmsnorm_kernels(ext, n, h, eps, with_dh):
    """The shapes of test_rmsnorm_kernels, for its reasons; 4096 holds two
    vectors per thread in registers, 1032 leaves the second one to 1 thread,
    16384 takes the looped form."""
    x, delta, w, dy, dh, hs, ref = _rms_case(n, h, eps)
    what = f"add_rmsnorm {n}x{h} eps {eps:g} dh {with_dh}"
    y0, inv0 = ext.rmsnorm_fwd(hs, w, eps)
    dxn, _ = ext.rmsnorm_bwd(dy, hs, w, inv0)
    dx0 = torch.add(dh, dxn) if with_dh else dxn
    keep = [t.clone() for t in (x, delta, w, dy, dh)]
    runs = []
    for run in range(2):
        hh, y, inv = ext.add_rmsnorm_fwd(x, delta, w, eps)
        dx, dw = ext.add_rmsnorm_bwd(dy, dh if with_dh else None, hh, w, inv)
        assert inv.dtype == F32 and dw.dtype == F32 and dw.shape == (h,)
        for got, want, name in ((hh, hs, "h"), (y, y0, "y"),
                                (inv, inv0, "invrms"), (dx, dx0, "dx")):
            _eq(got, want, f"{what} run {run} {name}")
        R.check_rmsnorm(ref, f"{what} run {run}", dw=dw)
        runs.append((hh, y, inv, dx))
    for a, b in zip(*runs):
        assert torch.equal(a, b), what
    for t, c in zip((x, delta, w, dy, dh), keep):
        assert torch.equal(t, c), f"{what}: an input changed"


@pytest.mark.parametrize("wdtype", [BF, F32], ids=["w_bf16", "w_fp32"])
@pytest.mark.parametrize("n,h", [(3, 1032), (37, 4096)])
def test_add_rmsnorm_op(ext, n, h, wdtype, monkeypatch):
    """ops.rmsnorm.add_rmsnorm against x + delta followed by ops.rmsnorm,
    both outputs used downstream (so h carries a gradient of its own):
    outputs and input gradients bit-equal, the weight gradient in the
    weight's dtype and within the dw bound."""
    from neuronx_distributed_training_amd.ops.rmsnorm import add_rmsnorm, rmsnorm

    monkeypatch.delenv("NXDT_FUSED_GLUE", raising=False)
    eps = 1e-5
    x, delta, w, dy, dh, hs, ref = _rms_case(n, h, eps)
    what = f"add_rmsnorm op {n}x{h} w {wdtype}"

    def run(fused):
        xl, dl = (t.clone().requires_grad_(True) for t in (x, delta))
        wl = w.clone().to(wdtype).requires_grad_(True)
        if fused:
            hh, y = add_rmsnorm(xl.view(1, n, h), dl.view(1, n, h), wl, eps)
            hh, y = hh.view(n, h), y.view(n, h)
        else:
            hh = xl + dl
            y = rmsnorm(hh, wl, eps)
        torch.autograd.backward([hh, y], [dh, dy])
        return hh.detach(), y.detach(), xl.grad, dl.grad, wl.grad

    got, want = run(True), run(False)
    for g, t, name in zip(got[:4], want[:4], ("h", "y", "dx", "ddelta")):
        _eq(g, t, f"{what} {name}")
    assert got[4].dtype == wdtype
    R.check_rmsnorm(ref, what, dw=got[4])
    # NXDT_FUSED_GLUE=0 is the two ops themselves
    monkeypatch.setenv("NXDT_FUSED_GLUE", "0")
    off = add_rmsnorm(x, delta, w.to(wdtype), eps)
    _eq(off[0], want[0], what + " switch off h")
    _eq(off[1], want[1], what + " switch off y")
    monkeypatch.setenv("NXDT_FUSED_GLUE", "2")
    with pytest.raises(ValueError):
        add_rmsnorm(x, delta, w, eps)


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


def test_add_rmsnorm_binding_contracts(ext):
    x = torch.randn(4, 64, device=DEV).to(BF)
    w = torch.ones(64, device=DEV, dtype=BF)
    h, _, inv = ext.add_rmsnorm_fwd(x, x, w, 1e-5)
    ext.add_rmsnorm_bwd(x, x, h, w, inv)
    w72 = torch.ones(72, device=DEV, dtype=BF)
    x60 = x[:, :60].contiguous()
    wide = torch.cat([x, x], 1)[:, ::2]
    for name, args in {
        "x fp32": (x.float(), x, w, 1e-5), "delta fp32": (x, x.float(), w, 1e-5),
        "delta fp16": (x, x.half(), w, 1e-5), "delta cpu": (x, x.cpu(), w, 1e-5),
        "x cpu": (x.cpu(), x, w, 1e-5),
        "delta shape": (x, x[:3].contiguous(), w, 1e-5),
        "delta strided": (x, wide, w, 1e-5), "x strided": (wide, x, w, 1e-5),
        "x 3-D": (x.reshape(2, 2, 64), x.reshape(2, 2, 64), w, 1e-5),
        "w numel": (x, x, w72, 1e-5), "w fp32": (x, x, w.float(), 1e-5),
        "w cpu": (x, x, w.cpu(), 1e-5),
        "H % 8": (x60, x60, w[:60].contiguous(), 1e-5),
    }.items():
        _rejects(ext.add_rmsnorm_fwd, args, f"add_rmsnorm_fwd {name}")
    for name, args in {
        "dy fp32": (x.float(), x, h, w, inv), "dh fp32": (x, x.float(), h, w, inv),
        "h fp32": (x, x, h.float(), w, inv), "dy cpu": (x.cpu(), x, h, w, inv),
        "dh cpu": (x, x.cpu(), h, w, inv),
        "dy shape": (x[:3].contiguous(), x, h, w, inv),
        "dh shape": (x, x[:3].contiguous(), h, w, inv),
        "dy strided": (wide, x, h, w, inv), "dh strided": (x, wide, h, w, inv),
        "h 3-D": (x, None, h.reshape(2, 2, 64), w, inv),
        "w numel": (x, x, h, w72, inv), "w fp32": (x, None, h, w.float(), inv),
        "invrms bf16": (x, x, h, w, inv.to(BF)),
        "invrms cpu": (x, None, h, w, inv.cpu()),
        "invrms numel": (x, x, h, w, inv[:3].contiguous()),
        "invrms strided": (x, x, h, w, torch.cat([inv, inv])[::2]),
        "H % 8": (x60, None, x60, w[:60].contiguous(), inv),
    }.items():
        _rejects(ext.add_rmsnorm_bwd, args, f"add_rmsnorm_bwd {name}")
    e = torch.empty(0, 64, device=DEV, dtype=BF)
    h0, y0, i0 = ext.add_rmsnorm_fwd(e, e, w, 1e-5)
    assert h0.shape == (0, 64) and y0.shape == (0, 64) and i0.shape == (0,)
    dx0, dw0 = ext.add_rmsnorm_bwd(e, None, e, w, i0)
    assert dx0.shape == (0, 64) and dw0.shape == (64,) and not dw0.any()
    torch.cuda.synchronize()


# ------------------------------------------------------------ RoPE pair
def _qk_views(layout, s, b, hq, hkv, d, seed, shift=0):
    """q [b, hq, s, d] and k [b, hkv, s, d] views. "split": q from an
    [s, b, hq d] buffer and k from the [s, b, 2 hkv d] kv buffer (different
    row strides); "fused": both from one [s, b, (hq + 2 hkv) d] QKV buffer.
    shift offsets both base pointers by that many elements."""
    g = torch.Generator().manual_seed(seed)

    def buf(width):
        t = torch.randn(s * b * width + shift, generator=g).to(BF).to(DEV)
        return t[shift:].view(s, b, width)

    if layout == "split":
        qb, kb = buf(hq * d), buf(2 * hkv * d)
        q, k = qb, kb[:, :, :hkv * d]
    else:
        qkv = buf((hq + 2 * hkv) * d)
        q, k = qkv[:, :, :hq * d], qkv[:, :, hq * d:(hq + hkv) * d]
    q = q.reshape(s, b, hq, d) if q.is_contiguous() else q.view(s, b, hq, d)
    k = k.view(s, b, hkv, d)
    return q.permute(1, 2, 0, 3), k.permute(1, 2, 0, 3)


def _pair_matches(ext, q, k, cos, sin, off, off2, what):
    for sign in (1.0, -1.0):
        tab = sin if sign > 0 else -sin
        wq = ext.rope_fwd(q, cos, tab, off, off2)
        wk = ext.rope_fwd(k, cos, tab, off, off2)
        for run in range(2):
            yq, yk = ext.rope_fwd_pair(q, k, cos, sin, off, off2, sign)
            assert yq.permute(2, 0, 1, 3).is_contiguous()
            assert yk.permute(2, 0, 1, 3).is_contiguous()
            _eq(yq, wq, f"{what} sign {sign:+.0f} run {run} q")
            _eq(yk, wk, f"{what} sign {sign:+.0f} run {run} k")


@pytest.mark.parametrize("tables", ["random", "real"])
@pytest.mark.parametrize("layout", ["split", "fused"])
@pytest.mark.parametrize("off,off2", [(0, -1), (37, -1), (96, 896)])
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("hq,hkv", [(4, 1), (4, 2), (4, 4)])
def test_rope_pair_matches_rope_fwd(ext, hq, hkv, d, off, off2, layout,
                                    tables):
    """Random tables hold independent values in all D columns of both
    tables, so a read from the wrong half shows; 5 to 8 head rows: one chunk
    that ends early, or a full one, with q and k rows mixed inside it."""
    b, s = 2, 96
    q, k = _qk_views(layout, s, b, hq, hkv, d, 800 + hq + hkv + d)
    cos, sin = (R.rope_random_tables(1024, d, 801, DEV) if tables == "random"
                else R.rope_real_tables(1024, d, device=DEV))
    _pair_matches(ext, q, k, cos, sin, off, off2,
                  f"rope pair {hq}/{hkv} D={d} off {off}/{off2} {layout} "
                  f"{tables}")


@pytest.mark.parametrize("shift", [0, 4], ids=["vector", "scalar"])
def test_rope_pair_long_sequence(ext, shift):
    """s 4200, hq 8, hkv 2: two head chunks per (s, b) and 525 blocks in the
    vector kernel; with the base pointers off by 4 elements the scalar
    kernel runs instead and takes its second grid-stride pass for q."""
    q, k = _qk_views("split", 4200, 2, 8, 2, 128, 810, shift)
    assert q.data_ptr() % 16 == (8 if shift else 0)
    cos, sin = R.rope_random_tables(4224, 128, 811, DEV)
    _pair_matches(ext, q, k, cos, sin, 0, -1, f"rope pair s=4200 shift {shift}")


@pytest.mark.parametrize("case", ["d16", "d24", "misaligned", "odd stride"])
def test_rope_pair_fallback(ext, case):
    """What the 16-byte path cannot take goes to the scalar kernel through
    the same binding and still matches: D = 24 (D / 2 is no multiple of 8),
    base pointers offset by 4 elements, a row stride that is no multiple of
    8. D = 16 is the narrowest row the 16-byte path does take: one thread
    per head row. Odd s, b and head counts throughout."""
    b, s, hq, hkv = 3, 37, 3, 2
    if case in ("d16", "d24"):
        d = int(case[1:])
        q, k = _qk_views("fused", s, b, hq, hkv, d, 820)
    elif case == "misaligned":
        d = 64
        q, k = _qk_views("split", s, b, hq, hkv, d, 821, shift=4)
        assert q.data_ptr() % 16 == 8 and k.data_ptr() % 16 == 8
    else:
        d = 64
        g = torch.Generator().manual_seed(822)
        qb = torch.randn(s, b, hq * d + 4, generator=g).to(BF).to(DEV)
        kb = torch.randn(s, b, hkv * d + 4, generator=g).to(BF).to(DEV)
        q = qb[:, :, :hq * d].view(s, b, hq, d).permute(1, 2, 0, 3)
        k = kb[:, :, :hkv * d].view(s, b, hkv, d).permute(1, 2, 0, 3)
        assert q.stride(0) % 8 == 4
    cos, sin = R.rope_random_tables(64, d, 823, DEV)
    _pair_matches(ext, q, k, cos, sin, 5, -1, f"rope pair fallback {case}")


def test_rope_pair_contracts_and_empty(ext):
    q = torch.randn(1, 2, 8, 16, device=DEV).to(BF)
    k = torch.randn(1, 1, 8, 16, device=DEV).to(BF)
    cos, sin = R.rope_real_tables(32, 16, device=DEV)
    ext.rope_fwd_pair(q, k, cos, sin, 24, -1, 1.0)   # rows 24 .. 31
    ext.rope_fwd_pair(q, k, cos, sin, 0, 28, -1.0)   # zigzag: 0 .. 3, 28 .. 31
    q7 = torch.randn(1, 2, 8, 7, device=DEV).to(BF)
    for name, args in {
        "q fp32": (q.float(), k, cos, sin, 0, -1), "k fp32": (q, k.float(), cos, sin, 0, -1),
        "k fp16": (q, k.half(), cos, sin, 0, -1), "q cpu": (q.cpu(), k, cos, sin, 0, -1),
        "k cpu": (q, k.cpu(), cos, sin, 0, -1),
        "k 3-D": (q, k[0], cos, sin, 0, -1),
        "k other s": (q, k[:, :, :6], cos, sin, 0, -1),
        "k other b": (q, torch.cat([k, k]), cos, sin, 0, -1),
        "k other d": (q, k[..., :8].contiguous(), cos, sin, 0, -1),
        "k d strided": (q, torch.cat([k, k], 3)[..., ::2], cos, sin, 0, -1),
        "cos fp64": (q, k, cos.double(), sin, 0, -1),
        "sin bf16": (q, k, cos, sin.to(BF), 0, -1),
        "cos cpu": (q, k, cos.cpu(), sin, 0, -1),
        "sin cpu": (q, k, cos, sin.cpu(), 0, -1),
        "too few rows": (q, k, cos, sin, 25, -1),
        "sin too few rows": (q, k, cos, sin[:31], 24, -1),
        "zigzag second half too few rows": (q, k, cos, sin, 0, 29),
        "negative offset": (q, k, cos, sin, -1, -1),
        "table width": (q, k, cos[:, :8], sin[:, :8], 0, -1),
        "odd D": (q7, q7[:, :1], cos[:, :7], sin[:, :7], 0, -1),
        "zigzag odd s": (q[:, :, :7], k[:, :, :7], cos, sin, 0, 16),
    }.items():
        _rejects(ext.rope_fwd_pair, args, f"rope_fwd_pair {name}")
    e = lambda *shape: torch.empty(*shape, device=DEV, dtype=BF)
    yq, yk = ext.rope_fwd_pair(e(1, 2, 0, 16), e(1, 1, 0, 16), cos, sin, 0, -1)
    assert yq.shape == (1, 2, 0, 16) and yk.shape == (1, 1, 0, 16)
    yq, yk = ext.rope_fwd_pair(e(0, 2, 4, 16), e(0, 1, 4, 16), cos, sin, 0, -1)
    assert yq.shape == (0, 2, 4, 16) and yk.shape == (0, 1, 4, 16)
    torch.cuda.synchronize()


def test_rope_pair_op(ext, monkeypatch):
    """apply_rotary_pos_emb_pair, forward and backward, against the two
    single calls: bit-equal; the backward negates no table."""
    from neuronx_distributed_training_amd.ops.rope import (
        apply_rotary_pos_emb, apply_rotary_pos_emb_pair,
    )

    monkeypatch.delenv("NXDT_FUSED_GLUE", raising=False)
    b, s, hq, hkv, d = 2, 96, 4, 2, 128
    cos, sin = R.rope_real_tables(1024, d, device=DEV)
    g = torch.Generator().manual_seed(830)
    dq = torch.randn(b, hq, s, d, generator=g).to(BF).to(DEV)
    dk = torch.randn(s, b, hkv, d, generator=g).to(BF).to(DEV).permute(1, 2, 0, 3)

    def run(pair, off):
        ql = torch.randn(s, b, hq * d, generator=torch.Generator().manual_seed(
            831)).to(BF).to(DEV).requires_grad_(True)
        kl = torch.randn(s, b, 2 * hkv * d, generator=torch.Generator(
        ).manual_seed(832)).to(BF).to(DEV).requires_grad_(True)
        q = ql.view(s, b, hq, d).permute(1, 2, 0, 3)
        k = kl[:, :, :hkv * d].view(s, b, hkv, d).permute(1, 2, 0, 3)
        if pair:
            yq, yk = apply_rotary_pos_emb_pair(q, k, cos, sin, off)
        else:
            yq = apply_rotary_pos_emb(q, cos, sin, off)
            yk = apply_rotary_pos_emb(k, cos, sin, off)
        torch.autograd.backward([yq, yk], [dq, dk])
        return yq.detach(), yk.detach(), ql.grad, kl.grad

    for off in (0, (96, 896)):
        want = run(False, off)
        for name, got in (("fused", run(True, off)),):
            for a, t, n in zip(got, want, ("yq", "yk", "dq", "dkv")):
                _eq(a, t, f"rope pair op off {off} {name} {n}")
        monkeypatch.setenv("NXDT_FUSED_GLUE", "0")
        for a, t in zip(run(True, off), want):
            assert torch.equal(a, t)
        monkeypatch.delenv("NXDT_FUSED_GLUE")


# ------------------------------------------------------------ model level
def _tiny_model(ckpt):
    from neuronx_distributed_training_amd.models.llama import (
        LlamaConfig, LlamaForCausalLM,
    )

    cfg = LlamaConfig(
        vocab_size=512, hidden_size=256, intermediate_size=512,
        num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
        max_position_embeddings=128, dtype="bfloat16",
        activation_checkpoint=ckpt,
    )
    return LlamaForCausalLM(cfg).to(DEV).train()


@pytest.mark.parametrize("ckpt", [None, "selective", "full"])
def test_model_arms_agree(ext, ckpt, monkeypatch):
    """Loss and backward of a 2-layer Llama once per arm of NXDT_FUSED_GLUE:
    the loss and every gradient but the RMSNorm weights' bit-equal. Those go
    to check_rmsnorm's dw bound, against the fp64 reference of each norm's
    own input and output gradient, which the unfused arm's rmsnorm calls
    hand over (the fused arm sees bit-equal ones, as the other gradients
    show)."""
    import importlib

    rms_mod = importlib.import_module(
        "neuronx_distributed_training_amd.ops.rmsnorm")  # ops.rmsnorm: the fn
    model = _tiny_model(ckpt)
    names = {id(p): n for n, p in model.named_parameters()}
    seen = {}
    plain = rms_mod.rmsnorm

    def recording(x, weight, eps=1e-5):
        y = plain(x, weight, eps)
        rec = seen.setdefault(names[id(weight)], {})
        rec["x"] = x.detach().reshape(-1, x.shape[-1])
        if y.requires_grad:
            y.register_hook(lambda g, rec=rec: rec.__setitem__(
                "dy", g.detach().reshape(-1, g.shape[-1])))
        return y

    ids = torch.randint(0, 512, (2, 128), device=DEV,
                        generator=torch.Generator(DEV).manual_seed(840))
    out = {}
    for arm in ("0", "1"):
        monkeypatch.setenv("NXDT_FUSED_GLUE", arm)
        monkeypatch.setattr(rms_mod, "rmsnorm",
                            recording if arm == "0" else plain)
        model.zero_grad(set_to_none=True)
        loss = model(ids, labels=ids)
        loss.backward()
        out[arm] = (loss.detach().clone(),
                    {n: p.grad.clone() for n, p in model.named_parameters()})
    assert torch.isfinite(out["1"][0])
    _eq(out["1"][0], out["0"][0], f"model ckpt {ckpt} loss")
    assert len(seen) == 5, sorted(seen)   # 2 x 2 layer norms + the final one
    for name, g0 in out["0"][1].items():
        g1 = out["1"][1][name]
        if name in seen:
            w = dict(model.named_parameters())[name].detach()
            ref = R.rmsnorm_ref(seen[name]["x"], w, seen[name]["dy"],
                                model.cfg.rms_norm_eps)
            R.check_rmsnorm(ref, f"ckpt {ckpt} {name} unfused", dw=g0)
            R.check_rmsnorm(ref, f"ckpt {ckpt} {name} fused", dw=g1)
        else:
            assert "norm" not in name
            _eq(g1, g0, f"model ckpt {ckpt} grad {name}")
