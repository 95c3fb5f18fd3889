"""LoRA adapter kernels on MI355X (ops/csrc/lora.hip: shrink, expand, wgrad)
through the three bindings, through ops.lora_delta_add and through
LoRAColumnParallelLinear, against one fp64 reference. Tiles that the shapes
straddle: shrink 16 rows x 8 waves of 32-wide k-windows, expand 64 x 64 (16
rows per wave), wgrad 64 columns x 32-row steps in chunks of 256 rows.
Measured figures: the docstrings below and profiles/README_lora.md."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
RANKS = [8, 16, 32, 64]
# T = 549 = 2 * 256 + 37: three wgrad chunks (LORA_WGRAD_CHUNK = 256 rows), the
# last one ragged and its second 32-row step ragged too
T_CHUNKS = 549
# (T, K, N): T = 1, one short of a 16-row tile, one over a 64-row tile, three
# chunks; K = 256 is 8 k-windows, one for every wave of the shrink kernel
SHAPES = [(1, 256, 8), (15, 8, 136), (65, 136, 256), (T_CHUNKS, 256, 136),
          (T_CHUNKS, 8, 256)]


@pytest.fixture(scope="module")
def ext():
    from neuronx_distributed_training_amd import ops

    return ops.require_extension()


def bf_round(t):
    return t.to(F32).to(BF).double()


def ref64(x, A, B, base, dout, s, rnd=lambda t: t, W=None):
    """The adapter forward and backward in fp64. rnd is applied where the
    kernels round (h, dh and every output): identity gives the reference,
    bf_round the values a kernel with exact sums returns. With a base weight
    W, base = x W^T and dx includes dout W, each a bf16 tensor of its own in
    the module."""
    x, A, B, dout = (t.double() for t in (x, A, B, dout))
    x2, d2 = x.reshape(-1, x.size(-1)), dout.reshape(-1, dout.size(-1))
    base = rnd(x2 @ W.double().T) if W is not None else base.double()
    h = rnd(x2 @ A.T)
    dh = rnd(s * (d2 @ B))
    dx = rnd(dh @ A)
    if W is not None:
        dx = rnd(rnd(d2 @ W.double()) + dx)
    return {"h": h, "out": rnd(base.reshape(d2.shape) + s * (h @ B.T)),
            "dh": dh, "dx": dx, "dA": rnd(dh.T @ x2),
            "dB": rnd(s * (d2.T @ h))}


def _poison(T, K, N, r):
    """NaN-filled, freed allocations of every output size: the outputs are
    torch::empty, so a tile the kernel leaves unwritten shows."""
    nan = float("nan")
    junk = [torch.full(s, nan, device="cuda", dtype=BF)
            for s in ((T, r), (T, N), (T, K), (N, r), (r, K))]
    junk += [torch.full((-(-T // 256), w, r), nan, device="cuda")
             for w in (K, N)]
    del junk


def _inputs(T, K, N, r, seed, kind):
    g = torch.Generator().manual_seed(seed)
    shapes = {"x": (T, K), "A": (r, K), "B": (N, r), "base": (T, N),
              "dout": (T, N)}
    if kind == "int":
        return {n: torch.randint(-1, 2, s, generator=g).to(BF)
                for n, s in shapes.items()}
    t = {n: torch.randn(s, generator=g) for n, s in shapes.items()}
    t["A"] /= K ** 0.5
    t["B"] /= r ** 0.5
    return {n: v.to(BF) for n, v in t.items()}


def _rel(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


def _check_floor(got, ref, emu, tag):
    """max|got - ref| / max|ref| at most twice the same measure of the fp64
    computation that rounds to bf16 only where the kernels do."""
    for n, g in got.items():
        err, floor = _rel(g, ref[n]), _rel(emu[n], ref[n])
        print(f"{tag} {n}: gpu {err:.4e} floor {floor:.4e} "
              f"ratio {err / floor:.3f}")
        assert err <= 2 * floor, (tag, n, err, floor)


# ---------------------------------------------------- a. exact, per binding
@pytest.mark.parametrize("T,K,N", SHAPES)
@pytest.mark.parametrize("r", RANKS)
def test_bindings_exact_on_integer_inputs(ext, r, T, K, N):
    """Inputs in {-1, 0, 1}, scaling 2: every sum is an integer that fp32
    holds, h and dh are at most 256 in magnitude and so exact in bf16, and
    all six outputs must equal the rounded fp64 reference bit for bit, twice.
    Measured on MI355X: 0 differing elements in all 20 cases."""
    c = _inputs(T, K, N, r, seed=T + K + r, kind="int")
    ref = ref64(**c, s=2.0, rnd=bf_round)
    assert ref["h"].abs().max() <= 256 and ref["dh"].abs().max() <= 256
    x, A, B, base, dout = (c[n].cuda() for n in ("x", "A", "B", "base", "dout"))
    Bt, At = B.t().contiguous(), A.t().contiguous()
    runs = []
    for _ in range(2):
        _poison(T, K, N, r)
        h = ext.lora_shrink(x, A, 1.0)
        dh = ext.lora_shrink(dout, Bt, 2.0)
        runs.append({"h": h, "out": ext.lora_expand(h, B, 2.0, base),
                     "dh": dh, "dx": ext.lora_expand(dh, At, 1.0, None),
                     "dA": ext.lora_wgrad(x, dh, 1.0, True),
                     "dB": ext.lora_wgrad(dout, h, 2.0, False)})
    for n, got in runs[0].items():
        assert got.dtype == BF and got.shape == ref[n].shape, n
        bad = int((got.double().cpu() != ref[n]).sum())
        print(f"r {r} T {T} K {K} N {N} {n}: {bad} differing elements")
        assert bad == 0, n
        assert torch.equal(got, runs[1][n]), f"{n}: two runs differ"


# ------------------------------------------------ b. Gaussian, through the op
@pytest.mark.parametrize("lead,K,N", [((3, 183), 136, 256), ((5, 13), 256, 136)])
@pytest.mark.parametrize("r", RANKS)
def test_lora_delta_add_within_twice_rounding_floor(ext, r, lead, K, N):
    """3-D x (3 * 183 = 549 rows, 5 * 13 = 65), forward and backward. Measured
    on MI355X: GPU error / floor = 1.000 for every tensor of all 8 cases (the
    largest error is a final bf16 rounding, which the emulation reproduces);
    floors 2.50e-3 .. 4.18e-3, e.g. r = 16, T = 549: out 3.541e-3, dx
    3.572e-3, dA 2.497e-3, dB 3.420e-3."""
    from neuronx_distributed_training_amd.ops import lora_delta_add

    T = lead[0] * lead[1]
    c = _inputs(T, K, N, r, seed=r + K, kind="gauss")
    s = 32.0 / r
    ref, emu = ref64(**c, s=s), ref64(**c, s=s, rnd=bf_round)
    leaf = {n: c[n].cuda().requires_grad_(True) for n in ("x", "A", "B", "base")}
    _poison(T, K, N, r)
    out = lora_delta_add(leaf["base"].view(*lead, N), leaf["x"].view(*lead, K),
                         leaf["A"], leaf["B"], s)
    assert type(out.grad_fn).__name__ == "_LoraDeltaAddBackward"
    dout = c["dout"].cuda().view(*lead, N)
    _poison(T, K, N, r)
    out.backward(dout)
    assert out.shape == (*lead, N)
    assert torch.equal(leaf["base"].grad.view_as(dout), dout)
    got = {"out": out.detach().view(T, N), "dx": leaf["x"].grad,
           "dA": leaf["A"].grad, "dB": leaf["B"].grad}
    _check_floor(got, ref, emu, f"op r {r} T {T} K {K} N {N}")


# ------------------------------------------------------ c. through the module
@pytest.mark.parametrize("kind", ["column", "row"])
def test_module_fused_and_eager(ext, monkeypatch, kind):
    """One wrapped ColumnParallelLinear / RowParallelLinear, TP = 1, bf16, no
    dropout: the fused path within twice the rounding floor of the fp64
    formula, and NXDT_LORA_FUSED=0 bit-equal to the expression the module
    evaluated before the op existed. Measured on MI355X, both kinds: GPU
    error / floor = 1.000; floors out 4.821e-3, dx 4.294e-3, dA 2.506e-3, dB
    2.470e-3."""
    from neuronx_distributed_training_amd.modules.lora import (
        LoRAColumnParallelLinear, LoraConfig,
    )
    from neuronx_distributed_training_amd.parallel.layers import (
        ColumnParallelLinear, RowParallelLinear,
    )

    T, K, N, r = 65, 136, 256, 16
    c = _inputs(T, K, N, r, seed=7, kind="gauss")
    cls = ColumnParallelLinear if kind == "column" else RowParallelLinear
    m = LoRAColumnParallelLinear(cls(K, N, dtype=BF, init_seed=3).cuda(),
                                 LoraConfig(lora_rank=r, lora_dropout=0.0))
    with torch.no_grad():
        m.lora_A.copy_(c["A"])
        m.lora_B.copy_(c["B"])
    W, s, dout = m.base.weight.detach(), m.scaling, c["dout"].cuda()

    def run(fn):
        m.zero_grad(set_to_none=True)
        x = c["x"].cuda().requires_grad_(True)
        out = fn(x)
        out.backward(dout)
        return {"out": out.detach(), "dx": x.grad, "dA": m.lora_A.grad,
                "dB": m.lora_B.grad}

    args = dict(x=c["x"], A=c["A"], B=c["B"], base=None, dout=c["dout"], s=s,
                W=W.cpu())
    _check_floor(run(m), ref64(**args), ref64(**args, rnd=bf_round),
                 f"module {kind}")
    monkeypatch.setenv("NXDT_LORA_FUSED", "0")
    got = run(m)
    want = run(lambda x: F.linear(x, W) + F.linear(
        F.linear(x, m.lora_A), m.lora_B) * s)
    for n in got:
        assert torch.equal(got[n], want[n]), f"{kind} eager {n}"


# ------------------------------------------------------- d. host contracts
@pytest.mark.parametrize("case", ["rank", "dtype", "k_mod_8", "empty"])
def test_host_contracts(ext, case):
    """What the kernels do not serve runs the eager expression through the op
    and raises from the raw bindings before any launch; T = 0 launches
    nothing and returns empty outputs and zero dA / dB."""
    from neuronx_distributed_training_amd.ops import lora_delta_add

    T, K, N, r, dt = {"rank": (5, 16, 8, 4, BF), "dtype": (5, 16, 8, 8, F32),
                      "k_mod_8": (5, 12, 8, 8, BF),
                      "empty": (0, 16, 8, 8, BF)}[case]
    g = torch.Generator().manual_seed(1)
    x, A, B, base = (
        torch.randn(s, generator=g).to(dt).cuda().requires_grad_(True)
        for s in ((T, K), (r, K), (N, r), (T, N)))
    out = lora_delta_add(base, x, A, B, 2.0)
    out.backward(torch.ones_like(out))
    if case == "empty":
        assert type(out.grad_fn).__name__ == "_LoraDeltaAddBackward"
        assert out.shape == (0, N) and x.grad.shape == (0, K)
        assert A.grad.shape == (r, K) and B.grad.shape == (N, r)
        assert not bool(A.grad.any() | B.grad.any())
        assert ext.lora_shrink(x.detach(), A.detach(), 1.0).shape == (0, r)
        return
    assert type(out.grad_fn).__name__ == "AddBackward0"
    assert torch.equal(out, base + F.linear(F.linear(x, A), B) * 2.0)
    h = torch.zeros(T, r, device="cuda", dtype=dt)
    xd, Ad, Bd = x.detach(), A.detach(), B.detach()
    for name, call in {
        "shrink": lambda: ext.lora_shrink(xd, Ad, 1.0),
        "expand": lambda: ext.lora_expand(
            h, Ad.t().contiguous() if case == "k_mod_8" else Bd, 1.0, None),
        "wgrad": lambda: ext.lora_wgrad(xd, h, 1.0, True),
    }.items():
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"{case}: lora_{name} accepted")
