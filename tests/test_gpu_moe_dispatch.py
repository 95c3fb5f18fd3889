"""The fused MoE token path (ops/csrc/moe_dispatch.hip, ops/moe_dispatch.py)
on the GPU: the plan against the integers the eager layer computes, the
permute / combine kernels and their backward against fp64 on the CPU, and the
MoE layer under NXDT_MOE_FUSED=1 against tests/moe_ref.py."""

import pytest
import torch

from tests import moe_ref as mr

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")


@pytest.fixture(scope="module")
def ext():
    from neuronx_distributed_training_amd import ops

    return ops.require_extension()


def _draw(T, k, E, weights, seed):
    """topi [T, k]: k distinct experts per token, expert e with odds
    weights[e]."""
    g = torch.Generator().manual_seed(seed)
    w = torch.tensor(weights, dtype=F32).expand(T, E)
    return torch.multinomial(w, k, generator=g)


def _tile_boundary():
    """k = 1, 2500 pairs (three plan chunks of 1024, the last ragged): 256
    pairs to expert 0, 257 to expert 1, none to expert 2, the rest to 3."""
    e = torch.cat([torch.full((n,), i) for i, n in
                   enumerate((256, 257, 0, 1987))])
    g = torch.Generator().manual_seed(11)
    return e[torch.randperm(2500, generator=g)].view(2500, 1)


# name -> (topi, E, capacity)
CASES = {
    "tile_boundary": (_tile_boundary(), 4, 0),
    "one_expert": (torch.full((300, 1), 5), 8, 0),
    "top2_three_chunks": (_draw(1300, 2, 8, [1.0] * 8, 12), 8, 0),
    # experts 0 and 1 overflow (about 270 of 600 pairs each), 2 and 3 do not;
    # late tokens that chose (0, 1) lose both pairs
    "capacity": (_draw(300, 2, 4, [8, 8, 1, 1], 13), 4, 150),
    "top8_of_64": (_draw(40, 8, 64, [1.0] * 64, 14), 64, 0),
}


def _eager_plan(topi, E, cap):
    """The layout integers as modules/moe.py and ops/moe_gemm.py compute
    them: stable argsort, rank < cap, bincount, _layout."""
    from neuronx_distributed_training_amd.ops.moe_gemm import _layout

    flat = topi.reshape(-1)
    order = torch.argsort(flat, stable=True)
    full = torch.bincount(flat, minlength=E)
    rank = torch.arange(flat.numel()) - (torch.cumsum(full, 0) - full)[flat[order]]
    kept_order = order[rank < cap] if cap else order
    counts = torch.bincount(flat[kept_order], minlength=E)
    pr, tile_e, pad_off, total, _ = _layout(counts, kept_order.numel())
    slot = torch.full((flat.numel(),), -1, dtype=torch.int32)
    slot[kept_order] = pr.int()
    return counts, pad_off, total, tile_e, slot


def _poison(value, *shapes_dtypes):
    """Fill-and-free buffers of the kernels' output sizes: every output is
    torch::empty, so an element the kernel leaves unwritten shows."""
    junk = [torch.full(shape, value, device="cuda", dtype=dt)
            for shape, dt in shapes_dtypes]
    del junk


def _plan(ext, name, poison=-7):
    topi, E, cap = CASES[name]
    P = topi.numel()
    Tp = (P + E * 255 + 255) // 256 * 256
    topi = topi.cuda()
    _poison(poison, ((E,), torch.int64), *[((n,), torch.int32) for n in
                                           (E + 1, 1, Tp // 256, P, Tp)])
    return ext.moe_plan(topi, E, cap)


@pytest.mark.parametrize("name", CASES)
def test_plan_equals_eager_layout(ext, name):
    topi, E, cap = CASES[name]
    counts, pad_off, total, tile_e, slot, row_src = (
        t.cpu() for t in _plan(ext, name))
    r_counts, r_pad, r_total, r_tile, r_slot = _eager_plan(topi, E, cap)
    full = torch.bincount(topi.reshape(-1), minlength=E)
    print(f"{name}: pairs per expert {full.tolist()}, kept {r_counts.tolist()}")
    if name == "capacity":   # drops from some experts, none from others
        assert (r_counts < full).any() and (r_counts[full > 0] == full[full > 0]).any()
    assert counts.dtype == torch.int64 and torch.equal(counts, r_counts)
    assert torch.equal(pad_off, r_pad) and torch.equal(total, r_total)
    n = r_tile.numel()   # _layout sizes the tile map by the kept pairs
    assert torch.equal(tile_e[:n], r_tile) and bool((tile_e[n:] == E - 1).all())
    assert torch.equal(slot, r_slot)
    kept = torch.nonzero(slot >= 0).squeeze(1)
    assert torch.equal(row_src[slot[kept].long()], kept.int())
    # a second run over differently poisoned allocations is bit-equal
    again = [t.cpu() for t in _plan(ext, name, poison=-9)]
    for a, b in zip(again[:5], (counts, pad_off, total, tile_e, slot)):
        assert torch.equal(a, b)
    assert torch.equal(again[5][slot[kept].long()], kept.int())


def _excess(got, ref, mag, n, half_ulp=2.0 ** -8):
    """max |got - ref| / (half_ulp * |ref| + n * 2**-23 * mag): one rounding
    of an fp32 sum of n products whose absolute values sum to mag (fp32
    accumulation in any order: (n - 1) * 2**-24 * mag; the factor 2 left
    covers the rounding of each product and the bound taken at ref)."""
    bound = half_ulp * ref.abs() + n * 2.0 ** -23 * mag
    err = (got.detach().cpu().to(F64) - ref).abs()
    assert err.numel() and not torch.isnan(err).any()
    return float((err / bound.clamp(min=1e-300)).max())


@pytest.mark.parametrize("kind", ["gauss", "int"])
@pytest.mark.parametrize("name,H", [(n, 128) for n in CASES]
                         + [("capacity", 640), ("capacity", 2176)])
def test_permute_combine_and_backward(ext, name, H, kind):
    """H = 128 / 640 / 2176: 16, 64 and 256 lanes a row, the last two with a
    ragged vector loop. gauss: bf16 weights, derived bounds; int: |values| <=
    3 and fp32 weights 1 or 2, every sum an exact integer: got == ref.
    Measured on MI355X, gauss, largest |got - ref| / bound over the cases:
    combine and unit 0.996, dy_pad 0.988 (an element that rounds by nearly
    half a bf16 ulp), dw 0.952."""
    topi, E, cap = CASES[name]
    T, k = topi.shape
    plan = _plan(ext, name)
    counts, pad_off, total, tile_e, slot, row_src = plan
    rows = (row_src, tile_e, pad_off, counts, total)
    Tp, tot = row_src.numel(), int(total)
    slot = slot.view(T, k)
    slot_c = slot.cpu().long()
    kept = slot_c >= 0
    pair_row = slot_c[kept]                              # padded row per kept pair
    pair_tok = torch.nonzero(kept)[:, 0]                 # its token
    g = torch.Generator().manual_seed(21)
    if kind == "int":
        x, y_pad, dy = (mr.int_inputs(s, -3, 3, g) for s in
                        ((T, H), (Tp, H), (T, H)))
        w = 2.0 ** torch.randint(0, 2, (T, k), generator=g).to(F32)
    else:
        x, y_pad, dy = (torch.randn(s, generator=g).to(BF) for s in
                        ((T, H), (Tp, H), (T, H)))
        w = torch.rand(T, k, generator=g).to(BF)
    y_pad[tot:] = NAN                                    # never to be read

    # permute: copies, zero padding rows, poison past total
    xc = x.cuda()
    _poison(NAN, ((Tp, H), BF))
    x_pad = ext.moe_permute(xc, k, *rows).cpu()
    is_pad = torch.ones(tot, dtype=torch.bool)
    is_pad[pair_row] = False
    assert torch.equal(x_pad[pair_row], x[pair_tok])
    assert bool((x_pad[:tot][is_pad] == 0).all())
    assert bool(torch.isnan(x_pad[tot:]).all())

    exact = kind == "int"
    w64, y64, dy64 = w.to(F64), y_pad.to(F64), dy.to(F64)
    for tag, wt, got in (
            ("combine", w64, ext.moe_combine(y_pad.cuda(), slot, w.cuda())),
            ("unit", torch.ones_like(w64), ext.moe_combine(y_pad.cuda(), slot))):
        terms = torch.zeros(T, k, H, dtype=F64)
        terms[kept] = wt[kept][:, None] * y64[pair_row]
        ref = terms.sum(1)
        ex = _excess(got, ref, terms.abs().sum(1), k)
        print(f"{name} H {H} {kind} {tag}: |got - ref| / bound = {ex:.4f}")
        assert ex == 0.0 if exact else ex <= 1.0
        dead = ~kept.any(1)                              # all pairs dropped
        assert name != "capacity" or bool(dead.any())
        assert bool((got.cpu()[dead] == 0).all())

    dy_pad, dw = ext.moe_combine_bwd(dy.cuda(), y_pad.cuda(), w.cuda(), slot,
                                     *rows)
    assert dw.dtype == w.dtype and dw.shape == w.shape
    dy_pad, dw = dy_pad.cpu(), dw.cpu()
    ref = w64[kept][:, None] * dy64[pair_tok]
    ex = _excess(dy_pad[pair_row], ref, ref.abs(), 1)
    assert bool((dy_pad[:tot][is_pad] == 0).all())
    prod = dy64[pair_tok] * y64[pair_row]
    ex_w = _excess(dw[kept], prod.sum(1), prod.abs().sum(1), H,
                   2.0 ** -24 if w.dtype == F32 else 2.0 ** -8)
    print(f"{name} H {H} {kind} bwd: dy_pad {ex:.4f} dw {ex_w:.4f} of bound")
    assert (ex == 0.0 and ex_w == 0.0) if exact else max(ex, ex_w) <= 1.0
    assert bool((dw[~kept] == 0).all())                  # dropped pairs


# ------------------------------------------------------------- the layer
def _layer(E, capacity, T, k=2, H=128, I=128):
    from neuronx_distributed_training_amd.modules.moe import (
        ExpertMLPs, MoE, RouterTopK)

    x, _, _, dout = mr.mlp_case([T], H, I, seed=61)
    _, gu, dn, _ = mr.mlp_case([0] * E, H, I, seed=62)
    router = RouterTopK(H, E, k, dtype=BF, init_seed=63).cuda()
    experts = ExpertMLPs(E, H, I, dtype=BF).cuda()
    with torch.no_grad():
        router.weight.mul_(5)       # logits of order one: uneven loads
        experts.gate_up.copy_(gu)
        experts.down.copy_(dn)
    return MoE(router, experts, capacity_factor=capacity), x, gu, dn, dout


def _run(moe, x, dout):
    seen = {}
    hook = moe.router.register_forward_hook(
        lambda m, i, o: seen.__setitem__("topi", o[1].detach().cpu()))
    try:
        moe.zero_grad(set_to_none=True)
        xd = x.cuda().requires_grad_(True)
        y, _ = moe(xd)
        y.backward(dout.cuda())
    finally:
        hook.remove()
    return {"y": y.detach(), "dx": xd.grad, "d_router": moe.router.weight.grad,
            "d_gate_up": moe.experts.gate_up.grad,
            "d_down": moe.experts.down.grad}, seen["topi"]


@pytest.mark.parametrize("capacity", [None, 1.0], ids=["dropless", "cap1"])
@pytest.mark.parametrize("E,T", [(4, 520), (8, 1040)])
def test_moe_layer_fused_within_twice_rounding_floor(ext, monkeypatch, E, T,
                                                     capacity):
    """Top-2, H = I = 128, about 260 pairs per expert so that counts fall on
    both sides of a 256-row tile. The fp64 reference uses the run's own topi
    and kept pairs; the bound is twice the rounding floor of the eager layer
    (moe_ref.ref_moe_layer with round_like_kernel), which models more
    rounding points than the fused path has. Measured on MI355X, error /
    floor, dropless (capacity 1.0): E = 4: y 0.953 (0.953), dx 0.912
    (0.912), d_router 1.017 (1.000), d_gate_up 1.000 (1.000), d_down 1.000
    (1.000); E = 8: y 0.999 (0.999), dx 1.000 (1.000), d_router 0.946
    (1.000), d_gate_up 1.000 (1.000), d_down 1.000 (1.000). Floors are 4.5e-3
    to 7.8e-3; capacity 1.0 drops 18 of 1040 and 77 of 2080 pairs."""
    from neuronx_distributed_training_amd.ops import moe_dispatch as op

    moe, x, gu, dn, dout = _layer(E, capacity, T)
    calls = []
    real = op.fused_moe_experts
    monkeypatch.setattr(op, "fused_moe_experts",
                        lambda *a, **kw: calls.append(1) or real(*a, **kw))
    monkeypatch.setenv("NXDT_MOE_FUSED", "1")
    got, topi = _run(moe, x, dout)
    assert calls == [1]
    full = torch.bincount(topi.reshape(-1), minlength=E)
    cap = -(-T * 2 // E) if capacity else T * 2   # ceil(1.0 * T * k / E)
    counts = full.clamp(max=cap)
    print(f"E {E} capacity {capacity}: pairs per expert {full.tolist()}, "
          f"{int((full - counts).sum())} dropped")
    assert counts.min() < 256 < counts.max()
    assert bool((full > counts).any()) == bool(capacity)
    args = (x, moe.router.weight, gu, dn, dout, topi,
            mr.kept_pairs(topi, counts))
    ref = mr.ref_moe_layer(*args)
    rounded = mr.ref_moe_layer(*args, round_like_kernel=True)
    floor = {n: mr.rel_err(rounded[n], ref[n]) for n in ref}
    mr.check_against_floor(got, ref, floor, f"fused MoE E {E} cap {capacity}")
    again, topi2 = _run(moe, x, dout)
    assert torch.equal(topi, topi2)
    for n in got:
        assert torch.equal(got[n], again[n]), n


def test_moe_fused_switch_rejects_other_values(ext, monkeypatch):
    moe, x, _, _, _ = _layer(4, None, 8)
    monkeypatch.setenv("NXDT_MOE_FUSED", "2")
    with pytest.raises(ValueError, match="NXDT_MOE_FUSED"):
        moe(x.cuda())
