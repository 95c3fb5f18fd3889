"""Grouped-GEMM MoE kernels on MI355X (ops/csrc/moe_gemm.hip: fwd, dgrad,
wgrad), one kernel at a time and through the layer, against the fp64
references of tests/moe_ref.py. Every case prints its mismatch count or
measured error before asserting, and every binding call runs behind
NaN-poisoned allocations because every output is torch::empty.

Shapes are the smallest at which the kernels can still go wrong: H = 128,
I = 128 or 256 (one to four 128-wide column tiles, 4 to 16 K chunks), over
the count patterns of moe_ref.COUNT_PATTERNS.

a. integer inputs through the three bindings: every row below `total` (the
   padding rows of a segment included: exactly zero) and every dW element
   equal to the reference; NaN in all input rows at or past `total` must not
   reach them; two runs bit-equal; K % 32 != 0 tails.
b. Gaussian inputs, bounds derived in moe_ref.assert_gemm_close.
c-e. grouped_expert_mlp, ExpertMLPs (grouped and library path) and the whole
   MoE layer, forward and backward: per tensor max|got - ref| / max|ref|
   must be at most twice the noise floor of the bf16 rounding points alone,
   which moe_ref computes on the CPU for the same inputs. Measured on
   MI355X: see the docstrings of the tests and tests/README.md.
f. host-side argument contracts of moe_gemm / moe_wgrad and the dispatch
   test grouped_path_supported."""

import pytest
import torch

from tests import moe_ref as mr

pytestmark = pytest.mark.gpu

BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32
H = 128
NAN = float("nan")


@pytest.fixture(scope="module")
def ext():
    from neuronx_distributed_training_amd import ops

    return ops.require_extension()  # fail loudly if the .so is missing


def _poison(*shapes_dtypes):
    """Fill-and-free NaN buffers of the kernels' output sizes: every output
    is torch::empty, so a block the kernel leaves unwritten shows."""
    junk = [torch.full(shape, NAN, device="cuda", dtype=dt)
            for shape, dt in shapes_dtypes]
    del junk


def _layout_for(counts):
    """The production layout (tile map, segment bounds, total, Tp), checked
    against the reference's own padding."""
    from neuronx_distributed_training_amd.ops.moe_gemm import _layout

    cdev = torch.tensor(counts, device="cuda")
    _, tile_e, pad_off, total, Tp = _layout(cdev, sum(counts))
    pad = mr.seg_bounds(counts)[2]
    assert pad_off.tolist() == pad and int(total) == pad[-1] <= Tp
    assert tile_e.numel() == Tp // mr.BM
    return tile_e, pad_off, total, Tp


def _w_shapes(E, I):
    return ((E, 2 * I, H), (E, H, I))   # gate_up, down


def _gemm(ext, counts, w_shape, trans_b, kind, seed):
    tile_e, _, total, Tp = _layout_for(counts)
    a, w = mr.gemm_case(counts, w_shape, trans_b, seed, kind)
    a_pad = mr.pad_rows(a, counts, Tp, tail=NAN)
    ad, wd = a_pad.cuda(), w.cuda()
    cols = w_shape[2] if trans_b else w_shape[1]
    tag = (f"{'dgrad' if trans_b else 'fwd'} {kind} counts {counts} "
           f"w {tuple(w_shape)}")
    _poison(((Tp, cols), BF))
    c1 = ext.moe_gemm(ad, wd, tile_e, total, trans_b)
    _poison(((Tp, cols), BF))
    c2 = ext.moe_gemm(ad, wd, tile_e, total, trans_b)
    assert c1.shape == (Tp, cols) and c1.dtype == BF
    mr.check_gemm(c1, a_pad, w, counts, trans_b, kind, tag)
    t = int(total)
    assert torch.equal(c1[:t], c2[:t]), f"{tag}: two runs differ"


def _wgrad(ext, counts, N, K, kind, seed):
    _, pad_off, _, Tp = _layout_for(counts)
    E = len(counts)
    dy, x = mr.wgrad_case(counts, N, K, seed, kind)
    dy_pad = mr.pad_rows(dy, counts, Tp, tail=NAN)
    x_pad = mr.pad_rows(x, counts, Tp, tail=NAN)
    dyd, xd = dy_pad.cuda(), x_pad.cuda()
    tag = f"wgrad {kind} counts {counts} {N}x{K}"
    _poison(((E, N, K), F32))
    d1 = ext.moe_wgrad(dyd, xd, pad_off, E)
    _poison(((E, N, K), F32))
    d2 = ext.moe_wgrad(dyd, xd, pad_off, E)
    assert d1.shape == (E, N, K) and d1.dtype == F32
    mr.check_wgrad(d1, dy_pad, x_pad, counts, kind, tag)
    for e, c in enumerate(counts):
        if c == 0:
            assert not bool(d1[e].any()), f"{tag}: empty expert {e} not zero"
    assert torch.equal(d1, d2), f"{tag}: two runs differ"


# ------------------------------------------------------ a. exact, per kernel
@pytest.mark.parametrize("trans_b", [False, True], ids=["fwd", "dgrad"])
@pytest.mark.parametrize("counts", mr.COUNT_PATTERNS, ids=mr.pattern_id)
def test_gemm_exact(ext, counts, trans_b):
    """Measured on MI355X: 0 mismatching elements in every case."""
    for I in (128, 256):
        for w_shape in _w_shapes(len(counts), I):
            _gemm(ext, counts, w_shape, trans_b, "int", seed=I)


@pytest.mark.parametrize("counts", mr.COUNT_PATTERNS, ids=mr.pattern_id)
def test_wgrad_exact(ext, counts):
    """Measured on MI355X: 0 mismatching elements in every case."""
    for I in (128, 256):
        for _, N, K in _w_shapes(len(counts), I):
            _wgrad(ext, counts, N, K, "int", seed=I)


@pytest.mark.parametrize("trans_b", [False, True], ids=["fwd", "dgrad"])
@pytest.mark.parametrize("counts", [[257], [3, 0, 0], mr.MIXED],
                         ids=mr.pattern_id)
def test_gemm_exact_k_tail(ext, counts, trans_b):
    """Contraction 136 = 4 * 32 + 8: the `k0 + col8 < K` guard of the A and
    W staging (fwd: w [E, 128, 136]) and the `n0 < K` guard of the
    transposed W staging (dgrad: w [E, 136, 128]). Bindings only; the Python
    op never gets here. Measured on MI355X: 0 mismatching elements."""
    E = len(counts)
    _gemm(ext, counts, (E, 136, 128) if trans_b else (E, 128, 136), trans_b,
          "int", seed=136)


# --------------------------------------------------- b. Gaussian, per kernel
@pytest.mark.parametrize("seed", mr.GAUSS_SEEDS)
def test_kernels_gaussian(ext, seed):
    """I = 256: gate_up has four column tiles. Measured on MI355X, max
    |got - ref| / bound over both seeds: fwd 0.973, dgrad 0.977 (an element
    that rounds by nearly half a bf16 ulp sits at 1 by construction), wgrad
    0.0017."""
    E = len(mr.MIXED)
    for w_shape in _w_shapes(E, 256):
        for trans_b in (False, True):
            _gemm(ext, mr.MIXED, w_shape, trans_b, "gauss", seed)
    for _, N, K in _w_shapes(E, 256):
        _wgrad(ext, mr.MIXED, N, K, "gauss", seed)


# ------------------------------------------------- c. grouped_expert_mlp
def _leaves(x, gu, dn):
    return tuple(t.cuda().requires_grad_(True) for t in (x, gu, dn))


MLP_CASES = [(c, 128) for c in mr.COUNT_PATTERNS] + [(mr.MIXED, 256)]


@pytest.mark.parametrize(
    "counts,I", MLP_CASES,
    ids=[f"{mr.pattern_id(c)}-I{i}" for c, i in MLP_CASES])
def test_grouped_expert_mlp_within_twice_rounding_floor(ext, counts, I):
    """fwd + bwd against ref_expert_mlp(round_like_kernel=False); the bound
    per tensor is twice the CPU noise floor of the rounding points for the
    same inputs. Measured on MI355X: in all ten cases and all four tensors
    the GPU error equals the floor to four digits (the largest error is a
    final bf16 rounding, which the emulation reproduces); floors between
    2.98e-3 (dx, mixed pattern) and 6.53e-3 (d_gate_up, [3, 0, 0]). Mixed
    pattern, I = 128, floor = GPU: y 3.864e-3, dx 2.978e-3, d_gate_up
    3.284e-3, d_down 4.087e-3."""
    from neuronx_distributed_training_amd.ops.moe_gemm import (
        grouped_expert_mlp,
    )

    x, gu, dn, dout = mr.mlp_case(counts, H, I, seed=I + len(counts))
    ref, floor = mr.mlp_floor(x, counts, gu, dn, dout)
    xd, gud, dnd = _leaves(x, gu, dn)
    Tp = _layout_for(counts)[3]
    _poison(((Tp, 2 * I), BF), ((Tp, I), BF), ((Tp, H), BF))
    y = grouped_expert_mlp(xd, torch.tensor(counts, device="cuda"), gud, dnd)
    _poison(((Tp, 2 * I), BF), ((Tp, I), BF), ((Tp, H), BF),
            (gu.shape, F32), (dn.shape, F32))
    y.backward(dout.cuda())
    got = {"y": y, "dx": xd.grad, "d_gate_up": gud.grad, "d_down": dnd.grad}
    mr.check_against_floor(got, ref, floor, f"grouped counts {counts} I {I}")
    for e, c in enumerate(counts):
        if c == 0:
            assert not bool(gud.grad[e].any() | dnd.grad[e].any()), e


# ----------------------------------------------------- d. ExpertMLPs A/B
def _expert_module(gu, dn, dtype=BF):
    from neuronx_distributed_training_amd.modules.moe import ExpertMLPs

    E, I2, Hh = gu.shape
    m = ExpertMLPs(E, Hh, I2 // 2, dtype=dtype).cuda()
    with torch.no_grad():
        m.gate_up.copy_(gu)
        m.down.copy_(dn)
    return m


def _spy(monkeypatch, owner, name, calls):
    real = getattr(owner, name)

    def wrapped(*a, **k):
        calls.append(name)
        return real(*a, **k)

    monkeypatch.setattr(owner, name, wrapped)


def _module_run(m, x, counts, dout):
    m.zero_grad(set_to_none=True)
    xd = x.cuda().requires_grad_(True)
    y = m(xd, torch.tensor(counts, device="cuda"))
    y.backward(dout.cuda())
    return {"y": y, "dx": xd.grad, "d_gate_up": m.gate_up.grad,
            "d_down": m.down.grad}


@pytest.mark.parametrize("counts,library", [([5, 5, 4, 5], "_forward_bmm"),
                                            (mr.MIXED, None)],
                         ids=["bmm", "loop"])
def test_expert_mlps_grouped_and_library_meet_the_same_bound(
        ext, monkeypatch, counts, library):
    """One module, same inputs, NXDT_MOE_GROUPED=1 and =0 (read per call):
    both within twice the rounding floor of the fp64 reference. [5, 5, 4, 5]
    takes _forward_bmm on the library side, the mixed pattern the per-expert
    loop. Measured on MI355X, floor = grouped = library to four digits:
    [5, 5, 4, 5]: y 4.036e-3, dx 4.085e-3, d_gate_up 6.247e-3, d_down
    4.687e-3; mixed: y 5.299e-3, dx 6.018e-3, d_gate_up 3.922e-3, d_down
    4.134e-3."""
    from neuronx_distributed_training_amd.modules.moe import ExpertMLPs
    from neuronx_distributed_training_amd.ops import moe_gemm as op

    x, gu, dn, dout = mr.mlp_case(counts, H, 128, seed=41)
    ref, floor = mr.mlp_floor(x, counts, gu, dn, dout)
    m = _expert_module(gu, dn)
    calls = []
    _spy(monkeypatch, op, "grouped_expert_mlp", calls)
    _spy(monkeypatch, ExpertMLPs, "_forward_bmm", calls)
    for force, want in (("1", ["grouped_expert_mlp"]),
                        ("0", [library] if library else [])):
        monkeypatch.setenv("NXDT_MOE_GROUPED", force)
        del calls[:]
        got = _module_run(m, x, counts, dout)
        assert calls == want, (force, calls)
        mr.check_against_floor(got, ref, floor,
                               f"ExpertMLPs NXDT_MOE_GROUPED={force} {counts}")


# ------------------------------------------------------- e. whole MoE layer
@pytest.mark.parametrize("capacity", [None, 1.0], ids=["dropless", "cap1"])
def test_moe_layer_grouped_within_twice_rounding_floor(ext, monkeypatch,
                                                       capacity):
    """E = 4, top-2, H = I = 128, T = 300, grouped path forced. The fp64
    reference y_t = sum_k w_tk MLP_e(x_t) uses the GPU run's own topi and
    kept (token, expert) pairs, so a bf16 tie in topk cannot flip a token.
    y and the gradients of x, router weight, gate_up and down: each within
    twice the CPU rounding floor. Measured on MI355X, floor = GPU to four
    digits: y 6.531e-3, dx 8.144e-3, d_router 5.427e-3 (5.792e-3 with the 7
    of 600 pairs that capacity 1.0 drops), d_gate_up 5.693e-3 (5.728e-3),
    d_down 6.294e-3 (6.359e-3)."""
    from neuronx_distributed_training_amd.modules.moe import MoE, RouterTopK
    from neuronx_distributed_training_amd.ops import moe_gemm as op

    E, k, I, T = 4, 2, 128, 300
    # T tokens from one draw, the E weight slabs from another
    x, _, _, dout = mr.mlp_case([T], H, I, seed=51)
    _, gu, dn, _ = mr.mlp_case([0] * E, H, I, seed=52)
    router = RouterTopK(H, E, k, dtype=BF, init_seed=53).cuda()
    with torch.no_grad():
        router.weight.mul_(5)       # logits of order one: uneven loads
    moe = MoE(router, _expert_module(gu, dn), capacity_factor=capacity)
    calls = []
    _spy(monkeypatch, op, "grouped_expert_mlp", calls)
    monkeypatch.setenv("NXDT_MOE_GROUPED", "1")
    got, topi, keep = mr.run_moe_capture(moe, x.cuda(), dout.cuda())
    assert calls == ["grouped_expert_mlp"]
    dropped = int((~keep).sum())
    print(f"capacity {capacity}: {dropped} of {keep.numel()} pairs dropped")
    assert (dropped > 0) == bool(capacity)
    args = (x, router.weight, gu, dn, dout, topi, keep)
    ref = mr.ref_moe_layer(*args)
    rounded = mr.ref_moe_layer(*args, round_like_kernel=True)
    floor = {n: mr.rel_err(rounded[n], ref[n]) for n in ref}
    mr.check_against_floor(got, ref, floor, f"MoE capacity {capacity}")


# ------------------------------------------------- f. argument contracts
def _z(*shape, dtype=BF, device="cuda"):
    return torch.zeros(*shape, device=device, dtype=dtype)


def test_moe_gemm_rejects_bad_arguments(ext):
    """Each of these raises on the host before any kernel launch."""
    a, w = _z(256, 128), _z(2, 128, 128)
    te, tot = _z(1, dtype=I32), _z(1, dtype=I32)
    ext.moe_gemm(a, w, te, tot, False)      # the valid call is accepted
    strided = _z(4, dtype=I32)[::2]
    assert not strided.is_contiguous()
    bad = {
        "a rank": (a.view(1, 256, 128), w, te, tot),
        "w rank": (a, w[0], te, tot),
        "contraction % 8": (_z(256, 132), _z(2, 128, 132), te, tot),
        "a dtype": (a.float(), w, te, tot),
        "w dtype": (a, w.float(), te, tot),
        "tile_expert device": (a, w, te.cpu(), tot),
        "total_rows device": (a, w, te, tot.cpu()),
        "tile_expert strided": (a, w, strided, tot),
        "total_rows strided": (a, w, te, strided),
        "tile_expert short": (_z(512, 128), w, te, tot),
        "tile_expert empty": (a, w, te[:0], tot),
        "total_rows numel": (a, w, te, _z(2, dtype=I32)),
        "total_rows dtype": (a, w, te, tot.long()),
    }
    for trans_b in (False, True):
        for name, args in bad.items():
            with pytest.raises(RuntimeError):
                ext.moe_gemm(*args, trans_b)
                pytest.fail(f"moe_gemm trans_b={trans_b}: {name} accepted")


def test_moe_wgrad_rejects_bad_arguments(ext):
    """Each of these raises on the host before any kernel launch."""
    dy, x = _z(256, 128), _z(256, 128)
    seg = torch.tensor([0, 256], device="cuda", dtype=I32)
    ext.moe_wgrad(dy, x, seg, 1)            # the valid call is accepted
    strided = _z(4, dtype=I32)[::2]
    bad = {
        "dy dtype": (dy.float(), x, seg, 1),
        "x dtype": (dy, x.half(), seg, 1),
        "x fp32": (dy, x.float(), seg, 1),
        "row counts differ": (_z(512, 128), x, seg, 1),
        "rows % 32": (_z(48, 128), _z(48, 128), seg, 1),
        "seg_start device": (dy, x, seg.cpu(), 1),
        "seg_start strided": (dy, x, strided, 1),
        "seg_start length": (dy, x, _z(3, dtype=I32), 1),
        "seg_start short": (dy, x, seg, 2),
        "seg_start dtype": (dy, x, seg.long(), 1),
    }
    for name, args in bad.items():
        with pytest.raises(RuntimeError):
            ext.moe_wgrad(*args)
            pytest.fail(f"moe_wgrad: {name} accepted")


def test_grouped_path_needs_bf16_contiguous_operands(ext):
    from neuronx_distributed_training_amd.ops.moe_gemm import (
        grouped_path_supported,
    )

    x, gu, dn = _z(8, 128), _z(2, 256, 128), _z(2, 128, 128)
    assert grouped_path_supported(x, gu, dn)
    assert not grouped_path_supported(x.float(), gu, dn)
    assert not grouped_path_supported(x, gu.float(), dn)
    assert not grouped_path_supported(x, gu, dn.float())
    assert not grouped_path_supported(_z(8, 256)[:, ::2], gu, dn)
    assert not grouped_path_supported(x, _z(2, 256, 256)[..., ::2], dn)
    assert not grouped_path_supported(x, gu, _z(2, 128, 256)[..., ::2])
    assert not grouped_path_supported(x.cpu(), gu.cpu(), dn.cpu())


def test_expert_mlps_fp32_weights_take_the_library_path(ext, monkeypatch):
    """"autocast" precision: fp32 parameters, bf16 activations. The grouped
    kernels take bf16 weights only, so this runs the library path (it used
    to raise "moe_gemm: bf16 only") and meets the rounding-floor bound
    against the reference on the bf16-rounded weights autocast multiplies
    with. The count is small enough for the grouped path otherwise.
    Measured on MI355X, floor = GPU: y 4.778e-3, dx 4.774e-3, d_gate_up
    4.235e-3, d_down 4.400e-3."""
    from neuronx_distributed_training_amd.ops import moe_gemm as op

    counts = mr.MIXED
    x, gu, dn, dout = mr.mlp_case(counts, H, 128, seed=61)
    ref, floor = mr.mlp_floor(x, counts, gu, dn, dout)
    m = _expert_module(gu, dn, dtype=F32)
    assert m.gate_up.dtype == F32
    calls = []
    _spy(monkeypatch, op, "grouped_expert_mlp", calls)
    monkeypatch.delenv("NXDT_MOE_GROUPED", raising=False)
    with torch.autocast("cuda", dtype=BF):
        got = _module_run(m, x, counts, dout)
    assert calls == [] and got["y"].dtype == BF
    assert got["d_gate_up"].dtype == F32
    mr.check_against_floor(got, ref, floor, "ExpertMLPs fp32 weights")
