"""CPU checks of tests/moe_ref.py, the reference and comparators behind
tests/test_gpu_moe_gemm.py: the fp64 reference agrees with fp64 autograd
through the module's library path; each way a grouped-GEMM kernel could be
subtly wrong makes the comparator meant for it raise; and the derived
Gaussian bound accepts a correct kernel's arithmetic (fp32 sum, bf16 cast)."""

import pytest
import torch

from tests import moe_ref as mr

BF = torch.bfloat16
H = 128
SQUARE = (5, 128, 128)      # down-shaped slabs, N == K
KINDS = ("int", "gauss")


# ----------------------------------------------------------- reference check
def _experts(E, Hh, I, seed):
    from neuronx_distributed_training_amd.modules.moe import ExpertMLPs

    m = ExpertMLPs(E, Hh, I, dtype=torch.float64, init_seed=seed)
    with torch.no_grad():       # unit-scale pre-activations
        m.gate_up.mul_(50 / Hh ** 0.5)
        m.down.mul_(50 / I ** 0.5)
    return m


@pytest.mark.parametrize("counts", [[5, 5, 4, 5], [7, 0, 1, 30], [3], [0, 2]],
                         ids=mr.pattern_id)
def test_reference_matches_fp64_autograd(counts):
    """[5, 5, 4, 5] takes _forward_bmm, the others the per-expert loop."""
    E, Hh, I = len(counts), 16, 24
    m = _experts(E, Hh, I, 3)
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(sum(counts), Hh, generator=gen, dtype=torch.float64,
                    requires_grad=True)
    dout = torch.randn(sum(counts), Hh, generator=gen, dtype=torch.float64)
    y = m(x, torch.tensor(counts))
    y.backward(dout)
    ref = mr.ref_expert_mlp(x, counts, m.gate_up, m.down, dout)
    got = {"y": y, "dx": x.grad, "d_gate_up": m.gate_up.grad,
           "d_down": m.down.grad}
    for n in mr.MLP_TENSORS:
        err = float((got[n].detach() - ref[n]).abs().max())
        print(f"{counts} {n}: max abs err {err:.3e}")
        assert err <= 1e-10, (n, err)


@pytest.mark.parametrize("capacity", [None, 1.0])
def test_layer_reference_matches_fp64_autograd(capacity):
    from neuronx_distributed_training_amd.modules.moe import MoE, RouterTopK

    E, k, Hh, I, T = 4, 2, 16, 24, 40
    router = RouterTopK(Hh, E, k, dtype=torch.float64, init_seed=5)
    with torch.no_grad():
        router.weight.mul_(20)      # spread the logits: uneven loads
    moe = MoE(router, _experts(E, Hh, I, 6), capacity_factor=capacity)
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(T, Hh, generator=gen, dtype=torch.float64)
    dout = torch.randn(T, Hh, generator=gen, dtype=torch.float64)
    got, topi, keep = mr.run_moe_capture(moe, x, dout)
    if capacity:
        assert not bool(keep.all()), "capacity 1.0 should drop pairs here"
    else:
        assert bool(keep.all())
    ref = mr.ref_moe_layer(x, router.weight, moe.experts.gate_up,
                           moe.experts.down, dout, topi, keep)
    # the router computes logits.float() and its softmax in fp32 by design,
    # so not 1e-10 here: 2**-24 per fp32 operation, a hundred-fold margin
    # for the softmax, normalisation and their backward -> 1e-5 relative.
    # A wrong term in the hand-written backward is an error of order one.
    for n, r in ref.items():
        err = mr.rel_err(got[n], r)
        print(f"capacity {capacity} {n}: rel err {err:.3e}")
        assert err <= 1e-5, (n, err)


def test_int_inputs_are_small_unsymmetric_integers():
    gen = torch.Generator().manual_seed(0)
    w = mr.int_inputs((3, 128, 136), -2, 3, gen)
    assert w.dtype == BF and float(w.min()) == -2 and float(w.max()) == 3
    assert bool((w == w.round()).all())
    assert not torch.equal(w[0], w[1])
    assert not torch.equal(w[0, :, :128], w[0, :, :128].t())


# ------------------------------------------------------------- sensitivity
def _emulate_gemm(a_pad, w, counts, trans_b, k_drop=0):
    """The kernel's arithmetic on the CPU: fp32 sum, bf16 cast; zero rows
    outside the experts' own tokens. k_drop leaves out the last k_drop
    elements of the contraction."""
    cl, _, pad = mr.seg_bounds(counts)
    K = a_pad.size(1) - k_drop
    out = torch.zeros(a_pad.size(0), w.size(2) if trans_b else w.size(1),
                      dtype=BF)
    for e, c in enumerate(cl):
        we = (w[e] if trans_b else w[e].t()).float()[:K]
        out[pad[e]:pad[e] + c] = (
            a_pad[pad[e]:pad[e] + c, :K].float() @ we).to(BF)
    return out


def _emulate_wgrad(dy_pad, x_pad, counts):
    """fp32 sums over whole padded segments, as the kernel walks them."""
    _, _, pad = mr.seg_bounds(counts)
    return torch.stack([
        dy_pad[pad[e]:pad[e + 1]].float().t()
        @ x_pad[pad[e]:pad[e + 1]].float() for e in range(len(counts))])


def _gemm_setup(kind, trans_b=False, w_shape=SQUARE, counts=mr.MIXED):
    a, w = mr.gemm_case(counts, w_shape, trans_b, 0, kind)
    Tp = mr.seg_bounds(counts)[2][-1] + mr.BM
    return mr.pad_rows(a, counts, Tp, tail=float("nan")), w


def _wgrad_setup(kind, counts=mr.MIXED):
    dy, x = mr.wgrad_case(counts, 128, H, 0, kind)
    Tp = mr.seg_bounds(counts)[2][-1] + mr.BM
    return (mr.pad_rows(dy, counts, Tp, tail=float("nan")),
            mr.pad_rows(x, counts, Tp, tail=float("nan")))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("trans_b", [False, True])
@pytest.mark.parametrize("counts", mr.COUNT_PATTERNS, ids=mr.pattern_id)
def test_correct_gemm_passes(counts, trans_b, kind):
    """Over every count pattern of the kernel tests, 2 column tiles."""
    a_pad, w = _gemm_setup(kind, trans_b, (len(counts), 256, 128), counts)
    good = _emulate_gemm(a_pad, w, counts, trans_b)
    mr.check_gemm(good, a_pad, w, counts, trans_b, kind, "good")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("counts", mr.COUNT_PATTERNS, ids=mr.pattern_id)
def test_correct_wgrad_passes(counts, kind):
    dy_pad, x_pad = _wgrad_setup(kind, counts)
    mr.check_wgrad(_emulate_wgrad(dy_pad, x_pad, counts), dy_pad, x_pad,
                   counts, kind, "good")


def test_one_bf16_ulp_fails_exact():
    a_pad, w = _gemm_setup("int")
    got = _emulate_gemm(a_pad, w, mr.MIXED, False)
    assert float(got[700, 77]) != 0
    got.view(torch.int16)[700, 77] += 1
    with pytest.raises(AssertionError, match="1 of .* tile 2, row 188 .*"
                                             "column 77"):
        mr.check_gemm(got, a_pad, w, mr.MIXED, False, "int", "ulp")


def _corrupt_fragment(a_pad, w, good):
    # rows 32..47 of expert 0, columns 64..79, from expert 1's weights
    got = good.clone()
    got[32:48, 64:80] = (a_pad[32:48].float()
                         @ w[1].t().float()[:, 64:80]).to(BF)
    return got


def _corrupt_k_chunk(a_pad, w, good):
    return _emulate_gemm(a_pad, w, mr.MIXED, False, k_drop=32)


def _corrupt_row_shift(a_pad, w, good):
    got = good.clone()
    got[256:511] = good[257:512]        # tile 1 (experts 1's padded segment
    got[768:1023] = good[769:1024]      # is mostly zeros) and tile 3
    return got


def _corrupt_transposed(a_pad, w, good):
    return _emulate_gemm(a_pad, w, mr.MIXED, True)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("corrupt", [_corrupt_fragment, _corrupt_k_chunk,
                                     _corrupt_row_shift, _corrupt_transposed],
                         ids=["fragment", "k-chunk", "row-shift",
                              "transposed"])
def test_corrupted_gemm_fails(corrupt, kind):
    a_pad, w = _gemm_setup(kind)
    good = _emulate_gemm(a_pad, w, mr.MIXED, False)
    mr.check_gemm(good, a_pad, w, mr.MIXED, False, kind, "good")
    with pytest.raises(AssertionError):
        mr.check_gemm(corrupt(a_pad, w, good), a_pad, w, mr.MIXED, False,
                      kind, "corrupt")


@pytest.mark.parametrize("kind", KINDS)
def test_nan_in_empty_experts_dw_fails(kind):
    dy_pad, x_pad = _wgrad_setup(kind)
    got = _emulate_wgrad(dy_pad, x_pad, mr.MIXED)
    got[3] = float("nan")               # expert 3 has no tokens
    with pytest.raises(AssertionError):
        mr.check_wgrad(got, dy_pad, x_pad, mr.MIXED, kind, "nan")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row", [255, 511])
def test_padded_row_leaking_into_dw_fails(row, kind):
    """Row 255 pads expert 0 (255 tokens), row 511 expert 1 (one token)."""
    dy_pad, x_pad = _wgrad_setup(kind)
    assert float(dy_pad[row].abs().sum()) == 0
    dy_leak, x_leak = dy_pad.clone(), x_pad.clone()
    dy_leak[row, 5] = 1.0
    x_leak[row, 9] = 1.0
    got = _emulate_wgrad(dy_leak, x_leak, mr.MIXED)
    with pytest.raises(AssertionError):
        mr.check_wgrad(got, dy_pad, x_pad, mr.MIXED, kind, "leak")


def test_assert_exact_reports_expert_row_column():
    ref = torch.zeros(3, 4, 5)
    got = ref.clone()
    got[2, 1, 3] = 1.0
    got[2, 3, 0] = float("nan")
    with pytest.raises(AssertionError, match="2 of 60 .*expert 2, row 1, "
                                             "column 3"):
        mr.assert_exact(got, ref, "dw")


# -------------------------------------------------------------- bound check
@pytest.mark.parametrize("seed", mr.GAUSS_SEEDS)
def test_derived_bound_accepts_fp32_sum_bf16_cast(seed):
    """The Gaussian cases of the GPU file (I = 256, the mixed pattern)."""
    I, E = 256, len(mr.MIXED)
    for w_shape in ((E, 2 * I, H), (E, H, I)):
        for trans_b in (False, True):
            a, w = mr.gemm_case(mr.MIXED, w_shape, trans_b, seed, "gauss")
            a_pad = mr.pad_rows(a, mr.MIXED, 1536)
            mr.check_gemm(_emulate_gemm(a_pad, w, mr.MIXED, trans_b), a_pad,
                          w, mr.MIXED, trans_b, "gauss",
                          f"seed {seed} {w_shape} trans_b {trans_b}")
    for N, K in ((2 * I, H), (H, I)):
        dy, x = mr.wgrad_case(mr.MIXED, N, K, seed, "gauss")
        dy_pad = mr.pad_rows(dy, mr.MIXED, 1536)
        x_pad = mr.pad_rows(x, mr.MIXED, 1536)
        mr.check_wgrad(_emulate_wgrad(dy_pad, x_pad, mr.MIXED), dy_pad,
                       x_pad, mr.MIXED, "gauss", f"seed {seed} wgrad {N}x{K}")
