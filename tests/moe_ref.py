"""fp64 references and comparators for the grouped-GEMM MoE kernels
(ops/csrc/moe_gemm.hip), shared by tests/test_moe_ref.py (CPU) and
tests/test_gpu_moe_gemm.py.

Everything here works from the per-expert token `counts` and builds the
256-row padded layout itself; it shares no code with ops/moe_gemm.py. The
padded layout: expert e owns rows [pad[e], pad[e] + ceil256(counts[e])) of a
[Tp, cols] array, its counts[e] tokens first, zero rows after them;
total = pad[E] <= Tp, and rows at or past `total` belong to nobody.

Two kinds of comparison:
- integer inputs (`int_inputs`): |a| <= 3, |w| <= 3, so with K * 9 < 2**24
  every partial sum is an integer fp32 holds exactly, whatever the summation
  order. The kernel's bf16 output must equal ref.to(bfloat16) and its fp32
  wgrad must equal the reference, element for element (`assert_exact`);
- Gaussian inputs: `assert_gemm_close` / `assert_wgrad_close`, bounds derived
  from the number formats alone (see their docstrings)."""

import torch

BM = 256  # row-tile height of the grouped kernel
F64 = torch.float64


# ------------------------------------------------------------------ layout
def seg_bounds(counts):
    """(counts, src, pad) as python ints: expert e's tokens are rows
    src[e]:src[e+1] of the sorted array and rows pad[e]:pad[e]+counts[e] of
    the padded one; pad[-1] is `total`."""
    counts = [int(c) for c in counts]
    src, pad = [0], [0]
    for c in counts:
        src.append(src[-1] + c)
        pad.append(pad[-1] + -(-c // BM) * BM)
    return counts, src, pad


def pad_rows(x, counts, Tp, tail=0.0):
    """Sorted [T, C] -> padded [Tp, C]: zeros in the padding rows of every
    segment, `tail` (NaN in the kernel tests) in the rows at or past total."""
    counts, src, pad = seg_bounds(counts)
    assert x.size(0) == src[-1] and pad[-1] <= Tp
    out = x.new_zeros(Tp, x.size(1))
    out[pad[-1]:] = tail
    for e, c in enumerate(counts):
        out[pad[e]:pad[e] + c] = x[src[e]:src[e + 1]]
    return out


# -------------------------------------------------------------- references
def ref_gemm(a, w, counts, trans_b):
    """a: padded [Tp, K]; w: [E, N, Kw]. fp64 [Tp, N] (trans_b False,
    a @ w[e]^T) or [Tp, Kw] (True, a @ w[e]) for each expert's own tokens;
    every other row is zero."""
    counts, _, pad = seg_bounds(counts)
    out = torch.zeros(a.size(0), w.size(2) if trans_b else w.size(1),
                      dtype=F64)
    for e, c in enumerate(counts):
        we = w[e].to(F64)
        ae = a[pad[e]:pad[e] + c].to(F64)
        out[pad[e]:pad[e] + c] = ae @ (we if trans_b else we.t())
    return out


def ref_wgrad(dy, x, counts):
    """dy: padded [Tp, N]; x: padded [Tp, K]. fp64 [E, N, K],
    dW[e] = dy_e^T @ x_e over expert e's own tokens; zero for an empty
    expert."""
    counts, _, pad = seg_bounds(counts)
    out = torch.zeros(len(counts), dy.size(1), x.size(1), dtype=F64)
    for e, c in enumerate(counts):
        sl = slice(pad[e], pad[e] + c)
        out[e] = dy[sl].to(F64).t() @ x[sl].to(F64)
    return out


def _rnd_bf16(t):
    # through fp32 first: the kernels round an fp32 accumulator to bf16
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def _rnd_none(t):
    return t


def _mlp_fwd(x, counts, gu, dn, rnd):
    """x: sorted [T, H] fp64. Returns (h [T, 2I], g [T, I], y [T, H])."""
    counts, src, _ = seg_bounds(counts)
    I = dn.size(2)
    h = x.new_zeros(x.size(0), 2 * I)
    g = x.new_zeros(x.size(0), I)
    y = x.new_zeros(x.size(0), dn.size(1))
    for e in range(len(counts)):
        sl = slice(src[e], src[e + 1])
        h[sl] = rnd(x[sl] @ gu[e].t())
        gate, up = h[sl, :I], h[sl, I:]
        g[sl] = rnd(gate * torch.sigmoid(gate) * up)
        y[sl] = rnd(g[sl] @ dn[e].t())
    return h, g, y


def _mlp_bwd(x, counts, gu, dn, h, g, dy, rnd):
    """Returns (dx [T, H], d_gate_up [E, 2I, H], d_down [E, H, I])."""
    counts, src, _ = seg_bounds(counts)
    I = dn.size(2)
    dx = torch.zeros_like(x)
    d_gu = torch.zeros_like(gu)
    d_dn = torch.zeros_like(dn)
    for e in range(len(counts)):
        sl = slice(src[e], src[e + 1])
        # dW: fp32 sum in the kernel, then the cast to the weights' bf16
        d_dn[e] = rnd(dy[sl].t() @ g[sl])
        dg = rnd(dy[sl] @ dn[e])
        gate, up = h[sl, :I], h[sl, I:]
        sig = torch.sigmoid(gate)
        dh = rnd(torch.cat((dg * up * sig * (1 + gate * (1 - sig)),
                            dg * gate * sig), dim=1))
        d_gu[e] = rnd(dh.t() @ x[sl])
        dx[sl] = rnd(dh @ gu[e])
    return dx, d_gu, d_dn


def ref_expert_mlp(x, counts, gu, dn, dout, round_like_kernel=False):
    """SwiGLU expert MLP forward and backward in fp64 from the (bf16) inputs:
    x sorted [T, H], gu [E, 2I, H], dn [E, H, I], dout [T, H]. Returns a dict
    y, dx, d_gate_up, d_down.

    round_like_kernel rounds to bf16 where the GPU path stores bf16: h, g, y
    in the forward; dg, dh, dx and dW (after its fp32 sum) in the backward.
    Use it only to measure the noise floor of those roundings."""
    rnd = _rnd_bf16 if round_like_kernel else _rnd_none
    x, gu, dn, dout = (t.detach().cpu().to(F64) for t in (x, gu, dn, dout))
    h, g, y = _mlp_fwd(x, counts, gu, dn, rnd)
    dx, d_gu, d_dn = _mlp_bwd(x, counts, gu, dn, h, g, dout, rnd)
    return {"y": y, "dx": dx, "d_gate_up": d_gu, "d_down": d_dn}


def ref_moe_layer(x, router_w, gu, dn, dout, topi, keep,
                  round_like_kernel=False):
    """Top-k MoE layer (softmax router, normalised top-k affinities) forward
    and backward in fp64 with the routing decisions given: topi [T, k] expert
    ids and keep [T, k] bool (False = pair dropped by the capacity limit).
    y_t = sum_k w_tk * MLP_{topi_tk}(x_t). Returns a dict y, dx, d_router,
    d_gate_up, d_down.

    round_like_kernel rounds to bf16 where modules/moe.py on bf16 tensors
    does: router logits, affinities, the expert MLP's points (see
    ref_expert_mlp), the weighted expert outputs, their per-token sum, and
    in the backward the gradients autograd hands over in bf16."""
    rnd = _rnd_bf16 if round_like_kernel else _rnd_none
    x, wr, gu, dn, dout = (t.detach().cpu().to(F64)
                           for t in (x, router_w, gu, dn, dout))
    topi, keep = topi.cpu(), keep.cpu()
    T, k = topi.shape
    E = wr.size(0)

    logits = rnd(x @ wr.t())
    probs = torch.softmax(logits, dim=-1)
    tw = probs.gather(1, topi)
    tsum = tw.sum(-1, keepdim=True)
    w = rnd(tw / tsum)

    flat_k = keep.reshape(-1)
    flat_e = topi.reshape(-1)[flat_k]
    flat_tok = torch.arange(T).repeat_interleave(k)[flat_k]
    order = torch.argsort(flat_e, stable=True)
    tok = flat_tok[order]
    w_s = w.reshape(-1)[flat_k][order]
    counts = torch.bincount(flat_e, minlength=E).tolist()

    xin = x[tok]
    h, g, yexp = _mlp_fwd(xin, counts, gu, dn, rnd)
    contrib = rnd(yexp * w_s[:, None])
    y = rnd(torch.zeros_like(x).index_add_(0, tok, contrib))

    dc = dout[tok]
    dyexp = rnd(dc * w_s[:, None])
    # autograd: elementwise product stored in bf16, then reduced over H
    dw_s = rnd(rnd(dc * yexp).sum(-1))
    dxin, d_gu, d_dn = _mlp_bwd(xin, counts, gu, dn, h, g, dyexp, rnd)
    dx = rnd(torch.zeros_like(x).index_add_(0, tok, dxin))

    dw_flat = torch.zeros(T * k, dtype=F64)
    dw_flat[torch.nonzero(flat_k).squeeze(1)[order]] = dw_s
    dw = dw_flat.view(T, k)
    dtw = dw / tsum - (dw * tw).sum(-1, keepdim=True) / tsum ** 2
    dprobs = torch.zeros_like(probs).scatter_(1, topi, dtw)
    dlogits = rnd(probs * (dprobs - (dprobs * probs).sum(-1, keepdim=True)))
    d_router = rnd(dlogits.t() @ x)
    dx = rnd(dx + rnd(dlogits @ wr))
    return {"y": y, "dx": dx, "d_router": d_router, "d_gate_up": d_gu,
            "d_down": d_dn}


def rel_err(got, ref):
    """max|got - ref| / max|ref|, the metric of the layer-level tests."""
    ref = ref.to(F64)
    return float((got.detach().cpu().to(F64) - ref).abs().max()
                 / ref.abs().max().clamp(min=1e-30))


# ------------------------------------------------------------------ inputs
def int_inputs(shape, lo, hi, gen):
    """bf16 tensor of integers in [lo, hi]: a seeded draw plus a ramp over
    the last two (and, for 3-D, the leading) indices modulo primes, wrapped
    into the range. Unsymmetric ranges and the ramp make a transposed
    operand, a shifted row or a swapped expert change the product."""
    span = hi - lo + 1
    base = torch.randint(0, span, shape, generator=gen)
    r = torch.arange(shape[-2])[:, None]
    c = torch.arange(shape[-1])[None, :]
    ramp = (3 * r) % 7 + (5 * c) % 11
    if len(shape) == 3:
        ramp = ramp[None] + (2 * torch.arange(shape[0]) % 5)[:, None, None]
    return (lo + (base + ramp) % span).to(torch.bfloat16)


# ------------------------------------------------------------- comparators
def _first_bad(bad, got, ref, tag):
    n = int(bad.sum())
    idx = torch.nonzero(bad)[0].tolist()
    if bad.dim() == 2:
        where = (f"tile {idx[0] // BM}, row {idx[0] % BM} (array row "
                 f"{idx[0]}), column {idx[1]}")
    else:
        where = f"expert {idx[0]}, row {idx[1]}, column {idx[2]}"
    i = tuple(idx)
    return (f"{tag}: {n} of {bad.numel()} elements wrong; first at {where}: "
            f"got {float(got[i])}, want {float(ref[i])}")


def count_mismatches(got, ref):
    """Number of elements of `got` that are NaN or differ from `ref` (which
    is cast to got's dtype first, round-to-nearest-even)."""
    return int(_mismatch(got, ref).sum())


def _mismatch(got, ref):
    got = got.detach().cpu()
    ref = ref.detach().cpu().to(got.dtype)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return (got != ref) | torch.isnan(got)


def assert_exact(got, ref, tag):
    """Every element of got equals ref.to(got.dtype) and none is NaN. On
    failure: the number of wrong elements and the first bad (tile, row,
    column) of a 2-D [rows, cols] array, or (expert, row, column) of a 3-D
    one."""
    bad = _mismatch(got, ref)
    if bad.any():
        g = got.detach().cpu()
        raise AssertionError(_first_bad(bad, g.to(F64), ref.cpu().to(g.dtype)
                                        .to(F64), tag))


def gemm_excess(got, a, w_e, ref, K):
    """max over elements of |got - ref| / bound (<= 1 passes) for
    assert_gemm_close; NaN in got counts as infinite."""
    a, w_e, ref = (t.detach().cpu().to(F64) for t in (a, w_e, ref))
    got = got.detach().cpu().to(F64)
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -22 * (a.abs() @ w_e.abs())
    return _excess(got, ref, bound)


def _excess(got, ref, bound):
    assert got.shape == ref.shape == bound.shape
    if got.numel() == 0:
        return 0.0
    ratio = (got - ref).abs() / bound.clamp(min=1e-300)
    ratio = torch.where(torch.isnan(got), torch.full_like(ratio, float("inf")),
                        ratio)
    return float(ratio.max())


def assert_gemm_close(got, a, w_e, ref, K, tag="gemm"):
    """One expert's rows of a bf16 GEMM output against the fp64 `ref` =
    a @ w_e, with a [n, K] and w_e [K, cols] as multiplied (so w[e].t() for
    fwd, w[e] for dgrad):

        |got - ref| <= 2**-8 * |ref| + K * 2**-22 * (|a| @ |w_e|)

    First term: bf16 round-to-nearest of the fp32 sum s is off by at most
    half an ulp, which is 2**-8 * |s| at the bottom of a binade (8
    significant bits). Second term: worst-case fp32 accumulation of K
    products in any order, |s - ref| <= (K - 1) * 2**-24 * sum|a||w|; the
    factor 4 left over covers MFMA-internal summation and the 2**-8 * |s -
    ref| by which the first term, taken at ref, falls short. Nothing here is
    measured. A correct kernel can come within a few per cent of the bound
    (an element that rounds by nearly half an ulp), never past it."""
    x = gemm_excess(got, a, w_e, ref, K)
    assert x <= 1.0, f"{tag}: |got - ref| is {x:.3g} times the derived bound"


def wgrad_excess(got, dy, x, ref, n):
    dy, x, ref = (t.detach().cpu().to(F64) for t in (dy, x, ref))
    got = got.detach().cpu().to(F64)
    # an empty segment has a zero bound: got must then equal ref (zero)
    bound = n * 2.0 ** -22 * (dy.abs().t() @ x.abs())
    return _excess(got, ref, bound)


def assert_wgrad_close(got, dy, x, ref, n, tag="wgrad"):
    """One expert's fp32 dW [N, K] against fp64 ref = dy^T @ x over its n
    tokens (dy [n, N], x [n, K]): the fp32 accumulation term of
    assert_gemm_close alone, n * 2**-22 * (|dy|^T @ |x|); the output is not
    rounded to bf16. An empty expert must give exact zeros."""
    e = wgrad_excess(got, dy, x, ref, n)
    assert e <= 1.0, f"{tag}: |got - ref| is {e:.3g} times the derived bound"


# ------------------------------------------------- shared cases and checkers
MIXED = [255, 1, 256, 0, 513]
COUNT_PATTERNS = [
    [256],                        # a full tile with no padding
    [257],                        # one row into the second tile
    [1],                          # a single token
    [0, 5, 0],                    # empty experts around a small one
    [0, 0, 3],                    # leading empty experts
    [3, 0, 0],                    # trailing empties, tiles past total
    MIXED,                        # mixed sizes
    [0, 0, 0, 0, 0, 0, 0, 300],   # E = 8, all tokens in the last expert
    [1, 0, 1, 0],                 # decode: one token, top-2
]
GAUSS_SEEDS = (0, 1)


def pattern_id(counts):
    return "-".join(str(c) for c in counts)


def _draw(shape, lo, hi, gen, kind):
    if kind == "int":
        return int_inputs(shape, lo, hi, gen)
    return torch.randn(shape, generator=gen).to(torch.bfloat16)


def gemm_case(counts, w_shape, trans_b, seed, kind):
    """Sorted a [T, K] and w [E, N, Kw] for one grouped GEMM; kind "int"
    (a in -3..3, w in -2..3) or "gauss" (standard normal), both bf16."""
    gen = torch.Generator().manual_seed(seed)
    K = w_shape[1] if trans_b else w_shape[2]
    a = _draw((sum(counts), K), -3, 3, gen, kind)
    return a, _draw(tuple(w_shape), -2, 3, gen, kind)


def wgrad_case(counts, N, K, seed, kind):
    """Sorted dy [T, N] and x [T, K] for one grouped wgrad."""
    gen = torch.Generator().manual_seed(seed)
    dy = _draw((sum(counts), N), -2, 3, gen, kind)
    return dy, _draw((sum(counts), K), -3, 3, gen, kind)


def check_gemm(got, a_pad, w, counts, trans_b, kind, tag):
    """got: a [Tp, cols] bf16 result for the padded a_pad. Prints the
    measured figure, then asserts. "int": every row below total equals the
    reference element for element (padding rows of a segment: exactly zero).
    "gauss": each expert's rows within the derived bound and the padding
    rows of every segment exactly zero."""
    cl, _, pad = seg_bounds(counts)
    total = pad[-1]
    got = got.detach().cpu()
    ref = ref_gemm(a_pad, w, counts, trans_b)
    if kind == "int":
        print(f"{tag}: {count_mismatches(got[:total], ref[:total])} "
              f"mismatching elements of {total * got.size(1)}")
        assert_exact(got[:total], ref[:total], tag)
        return
    K = a_pad.size(1)
    worst = 0.0
    for e, c in enumerate(cl):
        sl = slice(pad[e], pad[e] + c)
        w_e = w[e] if trans_b else w[e].t()
        worst = max(worst, gemm_excess(got[sl], a_pad[sl], w_e, ref[sl], K))
    print(f"{tag}: max |got - ref| / bound = {worst:.4f}")
    for e, c in enumerate(cl):
        sl = slice(pad[e], pad[e] + c)
        w_e = w[e] if trans_b else w[e].t()
        assert_gemm_close(got[sl], a_pad[sl], w_e, ref[sl], K,
                          f"{tag} expert {e}")
        zero = got[pad[e] + c:pad[e + 1]]
        assert not bool((zero != 0).any() | torch.isnan(zero).any()), (
            f"{tag} expert {e}: non-zero padding row")


def check_wgrad(got, dy_pad, x_pad, counts, kind, tag):
    """got: [E, N, K] fp32 for the padded dy_pad, x_pad. Prints the measured
    figure, then asserts; an empty expert's dW must be exactly zero."""
    cl, _, pad = seg_bounds(counts)
    got = got.detach().cpu()
    ref = ref_wgrad(dy_pad, x_pad, counts)
    if kind == "int":
        print(f"{tag}: {count_mismatches(got, ref)} mismatching elements of "
              f"{got.numel()}")
        assert_exact(got, ref, tag)
        return
    ex = [wgrad_excess(got[e], dy_pad[pad[e]:pad[e] + c],
                       x_pad[pad[e]:pad[e] + c], ref[e], c)
          for e, c in enumerate(cl)]
    print(f"{tag}: max |got - ref| / bound = {max(ex):.4f}")
    for e, c in enumerate(cl):
        sl = slice(pad[e], pad[e] + c)
        assert_wgrad_close(got[e], dy_pad[sl], x_pad[sl], ref[e], c,
                           f"{tag} expert {e}")


def mlp_case(counts, H, I, seed):
    """bf16 x [T, H], gate_up [E, 2I, H], down [E, H, I], dout [T, H] with
    unit-variance pre-activations."""
    gen = torch.Generator().manual_seed(seed)
    E, T = len(counts), sum(counts)
    x = torch.randn(T, H, generator=gen)
    gu = torch.randn(E, 2 * I, H, generator=gen) / H ** 0.5
    dn = torch.randn(E, H, I, generator=gen) / I ** 0.5
    dout = torch.randn(T, H, generator=gen)
    return tuple(t.to(torch.bfloat16) for t in (x, gu, dn, dout))


MLP_TENSORS = ("y", "dx", "d_gate_up", "d_down")


def mlp_floor(x, counts, gu, dn, dout):
    """(ref, floor): the fp64 reference and, per tensor, rel_err between the
    references with and without the kernel's rounding points."""
    ref = ref_expert_mlp(x, counts, gu, dn, dout)
    rounded = ref_expert_mlp(x, counts, gu, dn, dout, round_like_kernel=True)
    return ref, {n: rel_err(rounded[n], ref[n]) for n in MLP_TENSORS}


def check_against_floor(got, ref, floor, tag, factor=2.0):
    """got, ref, floor: dicts by tensor name. Prints floor and measured
    error for every tensor, then asserts error <= factor * floor."""
    errs = {n: rel_err(got[n], ref[n]) for n in floor}
    print(f"{tag}: " + "  ".join(
        f"{n} err {errs[n]:.3e} floor {floor[n]:.3e}" for n in floor))
    for n in floor:
        assert torch.isfinite(got[n].detach().float()).all(), f"{tag}: {n}"
        assert errs[n] <= factor * floor[n], (
            f"{tag}: {n} rel err {errs[n]:.3e} > {factor} x floor "
            f"{floor[n]:.3e}")
    return errs


def kept_pairs(topi, counts):
    """keep [T, k] bool from the run's own routing: of the (token, choice)
    pairs that chose expert e, in token-major order, the first counts[e]
    were processed (all of them in dropless mode)."""
    flat = topi.reshape(-1).cpu()
    keep = torch.zeros_like(flat, dtype=torch.bool)
    for e, c in enumerate(int(c) for c in counts):
        keep[torch.nonzero(flat == e).squeeze(1)[:c]] = True
    return keep.view(topi.shape)


def run_moe_capture(moe, x, dout):
    """One forward and backward of a modules.moe.MoE. Returns (tensors,
    topi, keep): y and the gradients by name, and the routing decisions the
    run itself took (router output and per-expert counts, by hooks)."""
    seen = {}
    h1 = moe.router.register_forward_hook(
        lambda m, i, o: seen.__setitem__("topi", o[1].detach().cpu()))
    h2 = moe.experts.register_forward_pre_hook(
        lambda m, i: seen.__setitem__("counts", i[1].detach().cpu().tolist()))
    try:
        for p in moe.parameters():
            p.grad = None
        x = x.detach().clone().requires_grad_(True)
        y, _ = moe(x)
        y.backward(dout)
    finally:
        h1.remove()
        h2.remove()
    out = {"y": y.detach(), "dx": x.grad, "d_router": moe.router.weight.grad,
           "d_gate_up": moe.experts.gate_up.grad,
           "d_down": moe.experts.down.grad}
    return out, seen["topi"], kept_pairs(seen["topi"], seen["counts"])
