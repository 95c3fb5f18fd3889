"""fp64 references, test inputs and comparators for the four small kernels
every model's forward and backward pass through: ops/csrc/rmsnorm.hip,
swiglu.hip, rope.hip and cross_entropy.hip. Shared by
tests/test_elementwise_ref.py (CPU) and tests/test_gpu_elementwise_exact.py.

Nothing here imports from ops/ or parallel/: every formula is written out in
fp64 from the same bf16 inputs the kernel reads, on whatever device they are.

One comparator (`assert_close`) holds a bf16 output to

    |got - ref| <= hu(ref) + k * 2^-23 * A + 2^-100

- hu(ref) = 2^(floor(log2 |ref|) - 8) is half a bf16 ulp of the reference:
  what the one final rounding to bf16 may cost, and never more;
- A is an fp64 magnitude of the terms that were added or cancelled on the way
  to that element, k the number of fp32 roundings (2^-23 each, one fp32 ulp
  relative, twice a correct rounding) on the kernel's path to it, counted
  from the kernel source below;
- 2^-100 covers results the kernel flushes to zero where fp64 still holds a
  number below the fp32 normal range times the inputs (sigmoid(-90) = 8e-40).
An fp32 output has no half-ulp term. Each check prints its worst err / tol
and raises `BoundExceeded` (with the factor in `.ratio`) past 1.

k, per kernel:
- RMSNorm (y, invrms, dx, dw's xhat): H / 256 + 16. A thread adds H / 256
  squares in sequence (H / 8 vectors over 256 threads, 8 elements each); the
  wave and block reductions add 6 + 2 levels; then the division by H, + eps,
  rsqrtf (assumed ~1 ulp) and the two or three multiplies of the output: 16
  covers those. The same count covers `c` of the backward, whose error enters
  dx through the third term of its A.
- RMSNorm dw: N + k. At most N fp32 adds per column (rows within a block in
  LDS, then one atomic per block), each relative to a partial sum that
  sum_rows |dy xhat| bounds, plus xhat's own k.
- SwiGLU: min(|g|, 90) + 8. __expf multiplies its argument by log2(e) in
  fp32 first, so the relative error of exp(-g) grows as |g| 2^-24; through
  1 - sig the backward turns an error of sig into |g| times that. Past
  |g| ~ 89 exp(-g) is 0 or inf in fp32 and sig is exactly 1 or 0: the growth
  stops, hence the cap. 8 covers the add, the division and the products.
- RoPE: 4. Two products and one add (or one product and one fma), and the
  sign product, which is exact.
- CE dlogits: the count sits inside A, (M - x) for the exp argument and
  V / 256 + 16 for the sum-exp it divides by (per-thread chain of V / 256
  adds, 6 + 4 combine steps), so k = 1.
- CE loss (fp32): 2^-23 (V / 256 + 16 + 2 (|M| + |lse| + |loss| + 1)): the
  sum-exp chain as above, and log, + max, - target each rounded at the size
  of its result.

What rests on hardware this file cannot know is the accuracy of __expf and
rsqrtf on gfx950 (assumed about 1 ulp); tests/README.md records what was
measured.

`assert_close(..., sharp=0.01)` also asserts that the bound is sharp for the
inputs at hand: the share of elements whose slack term k 2^-23 A exceeds a
quarter of the half-ulp term is at most 1 %. Otherwise the inputs are wrong
for the bound (all of the output would sit in a cancellation). And every
output element must be finite, which catches one that was never written into
its torch.empty buffer."""

import math
from types import SimpleNamespace

import torch

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U23 = 2.0 ** -23
FLOOR = 2.0 ** -100


class BoundExceeded(AssertionError):
    """An output is further from the reference than its bound; `.ratio` is
    the worst err / tol."""

    def __init__(self, msg, ratio):
        super().__init__(msg)
        self.ratio = ratio


# -------------------------------------------------------------- comparators
def hu(ref):
    """Half a bf16 ulp of each fp64 element: 2^(floor(log2 |ref|) - 8), the
    exponent held at the bf16 / fp32 minimum of -126; 0 for 0."""
    a = ref.abs()
    _, e = torch.frexp(a)                # a = m * 2^e, m in [0.5, 1)
    e = (e - 1).clamp(min=-126).to(F64)
    return torch.where(a > 0, torch.exp2(e - 8), torch.zeros_like(a))


def _f64(t, like):
    return t.detach().to(device=like.device, dtype=F64)


def assert_close(got, ref, what, A=None, k=1.0, half_ulp=True, sharp=None):
    """|got - ref| <= [hu(ref)] + k 2^-23 A + 2^-100 for every element, with
    A = |ref| by default; `half_ulp=False` for an fp32 output. Asserts shape,
    finiteness and, with `sharp`, the sharpness share. Prints and returns the
    worst err / tol."""
    assert tuple(got.shape) == tuple(ref.shape), (what, got.shape, ref.shape)
    g = _f64(got, ref)
    bad = int((~torch.isfinite(g)).sum())
    assert bad == 0, f"{what}: {bad} non-finite elements"
    A = ref.abs() if A is None else A
    slack = k * U23 * A
    half = hu(ref) if half_ulp else torch.zeros_like(ref)
    tol = half + slack + FLOOR
    ratio = float(((g - ref).abs() / tol).max()) if ref.numel() else 0.0
    line = f"{what}: worst err/tol {ratio:.4f}"
    if sharp is not None and ref.numel():
        share = float((slack > half / 4).double().mean())
        line += f"  unsharp share {share:.5f}"
    print(line)
    if sharp is not None and ref.numel():
        assert share <= sharp, (
            f"{what}: slack term above hu/4 on {share:.4f} of the elements "
            f"(> {sharp}): these inputs are wrong for this bound")
    if not ratio <= 1.0:
        raise BoundExceeded(f"{what}: err / tol = {ratio:.4g}", ratio)
    return ratio


def assert_exact(got, ref, what):
    """fp32 output that must equal the fp64 reference element for element
    (a maximum, a gathered logit: no arithmetic)."""
    g = _f64(got, ref)
    assert tuple(g.shape) == tuple(ref.shape), (what, g.shape, ref.shape)
    n = int((g != ref).sum())
    print(f"{what}: {n} elements differ")
    if n:
        raise BoundExceeded(f"{what}: {n} elements differ from the reference",
                            math.inf)
    return 0.0


# ------------------------------------------------------------------ RMSNorm
def rmsnorm_inputs(n, h, seed, device="cpu"):
    """x, w, dy in bf16. Rows r % 3 == 1 are scaled by 2^-10 (mean square
    ~1e-6: eps decides the result), rows r % 7 == 3 by 37; w = 1 + 0.3 randn
    (rounded to bf16, so an fp32 copy casts back without error)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, generator=g)
    rows = torch.arange(n)
    x[rows % 3 == 1] *= 2.0 ** -10
    x[rows % 7 == 3] *= 37.0
    w = 1 + 0.3 * torch.randn(h, generator=g)
    dy = torch.randn(n, h, generator=g)
    return tuple(t.to(BF).to(device) for t in (x, w, dy))


def rmsnorm_ref(x, w, dy, eps):
    """y = x r w, r = (mean x^2 + eps)^-1/2; dx = r (w dy - xhat c) with
    xhat = x r and c = mean(w dy xhat); dw = sum_rows dy xhat."""
    x, w, dy = (t.detach().to(F64) for t in (x, w, dy))
    n, h = x.shape
    r = 1.0 / torch.sqrt((x * x).sum(1, keepdim=True) / h + eps)
    xhat = x * r
    wdy = w * dy
    c = (wdy * xhat).sum(1, keepdim=True) / h
    cabs = (wdy * xhat).abs().sum(1, keepdim=True) / h
    return SimpleNamespace(
        n=n, h=h, k=h / 256 + 16,
        y=xhat * w, invrms=r.squeeze(1),
        dx=r * (wdy - xhat * c), dw=(dy * xhat).sum(0),
        A_dx=r * (wdy.abs() + (xhat * c).abs() + cabs * xhat.abs()),
        A_dw=(dy * xhat).abs().sum(0))


def check_rmsnorm(ref, what, y=None, invrms=None, dx=None, dw=None):
    """Checks whichever outputs are given; returns {name: worst err/tol}. dw
    in fp32 gets no half-ulp term, dw in bf16 does."""
    out = {}
    if y is not None:
        out["y"] = assert_close(y, ref.y, f"{what} y", k=ref.k, sharp=0.01)
    if invrms is not None:
        out["invrms"] = assert_close(invrms, ref.invrms, f"{what} invrms",
                                     k=ref.k, half_ulp=False)
    if dx is not None:
        out["dx"] = assert_close(dx, ref.dx, f"{what} dx", A=ref.A_dx,
                                 k=ref.k, sharp=0.01)
    if dw is not None:
        bf = dw.dtype == BF
        out["dw_bf16" if bf else "dw_fp32"] = assert_close(
            dw, ref.dw, f"{what} dw ({'bf16' if bf else 'fp32'})",
            A=ref.A_dw, k=ref.n + ref.k, half_ulp=bf)
    return out


# ------------------------------------------------------------------- SwiGLU
DSILU_ZERO = -1.2784645427610738  # 1 + g (1 - sigmoid(g)) = 0


def swiglu_inputs(n, i, seed, device="cpu"):
    """gate_up [n, 2 i] and dy [n, i] in bf16. Gates: 3 randn, with row 0 a
    linspace(-90, 90) and the first columns of the last row +-1e4, +-0, 88
    and, from 1024 elements up, the bf16 neighbours of the zero of dsilu."""
    g = torch.Generator().manual_seed(seed)
    gate = 3 * torch.randn(n, i, generator=g)
    gate[0] = torch.linspace(-90, 90, i)
    special = [1e4, -1e4, 0.0, -0.0, 88.0]
    if n * i >= 1024:   # dgate is a pure cancellation there: 3 elements
        special += [DSILU_ZERO, -1.28125, -1.2734375]  # stay under the 1 %
    gate[-1, :len(special)] = torch.tensor(special)
    up = torch.randn(n, i, generator=g)
    dy = torch.randn(n, i, generator=g)
    gu = torch.cat([gate, up], dim=1).to(BF)
    return gu.to(device), dy.to(BF).to(device)


def swiglu_ref(gu, dy):
    gu, dy = gu.detach().to(F64), dy.detach().to(F64)
    i = gu.size(1) // 2
    g, u = gu[:, :i], gu[:, i:]
    sig = torch.sigmoid(g)
    return SimpleNamespace(
        k=g.abs().clamp(max=90.0) + 8,
        y=g * sig * u,
        dgate=dy * u * sig * (1 + g * (1 - sig)),
        dup=dy * g * sig,
        A_dgate=(dy * u).abs() * sig * (1 + g.abs() * (1 - sig)))


def check_swiglu(ref, what, y=None, dgate=None, dup=None):
    out = {}
    if y is not None:
        out["y"] = assert_close(y, ref.y, f"{what} y", k=ref.k, sharp=0.01)
    if dgate is not None:
        out["dgate"] = assert_close(dgate, ref.dgate, f"{what} dgate",
                                    A=ref.A_dgate, k=ref.k, sharp=0.01)
    if dup is not None:
        out["dup"] = assert_close(dup, ref.dup, f"{what} dup", k=ref.k,
                                  sharp=0.01)
    return out


# --------------------------------------------------------------------- RoPE
def rope_real_tables(rows, d, base=500000.0, device="cpu"):
    """The tables a model uses: emb = cat(freqs, freqs), so both halves of a
    row are equal. fp32, as the kernel reads them."""
    inv = 1.0 / base ** (torch.arange(0, d, 2, dtype=F64) / d)
    emb = torch.outer(torch.arange(rows, dtype=F64), inv)
    emb = torch.cat((emb, emb), dim=1)
    return emb.cos().to(F32).to(device), emb.sin().to(F32).to(device)


def rope_random_tables(rows, d, seed, device="cpu"):
    """Independent values in all d columns of both tables: a kernel that
    reads c or s from the other half cannot hide behind equal halves."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, d, generator=g).to(device),
            torch.randn(rows, d, generator=g).to(device))


def rope_positions(s, off, off2=-1):
    """Row i takes position off + i; in the zigzag layout (off2 >= 0) rows
    [s/2, s) take off2 + (i - s/2)."""
    p = torch.arange(s) + off
    if off2 >= 0:
        p[s // 2:] = torch.arange(s - s // 2) + off2
    return p


def _rope_parts(x, cos, sin, off, off2):
    x = x.detach().to(F64)
    h = x.size(-1) // 2
    p = rope_positions(x.size(-2), off, off2).to(x.device)
    c, s = cos.to(F64)[p], sin.to(F64)[p]          # [s, d]
    return x[..., :h], x[..., h:], c[:, :h], c[:, h:], s[:, :h], s[:, h:]


def rope_fwd_ref(x, cos, sin, off=0, off2=-1):
    """The elementwise contract, any tables: x [b, h, s, d],
    y[d] = x[d] c[p,d] - x[d+D/2] s[p,d];
    y[d+D/2] = x[d+D/2] c[p,d+D/2] + x[d] s[p,d+D/2]."""
    x0, x1, c0, c1, s0, s1 = _rope_parts(x, cos, sin, off, off2)
    return SimpleNamespace(
        y=torch.cat((x0 * c0 - x1 * s0, x1 * c1 + x0 * s1), dim=-1),
        A=torch.cat(((x0 * c0).abs() + (x1 * s0).abs(),
                     (x1 * c1).abs() + (x0 * s1).abs()), dim=-1))


def rope_bwd_ref(dy, cos, sin, off=0, off2=-1):
    """The transpose of rope_fwd_ref's map:
    dx[d] = dy[d] c[p,d] + dy[d+D/2] s[p,d+D/2];
    dx[d+D/2] = dy[d+D/2] c[p,d+D/2] - dy[d] s[p,d].
    The kernel computes its backward as the forward with -sin, which equals
    this transpose only when the two halves of the sin table agree, as they
    do in every real table. So the backward is compared with real tables
    (rope_real_tables) only."""
    d0, d1, c0, c1, s0, s1 = _rope_parts(dy, cos, sin, off, off2)
    return SimpleNamespace(
        y=torch.cat((d0 * c0 + d1 * s1, d1 * c1 - d0 * s0), dim=-1),
        A=torch.cat(((d0 * c0).abs() + (d1 * s1).abs(),
                     (d1 * c1).abs() + (d0 * s0).abs()), dim=-1))


def check_rope(ref, got, what):
    return assert_close(got, ref.y, what, A=ref.A, k=4, sharp=0.01)


# ------------------------------------------------------------ cross-entropy
def ce_inputs(n, v, shards, seed, device="cpu"):
    """Full-vocabulary logits [n, shards * v] bf16, targets [n] and gout [n].
    Logits 4 randn; the second-to-last row (the only row at n = 1) has a
    60.0 outlier in the last column of shard shards // 2; row 0 has four
    -inf columns just before the last one (vocab padding). Targets: the
    shard edges (never the outlier's or a padded column: there the gradient
    is a pure cancellation and the loss infinite), and -100 in the last row
    when n > 1."""
    g = torch.Generator().manual_seed(seed)
    vt = shards * v
    full = 4 * torch.randn(n, vt, generator=g)
    full[max(n - 2, 0), v * (shards // 2 + 1) - 1] = 60.0
    full[0, vt - 5:vt - 1] = -math.inf
    edges = {1: [0, v - 1, 1, v - 2], 2: [v - 1, v, 2 * v - 1, 0],
             3: [v - 1, v, 2 * v - 1, 2 * v]}[shards]
    if n == 1:
        target = torch.tensor([v if shards > 1 else 0])
    else:
        target = torch.randint(0, vt - 5, (n,), generator=g)
        target[:4] = torch.tensor(edges)
        target[-1] = -100
    gout = torch.rand(n, generator=g) * 3 + 0.5
    gout[::2] *= -1
    return full.to(BF).to(device), target.to(device), gout.to(device)


def ce_ref(full, target, gout, shards):
    """Vocab-parallel cross-entropy over `shards` equal column shards.
    Per shard i: max_i, sumexp_i = sum exp(x - max_i), tgt_i = x[t] where the
    shard owns t, else 0. Combined: loss = M + log S - x[t] (x[t] = 0 for an
    ignored target, so the loss is the lse); dlogits = (p - onehot) gout."""
    x = full.detach().to(F64)
    n, vt = x.shape
    v = vt // shards
    gout = gout.to(F64)
    cols = torch.arange(vt, device=x.device)
    onehot = (cols[None, :] == target[:, None]).to(F64)   # none for -100
    per = []
    for i in range(shards):
        xs = x[:, i * v:(i + 1) * v]
        m = xs.max(1).values
        per.append(SimpleNamespace(
            max=m, sumexp=torch.exp(xs - m[:, None]).sum(1),
            tgt=(xs * onehot[:, i * v:(i + 1) * v]).nan_to_num(
                nan=0.0, neginf=0.0).sum(1)))
    M = x.max(1).values
    e = torch.exp(x - M[:, None])
    S = e.sum(1)
    lse = M + torch.log(S)
    tgt = sum(p.tgt for p in per)
    loss = lse - tgt
    p = e / S[:, None]
    gap = torch.where(p > 0, M[:, None] - x, torch.zeros_like(x))
    chain = v / 256 + 16
    for i, ps in enumerate(per):    # exp-argument term of each shard's sum
        xs = x[:, i * v:(i + 1) * v]
        es = torch.exp(xs - ps.max[:, None])
        gs = torch.where(es > 0, ps.max[:, None] - xs, torch.zeros_like(xs))
        ps.k_sumexp = chain + (es * gs).sum(1) / ps.sumexp
    return SimpleNamespace(
        n=n, v=v, shards=shards, per=per, M=M, S=S, lse=lse, loss=loss,
        tol_loss=U23 * (chain + 2 * (M.abs() + lse.abs() + loss.abs() + 1)),
        dlogits=(p - onehot) * gout[:, None],
        A_dl=(p * (gap + chain) + onehot) * gout.abs()[:, None])


def check_ce_stats(ref, i, what, lmax, lsum, tgt):
    """Shard i's forward outputs: max and target logit exact; sumexp within
    2^-23 (V / 256 + 16 + sum p |max - x|) relative, the last term being the
    exp-argument error weighted by each column's share of the sum."""
    ps = ref.per[i]
    assert_exact(lmax, ps.max, f"{what} shard {i} max")
    assert_exact(tgt, ps.tgt, f"{what} shard {i} tgt")
    return assert_close(lsum, ps.sumexp, f"{what} shard {i} sumexp",
                        k=ps.k_sumexp, half_ulp=False)


def check_ce_loss(ref, loss, what):
    return assert_close(loss, ref.loss, f"{what} loss",
                        A=ref.tol_loss / U23, k=1.0, half_ulp=False)


def check_ce_dlogits(ref, dl, what):
    """dl: [n, shards * v], the shards' outputs side by side."""
    return assert_close(dl, ref.dlogits, f"{what} dlogits", A=ref.A_dl,
                        k=1.0, sharp=0.01)
