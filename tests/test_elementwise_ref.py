"""CPU checks of tests/elementwise_ref.py, the references and comparators the
GPU file test_gpu_elementwise_exact.py rests on:

- the fp64 references agree with fp64 autograd of the plain formulas
  (F.silu, F.cross_entropy, the rotate-half expression) to 1e-12;
- a torch fp32 emulation of each kernel's operation order, rounded once to
  bf16, passes the comparator: the bounds accept correct fp32 arithmetic;
- 22 planted mistakes, each a way one of the kernels could be subtly wrong,
  make the comparator raise; each test prints the factor by which it fails.

The emulations follow the kernels' formulas (ops/csrc/*.hip) line by line
but sum with torch's fp32 reductions, not in the kernels' thread order."""

import math

import pytest
import torch
import torch.nn.functional as F

from tests import elementwise_ref as R
from tests.elementwise_ref import BF, F32, F64


def _agree(got, want, what, tol=1e-12):
    err = float(((got - want).abs() / (1 + want.abs())).max())
    print(f"{what}: max |got - want| / (1 + |want|) = {err:.3e}")
    assert err <= tol, (what, err)


# ------------------------------------------------------------- emulations
def emu_rmsnorm(x, w, dy, eps, bug=None):
    """rmsnorm_fwd_kernel / rmsnorm_bwd_kernel in torch fp32. Returns
    (y bf16, invrms fp32, dx bf16, dw fp32)."""
    xf, wf, df = x.float(), w.float(), dy.float()
    n, h = xf.shape
    count = h + 8 if bug == "count" else h
    ss = (xf * xf).sum(1)
    r = torch.rsqrt(ss / count + (0.0 if bug == "no_eps" else eps))
    y = (xf * r[:, None] * wf).to(BF)
    rb = r.roll(-1) if bug == "neighbour_invrms" else r
    rb = rb[:, None]
    c = ((df if bug == "c_without_w" else wf * df) * xf * rb).sum(1) / h
    if bug == "c_halved":
        c = c / 2
    xhat = xf * rb
    dx = ((wf * df - xhat * c[:, None]) * rb).to(BF)
    terms = df * (xf if bug == "dw_from_x" else xhat)
    if bug == "dw_last_row":
        terms = terms[:-1]
    return y, r, dx, terms.sum(0)


def emu_swiglu(gu, dy, bug=None):
    """swiglu_fwd_kernel / swiglu_bwd_kernel in torch fp32."""
    i = gu.size(1) // 2
    g, u, d = gu[:, :i].float(), gu[:, i:].float(), dy.float()
    if bug == "swapped":
        g, u = u, g
    e = torch.exp(-g)
    y = (g / (1 + e) * u).to(BF)
    sig = 1 / (1 + e)
    ds = sig if bug == "dsilu_short" else sig * (1 + g * (1 - sig))
    dgate = (d * u * ds).to(BF)
    dup = (d * (sig if bug == "dup_from_sig" else g * sig)).to(BF)
    return y, dgate, dup


def emu_rope(x, cos, sin, off, off2=-1, sin_sign=1.0, bug=None):
    """rope_fwd_kernel in torch fp32; the backward is a call with
    sin_sign = -1, as ops/rope.py makes it."""
    if bug == "zigzag_swapped":
        off, off2 = off2, off
    p = R.rope_positions(x.size(2), off, off2)
    if bug == "position":
        p = p + 1
    h = x.size(3) // 2
    c, s = cos[p], sin[p] * sin_sign
    c0, c1, s0, s1 = c[:, :h], c[:, h:], s[:, :h], s[:, h:]
    if bug == "c_other_half":
        c0, c1 = c1, c0
    if bug == "s_other_half":
        s0, s1 = s1, s0
    x0, x1 = x[..., :h].float(), x[..., h:].float()
    return torch.cat((x0 * c0 - x1 * s0, x1 * c1 + x0 * s1), dim=-1).to(BF)


def emu_ce(full, target, gout, shards, bug=None):
    """ce_fwd_kernel per shard, the combination of parallel/loss.py, and
    ce_bwd_kernel per shard, in torch fp32. Returns (stats, loss, dlogits)
    with stats a list of (max, sumexp, tgt) and dlogits [n, shards * v]."""
    n, vt = full.shape
    v = vt // shards
    stats = []
    for i in range(shards):
        xs = full[:, i * v:(i + 1) * v].float()
        m = torch.zeros(n) if bug == "no_max" else xs.max(1).values
        e = torch.exp(xs - m[:, None])
        if bug == "skip_column":
            e = e[:, torch.arange(v) % 256 != 255 % v]
        start = 0 if bug == "vocab_start" else i * v
        t = target - start
        own = (t >= 0) & (t < v)
        tg = torch.where(own, xs.gather(1, t.clamp(0, v - 1)[:, None])[:, 0],
                         torch.zeros(n))
        stats.append((m, e.sum(1), tg))
    gmax = torch.stack([s[0] for s in stats]).max(0).values
    gsum = sum(s[1] * torch.exp(s[0] - gmax) for s in stats)
    loss = gsum.log() + gmax - sum(s[2] for s in stats)
    go = torch.ones(n) if bug == "gout" else gout.float()
    dls = []
    for i in range(shards):
        xs = full[:, i * v:(i + 1) * v].float()
        t = target - (0 if bug == "vocab_start" else i * v)
        if bug == "onehot_shift":
            t = t + 1
        onehot = (torch.arange(v)[None, :] == t[:, None]).float()
        p = torch.exp(xs - gmax[:, None]) * (1 / gsum)[:, None]
        if bug == "softmax_doubled":
            p = 2 * p
        if bug == "softmax_dropped":
            p = 0 * p
        dls.append(((p - onehot) * go[:, None]).to(BF))
    return stats, loss, torch.cat(dls, dim=1)


# ------------------------------------------------- reference vs autograd
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
def test_rmsnorm_ref_matches_autograd(eps):
    x, w, dy = R.rmsnorm_inputs(37, 264, 1)
    ref = R.rmsnorm_ref(x, w, dy, eps)
    xa = x.double().requires_grad_(True)
    wa = w.double().requires_grad_(True)
    r = torch.rsqrt(xa.pow(2).mean(-1, keepdim=True) + eps)
    y = xa * r * wa
    y.backward(dy.double())
    _agree(ref.y, y.detach(), "y")
    _agree(ref.invrms, r.detach()[:, 0], "invrms")
    _agree(ref.dx, xa.grad, "dx")
    _agree(ref.dw, wa.grad, "dw")


def test_swiglu_ref_matches_autograd():
    gu, dy = R.swiglu_inputs(6, 264, 2)
    ref = R.swiglu_ref(gu, dy)
    ga = gu.double().requires_grad_(True)
    g, u = ga.chunk(2, dim=-1)
    y = F.silu(g) * u
    y.backward(dy.double())
    _agree(ref.y, y.detach(), "y")
    _agree(ref.dgate, ga.grad[:, :264], "dgate")
    _agree(ref.dup, ga.grad[:, 264:], "dup")


def _rotate_half(t):
    t1, t2 = t.chunk(2, dim=-1)
    return torch.cat((-t2, t1), dim=-1)


@pytest.mark.parametrize("tables", ["real", "random"])
@pytest.mark.parametrize("off,off2", [(0, -1), (5, -1), (3, 21)])
def test_rope_ref_matches_autograd(tables, off, off2):
    b, h, s, d = 2, 3, 10, 16
    cos, sin = (R.rope_real_tables(40, d) if tables == "real"
                else R.rope_random_tables(40, d, 3))
    g = torch.Generator().manual_seed(4)
    x = torch.randn(b, h, s, d, generator=g).to(BF)
    dy = torch.randn(b, h, s, d, generator=g).to(BF)
    p = R.rope_positions(s, off, off2)
    if off2 >= 0:
        assert p.tolist() == [3, 4, 5, 6, 7, 21, 22, 23, 24, 25]
    xa = x.double().requires_grad_(True)
    y = xa * cos.double()[p] + _rotate_half(xa) * sin.double()[p]
    y.backward(dy.double())
    _agree(R.rope_fwd_ref(x, cos, sin, off, off2).y, y.detach(), "y")
    # the reference backward is the true transpose, whatever the tables
    _agree(R.rope_bwd_ref(dy, cos, sin, off, off2).y, xa.grad, "dx")


@pytest.mark.parametrize("n,v,shards", [(5, 40, 1), (5, 24, 3), (1, 8, 2)])
def test_ce_ref_matches_autograd(n, v, shards):
    full, target, gout = R.ce_inputs(n, v, shards, 5)
    ref = R.ce_ref(full, target, gout, shards)
    xa = full.double().requires_grad_(True)
    loss = F.cross_entropy(xa, target, reduction="none", ignore_index=-100)
    live = target >= 0
    _agree(ref.loss[live], loss.detach()[live], "loss")
    _agree(ref.lse, torch.logsumexp(full.double(), 1), "lse")
    # an ignored target: the loss is the lse, dlogits softmax times gout
    assert torch.equal(ref.loss[~live], ref.lse[~live])
    lse = torch.logsumexp(xa, 1)
    (loss * gout.double()).sum().backward(retain_graph=True)
    want = xa.grad.clone()
    xa.grad = None
    (lse * gout.double() * (~live)).sum().backward()
    want += xa.grad
    _agree(ref.dlogits, want, "dlogits")
    # per-shard statistics recombine to the full-row ones
    gmax = torch.stack([p.max for p in ref.per]).max(0).values
    gsum = sum(p.sumexp * torch.exp(p.max - gmax) for p in ref.per)
    _agree(gmax + gsum.log(), ref.lse, "recombined lse")
    assert torch.equal(gmax, ref.M)


def test_half_ulp():
    ref = torch.tensor([1.0, 1.5, 1.9999, 2.0, -3.0, 0.0, 2.0 ** -130, 1e4],
                       dtype=F64)
    want = torch.tensor([2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7,
                         2.0 ** -7, 0.0, 2.0 ** -134, 2.0 ** 5], dtype=F64)
    assert torch.equal(R.hu(ref), want)
    # one rounding to bf16 never exceeds it
    t = (torch.randn(100000) * 7).double()
    assert bool(((t.float().to(BF).double() - t).abs() <= R.hu(t)).all())


# ------------------------------------- emulation passes the comparator
RMS_SHAPES = [(5, 8), (3, 1032), (37, 4096), (150, 256), (2, 16384)]


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("n,h", RMS_SHAPES)
def test_rmsnorm_emulation_passes(n, h, eps):
    x, w, dy = R.rmsnorm_inputs(n, h, 10)
    ref = R.rmsnorm_ref(x, w, dy, eps)
    y, r, dx, dw = emu_rmsnorm(x, w, dy, eps)
    R.check_rmsnorm(ref, f"emu {n}x{h}", y=y, invrms=r, dx=dx, dw=dw)
    R.check_rmsnorm(ref, f"emu {n}x{h}", dw=dw.to(BF))


@pytest.mark.parametrize("n,i", [(4, 8), (3, 1032), (40, 2048)])
def test_swiglu_emulation_passes(n, i):
    gu, dy = R.swiglu_inputs(n, i, 11)
    y, dgate, dup = emu_swiglu(gu, dy)
    R.check_swiglu(R.swiglu_ref(gu, dy), f"emu {n}x{i}", y=y, dgate=dgate,
                   dup=dup)


@pytest.mark.parametrize("d,off,off2", [(128, 0, -1), (64, 37, -1),
                                        (128, 96, 896)])
def test_rope_emulation_passes(d, off, off2):
    b, h, s = 2, 4, 96
    g = torch.Generator().manual_seed(12)
    x = torch.randn(b, h, s, d, generator=g).to(BF)
    cos, sin = R.rope_random_tables(1024, d, 13)
    R.check_rope(R.rope_fwd_ref(x, cos, sin, off, off2),
                 emu_rope(x, cos, sin, off, off2), f"emu D={d} fwd")
    cos, sin = R.rope_real_tables(1024, d)
    R.check_rope(R.rope_fwd_ref(x, cos, sin, off, off2),
                 emu_rope(x, cos, sin, off, off2), f"emu D={d} real fwd")
    R.check_rope(R.rope_bwd_ref(x, cos, sin, off, off2),
                 emu_rope(x, cos, sin, off, off2, sin_sign=-1.0),
                 f"emu D={d} real bwd")


def _check_ce(ref, stats, loss, dl, what):
    for i, s in enumerate(stats):
        R.check_ce_stats(ref, i, what, *s)
    R.check_ce_loss(ref, loss, what)
    R.check_ce_dlogits(ref, dl, what)


@pytest.mark.parametrize("shards", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("v", [8, 255, 1001, 2056, 16032])
def test_ce_emulation_passes(v, n, shards):
    full, target, gout = R.ce_inputs(n, v, shards, 14)
    ref = R.ce_ref(full, target, gout, shards)
    _check_ce(ref, *emu_ce(full, target, gout, shards),
              f"emu V={v} N={n} x{shards}")


# --------------------------------------------------------- planted mistakes
def _must_fail(what, fn):
    with pytest.raises(R.BoundExceeded) as ei:
        fn()
    print(f"planted {what}: fails by {ei.value.ratio:.3g} x")
    return ei.value.ratio


@pytest.mark.parametrize("bug,outputs", [
    ("no_eps", ("y", "invrms", "dx")),
    ("count", ("y", "invrms")),
    ("c_halved", ("dx",)),
    ("c_without_w", ("dx",)),
    ("dw_last_row", ("dw", "dw_bf16")),
    ("dw_from_x", ("dw", "dw_bf16")),
    ("neighbour_invrms", ("dx",)),
])
def test_rmsnorm_planted(bug, outputs):
    x, w, dy = R.rmsnorm_inputs(37, 1032, 20)
    ref = R.rmsnorm_ref(x, w, dy, 1e-5)
    y, r, dx, dw = emu_rmsnorm(x, w, dy, 1e-5, bug=bug)
    got = {"y": dict(y=y), "invrms": dict(invrms=r), "dx": dict(dx=dx),
           "dw": dict(dw=dw), "dw_bf16": dict(dw=dw.to(BF))}
    for name in outputs:
        _must_fail(f"rmsnorm {bug} ({name})",
                   lambda: R.check_rmsnorm(ref, bug, **got[name]))


@pytest.mark.parametrize("bug,outputs", [
    ("swapped", ("y", "dgate", "dup")),
    ("dsilu_short", ("dgate",)),
    ("dup_from_sig", ("dup",)),
])
def test_swiglu_planted(bug, outputs):
    gu, dy = R.swiglu_inputs(3, 1032, 21)
    ref = R.swiglu_ref(gu, dy)
    y, dgate, dup = emu_swiglu(gu, dy, bug=bug)
    for name, t in (("y", y), ("dgate", dgate), ("dup", dup)):
        if name in outputs:
            _must_fail(f"swiglu {bug} ({name})",
                       lambda: R.check_swiglu(ref, bug, **{name: t}))


@pytest.mark.parametrize("bug", ["position", "c_other_half", "s_other_half",
                                 "zigzag_swapped"])
def test_rope_planted_forward(bug):
    b, h, s, d = 2, 4, 96, 128
    x = torch.randn(b, h, s, d,
                    generator=torch.Generator().manual_seed(22)).to(BF)
    cos, sin = R.rope_random_tables(1024, d, 23)
    ref = R.rope_fwd_ref(x, cos, sin, 96, 896)
    R.check_rope(ref, emu_rope(x, cos, sin, 96, 896), "control")
    _must_fail(f"rope {bug}", lambda: R.check_rope(
        ref, emu_rope(x, cos, sin, 96, 896, bug=bug), bug))


def test_rope_real_tables_hide_the_other_half():
    """Why the forward is tested with random tables: with the real ones a
    kernel reading c and s from the wrong half is bit-equal to a right one."""
    x = torch.randn(1, 2, 32, 64,
                    generator=torch.Generator().manual_seed(24)).to(BF)
    cos, sin = R.rope_real_tables(64, 64)
    good = emu_rope(x, cos, sin, 0)
    assert torch.equal(good, emu_rope(x, cos, sin, 0, bug="c_other_half"))
    assert torch.equal(good, emu_rope(x, cos, sin, 0, bug="s_other_half"))


def test_rope_planted_backward_sin_sign():
    b, h, s, d = 2, 4, 96, 128
    dy = torch.randn(b, h, s, d,
                     generator=torch.Generator().manual_seed(25)).to(BF)
    cos, sin = R.rope_real_tables(1024, d)
    ref = R.rope_bwd_ref(dy, cos, sin, 96, 896)
    R.check_rope(ref, emu_rope(dy, cos, sin, 96, 896, sin_sign=-1.0),
                 "control")
    _must_fail("rope backward sin sign", lambda: R.check_rope(
        ref, emu_rope(dy, cos, sin, 96, 896, sin_sign=1.0), "sin sign"))


@pytest.mark.parametrize("bug,check", [
    ("skip_column", "loss"),
    ("softmax_doubled", "dlogits"),
    ("softmax_dropped", "dlogits"),
    ("onehot_shift", "dlogits"),
    ("vocab_start", "dlogits"),
    ("vocab_start", "tgt"),
    ("gout", "dlogits"),
    ("no_max", "max"),
])
def test_ce_planted(bug, check):
    n, v, shards = 5, 1001, 3
    full, target, gout = R.ce_inputs(n, v, shards, 26)
    ref = R.ce_ref(full, target, gout, shards)
    stats, loss, dl = emu_ce(full, target, gout, shards, bug=bug)
    what = f"ce {bug} ({check})"
    if check == "loss":
        _must_fail(what, lambda: R.check_ce_loss(ref, loss, bug))
    elif check == "dlogits":
        _must_fail(what, lambda: R.check_ce_dlogits(ref, dl, bug))
    else:   # a per-shard statistic of the middle shard
        _must_fail(what, lambda: R.check_ce_stats(ref, 1, bug, *stats[1]))


def test_comparator_rejects_unwritten_and_unsharp():
    ref = torch.ones(8, dtype=F64)
    got = torch.ones(8, dtype=BF)
    R.assert_close(got, ref, "ok", sharp=0.01)
    bad = got.clone()
    bad[3] = math.nan
    with pytest.raises(AssertionError, match="non-finite"):
        R.assert_close(bad, ref, "nan")
    with pytest.raises(AssertionError, match="wrong for this bound"):
        R.assert_close(got, ref, "loose", k=2.0 ** 14, sharp=0.01)
    with pytest.raises(R.BoundExceeded):
        R.assert_close(got * 1.0079, ref, "one ulp off")
