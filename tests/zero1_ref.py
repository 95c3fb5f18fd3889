"""fp64 reference, scenario and comparator for the ZeRO-1 AdamW optimizer
(optim/zero1.py driving ops/csrc/adamw.hip), shared by
tests/test_zero1_ref.py (CPU) and tests/test_gpu_zero1.py.

Nothing here imports optim/zero1.py or mirrors its code: `reference_run` is
plain AdamW with decoupled decay on one fp64 tensor per parameter, and the
comparator reaches the optimizer only through its public layout
(`named_params`, `offsets`, `param_flat`, `master_shard`, `exp_avg`,
`exp_avg_sq`, `expert_state`).

The scenario makes the gradient every hook sees known exactly. The loss of a
microbatch is sum_i (p_i.float() * c_i).sum() with c_i = k_i * 2^(s % 3) / den,
k_i small integers, so dL/dp_i = c_i is exact in bf16, the fp32 sum over
microbatches is exact, and (asserted in the builder) the sum of all squared
gradients of a step is an integer below 2^24 in the unit (2^(s % 3) / den)^2:
every partial sum is then exact in fp32 in any order, and the optimizer's
fp32 norm differs from the fp64 one by its final sqrt rounding alone."""

import math
from dataclasses import dataclass, field

import torch

F64 = torch.float64
ALIGN = 128  # per-parameter padding of the flat buffers

# the project's AdamW bound (test_gpu_elementwise_edges.py)
ATOL, RTOL = 1e-6, 1e-5
# grad_norm: one fp32 sqrt rounding (2^-24) of an exact sum, with room
NORM_RTOL = 2.0 ** -22

DEFAULT_PARAMS = (
    ("emb.weight", (33, 65)),
    ("l0.norm.weight", (129,)),
    ("l0.proj.weight", (127, 3)),
    ("l0.proj.bias", (3,)),
    ("scalar", (1,)),
    ("l1.w", (128, 2)),
    ("unused.weight", (5, 7)),
)


def decays(name, shape):
    return not (len(shape) <= 1 or "bias" in name or "norm" in name)


# --------------------------------------------------------------- reference
@dataclass
class RefResult:
    names: list
    params: list
    exp_avg: list
    exp_avg_sq: list
    norms: list  # python floats, one per step (before clipping)

    def index(self, name):
        return self.names.index(name)


def reference_run(params, names, grads, lrs, betas, eps, weight_decay, clip):
    """params: initial values, one tensor per name. grads[s][i]: the summed
    gradient of parameter i at step s. lrs[s]: that step's learning rate.
    clip <= 0 turns clipping off. Everything is computed in fp64 on the
    device of `params`; bias corrections are python doubles."""
    b1, b2 = betas
    p = [x.to(F64).clone() for x in params]
    m = [torch.zeros_like(x) for x in p]
    v = [torch.zeros_like(x) for x in p]
    norms = []
    for s, (gs, lr) in enumerate(zip(grads, lrs)):
        t = s + 1
        gs = [g.to(F64) for g in gs]
        norm = math.sqrt(sum(float((g * g).sum()) for g in gs))
        norms.append(norm)
        scale = min(clip / (norm + 1e-6), 1.0) if clip and clip > 0 else 1.0
        bc1 = 1.0 - b1 ** t
        bc2 = 1.0 - b2 ** t
        for i, g in enumerate(gs):
            g = g * scale
            m[i] = b1 * m[i] + (1.0 - b1) * g
            v[i] = b2 * v[i] + (1.0 - b2) * g * g
            if decays(names[i], tuple(p[i].shape)):
                p[i] = p[i] * (1.0 - lr * weight_decay)
            p[i] = p[i] - (lr / bc1) * m[i] / ((v[i] / bc2).sqrt() + eps)
    return RefResult(list(names), p, m, v, norms)


# ---------------------------------------------------------------- scenario
@dataclass
class Scenario:
    names: list
    shapes: list
    init: list            # fp64 CPU tensors, every value exact in bf16
    k: list               # k[s][mb][i]: int32 CPU tensor, or None (not in loss)
    den: int
    lrs: list
    betas: tuple = (0.9, 0.95)
    eps: float = 1e-5
    weight_decay: float = 0.1
    _cache: dict = field(default_factory=dict, repr=False)

    @property
    def steps(self):
        return len(self.k)

    def unit(self, s):
        return 2.0 ** (s % 3) / self.den

    def coeff(self, s, mb, i, device):
        """c_i of microbatch mb at step s as fp32 on `device`, or None."""
        key = (s, mb, i, str(device))
        if key not in self._cache:
            k = self.k[s][mb][i]
            self._cache[key] = None if k is None else (
                k.to(device=device, dtype=torch.float32) * self.unit(s))
        return self._cache[key]

    def summed_grads(self, device="cpu"):
        """grads[s][i] in fp64: the sum over microbatches; zeros for a
        parameter that took no part in the loss at step s."""
        out = []
        for s in range(self.steps):
            row = []
            for i, shape in enumerate(self.shapes):
                tot = torch.zeros(shape, dtype=F64)
                for mb in self.k[s]:
                    if mb[i] is not None:
                        tot += mb[i].to(F64) * self.unit(s)
                row.append(tot.to(device))
            out.append(row)
        return out

    def reference(self, clip, device="cpu", steps=None):
        n = self.steps if steps is None else steps
        return reference_run(
            [x.to(device) for x in self.init], self.names,
            self.summed_grads(device)[:n], self.lrs[:n], self.betas, self.eps,
            self.weight_decay, clip)


def build_scenario(named_shapes=DEFAULT_PARAMS, steps=4, micro=3, kmax=4,
                   den=16, skip_odd=("unused.weight",), seed=0):
    """Parameters start at bf16-rounded N(0, 1) values. k is uniform in
    [-kmax, kmax]; parameters named in `skip_odd` take part in the loss at
    even step indices only. lr of step index s is 1e-2 * (s + 1) / steps.
    eps is 1e-5, not AdamW's usual 1e-8: clipped gradients here are about
    0.02, and at 1e-8 an eps on the wrong side of the square root would move
    no update by more than the bound."""
    gen = torch.Generator().manual_seed(seed)
    names = [n for n, _ in named_shapes]
    shapes = [tuple(s) for _, s in named_shapes]
    init = [torch.randn(s, generator=gen).to(torch.bfloat16).to(F64)
            for s in shapes]
    k = []
    for s in range(steps):
        k.append([
            [None if (n in skip_odd and s % 2 == 1) else
             torch.randint(-kmax, kmax + 1, sh, generator=gen,
                           dtype=torch.int32)
             for n, sh in zip(names, shapes)]
            for _ in range(micro)])
    scn = Scenario(names, shapes, init, k, den,
                   [1e-2 * (s + 1) / steps for s in range(steps)])
    # c and its sum over microbatches must be exact in bf16 (8 bits) ...
    assert micro * kmax <= 256 and den & (den - 1) == 0
    # ... and the squared norm exact in fp32 whatever the summation order:
    # every partial sum is an integer number of units below 2^24
    for s in range(steps):
        units = 0
        for i in range(len(names)):
            ks = sum(mb[i].long() for mb in k[s] if mb[i] is not None)
            if torch.is_tensor(ks):
                units += int((ks * ks).sum())
        assert 0 < units < 2 ** 24, (s, units)
    return scn


def make_params(scn, device, dtype, expert=()):
    """Fresh leaf parameters at the scenario's initial values; those named in
    `expert` carry the expert-parallel tag."""
    out = []
    for n, x in zip(scn.names, scn.init):
        p = torch.nn.Parameter(x.to(device=device, dtype=dtype))
        if n in expert:
            p.expert_model_parallel = True
        out.append(p)
    return out


def make_optimizer(opt_cls, scn, params, grad_clip, **kw):
    return opt_cls(list(zip(scn.names, params)), lr=scn.lrs[0],
                   betas=scn.betas, eps=scn.eps,
                   weight_decay=scn.weight_decay, grad_clip=grad_clip, **kw)


def backward_step(opt, params, scn, s):
    """Everything of step s up to, not including, opt.step()."""
    opt.set_lr(scn.lrs[s])
    opt.zero_grad()
    dev = params[0].device
    for mb in range(len(scn.k[s])):
        loss = None
        for i, p in enumerate(params):
            c = scn.coeff(s, mb, i, dev)
            if c is None:
                continue
            term = (p.float() * c).sum()
            loss = term if loss is None else loss + term
        loss.backward()


def manual_grad_step(opt, params, scn, s):
    """Like backward_step, but the summed gradient is assigned to p.grad in
    the parameter's dtype instead of coming from backward()."""
    opt.set_lr(scn.lrs[s])
    opt.zero_grad()
    for i, p in enumerate(params):
        if any(mb[i] is not None for mb in scn.k[s]):
            g = sum(mb[i].long() for mb in scn.k[s] if mb[i] is not None)
            p.grad = (g.to(torch.float32) * scn.unit(s)).to(
                device=p.device, dtype=p.dtype)


def drive(opt, params, scn, steps=None, manual=False):
    """Run the given step indices; returns grad_norm of each as a float."""
    norms = []
    for s in (range(scn.steps) if steps is None else steps):
        (manual_grad_step if manual else backward_step)(opt, params, scn, s)
        opt.step()
        norms.append(float(opt.grad_norm))
    return norms


# -------------------------------------------------------------- comparator
def _worst(got, want):
    err = (got.to(F64) - want).abs()
    return float((err / (ATOL + RTOL * want.abs())).max())


def compare_with_reference(opt, params, ref, norms, model_dtype, label=""):
    """Assert that a data-parallel-size-1 optimizer and its model parameters
    agree with `ref` (see the module docstring); prints and returns the
    worst err / tol per tensor kind."""
    total = opt.param_flat.numel()
    assert opt.shard_start == 0 and opt.master_shard.numel() == total
    by_id = {id(p): ref.index(n) for n, p in zip(ref.names, params)}
    assert len(opt.named_params) + len(opt.expert_state) == len(params)

    state = []  # (name, ref index, master, exp_avg, exp_avg_sq)
    live = torch.zeros(total, dtype=torch.bool, device=opt.param_flat.device)
    for (n, p), o in zip(opt.named_params, opt.offsets):
        assert o % ALIGN == 0, (n, o)
        sl = slice(o, o + p.numel())
        live[sl] = True
        state.append((n, by_id[id(p)], opt.master_shard[sl],
                      opt.exp_avg[sl], opt.exp_avg_sq[sl]))
    for (n, p), st in zip(opt.expert_named_params, opt.expert_state):
        assert st["param"] is p
        state.append((n, by_id[id(p)], st["master"].reshape(-1),
                      st["exp_avg"].reshape(-1), st["exp_avg_sq"].reshape(-1)))

    worst = {"master": 0.0, "exp_avg": 0.0, "exp_avg_sq": 0.0}
    bad = []
    for n, i, mst, ea, eas in state:
        for kind, got, want in (("master", mst, ref.params[i]),
                                ("exp_avg", ea, ref.exp_avg[i]),
                                ("exp_avg_sq", eas, ref.exp_avg_sq[i])):
            assert got.dtype == torch.float32, (n, kind, got.dtype)
            want = want.reshape(-1).to(got.device)
            w = _worst(got, want) if bool(torch.isfinite(got).all()) \
                else float("inf")
            worst[kind] = max(worst[kind], w)
            if not w <= 1.0:
                bad.append(f"{n} {kind}: err / tol = {w:.3g}")
    norm_err = max(abs(a - b) / b for a, b in zip(norms, ref.norms))
    print(f"zero1 {label}: worst err / tol  master {worst['master']:.3g}  "
          f"exp_avg {worst['exp_avg']:.3g}  "
          f"exp_avg_sq {worst['exp_avg_sq']:.3g}  "
          f"grad_norm rel err {norm_err:.3g} (bound {NORM_RTOL:.3g})")
    assert not bad, "; ".join(bad)
    assert len(norms) == len(ref.norms)
    assert norm_err <= NORM_RTOL, f"grad_norm {norms} vs {ref.norms}"

    # the model sees exactly the rounded masters, in its own dtype
    for n, i, mst, _, _ in state:
        p = params[i]
        assert p.dtype == model_dtype, (n, p.dtype)
        assert torch.equal(p.detach().reshape(-1), mst.to(model_dtype)), (
            f"{n}: model parameter is not master.to({model_dtype})")
    for n, p in opt.named_params:
        assert p.data_ptr() >= opt.param_flat.data_ptr() and (
            p.data_ptr() < opt.param_flat.data_ptr()
            + total * opt.param_flat.element_size()), f"{n} left param_flat"

    # padding between parameters stays exactly zero
    pad = ~live
    for name in ("param_flat", "master_shard", "exp_avg", "exp_avg_sq"):
        assert not bool(getattr(opt, name)[pad].any()), f"{name}: padding != 0"
    worst["grad_norm"] = norm_err
    return worst
