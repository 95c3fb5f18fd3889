"""CPU checks of tests/zero1_ref.py: the fp64 reference against
torch.optim.AdamW, ZeRO1AdamW's torch fallback against the reference, and
proof that the comparator sees each way the fused step could be subtly wrong
(planted through the `_kernel_for` seam)."""

import pytest
import torch

from neuronx_distributed_training_amd.optim.zero1 import ZeRO1AdamW
from tests import zero1_ref as zr

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64

CLIPS = [1.0, 0.0, 1e4]  # active, off, on but inactive


@pytest.fixture(scope="module")
def scn():
    return zr.build_scenario()


@pytest.fixture(scope="module")
def refs(scn):
    return {c: scn.reference(c) for c in CLIPS}


def test_scenario_exercises_what_it_claims(scn, refs):
    # clip 1.0 is active at every step, 1e4 never
    assert all(1.0 < n < 1e4 for n in refs[1.0].norms), refs[1.0].norms
    # offsets: every parameter but the last two leaves a padding gap
    assert [zr.decays(n, s) for n, s in zip(scn.names, scn.shapes)] == [
        True, False, True, False, False, True, True]
    i = scn.names.index("unused.weight")
    assert all((mb[i] is None) == (s % 2 == 1)
               for s in range(scn.steps) for mb in scn.k[s])
    # decay and momentum move the unused parameter on a step without gradient
    one = scn.reference(1.0, steps=1)
    two = scn.reference(1.0, steps=2)
    assert not torch.equal(one.params[i], two.params[i])
    assert torch.equal(two.exp_avg[i], scn.betas[0] * one.exp_avg[i])


def test_reference_matches_torch_adamw_fp64(scn):
    """Clip off, a decay group and a no-decay group, the same schedule."""
    ref = scn.reference(0.0)
    params = [torch.nn.Parameter(x.clone()) for x in scn.init]
    dec = [zr.decays(n, s) for n, s in zip(scn.names, scn.shapes)]
    opt = torch.optim.AdamW(
        [{"params": [p for p, d in zip(params, dec) if d],
          "weight_decay": scn.weight_decay},
         {"params": [p for p, d in zip(params, dec) if not d],
          "weight_decay": 0.0}],
        lr=scn.lrs[0], betas=scn.betas, eps=scn.eps)
    for s, grads in enumerate(scn.summed_grads()):
        for grp in opt.param_groups:
            grp["lr"] = scn.lrs[s]
        for p, g in zip(params, grads):
            p.grad = g.clone()
        opt.step()
    for i, p in enumerate(params):
        st = opt.state[p]
        for what, got, want in (("p", p.detach(), ref.params[i]),
                                ("m", st["exp_avg"], ref.exp_avg[i]),
                                ("v", st["exp_avg_sq"], ref.exp_avg_sq[i])):
            err = float((got - want).abs().max())
            assert err <= 1e-12, (scn.names[i], what, err)


def _run(scn, opt_cls, dtype, clip, **kw):
    params = zr.make_params(scn, "cpu", dtype)
    opt = zr.make_optimizer(opt_cls, scn, params, clip, **kw)
    norms = zr.drive(opt, params, scn)
    return opt, params, norms


@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_fallback_matches_reference(scn, refs, dtype, clip):
    opt, params, norms = _run(scn, ZeRO1AdamW, dtype, clip)
    zr.compare_with_reference(opt, params, refs[clip], norms, dtype,
                              f"cpu fallback {dtype} clip {clip}")


def test_manual_grad_matches_reference(scn):
    params = zr.make_params(scn, "cpu", BF)
    opt = zr.make_optimizer(ZeRO1AdamW, scn, params, 1.0)
    norms = zr.drive(opt, params, scn, steps=[0], manual=True)
    zr.compare_with_reference(opt, params, scn.reference(1.0, steps=1), norms,
                              BF, "cpu manual p.grad")


def test_expert_parameter_matches_reference(scn, refs):
    params = zr.make_params(scn, "cpu", BF, expert=("l1.w",))
    opt = zr.make_optimizer(ZeRO1AdamW, scn, params, 1.0)
    assert [n for n, _ in opt.expert_named_params] == ["l1.w"]
    norms = zr.drive(opt, params, scn)
    zr.compare_with_reference(opt, params, refs[1.0], norms, BF, "cpu expert")


# ------------------------------------------------------- planted mistakes
class MirrorKernel:
    """fp32 CPU mirror of the fused step with one optional mistake."""

    MISTAKES = ("decay_everywhere", "bias_correction_t_minus_1",
                "grad_scale_ignored", "grad_scale_twice", "eps_inside_sqrt",
                "master_from_bf16", "bf16_from_old_master", "bf16_not_written")

    def __init__(self, mistake=None):
        assert mistake is None or mistake in self.MISTAKES
        self.mistake = mistake

    def adamw_step(self, p, g, m, v, wd_mask, lr, b1, b2, eps, wd, t,
                   grad_scale=None, p_bf16=None):
        mk = self.mistake
        if mk == "master_from_bf16" and p_bf16 is not None:
            p.copy_(p_bf16.float())
        old = p.clone()
        gg = g.clone()
        if grad_scale is not None and mk != "grad_scale_ignored":
            gg = gg * grad_scale
            if mk == "grad_scale_twice":
                gg = gg * grad_scale
        if mk == "bias_correction_t_minus_1":
            t = max(t - 1, 1)  # finite, so the numbers have to give it away
        m.mul_(b1).add_(gg, alpha=1 - b1)
        v.mul_(b2).addcmul_(gg, gg, value=1 - b2)
        vhat = v / (1 - b2 ** t)
        denom = (vhat + eps).sqrt() if mk == "eps_inside_sqrt" \
            else vhat.sqrt() + eps
        decay = torch.full_like(p, 1.0 - lr * wd)
        if mk != "decay_everywhere":
            decay = torch.where(wd_mask, decay, torch.ones_like(p))
        p.mul_(decay).addcdiv_(m, denom, value=-(lr / (1 - b1 ** t)))
        if p_bf16 is not None and mk != "bf16_not_written":
            src = old if mk == "bf16_from_old_master" else p
            p_bf16.copy_(src.to(p_bf16.dtype))


def _mirror_opt(mistake):
    kern = MirrorKernel(mistake)

    class _Opt(ZeRO1AdamW):
        def _kernel_for(self, shard):
            return kern

    return _Opt


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_correct_mirror_passes(scn, refs, dtype):
    """The seam itself (fused branch of step()) with nothing planted."""
    opt, params, norms = _run(scn, _mirror_opt(None), dtype, 1.0)
    zr.compare_with_reference(opt, params, refs[1.0], norms, dtype,
                              f"cpu mirror {dtype}")


@pytest.mark.parametrize("mistake", MirrorKernel.MISTAKES)
def test_comparator_catches_planted_mistake(scn, refs, mistake):
    opt, params, norms = _run(scn, _mirror_opt(mistake), BF, 1.0)
    with pytest.raises(AssertionError):
        zr.compare_with_reference(opt, params, refs[1.0], norms, BF, mistake)


def test_comparator_catches_stale_gradient(scn, refs):
    """A parameter without gradient this step keeps last step's values in
    the flat buffer unless _finalize_one zeroes them."""

    class _Stale(ZeRO1AdamW):
        def _finalize_one(self, i):
            if self._touched[i]:
                return
            p, gview = self._grad_views[i]
            if p.grad is not None:
                gview.copy_(p.grad)
            self._touched[i] = True

    opt, params, norms = _run(scn, _Stale, BF, 1.0)
    with pytest.raises(AssertionError):
        zr.compare_with_reference(opt, params, refs[1.0], norms, BF, "stale")


def test_comparator_catches_missing_expert_norm_term(scn, refs):
    """A grad_norm that leaves the expert parameter out fails the norm check
    on its own, with every tensor right."""
    params = zr.make_params(scn, "cpu", BF, expert=("l1.w",))
    opt = zr.make_optimizer(ZeRO1AdamW, scn, params, 1.0)
    zr.drive(opt, params, scn)
    i = scn.names.index("l1.w")
    short = [float(sum((g * g).sum() for j, g in enumerate(gs) if j != i)
                   .sqrt().float())
             for gs in scn.summed_grads()]
    with pytest.raises(AssertionError, match="grad_norm"):
        zr.compare_with_reference(opt, params, refs[1.0], short, BF,
                                  "expert term missing from the norm")
