"""ZeRO1AdamW on MI355X against the independent fp64 reference of
tests/zero1_ref.py: the fused branch (ops/csrc/adamw.hip writing the bf16
weights in place next to the fp32 masters), the torch fallback on the same
device, a flat buffer long enough for the kernel's second grid-stride pass,
an expert parameter, manually assigned p.grad, exact resume, determinism,
no host sync inside step(), and the adamw_step argument contract.

One process, no process group: uninitialised parallel state is world size 1.
Bounds are zero1_ref's (|err| <= 1e-6 + 1e-5 |ref| for masters and moments,
2^-22 relative for grad_norm, bit-equality for everything else); every case
prints its measured err / tol before asserting."""

import pytest
import torch

from neuronx_distributed_training_amd.optim.zero1 import ZeRO1AdamW
from tests import zero1_ref as zr

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DEV = "cuda"
CLIPS = [1.0, 0.0, 1e4]  # active, off, on but inactive


@pytest.fixture(scope="module")
def ext():
    from neuronx_distributed_training_amd import ops

    return ops.require_extension()  # fail loudly if the .so is missing


@pytest.fixture(scope="module")
def scn():
    return zr.build_scenario()


@pytest.fixture(scope="module")
def refs(scn):
    return {c: scn.reference(c, device=DEV) for c in CLIPS}


class _CountingExt:
    """The real extension, with adamw_step calls recorded."""

    def __init__(self, ext):
        self._ext = ext
        self.p_bf16 = []  # one entry per call

    def adamw_step(self, *args, **kw):
        self.p_bf16.append(kw.get("p_bf16"))
        return self._ext.adamw_step(*args, **kw)


def _fused_cls(ext):
    proxy = _CountingExt(ext)

    class _Fused(ZeRO1AdamW):
        def _kernel_for(self, shard):
            assert shard.is_cuda
            return proxy

    return _Fused, proxy


class _Fallback(ZeRO1AdamW):
    def _kernel_for(self, shard):
        return None


def _run(scn, opt_cls, dtype, clip, steps=None, manual=False, expert=()):
    params = zr.make_params(scn, DEV, dtype, expert=expert)
    opt = zr.make_optimizer(opt_cls, scn, params, clip)
    norms = zr.drive(opt, params, scn, steps=steps, manual=manual)
    return opt, params, norms


def _state(opt, params):
    out = [opt.master_shard, opt.exp_avg, opt.exp_avg_sq, opt.param_flat]
    return [t.detach().clone() for t in out + list(params)]


# ------------------------------------------------------------- the scenario
@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_fused_matches_reference(ext, scn, refs, dtype, clip):
    cls, proxy = _fused_cls(ext)
    opt, params, norms = _run(scn, cls, dtype, clip)
    # one launch per step; bf16 models get the in-place weight write, fp32
    # models (the autocast recipe) leave it to shard_slice.copy_
    assert len(proxy.p_bf16) == scn.steps
    if dtype == BF:
        assert all(torch.is_tensor(x) and x.dtype == BF and
                   x.data_ptr() == opt.param_flat.data_ptr()
                   for x in proxy.p_bf16)
    else:
        assert all(x is None for x in proxy.p_bf16)
    zr.compare_with_reference(opt, params, refs[clip], norms, dtype,
                              f"gpu fused {dtype} clip {clip}")


@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_fallback_on_device_matches_reference(scn, refs, dtype, clip):
    opt, params, norms = _run(scn, _Fallback, dtype, clip)
    zr.compare_with_reference(opt, params, refs[clip], norms, dtype,
                              f"gpu fallback {dtype} clip {clip}")


def test_default_kernel_lookup_is_the_extension(ext, scn, refs):
    """No seam: the optimizer as the trainer builds it."""
    opt, params, norms = _run(scn, ZeRO1AdamW, BF, 1.0)
    assert opt._kernel_for(opt.grad_flat) is ext
    zr.compare_with_reference(opt, params, refs[1.0], norms, BF,
                              "gpu default lookup bf16 clip 1.0")


def test_second_grid_stride_pass(ext):
    """8,410,000 + 2 * 128 flat elements: more than the 8192 * 256 * 4 one
    pass of the kernel covers, so the tail of the large parameter and both
    small ones are updated in the second pass."""
    big = zr.build_scenario(
        named_shapes=(("big.weight", (2900, 2900)), ("tail.norm.weight", (5,)),
                      ("tail.w", (3, 7))),
        steps=2, micro=1, kmax=1, den=16, skip_odd=(), seed=1)
    cls, proxy = _fused_cls(ext)
    opt, params, norms = _run(big, cls, BF, 1.0)
    assert opt.master_shard.numel() > 8192 * 256 * 4
    assert opt.offsets[1] > 8192 * 256 * 4
    assert len(proxy.p_bf16) == 2
    ref = big.reference(1.0, device=DEV)
    assert min(ref.norms) > 1.0  # clip active
    zr.compare_with_reference(opt, params, ref, norms, BF,
                              "gpu fused second pass bf16 clip 1.0")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "fallback"])
def test_expert_parameter(ext, scn, refs, fused):
    """The eagerly updated expert parameter and its share of the global norm
    answer to the same reference; the clip is active, so a missing expert
    term would move every other parameter too."""
    cls = _fused_cls(ext)[0] if fused else _Fallback
    opt, params, norms = _run(scn, cls, BF, 1.0, expert=("l1.w",))
    assert [n for n, _ in opt.expert_named_params] == ["l1.w"]
    assert "l1.w" not in [n for n, _ in opt.named_params]
    zr.compare_with_reference(opt, params, refs[1.0], norms, BF,
                              f"gpu expert fused={fused}")


def test_manual_grad(ext, scn):
    cls, proxy = _fused_cls(ext)
    opt, params, norms = _run(scn, cls, BF, 1.0, steps=[0], manual=True)
    assert len(proxy.p_bf16) == 1
    zr.compare_with_reference(opt, params, scn.reference(1.0, DEV, steps=1),
                              norms, BF, "gpu manual p.grad")


# ----------------------------------------------------- resume, determinism
def _to_cpu(x):
    if torch.is_tensor(x):
        return x.detach().cpu().clone()
    if isinstance(x, dict):
        return {k: _to_cpu(v) for k, v in x.items()}
    if isinstance(x, list):
        return [_to_cpu(v) for v in x]
    return x


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_resume_is_bit_exact(ext, scn, dtype):
    straight = _state(*_run(scn, ZeRO1AdamW, dtype, 1.0)[:2])

    opt, params, _ = _run(scn, ZeRO1AdamW, dtype, 1.0, steps=[0, 1])
    saved = _to_cpu(opt.state_dict())
    del opt, params
    params = zr.make_params(scn, DEV, dtype)
    opt = zr.make_optimizer(ZeRO1AdamW, scn, params, 1.0)
    opt.load_state_dict(saved)
    assert opt.step_count == 2
    zr.drive(opt, params, scn, steps=[2, 3])
    resumed = _state(opt, params)
    names = ["master_shard", "exp_avg", "exp_avg_sq", "param_flat"] + scn.names
    for n, a, b in zip(names, straight, resumed):
        assert a.dtype == b.dtype and torch.equal(a, b), f"{n} differs"


def test_two_runs_are_bit_equal(ext, scn):
    a = _state(*_run(scn, ZeRO1AdamW, BF, 1.0)[:2])
    b = _state(*_run(scn, ZeRO1AdamW, BF, 1.0)[:2])
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# -------------------------------------------------------------- host syncs
def test_step_does_not_sync_with_the_host(ext, scn):
    """grad_scale stays a device scalar, so step() never waits for the GPU."""
    params = zr.make_params(scn, DEV, BF)
    opt = zr.make_optimizer(ZeRO1AdamW, scn, params, 1.0)
    zr.drive(opt, params, scn, steps=[0])  # first-use initialisation
    zr.backward_step(opt, params, scn, 1)
    one = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            one.item()  # the detector works on this build
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    ref = scn.reference(1.0, DEV, steps=2)
    assert abs(float(opt.grad_norm) - ref.norms[1]) <= zr.NORM_RTOL * ref.norms[1]


# ------------------------------------------------------- argument contract
def test_adamw_step_rejects_bad_arguments(ext):
    """Every violation is refused on the host, before any launch, and leaves
    p, m and v as they were."""
    n = 1024
    gen = torch.Generator(device=DEV).manual_seed(3)

    def f32(k=n):
        return torch.randn(k, device=DEV, generator=gen)

    good = {
        "p": f32(), "g": f32(), "m": f32(), "v": f32().abs(),
        "wd_mask": torch.ones(n, dtype=torch.bool, device=DEV),
        "step": 1,
        "grad_scale": torch.tensor(0.5, device=DEV),
        "p_bf16": torch.zeros(n, dtype=BF, device=DEV),
    }
    # views one element into a larger buffer: 4 bytes off (fp32), 2 and 4
    # bytes off (bf16)
    off32 = {k: f32(n + 4)[1:n + 1] for k in "pgmv"}
    wide16 = torch.zeros(n + 8, dtype=BF, device=DEV)
    bad = {
        "g on the host": {"g": good["g"].cpu()},
        "m on the host": {"m": good["m"].cpu()},
        "v on the host": {"v": good["v"].cpu()},
        "wd_mask on the host": {"wd_mask": good["wd_mask"].cpu()},
        "p_bf16 on the host": {"p_bf16": good["p_bf16"].cpu()},
        "grad_scale on the host": {"grad_scale": torch.tensor(0.5)},
        "p fp64": {"p": good["p"].double()},
        "g bf16": {"g": good["g"].to(BF)},
        "m fp16": {"m": good["m"].half()},
        "v fp64": {"v": good["v"].double()},
        "wd_mask uint8": {"wd_mask": good["wd_mask"].to(torch.uint8)},
        "wd_mask fp32": {"wd_mask": good["wd_mask"].float()},
        "p_bf16 fp16": {"p_bf16": good["p_bf16"].half()},
        "g strided": {"g": f32(2 * n)[::2]},
        "m strided": {"m": f32(2 * n)[::2]},
        "v strided": {"v": f32(2 * n)[::2]},
        "wd_mask strided": {
            "wd_mask": torch.ones(2 * n, dtype=torch.bool, device=DEV)[::2]},
        "g short": {"g": f32(n - 4)},
        "m short": {"m": f32(n - 4)},
        "v short": {"v": f32(n - 4)},
        "g long": {"g": f32(n + 4)},
        "wd_mask short": {"wd_mask": good["wd_mask"][:n - 4]},
        "p_bf16 short": {"p_bf16": good["p_bf16"][:n - 4]},
        "grad_scale two elements": {"grad_scale": torch.ones(2, device=DEV)},
        "grad_scale empty": {"grad_scale": torch.ones(0, device=DEV)},
        "step 0": {"step": 0},
        "step -1": {"step": -1},
        "p misaligned": {"p": off32["p"]},
        "g misaligned": {"g": off32["g"]},
        "m misaligned": {"m": off32["m"]},
        "v misaligned": {"v": off32["v"]},
        "p_bf16 2 bytes off": {"p_bf16": wide16[1:n + 1]},
        "p_bf16 4 bytes off": {"p_bf16": wide16[2:n + 2]},
    }
    for what, change in bad.items():
        a = dict(good, **change)
        watched = [a["p"], a["m"], a["v"], a["p_bf16"]]
        before = [t.detach().clone() for t in watched]
        with pytest.raises(RuntimeError):
            ext.adamw_step(a["p"], a["g"], a["m"], a["v"], a["wd_mask"],
                           1e-3, 0.9, 0.95, 1e-8, 0.01, a["step"],
                           grad_scale=a["grad_scale"], p_bf16=a["p_bf16"])
            pytest.fail(f"{what}: accepted")
        torch.cuda.synchronize()
        for t, b in zip(watched, before):
            assert torch.equal(t, b), f"{what}: a tensor changed"
    # and the unmodified arguments are accepted, with and without optionals
    ext.adamw_step(good["p"], good["g"], good["m"], good["v"],
                   good["wd_mask"], 1e-3, 0.9, 0.95, 1e-8, 0.01, 1,
                   grad_scale=good["grad_scale"], p_bf16=good["p_bf16"])
    assert torch.equal(good["p_bf16"], good["p"].to(BF))
    ext.adamw_step(good["p"], good["g"], good["m"], good["v"],
                   good["wd_mask"], 1e-3, 0.9, 0.95, 1e-8, 0.01, 2)
    assert torch.isfinite(good["p"]).all()
    assert not torch.equal(good["p_bf16"], good["p"].to(BF))
