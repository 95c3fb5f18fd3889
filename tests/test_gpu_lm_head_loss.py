"""Fused LM-head + cross-entropy on MI355X (ops/csrc/lm_head_loss.hip) against
fp64 computed from the same bf16 inputs. The kernel's block is 128 tokens x
128 vocab columns with K steps of 64; the grid is reordered in groups of 8
token tiles, and over the 8 XCDs when the block count is a multiple of 8.
Shapes (N, H, V):
  (1, 64, 8)       one row, one K step, one 8-column group
  (127, 64, 136)   one row short of a token tile; V one group past a vocab tile
  (129, 192, 264)  one row over a token tile; 3 K steps; 3 vocab tiles
  (300, 256, 1032) 3 token tiles, 4 K steps, 9 vocab tiles (27 blocks)
  (1100, 256, 904) 9 token tiles = a full group of 8 and a ragged one, 8 vocab
                   tiles; 72 blocks, so the XCD reordering is active"""

import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SHAPES = [(1, 64, 8), (127, 64, 136), (129, 192, 264), (300, 256, 1032),
          (1100, 256, 904)]
VOCAB_START = 1000


def bf_round(t):
    return t.float().to(BF).double()


def _rel(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


def _inputs(N, H, V, vocab_start):
    """Logits of about +-60: sigma * sqrt(2 ln(N V)) = 60. The first rows'
    targets are the shard's first and last column, then the ids just below and
    just above it (the latter a masked column of the last tile)."""
    g = torch.Generator().manual_seed(N + H + V)
    sigma = 60.0 / (2 * math.log(N * V)) ** 0.5
    hidden = torch.randn(N, H, generator=g).to(BF)
    weight = (torch.randn(V, H, generator=g) * sigma / H ** 0.5).to(BF)
    target = torch.randint(0, V, (N,), generator=g) + vocab_start
    edge = torch.tensor([0, V - 1, -1, V]) + vocab_start
    target[:4] = edge[:N]
    return hidden, weight, target, torch.randn(N, generator=g)


def _poison(*shapes):
    """NaN-filled, freed allocations: an unwritten torch::empty tile shows."""
    junk = [torch.full(s, float("nan"), device="cuda", dtype=dt)
            for s in shapes for dt in (BF, torch.float32)]
    del junk


def _stats64(logits, target):
    local = target - VOCAB_START
    own = (local >= 0) & (local < logits.size(1))
    tgt = logits.gather(1, local.clamp(0, logits.size(1) - 1)[:, None])[:, 0]
    return logits.logsumexp(1), tgt * own, own


@pytest.mark.parametrize("N,H,V", SHAPES)
def test_statistics_at_least_as_accurate_as_bf16_logits(N, H, V):
    """Bound: the error of fp64 statistics of the logits rounded to bf16, what
    the replaced path holds. Measured on MI355X, error / bound: log(sum) + max
    8.8e-7 / 2.7e-2 (N = 1) .. 1.3e-5 / 1.2e-1 (N = 1100); target logit
    3.6e-7 / 2.9e-2 .. 7.3e-6 / 9.2e-2."""
    from neuronx_distributed_training_amd import ops

    hidden, weight, target, _ = _inputs(N, H, V, VOCAB_START)
    logits = hidden.double() @ weight.double().T
    lse, tgt, own = _stats64(logits, target)
    lse_b, tgt_b, _ = _stats64(bf_round(logits), target)
    bound = [float((lse_b - lse).abs().max()), float((tgt_b - tgt).abs().max())]
    assert min(bound) >= 1e-4, bound
    runs = []
    for _ in range(2):
        _poison((N,), (N, -(-V // 128), 2))
        runs.append(ops.require_extension().lmhead_ce_fwd(
            hidden.cuda(), weight.cuda(), target.cuda(), VOCAB_START))
    for a, b in zip(*runs):
        assert a.dtype == torch.float32 and a.shape == (N,)
        assert torch.equal(a, b) and not bool(a.isnan().any())
    lmax, lsum, got_tgt = (t.double().cpu() for t in runs[0])
    err = [float((lsum.log() + lmax - lse).abs().max()),
           float((got_tgt - tgt).abs().max())]
    print(f"N {N} H {H} V {V}: lse, tgt err {err} bound {bound}")
    assert bool((got_tgt[~own] == 0).all())  # exactly 0 outside the shard
    assert err[0] <= bound[0] and err[1] <= bound[1]


@pytest.mark.parametrize("N,H,V", SHAPES)
def test_gradients_within_twice_rounding_floor(N, H, V):
    """dH and dW against fp64 autograd, random upstream gradient, chunks of 48
    or 128 rows (three or more, the last ragged, 48 not a multiple of the
    token tile; N = 1 has one chunk). Floor: fp64 that rounds dS, dH, and dW
    after every chunk, to bf16. Measured on MI355X: error / floor = 1.000 for
    both at all five shapes; floors dH 3.76e-3 .. 4.51e-3, dW 3.40e-3 ..
    6.49e-3."""
    from neuronx_distributed_training_amd.parallel.loss import (
        parallel_linear_cross_entropy,
    )

    hidden, weight, target, gout = _inputs(N, H, V, 0)
    target = target.clamp(0, V - 1)
    chunk = 48 if N < 200 else 128
    h64, w64 = (t.double().requires_grad_(True) for t in (hidden, weight))
    F.cross_entropy(h64 @ w64.T, target, reduction="none").backward(gout.double())
    with torch.no_grad():
        p = (h64 @ w64.T).softmax(1)
        p[torch.arange(N), target] -= 1
        ds = bf_round(p * gout.double()[:, None])
        emu_dh, emu_dw = bf_round(ds @ w64), torch.zeros_like(w64)
        for r0 in range(0, N, chunk):
            emu_dw = bf_round(emu_dw + ds[r0:r0 + chunk].T @ h64[r0:r0 + chunk])
    runs = []
    for _ in range(2):
        h, w = (t.cuda().requires_grad_(True) for t in (hidden, weight))
        _poison((N,), (N, -(-V // 128), 2))
        loss = parallel_linear_cross_entropy(h, w, target.cuda(), chunk)
        assert type(loss.grad_fn).__name__ == "_LinearCrossEntropyBackward"
        _poison((min(chunk, N), V), (N, H), (V, H))
        loss.backward(gout.cuda())
        runs.append((h.grad, w.grad))
    for (name, ref, emu), got, again in zip(
            (("dH", h64.grad, emu_dh), ("dW", w64.grad, emu_dw)), *runs):
        assert torch.equal(got, again) and not bool(got.isnan().any()), name
        err, floor = _rel(got, ref), _rel(emu, ref)
        print(f"N {N} H {H} V {V} {name}: gpu {err:.4e} floor {floor:.4e} "
              f"ratio {err / floor:.3f}")
        assert err <= 2 * floor, (name, err, floor)


def test_peak_memory_below_one_logits_tensor():
    """Default chunking (8 chunks of 512 rows): forward + backward peaks below
    one bf16 logits tensor above the pre-call level: an eighth of it for dS,
    plus the partials, dW and dH. Measured on MI355X: 50.0 of 256 MiB."""
    from neuronx_distributed_training_amd.parallel.loss import (
        parallel_linear_cross_entropy,
    )

    N, H, V = 4096, 256, 32768
    h = torch.randn(N, H, device="cuda", dtype=BF, requires_grad=True)
    w = torch.randn(V, H, device="cuda", dtype=BF, requires_grad=True)
    target = torch.randint(0, V, (N,), device="cuda")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    parallel_linear_cross_entropy(h, w, target).mean().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"peak {peak / 2**20:.1f} MiB of {N * V * 2 / 2**20:.1f} MiB")
    assert peak < N * V * 2 and bool(w.grad.isfinite().all())


@pytest.mark.parametrize("tied", [False, True])
def test_model_flag_on_and_off(tied):
    """2-layer bf16 model, 2 x 65 distinct tokens (128 loss rows), the same
    weights with the flag off and on. Each loss is within the bf16-logits
    bound of the fp64 loss, and each lm_head.weight.grad within twice the
    floor of its fp64 reference: dS^T @ hidden from the run's bf16 hidden
    states plus, tied, the run's gradient at the embedding output (tokens are
    distinct, so the embedding backward sums nothing). Measured on MI355X,
    untied / tied: loss error 8.6e-8 / 1.2e-8 (on), 4.4e-6 / 1.0e-5 (off),
    bound 9.0e-4 / 9.9e-4; dW error / floor = 1.000, floors 3.12e-3 / 4.13e-3."""
    from neuronx_distributed_training_amd.models.llama import (
        LlamaConfig, LlamaForCausalLM,
    )

    cfg = LlamaConfig(
        vocab_size=264, hidden_size=64, intermediate_size=128,
        num_hidden_layers=2, num_attention_heads=1, num_key_value_heads=1,
        max_position_embeddings=128, tie_word_embeddings=tied, dtype="bfloat16")
    model = LlamaForCausalLM(cfg).cuda()
    ids = (torch.arange(130) * 7 % 264).view(2, 65).cuda()  # all distinct
    seen = {}

    def keep_dx(m, a, out):
        out.register_hook(lambda gr: seen.__setitem__("dx", gr.detach()))

    model.model.register_forward_hook(
        lambda m, a, out: seen.__setitem__("hidden", out.detach()))
    model.model.embed_tokens.register_forward_hook(keep_dx)
    for flag in (False, True):
        cfg.fused_lm_head_loss = flag
        model.zero_grad(set_to_none=True)
        loss = model(ids, labels=ids)
        loss.backward()
        h64 = seen["hidden"][:, :-1].reshape(-1, 64).double().cpu()
        w64 = model.lm_head.weight.detach().double().cpu()
        labels = ids[:, 1:].reshape(-1).cpu()
        logits = h64 @ w64.T
        per_tok = F.cross_entropy(logits, labels, reduction="none")
        bound = float((F.cross_entropy(bf_round(logits), labels,
                                       reduction="none") - per_tok).abs().max())
        p = logits.softmax(1)
        p[torch.arange(128), labels] -= 1
        ref, emu = p.T @ h64 / 128, bf_round(bf_round(p / 128).T @ h64)
        if tied:
            dx = torch.zeros_like(w64).index_add_(
                0, ids.reshape(-1).cpu(),
                seen["dx"].reshape(-1, 64).double().cpu())
            ref, emu = ref + dx, bf_round(emu + dx)
        err, floor = _rel(model.lm_head.weight.grad, ref), _rel(emu, ref)
        loss_err = abs(float(loss.detach()) - float(per_tok.mean()))
        print(f"tied {tied} fused {flag}: loss err {loss_err:.3e} bound "
              f"{bound:.3e}; dW {err:.4e} floor {floor:.4e} "
              f"ratio {err / floor:.3f}")
        assert loss_err <= bound and err <= 2 * floor
