"""Per-batch-row key ranges for flash attention (padded batches), CPU side:
mask_to_kv_range, the op's fp32 reference path with kv_range, and the tiny
fp32 Llama with padded_attention = "flash" vs "eager"."""

import pytest
import torch

from tests.kv_range_ref import dense_attention
from tests.test_llama_tp import TINY


# ---------------------------------------------------------------- helper
def test_mask_to_kv_range_pads():
    from neuronx_distributed_training_amd.ops import mask_to_kv_range

    am = torch.tensor([
        [0, 0, 0, 1, 1, 1, 1, 1],   # left pad
        [1, 1, 1, 1, 1, 0, 0, 0],   # right pad
        [0, 0, 1, 1, 1, 1, 0, 0],   # both sides
        [1, 1, 1, 1, 1, 1, 1, 1],   # all ones
        [0, 0, 0, 0, 0, 0, 0, 0],   # all zeros
        [0, 0, 0, 0, 0, 0, 0, 1],   # single token at the end
    ])
    lo, hi, contiguous = mask_to_kv_range(am)
    assert contiguous is True
    assert lo.dtype == torch.int32 and hi.dtype == torch.int32
    assert lo.tolist() == [3, 0, 2, 0, 0, 7]
    assert hi.tolist() == [8, 5, 6, 8, 0, 8]
    assert lo[4] == hi[4]                      # all-zero row: empty range


def test_mask_to_kv_range_hole():
    from neuronx_distributed_training_amd.ops import mask_to_kv_range

    am = torch.tensor([[1, 1, 1, 1, 1, 1], [0, 1, 1, 0, 1, 0]])
    lo, hi, contiguous = mask_to_kv_range(am)
    assert contiguous is False
    assert (lo.tolist(), hi.tolist()) == ([0, 1], [6, 5])
    # bool / float masks are accepted too
    assert mask_to_kv_range(am.bool())[2] is False
    assert mask_to_kv_range(am[:1].float())[2] is True


# ------------------------------------------------- op reference fwd / bwd
CASES = [
    # (sq, skv, ranges, causal, window)
    (40, 40, [(0, 40), (9, 40), (0, 17), (5, 23)], True, 0),
    (40, 40, [(12, 40), (0, 30)], True, 7),
    (8, 40, [(5, 40), (0, 35)], True, 0),          # S_q != S_kv
    (24, 24, [(3, 20), (7, 7)], False, 0),         # non-causal + degenerate
    (24, 24, [(6, 6), (0, 24)], True, 0),          # degenerate row
]


@pytest.mark.parametrize("sq,skv,ranges,causal,window", CASES)
def test_cpu_reference_kv_range(sq, skv, ranges, causal, window):
    from neuronx_distributed_training_amd.ops import flash_attn_func

    torch.manual_seed(11)
    b, hq, hkv, d = len(ranges), 4, 2, 16
    q = torch.randn(b, hq, sq, d, requires_grad=True)
    k = torch.randn(b, hkv, skv, d, requires_grad=True)
    v = torch.randn(b, hkv, skv, d, requires_grad=True)
    do = torch.randn(b, hq, sq, d) + 3.0       # non-zero on every row
    lo = torch.tensor([r[0] for r in ranges])
    hi = torch.tensor([r[1] for r in ranges])

    o = flash_attn_func(q, k, v, causal=causal, window=window,
                        kv_range=(lo, hi))
    o.backward(do)
    ro, rdq, rdk, rdv, alive = dense_attention(
        q, k, v, lo, hi, causal=causal, window=window, dout=do)

    for got, want in ((o, ro), (q.grad, rdq), (k.grad, rdk), (v.grad, rdv)):
        assert torch.isfinite(got).all()
        assert torch.allclose(got, want, atol=2e-5, rtol=1e-5), \
            (got - want).abs().max()
    # exact zeros: empty query rows, out-of-range keys
    empty = ~alive.any(-1).expand(b, hq, sq)             # [b, hq, sq]
    assert (o.detach()[empty] == 0).all()
    assert (q.grad[empty] == 0).all()
    j = torch.arange(skv)
    dead_key = (j[None] < lo[:, None]) | (j[None] >= hi[:, None])  # [b, skv]
    dead_key = dead_key[:, None].expand(b, hkv, skv)
    assert (k.grad[dead_key] == 0).all()
    assert (v.grad[dead_key] == 0).all()
    if causal and lo.max() > 0 and sq == skv:
        assert empty.any()                               # the case is live


def test_cpu_reference_full_range_is_dense():
    """kv_range = (0, S) for every row is the dense op."""
    from neuronx_distributed_training_amd.ops import flash_attn_func

    torch.manual_seed(12)
    q, k, v = (torch.randn(2, 2, 20, 16) for _ in range(3))
    full = (torch.zeros(2, dtype=torch.int32),
            torch.full((2,), 20, dtype=torch.int32))
    a = flash_attn_func(q, k, v, causal=True, kv_range=full)
    b = flash_attn_func(q, k, v, causal=True)
    assert torch.allclose(a, b, atol=1e-6)


def test_kv_range_is_clamped_and_checked():
    from neuronx_distributed_training_amd.ops import flash_attn_func

    torch.manual_seed(13)
    q, k, v = (torch.randn(2, 2, 12, 16) for _ in range(3))
    wild = (torch.tensor([-5, 9]), torch.tensor([99, 4]))   # hi < lo in row 1
    sane = (torch.tensor([0, 4]), torch.tensor([12, 4]))
    a = flash_attn_func(q, k, v, kv_range=wild)
    b = flash_attn_func(q, k, v, kv_range=sane)
    assert torch.equal(a, b)
    assert (a[1] == 0).all()
    with pytest.raises(ValueError):
        flash_attn_func(q, k, v, kv_range=(torch.zeros(3), torch.ones(3)))


# ------------------------------------------------------------ tiny Llama
def _model(padded_attention, activation_checkpoint=None, train=False):
    from neuronx_distributed_training_amd.parallel import state as ps
    from neuronx_distributed_training_amd.models.llama import (
        LlamaConfig, LlamaForCausalLM,
    )

    ps.destroy_model_parallel()
    ps.initialize_model_parallel()
    torch.manual_seed(7)
    m = LlamaForCausalLM(LlamaConfig(
        **TINY, padded_attention=padded_attention,
        activation_checkpoint=activation_checkpoint))
    return m.train() if train else m.eval()


def _batch(side, pad_token=0):
    """Two rows of 32 with 9 and 4 pad tokens on `side`."""
    g = torch.Generator().manual_seed(99)
    ids = torch.randint(1, 128, (2, 32), generator=g)
    am = torch.ones(2, 32, dtype=torch.long)
    for r, n in enumerate((9, 4)):
        sl = slice(0, n) if side == "left" else slice(32 - n, 32)
        am[r, sl] = 0
        ids[r, sl] = pad_token
    return ids, am


def _loss_and_grads(model, ids, am):
    model.zero_grad()
    # score a token only where it AND the position predicting it are real:
    # logits at pad positions are don't-care (and differ between the paths)
    lm = am.clone()
    lm[:, 1:] &= am[:, :-1]
    loss = model(ids, labels=ids, loss_mask=lm, attention_mask=am)
    loss.backward()
    return loss.detach(), {n: p.grad.clone()
                           for n, p in model.named_parameters()}


@pytest.mark.parametrize("side", ["left", "right"])
def test_llama_flash_matches_eager(side):
    ids, am = _batch(side)
    valid = am.bool()
    eager, flash = _model("eager"), _model("flash")
    with torch.no_grad():
        le = eager(ids, attention_mask=am)
        lf = flash(ids, attention_mask=am)
        # pad token VALUES must not matter at valid positions
        lf2 = flash(_batch(side, pad_token=77)[0], attention_mask=am)
    assert torch.isfinite(lf).all()
    assert torch.allclose(lf[valid], le[valid], atol=1e-5), \
        (lf[valid] - le[valid]).abs().max()
    assert torch.allclose(lf[valid], lf2[valid], atol=1e-5)

    loss_e, g_e = _loss_and_grads(eager, ids, am)
    loss_f, g_f = _loss_and_grads(flash, ids, am)
    assert abs(float(loss_e) - float(loss_f)) < 1e-5
    for n in g_e:
        assert torch.isfinite(g_f[n]).all(), n
        assert torch.allclose(g_f[n], g_e[n], atol=1e-5), \
            (n, (g_f[n] - g_e[n]).abs().max())


def test_llama_flash_takes_ranged_op(monkeypatch):
    """"flash" really routes through the ranged op (and "eager" / "auto" on
    CPU do not)."""
    from neuronx_distributed_training_amd.models import llama

    seen = []
    real = llama.flash_attn_func

    def spy(*a, **kw):
        seen.append(kw.get("kv_range"))
        return real(*a, **kw)

    monkeypatch.setattr(llama, "flash_attn_func", spy)
    ids, am = _batch("left")
    with torch.no_grad():
        _model("flash")(ids, attention_mask=am)
    assert len(seen) == TINY["num_hidden_layers"]
    assert all(r is not None for r in seen)
    assert seen[0][0].tolist() == [9, 4] and seen[0][1].tolist() == [32, 32]
    for mode in ("eager", "auto"):
        seen.clear()
        with torch.no_grad():
            _model(mode)(ids, attention_mask=am)
        assert seen == []                       # SDPA branch, as before


def test_llama_holed_mask_runs_eager():
    ids, am = _batch("right")
    am[0, 5] = 0                                # a hole inside row 0
    with torch.no_grad():
        le = _model("eager")(ids, attention_mask=am)
        lf = _model("flash")(ids, attention_mask=am)
    assert torch.equal(le, lf)


def test_llama_selective_checkpoint_ranged():
    ids, am = _batch("left")
    loss_a, g_a = _loss_and_grads(_model("flash", None, train=True), ids, am)
    loss_b, g_b = _loss_and_grads(
        _model("flash", "selective", train=True), ids, am)
    assert torch.allclose(loss_a, loss_b, atol=1e-6)
    for n in g_a:
        assert torch.allclose(g_a[n], g_b[n], atol=1e-6), n


def test_plain_fp32_llama_reference_matches_model():
    """The plain-PyTorch forward that the GPU model test uses as its fp32
    yardstick agrees with the model itself (CPU, fp32)."""
    from tests.kv_range_ref import llama_fp32_logits, masked_lm_loss

    ids, am = _batch("left")
    model = _model("eager")
    params = {n: p.detach().clone().requires_grad_(True)
              for n, p in model.named_parameters()}
    logits = llama_fp32_logits(params, model.cfg, ids, am)
    with torch.no_grad():
        want = model(ids, attention_mask=am)
    valid = am.bool()
    assert torch.allclose(logits[valid], want[valid], atol=1e-5)
    lm = am.clone()
    lm[:, 1:] &= am[:, :-1]
    loss = masked_lm_loss(logits, ids, lm)
    loss.backward()
    loss_m, g_m = _loss_and_grads(model, ids, am)
    assert abs(float(loss.detach()) - float(loss_m)) < 1e-5
    for n in g_m:
        assert torch.allclose(params[n].grad, g_m[n], atol=1e-5), n
