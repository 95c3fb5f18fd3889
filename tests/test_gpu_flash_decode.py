"""Split-KV flash decode on MI355X: ops.flash_attn_decode over NaN-filled
cache buffers against fp64 dense attention with an explicit mask, built per
batch row from the slice k[b, :, :kv_hi[b]]; the binding's argument checks;
and a tiny bf16 Llama decoding a left-padded batch from a StaticKVCache."""

import pytest
import torch

from tests.kv_range_ref import alive_mask, llama_fp32_logits

pytestmark = pytest.mark.gpu

CAP = 700
# shorter than a 64-key tile / not a multiple of it / kv_lo inside a tile /
# full capacity / empty
RAGGED = [(0, 1), (0, 37), (5, 300), (130, 700), (40, 40)]
WIN = [(0, 333), (20, 333)]
# Forward bound of test_gpu_kernels.py / test_gpu_flash_kv_range.py.
O_BOUND = 0.02
LSE_BOUND = 4 * 8.065e-4  # see test_decode_vs_dense


@pytest.fixture(scope="module")
def ext():
    from neuronx_distributed_training_amd import ops

    return ops.require_extension()  # fail loudly if the .so is missing


def _reference(q, kc, vc, ranges, window):
    """fp64 O [B, HQ, SQ, D] and LSE [B, HQ, SQ] (empty rows: 0 / -1e30)."""
    b, hq, sq, d = q.shape
    g = hq // kc.size(1)
    o = torch.zeros(b, hq, sq, d, dtype=torch.float64, device=q.device)
    lse = torch.full((b, hq, sq), -1e30, dtype=torch.float64,
                     device=q.device)
    for r, (lo, hi) in enumerate(ranges):
        if hi == 0:
            continue
        k = kc[r, :, :hi].double().repeat_interleave(g, 0)
        v = vc[r, :, :hi].double().repeat_interleave(g, 0)
        alive = alive_mask(1, sq, hi, [lo], [hi], True, window, q.device)[0]
        s = torch.matmul(q[r].double(), k.transpose(-1, -2)) * d ** -0.5
        s = s.masked_fill(~alive, float("-inf"))
        some = alive.any(-1).expand(hq, sq)
        l = torch.logsumexp(s, dim=-1)
        p = torch.exp(s - torch.where(some, l, torch.zeros_like(l))[..., None])
        o[r] = torch.matmul(p, v) * some[..., None]
        lse[r] = torch.where(some, l, lse[r])
    return o, lse


@pytest.mark.parametrize("d,hq,hkv,sq,ranges,window,splits,permuted", [
    (128, 8, 2, 1, RAGGED, 0, None, False),
    (64, 4, 4, 3, RAGGED, 0, 3, False),
    (128, 8, 1, 3, RAGGED, 0, 1, False),      # 24 stacked rows: 2 M-tiles
    (64, 8, 1, 1, RAGGED, 0, 64, False),      # more splits than key tiles
    (128, 8, 1, 5, RAGGED, 0, None, False),   # 40 stacked rows: 4 M-tiles
    (64, 8, 1, 5, RAGGED, 0, 3, False),
    (128, 8, 2, 1, WIN, 0, 3, False),
    (128, 8, 2, 1, WIN, 100, 3, False),
    (64, 8, 2, 3, WIN, 100, None, False),
    (128, 4, 4, 1, RAGGED, 0, 3, True),       # [cap, b, hkv, d] storage
])
def test_decode_vs_dense(ext, d, hq, hkv, sq, ranges, window, splits,
                         permuted):
    """Measured on MI355X over these cases: max abs error of O 3.899e-03,
    of LSE 8.065e-04 (non-empty rows; the (64, 8, 2, 3, window 100) case);
    LSE_BOUND is four times the latter, to cover other seeds and split
    counts."""
    from neuronx_distributed_training_amd.ops import flash_attn_decode

    torch.manual_seed(d + hq + sq)
    b, dev, bf = len(ranges), "cuda", torch.bfloat16
    q = torch.randn(b, hq, sq, d, device=dev, dtype=bf)
    kc = torch.randn(b, hkv, CAP, d, device=dev, dtype=bf)
    vc = torch.randn(b, hkv, CAP, d, device=dev, dtype=bf)
    shape = (CAP, b, hkv, d) if permuted else (b, hkv, CAP, d)
    k = torch.full(shape, float("nan"), device=dev, dtype=bf)
    v = torch.full(shape, float("nan"), device=dev, dtype=bf)
    if permuted:
        k, v = k.permute(1, 2, 0, 3), v.permute(1, 2, 0, 3)
    for r, (lo, hi) in enumerate(ranges):
        k[r, :, lo:hi] = kc[r, :, lo:hi]
        v[r, :, lo:hi] = vc[r, :, lo:hi]
    lo_t = torch.tensor([r[0] for r in ranges], device=dev, dtype=torch.int32)
    hi_t = torch.tensor([r[1] for r in ranges], device=dev, dtype=torch.int32)
    max_kv = max(r[1] for r in ranges)
    ro, rlse = _reference(q, kc, vc, ranges, window)

    def call():
        return flash_attn_decode(q, k, v, hi_t, lo_t, max_kv=max_kv,
                                 window=window, num_splits=splits,
                                 return_lse=True)

    o, lse = call()
    o2, lse2 = call()
    empty = rlse == -1e30
    o_err = float((o.double() - ro).abs().max())
    lse_err = float((lse.double() - rlse)[~empty].abs().max())
    print(f"O max err {o_err:.3e}  LSE max err {lse_err:.3e}")
    assert o.shape == q.shape and lse.shape == (b, hq, sq)
    assert torch.isfinite(o.float()).all()
    assert o_err < O_BOUND
    assert lse_err < LSE_BOUND
    assert empty[-1].all() == (ranges is RAGGED)   # the (40, 40) row
    assert (o[empty] == 0).all() and (lse[empty] == -1e30).all()
    assert torch.equal(o, o2) and torch.equal(lse, lse2)


def test_binding_checks_decode_args(ext):
    bf = torch.bfloat16
    q = torch.randn(2, 8, 1, 64, device="cuda", dtype=bf)
    kv = torch.randn(2, 2, 128, 64, device="cuda", dtype=bf)
    lo = torch.zeros(2, device="cuda", dtype=torch.int32)
    hi = torch.full((2,), 128, device="cuda", dtype=torch.int32)
    ext.flash_attn_decode(q, kv, kv, lo, hi, 128, 0.125, 0, 0)
    q65 = torch.randn(2, 2, 65, 64, device="cuda", dtype=bf)     # G * S_q
    bad = [
        (q, kv, lo, hi.long(), 128),                             # dtype
        (q, kv, lo.cpu(), hi, 128),                              # device
        (q, kv, lo[:1], hi, 128),                                # shape
        (q65, kv, lo, hi, 128),
        (q, kv, lo, hi, 129),                                    # > CAP
        (q, kv[:, :, :, :32], lo, hi, 128),                      # head_dim
        (q[:, :3], kv, lo, hi, 128),                             # HQ % HKV
    ]
    for qq, kk, l, h, mk in bad:
        with pytest.raises(RuntimeError):
            ext.flash_attn_decode(qq, kk, kk, l, h, mk, 0.125, 0, 0)


def _tiny_bf16(padded_attention):
    from neuronx_distributed_training_amd.parallel import state as ps
    from neuronx_distributed_training_amd.models.llama import (
        LlamaConfig, LlamaForCausalLM,
    )

    ps.destroy_model_parallel()
    ps.initialize_model_parallel()
    torch.manual_seed(21)
    cfg = LlamaConfig(
        vocab_size=512, hidden_size=256, intermediate_size=512,
        num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
        max_position_embeddings=160, dtype="bfloat16",
        padded_attention=padded_attention,
    )
    return LlamaForCausalLM(cfg).cuda().eval()


def test_model_static_cache_left_padded_vs_fp32(ext, monkeypatch):
    """Prefill + 4 decode steps from a StaticKVCache on a left-padded batch:
    logits at real positions are as close to the fp32 model run row by row
    without padding as the eager bf16 full recompute of the padded batch
    is (err <= 2 * err_eager + 1e-3, test_gpu_flash_kv_range.py's bound)."""
    from neuronx_distributed_training_amd.models.llama import StaticKVCache

    calls = []
    real = ext.flash_attn_decode
    monkeypatch.setattr(ext, "flash_attn_decode",
                        lambda *a, **kw: calls.append(1) or real(*a, **kw))
    lens, s, steps = [90, 37, 64], 90, 4
    g = torch.Generator().manual_seed(22)
    ids = torch.randint(1, 512, (3, s + steps), generator=g).cuda()
    am = torch.ones(3, s + steps, dtype=torch.long, device="cuda")
    for r, n in enumerate(lens):
        am[r, :s - n] = 0
    ids = ids * am
    valid = am.bool()

    model = _tiny_bf16("auto")
    with torch.no_grad():
        cache = StaticKVCache(2, 3, s + steps)
        got = [model(ids[:, :s], kv_cache=cache, attention_mask=am[:, :s])]
        for t in range(steps):
            got.append(model(ids[:, s + t:s + t + 1], kv_cache=cache))
        got = torch.cat(got, dim=1).float()
        assert len(calls) == 2 * steps          # 2 layers x 4 decode steps
        eager = _tiny_bf16("eager")(ids, attention_mask=am).float()
        assert len(calls) == 2 * steps
        params = {n: p.detach().float() for n, p in model.named_parameters()}
        for r, n in enumerate(lens):
            row = ids[r:r + 1, s - n:]
            ref = llama_fp32_logits(params, model.cfg, row,
                                    torch.ones_like(row))[0]
            err = float((got[r][valid[r]] - ref).abs().max())
            err_e = float((eager[r][valid[r]] - ref).abs().max())
            print(f"row {r}: static err {err:.3e}  eager err {err_e:.3e}")
            assert torch.isfinite(got[r][valid[r]]).all()
            assert err <= 2 * err_e + 1e-3, (r, err, err_e)
