"""Packed-sequence (segment-aware causal) flash attention, CPU side:
segment_bounds, the op's fp32 reference path with segment_ids, the argument
errors, ConcatDataset(segment_ids=True) and document isolation in the tiny
fp32 Llama."""

import pytest
import torch

from tests.segments_ref import dense_attention_seg, ids_from_lengths
from tests.test_llama_tp import TINY


# ------------------------------------------------------------ segment_bounds
def test_segment_bounds_layouts():
    from neuronx_distributed_training_amd.ops import segment_bounds

    seg = torch.tensor([
        [0, 0, 0, 0, 0, 0, 0, 0],   # a single segment
        [0, 0, 0, 1, 2, 2, 2, 2],   # a length-1 segment in the middle
        [0, 0, 0, 1, 1, 2, 2, 2],   # the last segment is a pad tail
        [5, 5, 7, 7, 7, 7, 9, 9],   # ids need not be consecutive
    ])
    q_start, k_end = segment_bounds(seg)
    assert q_start.dtype == torch.int32 and k_end.dtype == torch.int32
    assert q_start.shape == seg.shape and k_end.shape == seg.shape
    assert q_start.is_contiguous() and k_end.is_contiguous()
    assert q_start.tolist() == [
        [0, 0, 0, 0, 0, 0, 0, 0],
        [0, 0, 0, 3, 4, 4, 4, 4],
        [0, 0, 0, 3, 3, 5, 5, 5],
        [0, 0, 2, 2, 2, 2, 6, 6],
    ]
    assert k_end.tolist() == [
        [8, 8, 8, 8, 8, 8, 8, 8],
        [3, 3, 3, 4, 8, 8, 8, 8],
        [3, 3, 3, 5, 5, 8, 8, 8],
        [2, 2, 6, 6, 6, 6, 8, 8],
    ]
    # int32 ids work too; a 1-D tensor does not
    assert torch.equal(segment_bounds(seg.int())[0], q_start)
    with pytest.raises(ValueError):
        segment_bounds(seg[0])


# ------------------------------------------------- op reference fwd / bwd
@pytest.mark.parametrize("window", [0, 5])
def test_cpu_reference_segments(window):
    from neuronx_distributed_training_amd.ops import flash_attn_func

    torch.manual_seed(31)
    s = 40
    seg = ids_from_lengths([[40], [7, 1, 12, 20], [16, 16, 8]], s)
    b, hq, hkv, d = seg.size(0), 4, 2, 16
    q = torch.randn(b, hq, s, d, requires_grad=True)
    k = torch.randn(b, hkv, s, d, requires_grad=True)
    v = torch.randn(b, hkv, s, d, requires_grad=True)
    do = torch.randn(b, hq, s, d) + 3.0

    o = flash_attn_func(q, k, v, causal=True, window=window, segment_ids=seg)
    o.backward(do)
    ro, rdq, rdk, rdv = dense_attention_seg(q, k, v, seg, window=window,
                                            dout=do)
    for got, want in ((o, ro), (q.grad, rdq), (k.grad, rdk), (v.grad, rdv)):
        assert torch.isfinite(got).all()
        assert torch.allclose(got, want, atol=2e-5, rtol=1e-5), \
            (got - want).abs().max()
    # the single-segment row is plain causal attention
    dense = flash_attn_func(q[:1], k[:1], v[:1], causal=True, window=window)
    assert torch.allclose(o[:1], dense, atol=1e-6)


def test_segment_argument_errors():
    from neuronx_distributed_training_amd.ops import flash_attn_func

    torch.manual_seed(32)
    q, k, v = (torch.randn(2, 2, 12, 16) for _ in range(3))
    seg = ids_from_lengths([[12], [5, 7]], 12)
    flash_attn_func(q, k, v, segment_ids=seg)               # fine
    with pytest.raises(ValueError):                         # cross-length
        flash_attn_func(q[:, :, :4], k, v, segment_ids=seg[:, :4])
    with pytest.raises(ValueError):                         # non-causal
        flash_attn_func(q, k, v, causal=False, segment_ids=seg)
    with pytest.raises(ValueError):                         # both masks
        flash_attn_func(q, k, v, segment_ids=seg,
                        kv_range=(torch.zeros(2), torch.full((2,), 12)))
    with pytest.raises(ValueError):                         # wrong shape
        flash_attn_func(q, k, v, segment_ids=seg[:1])


# ------------------------------------------------------------ ConcatDataset
def _samples():
    mk = lambda a, n: {"input_ids": list(range(a, a + n)),
                       "labels": list(range(a, a + n))}
    # chunk 8: [3 + 4] pad 1 | [8 of the 10] | [2 left + 5] pad 1
    return [mk(10, 3), mk(20, 4), mk(30, 10), mk(50, 5)]


def test_concat_dataset_segment_ids():
    from neuronx_distributed_training_amd.data.packing import (
        ConcatDataset, IGNORE_INDEX,
    )

    ds = ConcatDataset(_samples(), 8, eos_token_id=2, segment_ids=True)
    assert len(ds) == 3
    seg = [ds[i]["segment_ids"].tolist() for i in range(3)]
    assert seg == [
        [0, 0, 0, 1, 1, 1, 1, 2],    # two samples, pad tail has its own id
        [0, 0, 0, 0, 0, 0, 0, 0],    # first 8 tokens of the split sample
        [0, 0, 1, 1, 1, 1, 1, 2],    # its rest starts a new segment
    ]
    I = IGNORE_INDEX
    assert ds[0]["labels"].tolist() == [I, 11, 12, I, 21, 22, 23, I]
    assert ds[1]["labels"].tolist() == [I, 31, 32, 33, 34, 35, 36, 37]
    assert ds[2]["labels"].tolist() == [I, 39, I, 51, 52, 53, 54, I]
    assert ds[0]["attention_mask"].tolist() == [1] * 7 + [0]
    assert ds[0]["input_ids"].tolist() == [10, 11, 12, 20, 21, 22, 23, 2]
    for i in range(3):
        it = ds[i]
        assert torch.equal(it["loss_mask"], (it["labels"] != I).float())
        # the pad tail is one trailing segment and nothing else
        pad = it["attention_mask"] == 0
        if pad.any():
            tail = it["segment_ids"][pad]
            assert (tail == tail[0]).all()
            assert (it["segment_ids"][~pad] != tail[0]).all()
        # non-decreasing
        assert (it["segment_ids"][1:] >= it["segment_ids"][:-1]).all()


def test_concat_dataset_default_unchanged():
    from neuronx_distributed_training_amd.data.packing import ConcatDataset

    ds = ConcatDataset(_samples(), 8, eos_token_id=2)
    assert len(ds) == 3
    it = ds[0]
    assert sorted(it) == ["attention_mask", "input_ids", "labels", "loss_mask"]
    assert it["input_ids"].tolist() == [10, 11, 12, 20, 21, 22, 23, 2]
    assert it["labels"].tolist() == [10, 11, 12, 20, 21, 22, 23, -100]
    assert it["attention_mask"].tolist() == [1] * 7 + [0]
    assert it["loss_mask"].tolist() == [1.0] * 7 + [0.0]
    assert ds[2]["labels"].tolist() == [38, 39, 50, 51, 52, 53, 54, -100]
    # same content with the flag on, apart from the first-token labels
    on = ConcatDataset(_samples(), 8, eos_token_id=2, segment_ids=True)
    for i in range(3):
        assert torch.equal(ds[i]["input_ids"], on[i]["input_ids"])
        assert torch.equal(ds[i]["attention_mask"], on[i]["attention_mask"])


def test_alignment_module_flag(tmp_path):
    """sft.packing_segment_mask reaches ConcatDataset; off by default."""
    import json
    from neuronx_distributed_training_amd.data.alignment import (
        ModelAlignmentDataModule,
    )

    path = tmp_path / "sft.jsonl"
    with open(path, "w") as f:
        for i in range(6):
            f.write(json.dumps({"prompt": f"q{i} ", "completion": "ab" * i})
                    + "\n")

    def items(**sft):
        cfg = {
            "data": {"kind": "alignment", "dataset_path": str(path),
                     "seq_length": 16, "global_batch_size": 1,
                     "micro_batch_size": 1, "tokenizer": "bytes"},
            "model_alignment_strategy": {"sft": {"packing": True, **sft}},
        }
        dm = ModelAlignmentDataModule(cfg)
        dm.setup()
        return [dm.train_ds[i] for i in range(len(dm.train_ds))]

    off = items()
    on = items(packing_segment_mask=True)
    assert all("segment_ids" not in it for it in off)
    assert all("segment_ids" in it for it in on)
    assert any(it["segment_ids"].max() > 0 for it in on)


# ------------------------------------------------------------ tiny Llama
def _model(activation_checkpoint=None, train=False):
    from neuronx_distributed_training_amd.parallel import state as ps
    from neuronx_distributed_training_amd.models.llama import (
        LlamaConfig, LlamaForCausalLM,
    )

    ps.destroy_model_parallel()
    ps.initialize_model_parallel()
    torch.manual_seed(7)
    m = LlamaForCausalLM(LlamaConfig(
        **TINY, activation_checkpoint=activation_checkpoint))
    return m.train() if train else m.eval()


def test_llama_documents_are_isolated():
    """Two documents in one row: document A's tokens do not reach document
    B's logits with segment_ids, and do without."""
    g = torch.Generator().manual_seed(41)
    ids = torch.randint(1, 128, (1, 32), generator=g)
    seg = ids_from_lengths([[13, 19]], 32)
    ids2 = ids.clone()
    ids2[0, :13] = torch.randint(1, 128, (13,), generator=g)
    assert not torch.equal(ids, ids2)
    model = _model()
    with torch.no_grad():
        a = model(ids, segment_ids=seg)
        b = model(ids2, segment_ids=seg)
        c = model(ids)
        d = model(ids2)
    assert torch.isfinite(a).all()
    assert (a[0, 13:] - b[0, 13:]).abs().max() <= 1e-6
    assert (a[0, :13] - b[0, :13]).abs().max() > 1e-3      # A itself moved
    assert (c[0, 13:] - d[0, 13:]).abs().max() > 1e-3      # dense leaks
    # document A alone is the same computation as A inside the pack
    with torch.no_grad():
        alone = model(ids[:, :13])
    assert torch.allclose(alone[0], a[0, :13], atol=1e-5)


def test_llama_segments_match_fp32_reference_and_checkpoint_modes():
    from tests.segments_ref import llama_fp32_logits_seg

    g = torch.Generator().manual_seed(42)
    ids = torch.randint(1, 128, (2, 32), generator=g)
    seg = ids_from_lengths([[9, 1, 14, 8], [32]], 32)
    lm = torch.ones(2, 32)
    lm[:, 1:] = (seg[:, 1:] == seg[:, :-1]).float()    # no cross-doc target

    def run(ckpt):
        model = _model(ckpt, train=True)
        loss = model(ids, labels=ids, loss_mask=lm, segment_ids=seg)
        loss.backward()
        return model, loss.detach(), {
            n: p.grad.clone() for n, p in model.named_parameters()}

    model, loss, grads = run(None)
    params = {n: p.detach().clone() for n, p in model.named_parameters()}
    with torch.no_grad():
        want = llama_fp32_logits_seg(params, model.cfg, ids, seg)
        got = model.eval()(ids, segment_ids=seg)
    assert torch.allclose(got, want, atol=1e-5), (got - want).abs().max()
    for ckpt in ("selective", "full"):
        _, loss_c, grads_c = run(ckpt)
        assert torch.allclose(loss, loss_c, atol=1e-6)
        for n in grads:
            assert torch.allclose(grads[n], grads_c[n], atol=1e-6), n


def test_llama_segment_rejections():
    from neuronx_distributed_training_amd.models.llama import KVCache

    ids = torch.randint(1, 128, (1, 32))
    seg = ids_from_lengths([[13, 19]], 32)
    model = _model()
    with pytest.raises(ValueError, match="KV cache"):
        model(ids, segment_ids=seg,
              kv_cache=KVCache(TINY["num_hidden_layers"]))
    with pytest.raises(ValueError, match="shape"):
        model(ids, segment_ids=seg[:, :16])


def test_trainer_module_passes_segment_ids():
    """model_fwd_calc_loss hands batch["segment_ids"] to the model."""
    from neuronx_distributed_training_amd.trainer.module import (
        BaseModelModule,
    )

    seen = {}

    class Stub:
        def __call__(self, input_ids, **kw):
            seen.update(kw)
            return torch.zeros(())

    class Mod:
        model = Stub()

    ids = torch.zeros(1, 4, dtype=torch.long)
    seg = torch.tensor([[0, 0, 1, 1]])
    BaseModelModule.model_fwd_calc_loss(Mod(), {"input_ids": ids})
    assert "segment_ids" not in seen
    BaseModelModule.model_fwd_calc_loss(
        Mod(), {"input_ids": ids, "segment_ids": seg})
    assert seen["segment_ids"] is seg
