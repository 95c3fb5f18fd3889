"""The swapped-operand forward kernel (flash_attn_fwd_pipe.hip, the default)
against the double-buffered kernel it replaced (the ``*_dbuf`` bindings), on
MI355X. The new kernel changes how data moves (S^T from swapped MFMA
operands, packed P stores, one row max per lane, alpha and l crossing between
two register layouts through LDS, clamped unconditional tile loads, O staged
through LDS), never what is computed or in which order it is summed, so the
two arms must agree bit for bit: ``torch.equal`` on O and LSE, which catches a
wrong lane map or a mis-timed staging write where a tolerance could let it
through. (The tolerance tests against fp32 are the existing dense / kv-range /
segments / ring / long-sequence files, which run the new kernel as the
default.)

Every case builds seeded bf16 randn inputs, NaN-poisons buffers of the output
sizes (O and LSE are torch::empty) before every call, calls the default
binding and its ``_dbuf`` twin on the same inputs, and requires O and LSE
finite and equal, and two calls of the new kernel equal to each other. Shapes
are the smallest at which this tile loop can go wrong: no next tile, a ragged
last tile, one row past S_q, a second q block at both block heights, head_dim
64 (half the block stages V), the XCD remap, S_q != S_kv, windows that start
the loop late, ranged rows with an empty range or a q block with no alive
tile, and packed segments whose boundaries fall on and inside tiles."""

import pytest
import torch

from tests.segments_ref import ids_from_lengths

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def ext():
    from neuronx_distributed_training_amd import ops

    return ops.require_extension()  # fail loudly if the .so is missing


def _poison(b, hq, sq, d):
    """Fill-and-free NaN buffers of the forward's output sizes: an unwritten
    row shows."""
    junk = [torch.full(shape, float("nan"), device="cuda", dtype=dt)
            for shape, dt in (((sq, b, hq, d), BF), ((b, hq, sq), F32))]
    del junk


def _inputs(b, hq, hkv, sq, skv, d, fused):
    """q, k, v as [b, h, s, d]; `fused` gives the strides of models/llama.py
    (one [s, b, (hq + 2 hkv) d] projection split by columns)."""
    dev = "cuda"
    if not fused:
        return (torch.randn(b, hq, sq, d, device=dev, dtype=BF),
                torch.randn(b, hkv, skv, d, device=dev, dtype=BF),
                torch.randn(b, hkv, skv, d, device=dev, dtype=BF))
    assert sq == skv
    nq, nkv = hq * d, hkv * d
    leaf = torch.randn(sq, b, nq + 2 * nkv, device=dev, dtype=BF)
    qs, ks, vs = leaf.split([nq, nkv, nkv], dim=-1)
    q = qs.view(sq, b, hq, d).permute(1, 2, 0, 3)
    k = ks.view(sq, b, hkv, d).permute(1, 2, 0, 3)
    v = vs.view(sq, b, hkv, d).permute(1, 2, 0, 3)
    assert not q.is_contiguous()
    return q, k, v


def _ab(tag, dims, new_fn, old_fn):
    """new_fn / old_fn: () -> (o, lse). Poison before every call. Returns
    the new kernel's (o, lse)."""
    _poison(*dims)
    got = new_fn()
    _poison(*dims)
    want = old_fn()
    _poison(*dims)
    again = new_fn()
    for name, a, w, a2 in zip(("o", "lse"), got, want, again):
        assert a.shape == w.shape, (tag, name)
        assert torch.isfinite(w.float()).all(), (tag, name, "dbuf")
        assert torch.isfinite(a.float()).all(), (tag, name, "pipe")
        assert torch.equal(a, w), (
            f"{tag}: {name} differs from the dbuf kernel in "
            f"{int((a != w).sum())} of {a.numel()} elements")
        assert torch.equal(a, a2), f"{tag}: {name} differs between two calls"
    return got


# (b, hq, hkv, sq, skv, d, causal, window, fused)
DENSE = [
    # no next tile, ragged last tile, one row past S_q, a second (129) and
    # a third (257) q block; B * HQ = 2: 128-row blocks
    (1, 2, 1, s, s, 128, True, 0, False) for s in (1, 63, 64, 65, 129, 257)
] + [
    # six tiles, ragged tail, production strides; head_dim 64 stages V with
    # half the block
    (2, 4, 2, 333, 333, 128, True, 0, True),
    (2, 8, 2, 333, 333, 64, True, 0, True),
    # 18 tiles, interior fast path, grid y = 8: XCD remap
    (1, 8, 2, 1100, 1100, 128, True, 0, False),
    # B * HQ = 256, two q blocks each: 256-row blocks (NSB 2), group 8
    (4, 64, 8, 300, 300, 128, True, 0, False),
    (4, 64, 8, 300, 300, 64, True, 0, False),
    # non-causal, S_q != S_kv: the ring's hop shape
    (1, 4, 1, 256, 384, 128, False, 0, False),
    (1, 4, 1, 256, 384, 64, False, 0, False),
    # the same non-causal shape with B * HQ = 256: 256-row blocks
    (4, 64, 8, 256, 384, 128, False, 0, False),
    (4, 64, 8, 256, 384, 64, False, 0, False),
    # bottom-right causal with a window that starts the tile loop late
    (1, 4, 2, 128, 512, 128, True, 160, False),
    (1, 4, 2, 384, 384, 128, True, 100, False),
    # decode-like: one query, bottom-right causal
    (2, 4, 2, 1, 300, 128, True, 0, False),
]


@pytest.mark.parametrize(
    "case", DENSE, ids=["-".join(str(x) for x in c) for c in DENSE])
def test_dense_pipe_equals_dbuf(ext, case):
    b, hq, hkv, sq, skv, d, causal, window, fused = case
    torch.manual_seed(DENSE.index(case))
    scale = d ** -0.5
    q, k, v = _inputs(b, hq, hkv, sq, skv, d, fused)
    args = (q, k, v, causal, scale, window)
    _ab(str(case), (b, hq, sq, d),
        lambda: ext.flash_attn_fwd(*args),
        lambda: ext.flash_attn_fwd_dbuf(*args))


# (b, hq): 128-row blocks (few B * HQ blocks) and 256-row blocks (many)
@pytest.mark.parametrize("b,hq", [(3, 4), (3, 256)], ids=["bm128", "bm256"])
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
def test_ranged_pipe_equals_dbuf(ext, b, hq, causal):
    """S 200. Rows: [40, 200) left pad (tile 0 is half dead); [0, 150) right
    pad (the range ends inside tile 2, and the causal rows above 150 see
    their alive keys only below the diagonal tile); [130, 130) lo == hi: no
    tile at all, O exactly 0 and LSE exactly what dbuf stores."""
    torch.manual_seed(60 + b + hq + causal)
    hkv, s, d = hq // 2, 200, 128
    scale = d ** -0.5
    q, k, v = _inputs(b, hq, hkv, s, s, d, False)
    lo = torch.tensor([40, 0, 130], device="cuda", dtype=torch.int32)
    hi = torch.tensor([200, 150, 130], device="cuda", dtype=torch.int32)
    args = (q, k, v, lo, hi, causal, scale, 0)
    o, _ = _ab(f"ranged b{b} hq{hq} causal{causal}", (b, hq, s, d),
               lambda: ext.flash_attn_fwd_range(*args),
               lambda: ext.flash_attn_fwd_range_dbuf(*args))
    assert (o[2] == 0).all(), "lo == hi: O must be exactly 0"


@pytest.mark.parametrize("d", [128, 64])
def test_ranged_two_sided_and_block_without_tile(ext, d):
    """S 200, causal, 128-row blocks. Rows: [140, 180) two-sided inside
    tile 2: q block 0 (rows 0..127) ends at key 128 and starts at tile 2, so
    it has no alive tile, q block 1 has one; [0, 200) the whole row;
    [64, 128) two-sided on tile edges (exactly tile 1)."""
    torch.manual_seed(70 + d)
    b, hq, hkv, s = 3, 4, 2, 200
    scale = d ** -0.5
    q, k, v = _inputs(b, hq, hkv, s, s, d, False)
    lo = torch.tensor([140, 0, 64], device="cuda", dtype=torch.int32)
    hi = torch.tensor([180, 200, 128], device="cuda", dtype=torch.int32)
    args = (q, k, v, lo, hi, True, scale, 0)
    o, _ = _ab(f"ranged two-sided d{d}", (b, hq, s, d),
               lambda: ext.flash_attn_fwd_range(*args),
               lambda: ext.flash_attn_fwd_range_dbuf(*args))
    assert (o[0, :, :140] == 0).all(), "rows that see no key: O exactly 0"


# per-row segment lengths at S 300: boundaries on tile edges (64, 128) and
# inside tiles (70, 200), a single-token segment, a whole-row segment
SEG_LAYOUTS = [[64, 64, 72, 100], [70, 1, 129, 100], [300]]


@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("hq", [4, 128], ids=["bm128", "bm256"])
def test_segmented_pipe_equals_dbuf(ext, hq, d):
    from neuronx_distributed_training_amd.ops.flash_attn import segment_bounds

    torch.manual_seed(80 + d + hq)
    s = 300
    b, hkv = len(SEG_LAYOUTS), hq // 2
    scale = d ** -0.5
    q, k, v = _inputs(b, hq, hkv, s, s, d, False)
    qs, ke = segment_bounds(ids_from_lengths(SEG_LAYOUTS, s, device="cuda"))
    args = (q, k, v, qs, ke, scale, 0)
    _ab(f"segmented hq={hq} d={d}", (b, hq, s, d),
        lambda: ext.flash_attn_fwd_seg(*args),
        lambda: ext.flash_attn_fwd_seg_dbuf(*args))


def test_fwd_arm_switch(ext, monkeypatch):
    """NXDT_ATTN_FWD picks the binding the Python ops call; default pipe."""
    from neuronx_distributed_training_amd.ops.flash_attn import (
        _fwd_fn, v2_fwd_fn)

    monkeypatch.delenv("NXDT_ATTN_V3", raising=False)
    monkeypatch.delenv("NXDT_ATTN_FWD", raising=False)
    assert v2_fwd_fn(ext) is ext.flash_attn_fwd
    assert _fwd_fn(ext, 64, 64) is ext.flash_attn_fwd
    monkeypatch.setenv("NXDT_ATTN_FWD", "dbuf")
    assert v2_fwd_fn(ext) is ext.flash_attn_fwd_dbuf
    assert _fwd_fn(ext, 64, 64) is ext.flash_attn_fwd_dbuf
    assert v2_fwd_fn(ext, "_range") is ext.flash_attn_fwd_range_dbuf
    assert v2_fwd_fn(ext, "_seg") is ext.flash_attn_fwd_seg_dbuf
    monkeypatch.setenv("NXDT_ATTN_FWD", "pipe")
    assert v2_fwd_fn(ext) is ext.flash_attn_fwd
    assert v2_fwd_fn(ext, "_seg") is ext.flash_attn_fwd_seg
    monkeypatch.setenv("NXDT_ATTN_FWD", "other")
    with pytest.raises(ValueError):
        v2_fwd_fn(ext)
