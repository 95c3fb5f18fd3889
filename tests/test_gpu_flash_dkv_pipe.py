"""The pipelined dK/dV backward kernel (flash_attn_bwd_dkv_pipe.hip, the
default) against the single-buffered kernel it replaced (the ``*_sbuf``
bindings), on MI355X. The new kernel changes how data moves, never what is
computed or in which order it is summed, so the two arms must agree bit for
bit: ``torch.equal`` on dQ, dK and dV, which catches a wrong LDS layout or a
mis-timed prefetch where a tolerance could let it through. (The tolerance
tests against fp32 are the existing dense / kv-range / segments files, which
run the new kernel as the default.)

Every case builds bf16 randn inputs, takes o / lse from the forward binding,
NaN-poisons the output sizes (every output is torch::empty), calls the
default binding and its ``_sbuf`` twin on the same inputs, and requires all
three gradients finite and equal, and two calls of the new kernel equal to
each other. Shapes are the smallest at which the new tile loop can go wrong:
zero to four q tiles (pipelines with no next tile), odd lengths (one row of
the last row pair past S_q), two or more key blocks, head_dim 64 (only half
the block stages), the XCD remap, windows that end the loop early, ranged
rows whose blocks have no tile (no tile load may be issued) and packed
segments whose boundaries fall on and inside tiles."""

import pytest
import torch

from tests.segments_ref import ids_from_lengths

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def ext():
    from neuronx_distributed_training_amd import ops

    return ops.require_extension()  # fail loudly if the .so is missing


def _poison(b, hq, hkv, sq, skv, d):
    """Fill-and-free NaN buffers of the backward's output sizes, as
    test_gpu_flash_dense.py does: an unwritten block shows."""
    g = hq // hkv
    junk = [torch.full(shape, float("nan"), device="cuda", dtype=dt)
            for shape, dt in (((sq, b, hq, d), BF),
                              ((g, skv, b, hkv, d), F32),
                              ((g, skv, b, hkv, d), F32),
                              ((b, hq, sq), F32))]
    del junk


def _inputs(b, hq, hkv, sq, skv, d, fused):
    """q, k, v, dout as [b, h, s, d]; `fused` gives the strides of
    models/llama.py (one [s, b, (hq + 2 hkv) d] projection split by
    columns)."""
    dev = "cuda"
    if not fused:
        return (torch.randn(b, hq, sq, d, device=dev, dtype=BF),
                torch.randn(b, hkv, skv, d, device=dev, dtype=BF),
                torch.randn(b, hkv, skv, d, device=dev, dtype=BF),
                torch.randn(b, hq, sq, d, device=dev, dtype=BF))
    assert sq == skv
    nq, nkv = hq * d, hkv * d
    leaf = torch.randn(sq, b, nq + 2 * nkv, device=dev, dtype=BF)
    qs, ks, vs = leaf.split([nq, nkv, nkv], dim=-1)
    q = qs.view(sq, b, hq, d).permute(1, 2, 0, 3)
    k = ks.view(sq, b, hkv, d).permute(1, 2, 0, 3)
    v = vs.view(sq, b, hkv, d).permute(1, 2, 0, 3)
    assert not q.is_contiguous()
    dout = torch.randn(sq, b, hq, d, device=dev, dtype=BF).permute(1, 2, 0, 3)
    return q, k, v, dout


def _ab(tag, dims, new_fn, old_fn):
    """new_fn / old_fn: () -> (dq, dk, dv). Poison before every call."""
    _poison(*dims)
    got = new_fn()
    _poison(*dims)
    want = old_fn()
    _poison(*dims)
    again = new_fn()
    for name, a, w, a2 in zip(("dq", "dk", "dv"), got, want, again):
        assert a.shape == w.shape, (tag, name)
        assert torch.isfinite(w.float()).all(), (tag, name, "sbuf")
        assert torch.isfinite(a.float()).all(), (tag, name, "pipe")
        assert torch.equal(a, w), (
            f"{tag}: {name} differs from the sbuf kernel in "
            f"{int((a != w).sum())} of {a.numel()} elements")
        assert torch.equal(a, a2), f"{tag}: {name} differs between two calls"


# (b, hq, hkv, sq, skv, d, causal, window, fused)
DENSE = [
    # zero to four tiles; odd lengths put one row of the last pair past S_q
    (1, 2, 1, s, s, 128, True, 0, False) for s in (1, 63, 64, 65, 129, 193)
] + [
    # two key blocks (the second starts at tile 4), six tiles, ragged tail,
    # production strides; head_dim 64 stages with half the block
    (2, 4, 2, 333, 333, 128, True, 0, True),
    (2, 8, 2, 333, 333, 64, True, 0, True),
    # five key blocks, 18 tiles, interior fast path, grid y = 8: XCD remap
    (1, 8, 2, 1100, 1100, 128, True, 0, False),
    # many blocks per head group, group 8
    (4, 64, 8, 300, 300, 128, True, 0, False),
    # non-causal, S_q != S_kv: the ring's hop shape
    (1, 4, 1, 256, 384, 128, False, 0, False),
    (1, 4, 1, 256, 384, 64, False, 0, False),
    # bottom-right causal with a window that ends the tile loop early
    (1, 4, 2, 128, 512, 128, True, 160, False),
    (1, 4, 2, 384, 384, 128, True, 100, False),
]


@pytest.mark.parametrize(
    "case", DENSE, ids=["-".join(str(x) for x in c) for c in DENSE])
def test_dense_pipe_equals_sbuf(ext, case):
    b, hq, hkv, sq, skv, d, causal, window, fused = case
    torch.manual_seed(DENSE.index(case))
    scale = d ** -0.5
    q, k, v, do = _inputs(b, hq, hkv, sq, skv, d, fused)
    o, lse = ext.flash_attn_fwd(q, k, v, causal, scale, window)
    args = (do, q, k, v, o, lse, causal, scale, window)
    _ab(str(case), (b, hq, hkv, sq, skv, d),
        lambda: ext.flash_attn_bwd(*args),
        lambda: ext.flash_attn_bwd_sbuf(*args))


def test_ranged_pipe_equals_sbuf(ext):
    """Rows: full; left pad; [270, 300) — key block 0 has no alive key, so no
    tile and no tile load; [100, 100) — every block empty."""
    torch.manual_seed(40)
    b, hq, hkv, s, d = 4, 4, 2, 333, 128
    scale = d ** -0.5
    q, k, v, do = _inputs(b, hq, hkv, s, s, d, False)
    lo = torch.tensor([0, 40, 270, 100], device="cuda", dtype=torch.int32)
    hi = torch.tensor([333, 333, 300, 100], device="cuda", dtype=torch.int32)
    o, lse = ext.flash_attn_fwd_range(q, k, v, lo, hi, True, scale, 0)
    args = (do, q, k, v, o, lse, lo, hi, True, scale, 0)
    _ab("ranged", (b, hq, hkv, s, s, d),
        lambda: ext.flash_attn_bwd_range(*args),
        lambda: ext.flash_attn_bwd_range_sbuf(*args))


# (s, per-row segment lengths)
SEGMENTED = [
    # a boundary on a tile edge, a one-token segment, a boundary inside a
    # tile; and one row that is a single segment
    (333, [[64, 1, 130, 138], [333]]),
    # key block 1 runs tiles 4-7 only, block 0 ends at tile 4
    (600, [[256, 256, 88]]),
]


@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("s,layouts", SEGMENTED, ids=["s333", "s600"])
def test_segmented_pipe_equals_sbuf(ext, s, layouts, d):
    from neuronx_distributed_training_amd.ops.flash_attn import segment_bounds

    torch.manual_seed(50 + d + s)
    b, hq, hkv = len(layouts), 4, 2
    scale = d ** -0.5
    q, k, v, do = _inputs(b, hq, hkv, s, s, d, False)
    qs, ke = segment_bounds(ids_from_lengths(layouts, s, device="cuda"))
    o, lse = ext.flash_attn_fwd_seg(q, k, v, qs, ke, scale, 0)
    args = (do, q, k, v, o, lse, qs, ke, scale, 0)
    _ab(f"segmented s={s} d={d}", (b, hq, hkv, s, s, d),
        lambda: ext.flash_attn_bwd_seg(*args),
        lambda: ext.flash_attn_bwd_seg_sbuf(*args))


def test_dkv_arm_switch(ext, monkeypatch):
    """NXDT_ATTN_DKV picks the binding the Python ops call; default pipe."""
    from neuronx_distributed_training_amd.ops.flash_attn import v2_bwd_fn

    monkeypatch.delenv("NXDT_ATTN_DKV", raising=False)
    assert v2_bwd_fn(ext) is ext.flash_attn_bwd
    monkeypatch.setenv("NXDT_ATTN_DKV", "sbuf")
    assert v2_bwd_fn(ext) is ext.flash_attn_bwd_sbuf
    assert v2_bwd_fn(ext, "_range") is ext.flash_attn_bwd_range_sbuf
    assert v2_bwd_fn(ext, "_seg") is ext.flash_attn_bwd_seg_sbuf
    monkeypatch.setenv("NXDT_ATTN_DKV", "pipe")
    assert v2_bwd_fn(ext, "_seg") is ext.flash_attn_bwd_seg
    monkeypatch.setenv("NXDT_ATTN_DKV", "other")
    with pytest.raises(ValueError):
        v2_bwd_fn(ext)
