"""Ring-attention hop math in ONE process: a ring emulator drives
ops/ring_attn.py's _ring_fwd_hop / _ring_bwd_hop, the functions the
distributed autograd Function calls, for every (rank, hop) of a zigzag
ring and compares O, dQ, dK, dV of every rank with fp32 full causal
attention over the global sequence (GQA included).

The CPU variant (fp32) proves the emulator; the GPU variant runs the same
emulator through the HIP block kernels, where the j > r hop hands the
backward strided views (q_hi, o_hi, lse_hi) of the local tensors."""

import pytest
import torch

from neuronx_distributed_training_amd.ops import kernels_for
from neuronx_distributed_training_amd.ops.ring_attn import (
    _ring_bwd_hop, _ring_fwd_hop,
)
from tests.kv_range_ref import dense_attention


def _zigzag(t, R):
    """Global [b, h, 2R*c, d] -> per-rank local tensors, as parallel/cp.py
    places them: rank r holds chunks (r, 2R-1-r) concatenated."""
    ch = t.chunk(2 * R, dim=2)
    return [torch.cat([ch[r], ch[2 * R - 1 - r]], dim=2).contiguous()
            for r in range(R)]


def _unzigzag(parts):
    R = len(parts)
    slots = [None] * (2 * R)
    for r, p in enumerate(parts):
        lo, hi = p.chunk(2, dim=2)
        slots[r], slots[2 * R - 1 - r] = lo, hi
    return torch.cat(slots, dim=2)


def _emulate_ring(R, q, k, v, dout, scale):
    """Run every rank's forward hops, then every rank's backward hops, in
    the order and with the buffers _RingFlashAttnFn uses (communication
    replaced by indexing the peer's tensors). Returns global O, dQ, dK,
    dV."""
    kern = kernels_for(q)
    ql, kl, vl, dol = (_zigzag(t, R) for t in (q, k, v, dout))
    half = ql[0].size(2) // 2
    outs, lses = [], []
    for r in range(R):
        acc_o = torch.zeros(ql[r].shape, dtype=torch.float32, device=q.device)
        acc_lse = torch.full(ql[r].shape[:3], -1e30, dtype=torch.float32,
                             device=q.device)
        for t in range(R):
            j = (r - t) % R
            _ring_fwd_hop(kern, r, j, ql[r], kl[j], vl[j], acc_o, acc_lse,
                          scale)
        outs.append(acc_o.to(q.dtype))
        lses.append(acc_lse)

    dqs = []
    dks = [torch.zeros_like(x) for x in kl]   # the riding accumulators
    dvs = [torch.zeros_like(x) for x in vl]
    for r in range(R):
        dq_acc = torch.zeros_like(ql[r])
        for t in range(R):
            j = (r - t) % R
            dk_j, dv_j, lo_only = _ring_bwd_hop(
                kern, r, j, dol[r].contiguous(), ql[r], kl[j], vl[j],
                outs[r].contiguous(), lses[r], dq_acc, scale)
            if lo_only:
                dks[j][:, :, :half].add_(dk_j)
                dvs[j][:, :, :half].add_(dv_j)
            else:
                dks[j].add_(dk_j)
                dvs[j].add_(dv_j)
        dqs.append(dq_acc)
    return tuple(_unzigzag(x) for x in (outs, dqs, dks, dvs))


def _case(R, b, hq, hkv, c, d, dtype, device, seed):
    torch.manual_seed(seed)
    s = 2 * R * c
    q = torch.randn(b, hq, s, d, device=device).to(dtype)
    k = torch.randn(b, hkv, s, d, device=device).to(dtype)
    v = torch.randn(b, hkv, s, d, device=device).to(dtype)
    dout = torch.randn(b, hq, s, d, device=device).to(dtype)
    scale = d ** -0.5
    got = _emulate_ring(R, q, k, v, dout, scale)
    ref = dense_attention(q, k, v, [0] * b, [s] * b, causal=True,
                          scale=scale, dout=dout)[:4]
    return got, ref


@pytest.mark.parametrize("R", [2, 4])
def test_ring_hops_cpu_match_full_attention(R):
    got, ref = _case(R, 2, 4, 2, 8, 16, torch.float32, "cpu", seed=R)
    for name, g, r in zip(("o", "dq", "dk", "dv"), got, ref):
        err = float((g - r).abs().max())
        print(f"R={R} {name}: max err {err:.3e}")
        assert torch.allclose(g, r, atol=1e-4), (name, err)


@pytest.mark.gpu
@pytest.mark.parametrize("R,d", [(2, 128), (4, 128), (2, 64)])
def test_ring_hops_gpu_match_full_attention(R, d):
    """bf16 through the HIP kernels; the local half (c = 80) is no multiple
    of the 64-key tile or of any q-block size. Tolerances are
    test_gpu_kernels.py's: O max abs err < 0.02, grads
    max|err| / max(1, max|ref|) < 0.05."""
    got, ref = _case(R, 2, 4, 2, 80, d, torch.bfloat16, "cuda", seed=10 + R)
    o, ro = got[0], ref[0]
    assert torch.isfinite(o.float()).all()
    err = float((o.float() - ro).abs().max())
    print(f"R={R} d={d} o: max err {err:.5f}")
    assert err < 0.02, f"o max err {err}"
    for name, g, r in zip(("dq", "dk", "dv"), got[1:], ref[1:]):
        assert torch.isfinite(g.float()).all(), name
        rel = float((g.float() - r).abs().max() / r.abs().max().clamp(min=1))
        print(f"R={R} d={d} {name}: rel err {rel:.5f}")
        assert rel < 0.05, f"{name} rel err {rel}"
