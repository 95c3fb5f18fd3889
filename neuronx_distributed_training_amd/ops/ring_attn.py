"""Context-parallel ring attention over RCCL/xGMI P2P — zigzag layout.

Replaces the reference's NKI ring-attention kernel contract
(``nki_ring_attn_func(q, k, v, rank, cp_src_tgt_pairs)``, call site
modeling_llama.py:484 — SURVEY.md §2.3). MI355X-native decomposition:

- ZIGZAG placement (parallel/cp.py): rank r holds global chunks
  (c_r, c_{2R-1-r}) concatenated, so causal work is balanced across the
  ring — every hop is either the diagonal (causal, full local size) or a
  half-block (non-causal, half the score area), identical on all ranks.
- per hop, against the K/V of ring peer j:
    j == r: causal flash over the local chunk pair (positions of the
            concatenated halves are globally sorted, so plain causal
            masking is exact);
    j <  r: both key chunks of peer j... the LOW chunk c_j precedes all
            local queries (full attention), the HIGH chunk c_{2R-1-j}
            follows them (fully masked) → flash(q, k_lo, v_lo, non-causal);
    j >  r: both of peer j's chunks lie strictly between the local low
            and high chunks → flash(q_hi, k, v, non-causal), low-half
            queries see nothing.
- COMM/COMPUTE OVERLAP: the next hop's K/V irecv+isend are posted
  (batch_isend_irecv) BEFORE the current block's flash kernels run, so
  the xGMI hop hides under compute (round-1 had a blocking recv after
  each block — VERDICT weak #5).
- forward partials merge by log-sum-exp in fp32; backward evaluates each
  block's flash backward with the GLOBAL merged LSE (and delta from the
  global O), so the per-block pieces sum to the exact full-attention
  gradient. dK/dV accumulators ride the ring one hop behind their K/V
  block and arrive home after a final hop.
"""

from __future__ import annotations

import math
from typing import List

import torch
import torch.distributed as dist

from ..parallel import state as ps
from .flash_attn import _FlashAttnFn, _cpu_ref_fwd, _make_mask, v2_bwd_fn
from . import kernels_for


def _neighbors():
    ring = ps.get_context_model_parallel_ring_ranks()
    me = ps.get_context_model_parallel_rank()
    return ring[(me + 1) % len(ring)], ring[(me - 1) % len(ring)]


def _post_shift(send_tensors, recv_buffers):
    """Post one ring hop (send to next, recv from prev) WITHOUT blocking:
    returns the pending works to wait on after compute."""
    nxt, prv = _neighbors()
    group = ps.get_context_model_parallel_group()
    ops = []
    for t in send_tensors:
        ops.append(dist.P2POp(dist.isend, t, nxt, group=group))
    for b in recv_buffers:
        ops.append(dist.P2POp(dist.irecv, b, prv, group=group))
    return dist.batch_isend_irecv(ops)


def _fwd_block(kern, q, k, v, causal, scale):
    if kern is not None:
        o, lse = kern.flash_attn_fwd(q, k, v, causal, scale)
        return o, lse
    return _cpu_ref_fwd(q, k, v, causal, scale)


def _merge_into(acc_o, acc_lse, o, lse):
    """Online log-sum-exp merge of a block partial into the fp32 running
    accumulator (in place)."""
    new_lse = torch.logaddexp(acc_lse, lse)
    acc_o.mul_(torch.exp(acc_lse - new_lse).unsqueeze(-1))
    acc_o.add_(o.float() * torch.exp(lse - new_lse).unsqueeze(-1))
    acc_lse.copy_(new_lse)


def _cpu_block_bwd(do, q, k, v, out, lse, causal, scale):
    """Per-block flash backward with an externally-supplied (global) LSE."""
    hq, hkv = q.size(1), k.size(1)
    g = hq // hkv
    kx = k.repeat_interleave(g, 1).float()
    vx = v.repeat_interleave(g, 1).float()
    qf, dof = q.float(), do.float()
    s = torch.matmul(qf, kx.transpose(-1, -2)) * scale
    if causal:
        mask = _make_mask(q.size(-2), k.size(-2), True, 0, q.device)
        s = s.masked_fill(mask, float("-inf"))
    p = torch.exp(s - lse.unsqueeze(-1))
    dv = torch.matmul(p.transpose(-1, -2), dof)
    dp = torch.matmul(dof, vx.transpose(-1, -2))
    delta = (dof * out.float()).sum(-1, keepdim=True)
    ds = p * (dp - delta) * scale
    dq = torch.matmul(ds, kx)
    dk = torch.matmul(ds.transpose(-1, -2), qf)
    if g > 1:
        dk = dk.reshape(dk.size(0), hkv, g, dk.size(-2), dk.size(-1)).sum(2)
        dv = dv.reshape(dv.size(0), hkv, g, dv.size(-2), dv.size(-1)).sum(2)
    return dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype)


def _bwd_block(kern, do, q, k, v, out, lse, causal, scale):
    if kern is not None:
        return v2_bwd_fn(kern)(
            do.contiguous(), q, k, v, out, lse, causal, scale
        )
    return _cpu_block_bwd(do, q, k, v, out, lse, causal, scale)


def _ring_fwd_hop(kern, r, j, q, k_blk, v_blk, acc_o, acc_lse, scale):
    """One forward hop of rank ``r`` against ring peer ``j``'s K/V block:
    picks the zigzag case, slices, runs the block kernel and merges the
    partial into the fp32 accumulators (in place)."""
    half = q.size(2) // 2
    if j == r:
        o, lse = _fwd_block(kern, q, k_blk, v_blk, True, scale)
        _merge_into(acc_o, acc_lse, o, lse)
    elif j < r:
        o, lse = _fwd_block(
            kern, q, k_blk[:, :, :half], v_blk[:, :, :half], False, scale,
        )
        _merge_into(acc_o, acc_lse, o, lse)
    else:  # j > r: only the high-half queries see this block
        o, lse = _fwd_block(kern, q[:, :, half:], k_blk, v_blk, False, scale)
        _merge_into(acc_o[:, :, half:], acc_lse[:, :, half:], o, lse)


def _ring_bwd_hop(kern, r, j, dout, q, k_blk, v_blk, out, lse, dq_acc, scale):
    """One backward hop of rank ``r`` against ring peer ``j``'s K/V block,
    with the GLOBAL merged ``lse`` and ``out``. Adds this block's dQ into
    ``dq_acc`` (in place) and returns ``(dk_j, dv_j, lo_only)``; with
    ``lo_only`` the gradients cover only the block's LOW half."""
    half = q.size(2) // 2
    lo_only = j < r  # only this block's LOW chunk was visible
    if j == r:
        dq_j, dk_j, dv_j = _bwd_block(
            kern, dout, q, k_blk, v_blk, out, lse, True, scale
        )
        dq_acc += dq_j
    elif j < r:
        dq_j, dk_j, dv_j = _bwd_block(
            kern, dout, q, k_blk[:, :, :half], v_blk[:, :, :half],
            out, lse, False, scale,
        )
        dq_acc += dq_j
    else:  # j > r
        dq_j, dk_j, dv_j = _bwd_block(
            kern, dout[:, :, half:], q[:, :, half:], k_blk, v_blk,
            out[:, :, half:], lse[:, :, half:], False, scale,
        )
        dq_acc[:, :, half:] += dq_j
    return dk_j, dv_j, lo_only


class _RingFlashAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale):
        R = ps.get_context_model_parallel_world_size()
        r = ps.get_context_model_parallel_rank()
        kern = kernels_for(q)
        s_loc = q.size(2)
        assert s_loc % 2 == 0, "zigzag CP needs an even local sequence"
        k_cur, v_cur = k.contiguous(), v.contiguous()
        # TWO fresh recv buffers: the ping-pong must never receive into the
        # original k/v (they are saved for backward — aliasing them
        # corrupts the saved tensors from hop 2 on)
        k_bufs = [torch.empty_like(k_cur), torch.empty_like(k_cur)]
        v_bufs = [torch.empty_like(v_cur), torch.empty_like(v_cur)]

        acc_o = torch.zeros(q.shape, dtype=torch.float32, device=q.device)
        acc_lse = torch.full(
            (q.size(0), q.size(1), s_loc), -1e30,
            dtype=torch.float32, device=q.device,
        )
        with torch.no_grad():
            for t in range(R):
                j = (r - t) % R
                works: List = []
                if t < R - 1:
                    works = _post_shift(
                        (k_cur, v_cur), (k_bufs[t % 2], v_bufs[t % 2])
                    )
                _ring_fwd_hop(
                    kern, r, j, q, k_cur, v_cur, acc_o, acc_lse, scale
                )
                for w in works:
                    w.wait()
                if t < R - 1:
                    k_cur, v_cur = k_bufs[t % 2], v_bufs[t % 2]
            out = acc_o.to(q.dtype)
        ctx.save_for_backward(q, k, v, out, acc_lse)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        scale = ctx.scale
        R = ps.get_context_model_parallel_world_size()
        r = ps.get_context_model_parallel_rank()
        kern = kernels_for(q)
        half = q.size(2) // 2
        dout = dout.contiguous()
        out = out.contiguous()
        k_cur, v_cur = k.contiguous(), v.contiguous()
        k_bufs = [torch.empty_like(k_cur), torch.empty_like(k_cur)]
        v_bufs = [torch.empty_like(v_cur), torch.empty_like(v_cur)]
        # the K/V-block gradient accumulators ride the ring with their
        # block; ping-pong buffers so the isend source stays untouched
        dk_cur = torch.zeros_like(k_cur)
        dv_cur = torch.zeros_like(v_cur)
        dk_buf = torch.empty_like(dk_cur)
        dv_buf = torch.empty_like(dv_cur)
        dq_acc = torch.zeros_like(q)

        acc_works: List = []
        for t in range(R):
            j = (r - t) % R
            kv_works: List = []
            if t < R - 1:
                # prefetch next hop's K/V while this block computes
                kv_works = _post_shift(
                    (k_cur, v_cur), (k_bufs[t % 2], v_bufs[t % 2])
                )
            dk_j, dv_j, lo_only = _ring_bwd_hop(
                kern, r, j, dout, q, k_cur, v_cur, out, lse, dq_acc, scale
            )
            # fold into the accumulator that traveled with this block
            for w in acc_works:
                w.wait()
            if t > 0:
                dk_cur, dk_buf = dk_buf, dk_cur
                dv_cur, dv_buf = dv_buf, dv_cur
            if lo_only:
                dk_cur[:, :, :half].add_(dk_j)
                dv_cur[:, :, :half].add_(dv_j)
            else:
                dk_cur.add_(dk_j)
                dv_cur.add_(dv_j)
            # ship the updated accumulator along the ring (it must make
            # R - t more hops to reach its owner; the final hop below)
            acc_works = _post_shift((dk_cur, dv_cur), (dk_buf, dv_buf))
            for w in kv_works:
                w.wait()
            if t < R - 1:
                k_cur, v_cur = k_bufs[t % 2], v_bufs[t % 2]
        for w in acc_works:
            w.wait()
        return dq_acc, dk_buf, dv_buf, None


def ring_flash_attn(
    q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float = None
) -> torch.Tensor:
    """q/k/v: local zigzag sequence chunk [b, h, s_local, d] (the two
    halves are the rank's two global chunks — parallel/cp.py); returns
    the local O."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.size(-1))
    if ps.get_context_model_parallel_world_size() == 1:
        return _FlashAttnFn.apply(q, k, v, True, scale)
    return _RingFlashAttnFn.apply(q, k, v, scale)
