"""Causal flash attention, hand-written CDNA4 HIP (MFMA + LDS online softmax).

Replaces the reference's NKI flash kernel contract
(``nki_flash_attn_func``, call site modeling_llama.py:486): causal,
bf16, GQA via kv-head grouping (no repeat_kv materialization — the kernel
indexes kv_head = q_head // group), seq up to 8k+, head_dim 128.

Layout: q [b, hq, s, d], k/v [b, hkv, s, d] — all bf16 contiguous.
Returns o [b, hq, s, d]; saves per-row LSE [b, hq, s] fp32 for the
recompute backward (FlashAttention-2 style two-kernel dKV/dQ backward).

CPU path: exact fp32 reference via scaled_dot_product_attention (tests
compare the HIP kernel against this).

Padded batches: ``kv_range=(kv_lo, kv_hi)`` gives every batch row a visible
key range ``[kv_lo[b], kv_hi[b])`` on top of the causal / window mask
(key-side only). A query row with no alive key gets O = 0, dQ = 0 and a
finite LSE; keys outside the range get dK = dV = 0. Ranged calls always run
the v2 kernels.

Packed sequences: ``segment_ids`` [B, S] (non-decreasing along each row)
makes the causal mask block-diagonal: query i sees key j iff they share a
segment id, ``j <= i`` and j is inside the sliding window if there is one.
Every query sees itself, so there are no empty rows. The kernels take the
two derived arrays of :func:`segment_bounds`, not the ids. Segmented calls
need ``S_q == S_kv`` and ``causal=True``, exclude ``kv_range`` and always
run the v2 kernels.
"""

from __future__ import annotations

import math
import os

import torch

from . import kernels_for


def _attn_version() -> str:
    """Kernel generation: '2' = 16x16x32 MFMA 8-wave (default), '3' =
    32x32x16 swapped-operand register-softmax, 'fwd' = v3 forward with v2
    backward (r2 A/B: v3 end-to-end measured slower than v2).
    NXDT_ATTN_V3=1/0/fwd overrides."""
    env = os.environ.get("NXDT_ATTN_V3", "")
    if env == "1":
        return "3"
    if env == "fwd":
        return "fwd"
    return "2"


def _fwd_fn(kern, sq=None, skv=None):
    # v3 covers the training shape (S_q == S_kv); decode / ring half-blocks
    # (S_q != S_kv) always go through v2, which supports them.
    if _attn_version() in ("3", "fwd") and (sq is None or sq == skv):
        return kern.flash_attn_fwd_v3
    return kern.flash_attn_fwd


def _dkv_arm() -> str:
    """dK/dV kernel of the v2 backward: 'pipe' = pipelined tile loop
    (default), 'sbuf' = the single-buffered kernel it replaced, kept for
    A/B; the two are bit-identical. NXDT_ATTN_DKV=pipe/sbuf overrides."""
    env = os.environ.get("NXDT_ATTN_DKV", "") or "pipe"
    if env not in ("pipe", "sbuf"):
        raise ValueError(f"NXDT_ATTN_DKV must be 'pipe' or 'sbuf', got {env!r}")
    return env


def v2_bwd_fn(kern, kind=""):
    """The v2 backward binding of `kind` ('' dense, '_range', '_seg') for
    the dK/dV arm NXDT_ATTN_DKV selects."""
    suffix = "_sbuf" if _dkv_arm() == "sbuf" else ""
    return getattr(kern, f"flash_attn_bwd{kind}{suffix}")


def _bwd_fn(kern, sq=None, skv=None):
    if _attn_version() == "3" and (sq is None or sq == skv):
        return kern.flash_attn_bwd_v3
    return v2_bwd_fn(kern)


def mask_to_kv_range_tensors(attention_mask):
    """Device-side part of :func:`mask_to_kv_range`: returns int32
    ``kv_lo``, ``kv_hi`` [B] and a 0-dim bool tensor ``contiguous`` without
    a host sync."""
    m = attention_mask != 0
    s = m.size(1)
    mi = m.to(torch.int32)
    has = m.any(dim=1)
    lo = torch.argmax(mi, dim=1)                     # first non-zero
    hi = s - torch.argmax(mi.flip(1), dim=1)         # one past the last
    zero = torch.zeros_like(lo)
    lo = torch.where(has, lo, zero)
    hi = torch.where(has, hi, zero)                  # all-zero row: lo == hi
    contiguous = (mi.sum(dim=1) == hi - lo).all()
    return lo.to(torch.int32), hi.to(torch.int32), contiguous


def mask_to_kv_range(attention_mask):
    """[B, S] padding mask (non-zero = real token) -> (kv_lo, kv_hi,
    contiguous). ``[kv_lo[b], kv_hi[b])`` spans the first to the last real
    token of row b (``lo == hi`` for a row of all zeros); ``contiguous`` is
    False if any row has a hole inside that span, in which case the range
    does not describe the mask."""
    lo, hi, contiguous = mask_to_kv_range_tensors(attention_mask)
    return lo, hi, bool(contiguous)


def _norm_kv_range(kv_range, b, skv, device):
    """Clamp to 0 <= lo <= hi <= S_kv (the kernels trust this) and make the
    pair contiguous int32 [B] on `device`."""
    lo, hi = kv_range
    lo = torch.as_tensor(lo, device=device).to(torch.int32).reshape(-1)
    hi = torch.as_tensor(hi, device=device).to(torch.int32).reshape(-1)
    if lo.numel() != b or hi.numel() != b:
        raise ValueError(
            f"kv_range tensors must have shape [{b}], got "
            f"{tuple(lo.shape)} / {tuple(hi.shape)}"
        )
    hi = hi.clamp(0, skv)
    lo = torch.minimum(lo.clamp(0, skv), hi)
    return lo.contiguous(), hi.contiguous()


def segment_bounds(segment_ids):
    """[B, S] segment ids (non-decreasing along each row) -> int32 [B, S]
    ``(q_start, k_end)``: ``q_start[b, i]`` is the first position of token
    i's segment (the first key query i may see), ``k_end[b, j]`` one past
    its last position (one past the last query that may see key j). Both
    are non-decreasing. Runs on the ids' device without a host sync."""
    if segment_ids.dim() != 2:
        raise ValueError(
            f"segment_ids must be [B, S], got {tuple(segment_ids.shape)}"
        )
    b, s = segment_ids.shape
    pos = torch.arange(s, device=segment_ids.device, dtype=torch.int32)
    pos = pos.expand(b, s)
    new = torch.ones(b, s, dtype=torch.bool, device=segment_ids.device)
    new[:, 1:] = segment_ids[:, 1:] != segment_ids[:, :-1]
    # start: running max of "position if a segment starts here"
    q_start = torch.cummax(torch.where(new, pos, torch.zeros_like(pos)),
                           dim=1).values
    # end: running min from the right of "position + 1 if one ends here"
    last = torch.ones_like(new)
    last[:, :-1] = new[:, 1:]
    end = torch.where(last, pos + 1, torch.full_like(pos, s))
    k_end = torch.cummin(end.flip(1), dim=1).values.flip(1)
    return (q_start.to(torch.int32).contiguous(),
            k_end.to(torch.int32).contiguous())


def _make_mask(sq, sk, causal, window, device, kv_lo=None, kv_hi=None,
               q_start=None):
    """True = dead. [sq, sk], or [b, 1, sq, sk] with a key range or
    segment starts."""
    # S_q != S_kv: bottom-right alignment (query i sees keys
    # j <= i + sk - sq) — matches the HIP kernel's decode convention
    mask = torch.zeros(sq, sk, dtype=torch.bool, device=device)
    if causal:
        diag = sk - sq
        mask |= torch.ones(sq, sk, dtype=torch.bool, device=device).triu(
            1 + diag
        )
        if window and window > 0:
            mask |= torch.ones(sq, sk, dtype=torch.bool, device=device).tril(
                diag - window
            )
    if kv_lo is not None:
        j = torch.arange(sk, device=device)
        out = (j[None, :] < kv_lo[:, None]) | (j[None, :] >= kv_hi[:, None])
        mask = mask[None, None] | out[:, None, None, :]
    if q_start is not None:
        # with the causal mask, "same segment" is "key not below the start
        # of the query's segment"
        j = torch.arange(sk, device=device)
        out = j[None, None, :] < q_start[:, :, None]         # [b, sq, sk]
        mask = mask[None, None] | out[:, None]
    return mask


def _ranged_softmax(s, mask):
    """softmax over alive keys; rows with no alive key give p = 0 exactly
    (no NaN from an all -inf row) and LSE = -1e30 like the kernel."""
    s = s.masked_fill(mask, float("-inf"))
    m = s.amax(dim=-1, keepdim=True)
    empty = torch.isinf(m)
    m = torch.where(empty, torch.zeros_like(m), m)
    e = torch.exp(s - m)                             # dead -> exactly 0
    l = e.sum(dim=-1, keepdim=True)
    p = e / torch.where(empty, torch.ones_like(l), l)
    lse = torch.where(empty, torch.full_like(m, -1e30), m + torch.log(l))
    return p, lse.squeeze(-1)


def _cpu_ref_fwd(q, k, v, causal, scale, window=0, kv_lo=None, kv_hi=None,
                 q_start=None):
    hq, hkv = q.size(1), k.size(1)
    if hq != hkv:
        k = k.repeat_interleave(hq // hkv, dim=1)
        v = v.repeat_interleave(hq // hkv, dim=1)
    qf, kf, vf = q.float(), k.float(), v.float()
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    mask = _make_mask(q.size(-2), k.size(-2), causal, window, q.device,
                      kv_lo, kv_hi, q_start)
    if kv_lo is not None:
        p, lse = _ranged_softmax(s, mask)
    else:
        s = s.masked_fill(mask, float("-inf"))
        lse = torch.logsumexp(s, dim=-1)
        p = torch.softmax(s, dim=-1)
    o = torch.matmul(p, vf)
    return o.to(q.dtype), lse


class _FlashAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal: bool, scale: float, window: int = 0,
                kv_lo=None, kv_hi=None, q_start=None, k_end=None):
        kern = kernels_for(q)
        ranged = kv_lo is not None
        segmented = q_start is not None
        if kern is not None and segmented:
            # segmented calls always use the v2 kernels too
            o, lse = kern.flash_attn_fwd_seg(
                q, k, v, q_start, k_end, scale, window
            )
        elif kern is not None and ranged:
            # ranged calls always use the v2 kernels (like S_q != S_kv)
            o, lse = kern.flash_attn_fwd_range(
                q, k, v, kv_lo, kv_hi, causal, scale, window
            )
        elif kern is not None:
            # kernel takes arbitrary-strided [b, h, s, d] views (d contig)
            o, lse = _fwd_fn(kern, q.size(2), k.size(2))(
                q, k, v, causal, scale, window
            )
        else:
            o, lse = _cpu_ref_fwd(q, k, v, causal, scale, window,
                                  kv_lo, kv_hi, q_start)
        if segmented:
            ctx.save_for_backward(q, k, v, o, lse, q_start, k_end)
        elif ranged:
            ctx.save_for_backward(q, k, v, o, lse, kv_lo, kv_hi)
        else:
            ctx.save_for_backward(q, k, v, o, lse)
        ctx.ranged = ranged
        ctx.segmented = segmented
        ctx.causal = causal
        ctx.scale = scale
        ctx.window = window
        return o

    @staticmethod
    def backward(ctx, do):
        kv_lo = kv_hi = q_start = k_end = None
        none7 = (None,) * 7
        if ctx.segmented:
            q, k, v, o, lse, q_start, k_end = ctx.saved_tensors
        elif ctx.ranged:
            q, k, v, o, lse, kv_lo, kv_hi = ctx.saved_tensors
        else:
            q, k, v, o, lse = ctx.saved_tensors
        kern = kernels_for(q)
        if kern is not None and ctx.segmented:
            dq, dk, dv = v2_bwd_fn(kern, "_seg")(
                do, q, k, v, o, lse, q_start, k_end, ctx.scale, ctx.window
            )
            return (dq, dk, dv) + none7
        if kern is not None and ctx.ranged:
            dq, dk, dv = v2_bwd_fn(kern, "_range")(
                do, q, k, v, o, lse, kv_lo, kv_hi, ctx.causal, ctx.scale,
                ctx.window,
            )
            return (dq, dk, dv) + none7
        if kern is not None:
            dq, dk, dv = _bwd_fn(kern, q.size(2), k.size(2))(
                do, q, k, v, o, lse, ctx.causal, ctx.scale, ctx.window
            )
            return (dq, dk, dv) + none7
        # CPU reference backward (fp32, explicit)
        hq, hkv = q.size(1), k.size(1)
        g = hq // hkv
        kx = k.repeat_interleave(g, dim=1).float()
        vx = v.repeat_interleave(g, dim=1).float()
        qf, dof = q.float(), do.float()
        s = torch.matmul(qf, kx.transpose(-1, -2)) * ctx.scale
        mask = _make_mask(q.size(-2), k.size(-2), ctx.causal, ctx.window,
                          q.device, kv_lo, kv_hi, q_start)
        if ctx.ranged:
            p, _ = _ranged_softmax(s, mask)
        else:
            s = s.masked_fill(mask, float("-inf"))
            p = torch.softmax(s, dim=-1)
        dv = torch.matmul(p.transpose(-1, -2), dof)
        dp = torch.matmul(dof, vx.transpose(-1, -2))
        delta = (dof * o.float()).sum(-1, keepdim=True)
        ds = p * (dp - delta) * ctx.scale
        dq = torch.matmul(ds, kx)
        dk = torch.matmul(ds.transpose(-1, -2), qf)
        if g > 1:
            dk = dk.reshape(dk.size(0), hkv, g, dk.size(-2), dk.size(-1)).sum(2)
            dv = dv.reshape(dv.size(0), hkv, g, dv.size(-2), dv.size(-1)).sum(2)
        return (dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype)) + none7


def flash_attn_func(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    causal: bool = True,
    scale: float | None = None,
    window: int | None = None,
    kv_range=None,
    segment_ids=None,
    seg_bounds=None,
) -> torch.Tensor:
    """window: sliding-window size (attend to the last `window` keys);
    None/0 disables (Mixtral sliding_window parity).

    kv_range: optional pair ``(kv_lo, kv_hi)`` of int tensors [B]; batch
    row b only sees keys ``kv_lo[b] <= j < kv_hi[b]`` (see
    :func:`mask_to_kv_range`). None = dense attention.

    segment_ids: optional int tensor [B, S], non-decreasing along each row
    (packed sequences). Query i sees key j iff both carry the same id,
    ``j <= i`` and j is inside the window; a pad tail is its own trailing
    segment. Needs ``causal=True`` and ``S_q == S_kv``; excludes
    ``kv_range``. ``seg_bounds`` passes the precomputed result of
    :func:`segment_bounds` instead (a model computes it once per forward)."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.size(-1))
    if segment_ids is not None or seg_bounds is not None:
        if segment_ids is not None and seg_bounds is not None:
            raise ValueError("give segment_ids or seg_bounds, not both")
        if kv_range is not None:
            raise ValueError("segment_ids and kv_range are mutually exclusive")
        if not causal:
            raise ValueError("segment_ids needs causal=True")
        if q.size(2) != k.size(2):
            raise ValueError(
                f"segment_ids needs S_q == S_kv, got {q.size(2)} / {k.size(2)}"
            )
        if seg_bounds is None:
            seg_bounds = segment_bounds(
                torch.as_tensor(segment_ids, device=q.device)
            )
        q_start, k_end = seg_bounds
        want = (q.size(0), q.size(2))
        if tuple(q_start.shape) != want or tuple(k_end.shape) != want:
            raise ValueError(
                f"segment_ids must have shape {list(want)}, got "
                f"{tuple(q_start.shape)}"
            )
        return _FlashAttnFn.apply(
            q, k, v, True, scale, int(window or 0), None, None,
            q_start, k_end,
        )
    if kv_range is None:
        return _FlashAttnFn.apply(q, k, v, causal, scale, int(window or 0))
    kv_lo, kv_hi = _norm_kv_range(kv_range, q.size(0), k.size(2), q.device)
    return _FlashAttnFn.apply(
        q, k, v, causal, scale, int(window or 0), kv_lo, kv_hi
    )
