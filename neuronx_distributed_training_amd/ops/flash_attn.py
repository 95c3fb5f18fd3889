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

Attention dropout: ``dropout_p`` drops probabilities inside the kernels with
a counter-based keep mask that forward and backward regenerate from
``(seed, offset)`` (``dropout_rng``, or the device's default generator).
Dense masks only; always the v2 kernels. See :func:`flash_attn_func`.
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


_U64 = (1 << 64) - 1


def dropout_threshold(p: float) -> int:
    """8-bit drop threshold ``t = round(256 * p)``: an element is dropped
    iff its random byte is below t. 0 means no dropout; ``p`` outside
    ``[0, 1)``, or so close to 1 that t would be 256, raises ValueError."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout_p must be in [0, 1), got {p}")
    t = int(math.floor(256.0 * p + 0.5))
    if t > 255:
        raise ValueError(
            f"dropout_p {p} rounds to 256/256: the threshold has 8 bits"
        )
    return t


def dropout_keep_scale(p: float) -> float:
    """Factor on kept probabilities, ``256 / (256 - t)``: the inverse of the
    quantised keep probability, so the expectation is exact."""
    return 256.0 / (256 - dropout_threshold(p))


def draw_dropout_rng(device):
    """(seed, offset) from the default generator of `device`, which is
    advanced: ``torch.manual_seed``, ``torch.cuda.set_rng_state`` and
    ``RNGStatesTracker.fork()`` govern the pair and successive draws differ.
    No device sync."""
    if device.type == "cuda":
        idx = device.index
        if idx is None:
            idx = torch.cuda.current_device()
        gen = torch.cuda.default_generators[idx]
        seed, offset = gen.initial_seed(), gen.get_offset()
        gen.set_offset(offset + 4)  # the generator wants multiples of 4
        return int(seed) & _U64, int(offset) & _U64
    # the CPU generator has no offset: draw one from its stream
    gen = torch.default_generator
    offset = int(torch.randint(0, 1 << 62, (1,), generator=gen))
    return int(gen.initial_seed()) & _U64, offset


def dropout_keep_mask(b, hq, sq, skv, p, rng, device):
    """Bool [b, hq, sq, skv], True = keep: exactly the mask a
    ``flash_attn_func`` call with ``dropout_p=p, dropout_rng=rng`` applies to
    its probabilities on `device`. On GPU it is written by the kernel-side
    definition (``flash_attn_dropout_mask``), a pure function of
    ``(seed, offset, b, hq, i, j, t)``; on CPU it comes from a
    ``torch.Generator`` seeded from ``(seed, offset)``, and is a function of
    the four sizes as well."""
    t = dropout_threshold(p)
    seed, offset = int(rng[0]) & _U64, int(rng[1]) & _U64
    device = torch.device(device)
    if device.type == "cuda":
        from . import require_extension

        with torch.cuda.device(device):
            m = require_extension().flash_attn_dropout_mask(
                b, hq, sq, skv, float(p), seed, offset
            )
        return m != 0
    gen = torch.Generator()
    gen.manual_seed((seed * 0x9E3779B97F4A7C15 + offset) & ((1 << 63) - 1))
    byte = torch.randint(0, 256, (b, hq, sq, skv), generator=gen)
    return byte >= t


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


def _cpu_drop_factor(q, k, drop):
    """keep mask * keep_scale of drop = (p, seed, offset), fp32."""
    p, seed, offset = drop
    keep = dropout_keep_mask(q.size(0), q.size(1), q.size(2), k.size(2), p,
                             (seed, offset), q.device)
    return keep.float() * dropout_keep_scale(p)


def _cpu_ref_fwd(q, k, v, causal, scale, window=0, kv_lo=None, kv_hi=None,
                 q_start=None, drop=None):
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
    if drop is not None:      # LSE stays that of the undropped softmax
        p = p * _cpu_drop_factor(q, k, drop)
    o = torch.matmul(p, vf)
    return o.to(q.dtype), lse


class _FlashAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal: bool, scale: float, window: int = 0,
                kv_lo=None, kv_hi=None, q_start=None, k_end=None, drop=None):
        # drop: None, or (p, seed, offset) with t > 0, as Python numbers; the
        # backward regenerates the mask from them (no mask tensor is saved)
        kern = kernels_for(q)
        ranged = kv_lo is not None
        segmented = q_start is not None
        if kern is not None and drop is not None:
            # dropout calls always use the v2 kernels
            o, lse = kern.flash_attn_fwd_drop(
                q, k, v, causal, scale, window, *drop
            )
        elif kern is not None and segmented:
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
                                  kv_lo, kv_hi, q_start, drop)
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
        ctx.drop = drop
        return o

    @staticmethod
    def backward(ctx, do):
        kv_lo = kv_hi = q_start = k_end = None
        none7 = (None,) * 8
        if ctx.segmented:
            q, k, v, o, lse, q_start, k_end = ctx.saved_tensors
        elif ctx.ranged:
            q, k, v, o, lse, kv_lo, kv_hi = ctx.saved_tensors
        else:
            q, k, v, o, lse = ctx.saved_tensors
        kern = kernels_for(q)
        if kern is not None and ctx.drop is not None:
            # always the pipelined dK/dV kernel, whatever NXDT_ATTN_DKV says
            dq, dk, dv = kern.flash_attn_bwd_drop(
                do, q, k, v, o, lse, ctx.causal, ctx.scale, ctx.window,
                *ctx.drop
            )
            return (dq, dk, dv) + none7
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
        if ctx.drop is None:
            dv = torch.matmul(p.transpose(-1, -2), dof)
            dp = torch.matmul(dof, vx.transpose(-1, -2))
        else:
            # dV = (P . M ks)^T dO ; dS = P . (M ks . dP - delta) * scale
            mk = _cpu_drop_factor(q, k, ctx.drop)
            dv = torch.matmul((p * mk).transpose(-1, -2), dof)
            dp = torch.matmul(dof, vx.transpose(-1, -2)) * mk
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
    dropout_p: float = 0.0,
    dropout_rng=None,
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
    :func:`segment_bounds` instead (a model computes it once per forward).

    dropout_p: dropout on the attention probabilities, inside the kernels:
    ``O = ((P . M) V) * keep_scale`` with a keep mask M that the forward,
    the dQ and the dK/dV kernel each regenerate from a counter-based
    generator (no mask tensor exists or is saved). Probabilities have 8
    bits: an element is dropped with probability ``t / 256``,
    ``t = round(256 * dropout_p)``, and kept ones are scaled by
    ``256 / (256 - t)`` (:func:`dropout_keep_scale`). 0.0, or any value
    that rounds to ``t == 0``, takes exactly the code path of a call
    without the argument. The caller decides when dropout applies (a model
    passes 0.0 in eval mode). Dense masks only: ``kv_range``,
    ``segment_ids`` and ``seg_bounds`` raise ValueError with
    ``dropout_p > 0``, as does ``dropout_p`` outside ``[0, 1)``. Dropout
    calls always run the v2 kernels, with the pipelined dK/dV kernel.

    dropout_rng: ``(seed, offset)``, two ints that fix the random stream;
    :func:`dropout_keep_mask` returns the mask such a call uses. None draws
    the pair from the default generator of ``q``'s device and advances it
    (no device sync), so ``torch.manual_seed``, ``torch.cuda.set_rng_state``
    and ``RNGStatesTracker.fork()`` govern it and successive calls differ.
    The pair is read on the host when the call is made, so hipGraph capture
    of a call with ``dropout_p > 0`` is not supported: every replay would
    reuse the captured pair."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.size(-1))
    if dropout_p != 0.0 and dropout_threshold(dropout_p) > 0:
        if kv_range is not None:
            raise ValueError("dropout_p > 0 does not support kv_range")
        if segment_ids is not None or seg_bounds is not None:
            raise ValueError(
                "dropout_p > 0 does not support segment_ids / seg_bounds"
            )
        if dropout_rng is None:
            dropout_rng = draw_dropout_rng(q.device)
        drop = (float(dropout_p), int(dropout_rng[0]) & _U64,
                int(dropout_rng[1]) & _U64)
        return _FlashAttnFn.apply(
            q, k, v, causal, scale, int(window or 0), None, None, None, None,
            drop,
        )
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
