"""MI355X-native fused ops (hand-written HIP/CDNA4 kernels).

Every op has two paths:
- the in-tree HIP extension (``_C``), built by ``setup.py build_ext
  --inplace`` / ``__graft_entry__.build()`` for gfx950 — the ONLY path used
  for the dtypes the kernels are written for (bf16 activations) on a GPU
  device; if the extension is missing while such a tensor is on GPU the op
  raises instead of silently falling back;
- a plain PyTorch fp32 reference path used on CPU (unit tests, gloo runs)
  and, for RMSNorm / SwiGLU / RoPE / LayerNorm / GELU / GEGLU, for GPU
  tensors that are not bf16 and so have no kernel (``bf16_kernels_for``).

Kernel inventory (replacing the reference's NKI/apex device stack, SURVEY.md
§2.3): rmsnorm fwd/bwd (also with the residual add in front of it fused in,
both ways), rope fwd/bwd (also Q and K in one vectorised launch), swiglu
fwd/bwd, layernorm fwd/bwd (wave per row up to H = 2048, block per row
beyond; two-stage atomic-free dw / db), exact gelu and geglu fwd/bwd (the
Megatron GPT family's glue, NXDT_GPT_GLUE), flash attention
fwd/bwd (causal, GQA, bf16, MFMA+LDS online softmax; padded batches, packed
sequences, and attention dropout regenerated in-kernel from a counter-based
keep mask, with a stand-alone mask kernel for tests), split-KV flash decode
over a preallocated KV cache (forward only), vocab-parallel CE statistics,
fused AdamW(fp32 state), grouped MoE expert GEMMs, the LoRA adapter
products (skinny shrink, expand-add fused with the base output, two-stage
wgrad; bf16, r in 8/16/32/64), and the fused LM-head + cross-entropy (the
NT MFMA GEMM hidden @ lm_head^T with the softmax statistics, or the logit
gradient of a row chunk, as its epilogue: the [tokens, vocab] logits are
never stored; opt-in, model.fused_lm_head_loss), and the MoE token path
around the grouped GEMMs (moe_dispatch: a deterministic counting-sort plan
from topi straight into the padded layout, the permute into it, the fp32
combine out of it and the combine's backward with the routing-weight
gradient; opt-in, NXDT_MOE_FUSED=1).
"""

from __future__ import annotations

import os

import torch

_C = None
_LOAD_ERR: str = ""


def _try_load():
    global _C, _LOAD_ERR
    if _C is not None:
        return _C
    try:
        import importlib
        mod = importlib.import_module(
            "neuronx_distributed_training_amd.ops._C"
        )  # built in-tree by setup.py build_ext --inplace
        _C = mod
    except ImportError:
        # in-tree .so next to this file (hipcc -shared direct build)
        import importlib.util
        import glob
        here = os.path.dirname(__file__)
        cands = glob.glob(os.path.join(here, "_C*.so"))
        if cands:
            spec = importlib.util.spec_from_file_location(
                "neuronx_distributed_training_amd.ops._C", cands[0]
            )
            mod = importlib.util.module_from_spec(spec)
            try:
                spec.loader.exec_module(mod)
                _C = mod
            except Exception as e:  # pragma: no cover
                _LOAD_ERR = str(e)
        else:
            _LOAD_ERR = "extension _C*.so not found (run __graft_entry__.build())"
    return _C


def have_extension() -> bool:
    return _try_load() is not None


def require_extension():
    mod = _try_load()
    if mod is None:
        raise RuntimeError(
            "MI355X HIP extension not loaded on a GPU tensor — refusing the "
            f"eager fallback. Build it with __graft_entry__.build(). ({_LOAD_ERR})"
        )
    return mod


def kernels_for(t: torch.Tensor):
    """Return the extension module for GPU tensors, None for CPU."""
    if t.is_cuda:
        return require_extension()
    return None


def bf16_kernels_for(t: torch.Tensor):
    """The extension for a bf16 GPU tensor: the RMSNorm, SwiGLU, RoPE,
    LayerNorm and GELU / GEGLU kernels read bf16 and nothing else. None for CPU tensors and for GPU
    tensors of any other dtype (fp32 / fp16 / fp64 modules), which have no
    kernel and take the plain torch formulas on their own device."""
    if t.is_cuda and t.dtype == torch.bfloat16:
        return require_extension()
    return None


def fused_glue() -> bool:
    """The residual add fused into RMSNorm (ops.rmsnorm.add_rmsnorm) and the
    one-launch RoPE of Q and K (ops.rope.apply_rotary_pos_emb_pair) are the
    default; NXDT_FUSED_GLUE=0 (read per call) makes both evaluate the
    unfused calls they replaced, for A/B. The two are bit-identical except
    for the RMSNorm weight gradient's cross-block atomic order."""
    env = os.environ.get("NXDT_FUSED_GLUE", "") or "1"
    if env not in ("0", "1"):
        raise ValueError(f"NXDT_FUSED_GLUE must be '0' or '1', got {env!r}")
    return env == "1"


def gpt_glue() -> bool:
    """The Megatron GPT family's LayerNorm module and MLP activation
    (ops.layernorm.LayerNorm, and gelu / geglu in ParallelMLP) run the HIP
    kernels by default; NXDT_GPT_GLUE=0 (read per call) makes them evaluate
    the torch calls they replaced (nn.LayerNorm.forward, F.gelu), for A/B.
    The functions ops.layernorm, ops.gelu and ops.geglu themselves always
    take the kernels for bf16 GPU tensors."""
    env = os.environ.get("NXDT_GPT_GLUE", "") or "1"
    if env not in ("0", "1"):
        raise ValueError(f"NXDT_GPT_GLUE must be '0' or '1', got {env!r}")
    return env == "1"


def moe_fused() -> bool:
    """NXDT_MOE_FUSED=1 (read per call; unset or empty means 0) makes
    modules.moe.MoE take the fused token path of ops.moe_dispatch where it
    applies: bf16 on the GPU, EP = 1, at most 64 experts and top-8, and a
    token count at which ExpertMLPs would choose the grouped kernel. Anywhere
    else, and with 0, the layer evaluates the eager code unchanged."""
    env = os.environ.get("NXDT_MOE_FUSED", "") or "0"
    if env not in ("0", "1"):
        raise ValueError(f"NXDT_MOE_FUSED must be '0' or '1', got {env!r}")
    return env == "1"


from .rmsnorm import rmsnorm  # noqa: E402
from .layernorm import layernorm  # noqa: E402
from .gelu import geglu, gelu  # noqa: E402
from .rope import apply_rotary_pos_emb  # noqa: E402
from .swiglu import swiglu  # noqa: E402
from .flash_attn import (  # noqa: E402
    dropout_keep_mask,
    dropout_keep_scale,
    flash_attn_func,
    mask_to_kv_range,
    segment_bounds,
)
from .flash_decode import flash_attn_decode  # noqa: E402
from .lora import lora_delta_add  # noqa: E402
from .lm_head_loss import linear_cross_entropy  # noqa: E402
from .moe_dispatch import fused_moe_experts  # noqa: E402

__all__ = [
    "have_extension",
    "require_extension",
    "kernels_for",
    "bf16_kernels_for",
    "rmsnorm",
    "apply_rotary_pos_emb",
    "swiglu",
    "layernorm",
    "gelu",
    "geglu",
    "flash_attn_func",
    "flash_attn_decode",
    "lora_delta_add",
    "linear_cross_entropy",
    "fused_moe_experts",
    "dropout_keep_mask",
    "dropout_keep_scale",
    "mask_to_kv_range",
    "segment_bounds",
]
