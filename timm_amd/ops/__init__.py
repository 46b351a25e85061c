"""MI355X-native op layer.

Every hot-path op in the reference framework (`timm`) is a stock PyTorch op —
see SURVEY.md §2.10 for the op-by-op map.  Here each of them dispatches to a
hand-written CDNA4 (gfx950) HIP kernel compiled into the in-tree extension
`timm_amd._C`:

 * layer_norm / rms_norm (+LayerScale fusion)          — one read of x, two-pass fp32 statistics
 * attention (flash-style fused SDPA, bf16)            — MFMA 16x16x32, online softmax;
   any head_dim % 8 == 0 up to 128 (72 / 80 / 88 / 104 / 48 included), fwd + bwd
 * attention bias gradient (learned rel-pos bias)      — flash dBias pass, fp32, no atomics
 * key-padding attention (bool [B,1,1,Nk] attn_mask)   — validity as bits in scalar registers,
   all-padding key tiles skipped before their loads, fwd + bwd (head_dim 64); bool masks
   mean "True takes part" on every attention path
 * decomposed rel-pos attention (rel_pos_hw= tables)   — SAM / MViT-v2 bias from its [B,H,N,Kh] and
   [B,H,N,Kw] tables in LDS, table gradients as row sums of dS in the dQ kernel (head_dim 64)
 * window_attention (Swin W-MSA / SW-MSA on the map)   — shift, partition, reverse and shift mask
   as addressing; one wave per (window, head), single-pass bwd with dBias (head_dim 32, N <= 64)
 * window_attention(..., logit_scale=) (SwinV2 cosine) — q / k normalised in the kernels, fp32 logit
   scale, one workgroup per (window, head), bwd with d logit_scale and dBias (head_dim 32, N <= 256)
 * cross_covariance_attention (XCiT's XCA)              — softmax over the d x d channel matrix of
   token-normalised q, k on the packed qkv; one workgroup per (batch, head), two passes over the
   tokens, closed-form bwd with d temperature (head_dim 32 / 48 / 64, any N)
 * bias_act (bias+GELU/SiLU epilogue after GEMM)
 * residual add (+ LayerScale + DropPath) epilogue
 * multi-tensor fused optimizer steps (AdamW/LAMB/SGD/lerp-EMA)
 * apply_rope_qk (rotary embedding of q and k, fwd/bwd) — one launch for both tensors

Dispatch rules:
 * CUDA/ROCm tensor + extension available  -> HIP kernel.
 * CUDA/ROCm tensor + extension missing    -> RuntimeError (loud, no silent
   eager fallback on a GPU box).
 * CPU tensor                              -> plain PyTorch reference path
   (keeps the full test-suite runnable without a GPU; this is also the
   numerics reference the GPU tests compare against).
"""
import os

import torch

_C = None
_C_ERR = None


def _load_extension():
    global _C, _C_ERR
    if _C is not None or _C_ERR is not None:
        return _C
    try:
        from timm_amd import _C as _ext  # built in-tree via setup.py build_ext --inplace
        _C = _ext
    except ImportError as e:
        _C_ERR = e
    return _C


def has_ext() -> bool:
    return _load_extension() is not None


def require_ext():
    ext = _load_extension()
    if ext is None:
        raise RuntimeError(
            "timm_amd HIP extension (timm_amd._C) is not built. On a GPU box this is a "
            "hard error - the native gfx950 kernels must run, not an eager fallback. "
            f"Build with `python setup.py build_ext --inplace`. Import error: {_C_ERR}")
    return ext


_ALLOW_EAGER_GPU = os.environ.get('TIMM_AMD_ALLOW_EAGER_GPU', '0') == '1'


def use_hip(x: torch.Tensor) -> bool:
    """True if op should take the HIP kernel path for tensor x."""
    if not x.is_cuda:
        return False
    if has_ext():
        return True
    if _ALLOW_EAGER_GPU:
        return False
    require_ext()  # raises


from .conv import depthwise_conv2d  # noqa: E402
from .layer_norm import layer_norm_act, rms_norm_act, layer_norm, rms_norm  # noqa: E402
from .attention import flash_attention, flash_attention_qkv, attention_available  # noqa: E402
from .window_attention import window_attention  # noqa: E402
from .xca_attention import cross_covariance_attention  # noqa: E402
from .elementwise import bias_act, residual_scale_add  # noqa: E402
from .fused_optim import fused_adamw_step, fused_lamb_step, fused_lerp_, fused_l2norm  # noqa: E402
from .loss import fused_cross_entropy  # noqa: E402
from .data import u8_normalize, masked_global_pool  # noqa: E402
from .rope import apply_rope_qk, rope_available  # noqa: E402

__all__ = [
    'has_ext', 'require_ext', 'use_hip',
    'depthwise_conv2d',
    'layer_norm', 'layer_norm_act', 'rms_norm', 'rms_norm_act',
    'flash_attention', 'flash_attention_qkv', 'attention_available', 'window_attention',
    'cross_covariance_attention',
    'bias_act', 'residual_scale_add',
    'fused_adamw_step', 'fused_lamb_step', 'fused_lerp_', 'fused_l2norm',
    'fused_cross_entropy', 'u8_normalize', 'masked_global_pool',
    'apply_rope_qk', 'rope_available',
]
