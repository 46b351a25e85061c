"""Fused rotary position embedding for q and k.

The reference applies RoPE as an eager chain per tensor
(`timm/models/eva.py:239-243`, `timm/layers/attention.py:263-269`): slice off
the prefix tokens, build rot(x) from strided slices, two multiplies and an add
in the table's dtype, cat the prefix back on, cast to v's dtype.  Here q and k
go through one HIP kernel launch (`csrc/rope.hip`) in forward and one in
backward; every [sin | cos] chunk is loaded once and used for both tensors.

Device path: `_C.rope_qk` (16B vector accesses, fp32 math, one rounding).
CPU path / unsupported inputs: the eager composition, which doubles as the
numerics oracle.  A table that requires grad (RotaryEmbeddingMixed learns its
frequencies) always takes the eager path so autograd reaches it.
"""
from typing import Optional, Tuple

import torch

from . import _load_extension

_DTYPE_COMBOS = (
    (torch.bfloat16, torch.bfloat16),
    (torch.float32, torch.float32),
    (torch.float32, torch.bfloat16),  # qk-norm output under autocast feeding a bf16 v
)


def _rope_4d(q: torch.Tensor, rope: torch.Tensor) -> Optional[torch.Tensor]:
    """Left-pad `rope` to [B|1, H|1, Np, 2D] exactly as eager broadcasting
    against [B, H, Np, D] would; None if it does not broadcast."""
    if rope.dim() < 2 or rope.dim() > 4 or q.dim() != 4:
        return None
    while rope.dim() < 4:
        rope = rope.unsqueeze(0)
    B, H = q.shape[0], q.shape[1]
    if rope.shape[0] not in (1, B) or rope.shape[1] not in (1, H):
        return None
    if rope.shape[3] != 2 * q.shape[3]:
        return None
    return rope


def rope_available(
        q: torch.Tensor,
        k: torch.Tensor,
        rope: torch.Tensor,
        half: bool = False,
        out_dtype: Optional[torch.dtype] = None,
) -> bool:
    """True if `apply_rope_qk` will run the HIP kernel for these inputs."""
    if not (q.is_cuda and k.is_cuda and rope.is_cuda) or _load_extension() is None:
        return False
    if q.dim() != 4 or q.shape != k.shape or q.dtype != k.dtype:
        return False
    if (q.dtype, out_dtype or q.dtype) not in _DTYPE_COMBOS:
        return False
    if rope.dtype not in (torch.float32, torch.bfloat16):
        return False
    if q.shape[-1] % (16 if half else 8) != 0:
        return False
    if _rope_4d(q, rope) is None:
        return False
    # a learned table must keep receiving gradients: eager path
    if rope.requires_grad and torch.is_grad_enabled():
        return False
    return True


def _aligned(t: torch.Tensor) -> bool:
    # kernel contract: contiguous last dim, 16B-aligned base and b/h/n strides
    if t.stride(-1) != 1 or t.data_ptr() % 16 != 0:
        return False
    es = t.element_size()
    return all(n <= 1 or (s * es) % 16 == 0 for n, s in zip(t.shape[:-1], t.stride()[:-1]))


def _prep(t: torch.Tensor) -> torch.Tensor:
    return t if _aligned(t) else t.contiguous()


class _RopeQkFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, rope, npt, half, out_dtype):
        ext = _load_extension()
        q_rot, k_rot = ext.rope_qk(_prep(q), _prep(k), rope, npt, half, False, out_dtype)
        ctx.save_for_backward(rope)
        ctx.npt = npt
        ctx.half = half
        ctx.in_dtype = q.dtype
        return q_rot, k_rot

    @staticmethod
    def backward(ctx, dq, dk):
        ext = _load_extension()
        rope, = ctx.saved_tensors
        dq, dk = ext.rope_qk(_prep(dq), _prep(dk), rope, ctx.npt, ctx.half, True, ctx.in_dtype)
        return dq, dk, None, None, None, None


def _rope_eager(q, k, rope, npt, half, out_dtype):
    from ..layers.pos_embed_sincos import apply_rot_embed_cat
    q = torch.cat([q[:, :, :npt, :], apply_rot_embed_cat(q[:, :, npt:, :], rope, half=half)], 2).to(out_dtype)
    k = torch.cat([k[:, :, :npt, :], apply_rot_embed_cat(k[:, :, npt:, :], rope, half=half)], 2).to(out_dtype)
    return q, k


def apply_rope_qk(
        q: torch.Tensor,
        k: torch.Tensor,
        rope: torch.Tensor,
        num_prefix_tokens: int = 0,
        half: bool = False,
        out_dtype: Optional[torch.dtype] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Rotate q and k ([B, H, N, D]) past the first `num_prefix_tokens` rows.

    rope: [sin | cos] table, [Np, 2D], [H|1, Np, 2D] or [B|1, H|1, Np, 2D]
    with Np = N - num_prefix_tokens (batched tables arrive as [B, 1, Np, 2D]).
    half selects the half-rotation layout instead of interleaved pairs.
    Outputs are cast to out_dtype (default: q.dtype).
    """
    if out_dtype is None:
        out_dtype = q.dtype
    if rope_available(q, k, rope, half, out_dtype):
        rope4 = _prep(_rope_4d(q, rope))
        return _RopeQkFn.apply(q, k, rope4, num_prefix_tokens, half, out_dtype)
    if q.is_cuda:
        from . import use_hip
        use_hip(q)  # raises when the extension is missing on a GPU box
    return _rope_eager(q, k, rope, num_prefix_tokens, half, out_dtype)
