"""Windowed attention on the un-partitioned feature map (Swin W-MSA / SW-MSA).

`window_attention` takes the qkv Linear's output on the `[B, Hf, Wf, C]` map
and returns O on the same map, ready for `proj`.  The cyclic shift, the window
partition / reverse and the shift mask are addressing inside the kernels of
csrc/window_attention.hip (one wave per (window, head) pair, direct softmax,
dQ / dK / dV / dBias in a single backward pass), so none of roll, pad,
partition, the qkv permute, reverse or the `[nW, heads, N, N]` bias + mask
tensor is ever materialised.

Addressing (kernels and composition agree): window `w = wy * (Wf / ww) + wx`,
token `n = i * ww + j`, shifted coordinate `(y', x') = (wy*wh + i, wx*ww + j)`,
map coordinate `((y' + sh) % Hf, (x' + sw) % Wf)`.  The shift mask adds -100
where the labels `3 * r_h(y') + r_w(x')` of query and key differ; `r` is 0
without a shift in that dim, else 0 / 1 / 2 for `c < size - win`,
`c < size - shift` and beyond.

Kernel range: bf16, head_dim 32, window area <= 64, no padding
(`Hf % wh == 0`, `Wf % ww == 0`), `0 <= shift < window`, contiguous qkv.
Everything else (CPU, fp32, other shapes) runs the plain composition below,
which is also the numerics oracle of the GPU tests.
"""
import math
from typing import Optional, Tuple, Union

import torch

from . import _load_extension
from .attention import _dbias_nsplit

_HEAD_DIM = 32
_MAX_AREA = 64
# kernel launches since import: lets a test assert which path a model took
WINDOW_ATTN_CALLS = {'fwd': 0, 'bwd': 0}


def _pair(v) -> Tuple[int, int]:
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def _kernel_supported(qkv, num_heads, ws, ss) -> bool:
    if not qkv.is_cuda or qkv.dtype != torch.bfloat16 or qkv.dim() != 4:
        return False
    if _load_extension() is None:
        return False
    _, Hf, Wf, C3 = qkv.shape
    return (C3 == 3 * num_heads * _HEAD_DIM and ws[0] * ws[1] <= _MAX_AREA
            and Hf % ws[0] == 0 and Wf % ws[1] == 0
            and 0 <= ss[0] < ws[0] and 0 <= ss[1] < ws[1]
            and qkv.is_contiguous() and qkv.data_ptr() % 16 == 0 and qkv.numel() > 0)


def _shift_labels(size: int, win: int, shift: int, device) -> torch.Tensor:
    c = torch.arange(size, device=device)
    if shift == 0:
        return torch.zeros_like(c)
    return (c >= size - win).long() + (c >= size - shift).long()


def _windows(x, ws):
    """[B, Hf, Wf, ...] -> [B * nW, N, ...]"""
    B, Hf, Wf = x.shape[:3]
    rest = x.shape[3:]
    x = x.reshape(B, Hf // ws[0], ws[0], Wf // ws[1], ws[1], *rest)
    x = x.permute(0, 1, 3, 2, 4, *range(5, x.dim()))
    return x.reshape(-1, ws[0] * ws[1], *rest)


def _math_window_attention(qkv, num_heads, ws, ss, bias, scale):
    """roll -> partition -> softmax(scale QK^T + bias + mask) V (fp32 softmax)
    -> reverse -> roll."""
    B, Hf, Wf, C3 = qkv.shape
    D = C3 // (3 * num_heads)
    shifted = any(ss)
    if shifted:
        qkv = torch.roll(qkv, shifts=(-ss[0], -ss[1]), dims=(1, 2))
    win = _windows(qkv, ws).reshape(-1, ws[0] * ws[1], 3, num_heads, D)
    q, k, v = win.permute(2, 0, 3, 1, 4).float().unbind(0)  # [B*nW, heads, N, D]
    attn = (q @ k.transpose(-2, -1)) * scale
    if bias is not None:
        attn = attn + bias.float()
    if shifted:
        labels = (3 * _shift_labels(Hf, ws[0], ss[0], qkv.device)[:, None]
                  + _shift_labels(Wf, ws[1], ss[1], qkv.device)[None, :])
        labels = _windows(labels[None], ws)  # [nW, N]
        mask = (labels[:, :, None] != labels[:, None, :]).float() * -100.0
        nW = mask.shape[0]
        attn = (attn.view(B, nW, num_heads, *mask.shape[1:]) + mask[None, :, None]).flatten(0, 1)
    out = attn.softmax(dim=-1) @ v  # [B*nW, heads, N, D]
    out = out.transpose(1, 2).reshape(B, Hf // ws[0], Wf // ws[1], ws[0], ws[1], num_heads * D)
    out = out.permute(0, 1, 3, 2, 4, 5).reshape(B, Hf, Wf, num_heads * D)
    if shifted:
        out = torch.roll(out, shifts=ss, dims=(1, 2))
    return out.to(qkv.dtype)


class _WindowAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, bias, num_heads, ws, ss, scale):
        ext = _load_extension()
        WINDOW_ATTN_CALLS['fwd'] += 1
        o, lse = ext.window_attention_fwd(qkv, bias, num_heads, ws[0], ws[1], ss[0], ss[1], scale)
        ctx.save_for_backward(qkv, o, lse)
        ctx.bias = bias
        ctx.args = (num_heads, ws, ss, scale)
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse = ctx.saved_tensors
        num_heads, ws, ss, scale = ctx.args
        ext = _load_extension()
        WINDOW_ATTN_CALLS['bwd'] += 1
        need_dbias = ctx.bias is not None and ctx.needs_input_grad[1]
        if not do.is_contiguous() or do.data_ptr() % 16 != 0:
            do = do.contiguous()
        N = ws[0] * ws[1]
        n_win = qkv.shape[0] * (qkv.shape[1] // ws[0]) * (qkv.shape[2] // ws[1])
        # one workgroup (and one dBias slab) per chunk of windows and head
        nsplit = _dbias_nsplit(n_win, num_heads, num_heads * N * N * 4)
        dqkv, dbias = ext.window_attention_bwd(
            qkv, o, lse, do, ctx.bias, num_heads, ws[0], ws[1], ss[0], ss[1], scale,
            need_dbias, nsplit)
        return dqkv, dbias, None, None, None, None


def window_attention(
        qkv: torch.Tensor,
        num_heads: int,
        window_size: Union[int, Tuple[int, int]],
        shift_size: Union[int, Tuple[int, int]],
        bias: Optional[torch.Tensor] = None,
        scale: Optional[float] = None,
) -> torch.Tensor:
    """Shifted-window attention on the map.  qkv: [B, Hf, Wf, 3*heads*D] (the
    qkv Linear's output, channel order (3, heads, D)); bias: [heads, N, N] or
    [1, heads, N, N], shared by every window.  Returns [B, Hf, Wf, heads*D]."""
    ws, ss = _pair(window_size), _pair(shift_size)
    D = qkv.shape[-1] // (3 * num_heads)
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    N = ws[0] * ws[1]
    if bias is not None:
        bias = bias.reshape(num_heads, N, N)
    if _kernel_supported(qkv, num_heads, ws, ss):
        if bias is not None:
            # outside the Function, as _prep_mask: autograd casts the fp32
            # gradient back to the parameter's dtype
            bias = bias.contiguous().to(torch.float32)
        return _WindowAttnFn.apply(qkv, bias, num_heads, ws, ss, float(scale))
    if qkv.is_cuda:
        from . import use_hip
        use_hip(qkv)  # raises when the extension is missing on a GPU box
    return _math_window_attention(qkv, num_heads, ws, ss, bias, scale)
