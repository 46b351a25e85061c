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

With `logit_scale` the op is SwinV2's cosine attention,
`softmax(logit_scale[h] * normalize(q) normalize(k)^T + bias + mask) V`, served
by csrc/window_cos_attention.hip (one workgroup per (window, head) pair, window
area <= 256, fp32 norms and scale, dBias in a kernel of its own).

Kernel range: bf16, head_dim 32, window area <= 64 (cosine: <= 256), no padding
(`Hf % wh == 0`, `Wf % ww == 0`), `0 <= shift < window`, contiguous qkv.
Everything else (CPU, fp32, other shapes) runs the plain composition below,
which is also the numerics oracle of the GPU tests.
"""
import math
from typing import Optional, Tuple, Union

import torch
import torch.nn.functional as F

from . import _load_extension
from .attention import _dbias_nsplit

_HEAD_DIM = 32
_MAX_AREA = 64
_MAX_COS_AREA = 256
# kernel launches since import: lets a test assert which path a model took
WINDOW_ATTN_CALLS = {'fwd': 0, 'bwd': 0}
WINDOW_COS_ATTN_CALLS = {'fwd': 0, 'bwd': 0}


def _pair(v) -> Tuple[int, int]:
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def _kernel_supported(qkv, num_heads, ws, ss, max_area=_MAX_AREA) -> bool:
    if not qkv.is_cuda or qkv.dtype != torch.bfloat16 or qkv.dim() != 4:
        return False
    if _load_extension() is None:
        return False
    _, Hf, Wf, C3 = qkv.shape
    return (C3 == 3 * num_heads * _HEAD_DIM and ws[0] * ws[1] <= max_area
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


def _math_window_attention(qkv, num_heads, ws, ss, bias, scale, logit_scale=None):
    """roll -> partition -> softmax(scale QK^T + bias + mask) V (fp32 softmax)
    -> reverse -> roll.  With `logit_scale` ([heads]) q and k are normalised
    and the per-head logit_scale takes the place of `scale`."""
    B, Hf, Wf, C3 = qkv.shape
    D = C3 // (3 * num_heads)
    shifted = any(ss)
    if shifted:
        qkv = torch.roll(qkv, shifts=(-ss[0], -ss[1]), dims=(1, 2))
    win = _windows(qkv, ws).reshape(-1, ws[0] * ws[1], 3, num_heads, D)
    q, k, v = win.permute(2, 0, 3, 1, 4).float().unbind(0)  # [B*nW, heads, N, D]
    if logit_scale is not None:
        q, k = F.normalize(q, dim=-1), F.normalize(k, dim=-1)
        scale = logit_scale.float().view(1, num_heads, 1, 1)
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


class _WindowCosAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, bias, logit_scale, num_heads, ws, ss):
        ext = _load_extension()
        WINDOW_COS_ATTN_CALLS['fwd'] += 1
        o, lse = ext.window_cos_attention_fwd(
            qkv, bias, logit_scale, num_heads, ws[0], ws[1], ss[0], ss[1])
        ctx.save_for_backward(qkv, o, lse, logit_scale)
        ctx.bias = bias
        ctx.args = (num_heads, ws, ss)
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse, logit_scale = ctx.saved_tensors
        num_heads, ws, ss = ctx.args
        ext = _load_extension()
        WINDOW_COS_ATTN_CALLS['bwd'] += 1
        need_dbias = ctx.bias is not None and ctx.needs_input_grad[1]
        if not do.is_contiguous() or do.data_ptr() % 16 != 0:
            do = do.contiguous()
        N = ws[0] * ws[1]
        n_win = qkv.shape[0] * (qkv.shape[1] // ws[0]) * (qkv.shape[2] // ws[1])
        # the dBias kernel runs one wave (and one slab row block) per head,
        # 16-query block and chunk of windows
        nsplit = _dbias_nsplit(n_win, num_heads * -(-N // 16), num_heads * N * N * 4)
        dqkv, dscale, dbias = ext.window_cos_attention_bwd(
            qkv, o, lse, do, ctx.bias, logit_scale, num_heads, ws[0], ws[1], ss[0], ss[1],
            need_dbias, nsplit)
        # one partial per (window, head), summed in a fixed order
        dscale = dscale.sum(0) if ctx.needs_input_grad[2] else None
        return dqkv, dbias, dscale, None, None, None


def window_attention(
        qkv: torch.Tensor,
        num_heads: int,
        window_size: Union[int, Tuple[int, int]],
        shift_size: Union[int, Tuple[int, int]],
        bias: Optional[torch.Tensor] = None,
        scale: Optional[float] = None,
        logit_scale: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Shifted-window attention on the map.  qkv: [B, Hf, Wf, 3*heads*D] (the
    qkv Linear's output, channel order (3, heads, D)); bias: [heads, N, N] or
    [1, heads, N, N], shared by every window.  Returns [B, Hf, Wf, heads*D].

    `logit_scale` (`num_heads` elements, any shape) selects SwinV2's cosine
    attention: q and k are normalised (`F.normalize`) and their cosine is
    multiplied by `logit_scale[h]`, i.e. the model passes
    `clamp(logit_scale, max=log(100)).exp()`; `scale` must then be None."""
    ws, ss = _pair(window_size), _pair(shift_size)
    D = qkv.shape[-1] // (3 * num_heads)
    N = ws[0] * ws[1]
    if bias is not None:
        bias = bias.reshape(num_heads, N, N)
    if logit_scale is not None:
        if scale is not None:
            raise ValueError('window_attention: scale must be None when logit_scale is given')
        logit_scale = logit_scale.reshape(num_heads)
        if _kernel_supported(qkv, num_heads, ws, ss, _MAX_COS_AREA):
            # fp32 outside the Function: autograd casts the gradients back
            if bias is not None:
                bias = bias.contiguous().to(torch.float32)
                if bias.data_ptr() % 16 != 0:
                    bias = bias.clone()
            return _WindowCosAttnFn.apply(
                qkv, bias, logit_scale.contiguous().to(torch.float32), num_heads, ws, ss)
        if qkv.is_cuda:
            from . import use_hip
            use_hip(qkv)  # raises when the extension is missing on a GPU box
        return _math_window_attention(qkv, num_heads, ws, ss, bias, None, logit_scale)
    if scale is None:
        scale = 1.0 / math.sqrt(D)
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
