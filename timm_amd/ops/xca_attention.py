"""Cross-covariance attention (XCiT's XCA) on the packed qkv.

`cross_covariance_attention` takes the qkv Linear's output `[B, N, 3*C]`
(channel order (3, heads, d)) and returns `[B, N, C]`, ready for `proj`:

    q^, k^ = q, k L2-normalised over the N tokens (`F.normalize`, eps 1e-12)
    A = softmax_rows(temperature[h] * q^^T k^)        (d x d per head)
    O[n, :] = A v[n, :]

The kernels of csrc/xca_attention.hip read q, k and v in place (one workgroup
per (batch, head), two passes over the tokens), so the `[3, B, H, d, N]`
permute, the two normalised copies, the d x d logits and the output permute
never reach memory; the backward is a closed form on the saved cosines and
inverse norms and writes one `[B, N, 3, H, d]` gradient buffer.

Kernel range: bf16, head_dim 32 / 48 / 64, contiguous 16-byte-aligned qkv,
`dropout_p == 0`.  Everything else (CPU, fp32 / fp16, other head dims, strided
input, attention dropout) runs the plain composition `_math_xca`, which is also
the numerics oracle of the GPU tests.  `set_fused_xca(False)` /
`TIMM_AMD_FUSED_XCA=0` leaves the composition in the input's dtype, op for op
what `XCA.forward` in models/xcit.py computes.

`XCA.forward` does not call this op yet: see "Not wired into the model" in
profiles/xca_attention/README.md.
"""
import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _load_extension

_HEAD_DIMS = (32, 48, 64)
# kernel launches since import: lets a test assert which path a model took
XCA_ATTN_CALLS = {'fwd': 0, 'bwd': 0}


def _kernel_supported(qkv, num_heads, dropout_p) -> bool:
    if not qkv.is_cuda or qkv.dtype != torch.bfloat16 or qkv.dim() != 3 or dropout_p > 0.:
        return False
    if _load_extension() is None:
        return False
    return (qkv.shape[-1] % (3 * num_heads) == 0
            and qkv.shape[-1] // (3 * num_heads) in _HEAD_DIMS
            and qkv.is_contiguous() and qkv.data_ptr() % 16 == 0 and qkv.numel() > 0)


def _math_xca(qkv, num_heads, temperature, dropout_p=0., fp32_softmax=True):
    """permute -> normalize over tokens -> softmax(temperature * q k^T) v ->
    permute.  `fp32_softmax=False` is the XCA module's composition: every op in
    the input's dtype."""
    B, N, C3 = qkv.shape
    C = C3 // 3
    # (qkv, B, heads, C-per-head, N)
    q, k, v = qkv.reshape(B, N, 3, num_heads, C // num_heads).permute(2, 0, 3, 4, 1).unbind(0)
    q = F.normalize(q, dim=-1)
    k = F.normalize(k, dim=-1)
    attn = (q @ k.transpose(-2, -1)) * temperature.reshape(num_heads, 1, 1)
    if fp32_softmax:
        attn = attn.softmax(dim=-1, dtype=torch.float32).to(v.dtype)
    else:
        attn = attn.softmax(dim=-1)
    if dropout_p > 0.:
        attn = F.dropout(attn, dropout_p)
    x = attn @ v
    return x.permute(0, 3, 1, 2).reshape(B, N, C)


class _XcaFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, temperature, num_heads):
        ext = _load_extension()
        XCA_ATTN_CALLS['fwd'] += 1
        o, c, inv = ext.xca_attention_fwd(qkv, temperature, num_heads)
        ctx.save_for_backward(qkv, temperature, c, inv)
        ctx.num_heads = num_heads
        return o

    @staticmethod
    @once_differentiable
    def backward(ctx, do):
        qkv, temperature, c, inv = ctx.saved_tensors
        ext = _load_extension()
        XCA_ATTN_CALLS['bwd'] += 1
        if not do.is_contiguous() or do.data_ptr() % 16 != 0:
            do = do.contiguous()
        dqkv, dtau = ext.xca_attention_bwd(qkv, do, temperature, c, inv, ctx.num_heads)
        # one partial per (batch, head), summed in a fixed order
        dtau = dtau.sum(0) if ctx.needs_input_grad[1] else None
        return dqkv, dtau, None


def cross_covariance_attention(
        qkv: torch.Tensor,
        num_heads: int,
        temperature: torch.Tensor,
        dropout_p: float = 0.,
) -> torch.Tensor:
    """Cross-covariance attention.  qkv: [B, N, 3*C], the qkv Linear's output
    (channel order (3, heads, C // heads)); temperature: `num_heads` elements,
    any shape and dtype (its gradient comes back in that shape and dtype);
    `dropout_p > 0` drops entries of the d x d attention matrix.  Returns
    [B, N, C]."""
    from ..layers.config import use_fused_xca
    if not use_fused_xca():
        return _math_xca(qkv, num_heads, temperature, dropout_p, fp32_softmax=False)
    if _kernel_supported(qkv, num_heads, dropout_p):
        # fp32 outside the Function: autograd casts and reshapes the gradient back
        tau = temperature.reshape(num_heads).to(torch.float32).contiguous()
        return _XcaFn.apply(qkv, tau, num_heads)
    if qkv.is_cuda:
        from . import use_hip
        use_hip(qkv)  # raises when the extension is missing on a GPU box
    return _math_xca(qkv, num_heads, temperature, dropout_p)
