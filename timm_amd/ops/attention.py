"""Fused multi-head attention dispatch (SDPA replacement).

The reference leans on `F.scaled_dot_product_attention`
(`timm/layers/attention.py:124-129`, `timm/models/eva.py:239-251`).  Here both
directions are hand-written flash-style gfx950 HIP kernels:

 * forward: MFMA 16x16x32 bf16 QK^T + online softmax + PV, returns O and
   logsumexp (LSE) per row.  Supports optional additive mask (NaFlex padding
   masks, rel-pos bias broadcast over batch).
 * backward: fused flash backward — softmax recomputed from LSE inside the
   tile loop, dQ/dK/dV accumulated in fp32 MFMA registers, no [B,H,Nq,Nk]
   tensor ever touches HBM.  Two implementations, chosen per call by
   `_select_bwd_path` (rule and numbers next to it):
     - single-pass (attn_bwd_single_pass kernel): head_dim 64 and
       49 <= Nk <= 256 (ViT / DeiT / BEiT at 224², windows of 49..144
       tokens).  One workgroup per (batch, head) owns every key, S / dP / P /
       dS are computed once, dK / dV stay in registers over the whole sweep
       of the query rows, dQ is completed inside the workgroup (no atomics),
       and delta = rowsum(dO o O) is formed in the kernel from strided dO
       and O, so attn_bwd_preprocess is not launched unless a bias gradient
       is wanted.
     - two-pass (attn_bwd_dq / attn_bwd_dkdv kernels behind
       attn_bwd_preprocess): everything else — Nk > 256, other head dims.
   TIMM_AMD_ATTN_BWD=two_pass forces the two-pass kernels for a process,
   `set_attn_bwd_path` forces either from code; the round-1 hipBLASLt
   GEMM-recompute chain remains available via TIMM_AMD_ATTN_BWD=gemm for A/B
   comparison (both entries).
 * bias gradient: when the additive mask requires grad (learned rel-pos bias
   of Swin / BEiT / vit_relpos / ...), a third flash pass (attn_bwd_dbias
   kernel) recomputes P and dP per 64x64 tile and sums the unscaled
   dS = P o (dP - delta) in fp32 registers over the batches (and heads) that
   share a bias element.  The batch loop is split over the grid into fp32
   slabs that a small kernel sums in a fixed order - no atomics, so the
   result is bit-reproducible.  Masks that need no gradient (padding masks,
   inference) cost no extra launch or allocation.  Broadcast shapes are
   reduced by autograd through `_prep_mask`, which stays outside the
   autograd Function.
 * flash_attention_qkv: packed-qkv entry — takes the [B,N,3,H,D] projection
   output directly and writes gradients into one packed dqkv buffer, so the
   qkv-unbind `aten::copy_`/stack grad chain never appears in the graph.

CPU path = reference math composition (fp32 softmax), which doubles as the
numerics oracle for the GPU tests.
"""
import math
import os
from typing import Optional

import torch
import torch.nn.functional as F

from . import _load_extension

_BWD_MODE = os.environ.get('TIMM_AMD_ATTN_BWD', 'fused')


def attention_available(q: torch.Tensor) -> bool:
    if not q.is_cuda or _load_extension() is None:
        return False
    D = q.shape[-1]
    return D <= 128 and D % 32 == 0 and q.dtype == torch.bfloat16


def _cyclic_mask(attn_mask, B):
    """The kernels read a [mB,...] mask with 1 < mB < B, B % mB == 0 as
    mask[b % mB] (Swin shift masks); the compositions take the same layout."""
    if attn_mask.dim() == 4 and 1 < attn_mask.shape[0] < B and B % attn_mask.shape[0] == 0:
        return attn_mask.repeat(B // attn_mask.shape[0], 1, 1, 1)
    return attn_mask


def _math_sdpa(q, k, v, attn_mask=None, scale=None):
    """Reference composition (matches F.scaled_dot_product_attention semantics)."""
    scale = scale if scale is not None else 1.0 / math.sqrt(q.shape[-1])
    attn = (q.float() @ k.float().transpose(-2, -1)) * scale
    if attn_mask is not None:
        attn = attn + _cyclic_mask(attn_mask, q.shape[0]).float()
    attn = attn.softmax(dim=-1)
    out = attn @ v.float()
    return out.to(q.dtype)


def _strides_ok(t):
    return t.stride(-1) == 1 and all(s % 8 == 0 or s == 0 for s in t.stride()[:3])


def _prep_mask(attn_mask, q, k):
    # kernel accepts [B|1, H|1, Nq, Nk]: keep batch/head dims unexpanded
    # (rel-pos bias is [1,H,N,N], padding masks [B,1,N,N]) so the contiguous
    # copy stays small.
    while attn_mask.dim() < 4:
        attn_mask = attn_mask.unsqueeze(0)
    attn_mask = attn_mask.expand(
        attn_mask.shape[0], attn_mask.shape[1], q.shape[2], k.shape[2])
    return attn_mask.contiguous().to(torch.float32)


# dBias pass split heuristic (see profiles/attn_dbias/README.md for the sweep):
# aim for _DBIAS_TARGET_BLOCKS blocks in the grid (a few per CU on 256 CUs),
# give every split at least _DBIAS_MIN_CHUNK reduced (batch, head) pairs so the
# slab write and the second kernel stay small next to the loop, and keep the
# fp32 slab workspace under _DBIAS_MAX_WORKSPACE bytes.
_DBIAS_TARGET_BLOCKS = 1024
_DBIAS_MIN_CHUNK = 4
_DBIAS_MAX_WORKSPACE = 64 << 20
_DBIAS_NSPLIT_FORCED: Optional[int] = None


def set_dbias_nsplit(nsplit: Optional[int] = None):
    """Force the dBias split count (tools/bench_attn_bias.py sweeps it);
    None goes back to the heuristic."""
    global _DBIAS_NSPLIT_FORCED
    _DBIAS_NSPLIT_FORCED = None if nsplit is None else max(int(nsplit), 1)


def _dbias_nsplit(n_red: int, n_tiles: int, slab_bytes: int) -> int:
    """Number of chunks the dBias reduction loop is cut into.

    n_red: (batch, head) pairs summed into one bias element,
    n_tiles: 64x64 output tiles of the whole bias (= blocks at nsplit 1),
    slab_bytes: size of one fp32 copy of the bias gradient.
    """
    if n_red <= 1:
        return 1
    nsplit = -(-_DBIAS_TARGET_BLOCKS // max(n_tiles, 1))
    nsplit = min(nsplit, n_red // _DBIAS_MIN_CHUNK,
                 max(_DBIAS_MAX_WORKSPACE // max(slab_bytes, 1), 1))
    if nsplit <= 1:
        return 1
    chunk = -(-n_red // nsplit)
    return -(-n_red // chunk)  # drop chunks that would be empty


def _mask_nsplit(q, k, attn_mask) -> int:
    if _DBIAS_NSPLIT_FORCED is not None:
        return _DBIAS_NSPLIT_FORCED
    B, H, Nq = q.shape[:3]
    Nk = k.shape[2]
    mB, Hm = attn_mask.shape[:2]
    n_red = (B // mB) * (H if Hm == 1 else 1)
    n_tiles = mB * Hm * (-(-Nq // 64)) * (-(-Nk // 64))
    return _dbias_nsplit(n_red, n_tiles, mB * Hm * Nq * Nk * 4)


# Which fused backward runs (numbers: profiles/attn_bwd_single_pass/README.md):
# the single-pass kernel (one workgroup per (batch, head) owns every key)
# takes head_dim 64 with _SINGLE_PASS_MIN_NK <= Nk <= 256 and 16-byte-aligned
# rows, with or without a mask: it was measured faster than the two-pass
# kernels without a mask at Nk = 49, 64, 144 and 197, and with one ([1,H,N,N]
# bias, cyclic [mB,H,N,N] bias + shift mask) at Nk = 49, 64, 100, 144 and 197
# (smallest margin: 28 us of 380 at Nk = 64 with a bias).  Everything else -
# longer sequences, other head dims, and Nk < 49, which was not measured -
# stays on the two-pass kernels.  Where no bias gradient is wanted the single-pass
# kernel reads dO and O through their strides and forms delta itself, so
# attn_bwd_preprocess is not launched; with a bias gradient the preprocess
# still runs, because the dBias kernel needs its contiguous dO and delta.
_SINGLE_PASS_MAX_NK = 256
_SINGLE_PASS_MIN_NK = 49
_BWD_PATHS = ('two_pass', 'single_pass', 'single_pass_preprocess')
_BWD_PATH_FORCED: Optional[str] = None
# calls per path since import: lets a test assert which kernels ran
BWD_PATH_CALLS = {'two_pass': 0, 'single_pass': 0}


def set_attn_bwd_path(path: Optional[str] = None):
    """Force the fused backward: 'two_pass', 'single_pass' (wherever the
    single-pass kernel supports the shape) or 'single_pass_preprocess' (the
    same kernel fed by attn_bwd_preprocess, for tools/bench_attn_bwd.py);
    None goes back to the measured rule.  TIMM_AMD_ATTN_BWD=two_pass sets the
    first of these for a whole process."""
    global _BWD_PATH_FORCED
    assert path is None or path in _BWD_PATHS, path
    _BWD_PATH_FORCED = path


def _aligned16(t):
    return (t.dim() == 4 and t.stride(-1) == 1 and t.data_ptr() % 16 == 0
            and all(s % 8 == 0 for s in t.stride()[:3]))


def _single_pass_supported(q, k, v, dq, dk, dv):
    return (q.shape[-1] == 64 and 1 <= k.shape[2] <= _SINGLE_PASS_MAX_NK
            and q.numel() > 0 and all(_aligned16(t) for t in (q, k, v, dq, dk, dv)))


def _select_bwd_path(q, k, v, dq, dk, dv) -> str:
    forced = _BWD_PATH_FORCED
    if forced is None and _BWD_MODE == 'two_pass':
        forced = 'two_pass'
    if forced == 'two_pass' or not _single_pass_supported(q, k, v, dq, dk, dv):
        return 'two_pass'
    if forced is not None:
        return forced
    return 'single_pass' if k.shape[2] >= _SINGLE_PASS_MIN_NK else 'two_pass'


def _fused_backward(ext, q, k, v, o, lse, do, attn_mask, scale, dq, dk, dv, need_dbias=False):
    """Shared fused-backward driver writing into preallocated dq/dk/dv.
    Returns the fp32 mask gradient when `need_dbias`, else None."""
    path = _select_bwd_path(q, k, v, dq, dk, dv)
    if path == 'single_pass' and not need_dbias:
        BWD_PATH_CALLS['single_pass'] += 1
        if not _aligned16(do):
            do = do.contiguous()
        ext.attention_bwd_single_pass(
            q, k, v, do, o, lse, None, attn_mask, dq, dk, dv, scale)
        return None
    if do.dim() == 4 and do.stride(-1) == 1 and do.shape[-1] % 32 == 0 and do.shape[-1] <= 128:
        do_c, delta = ext.attn_bwd_preprocess(do, o)
    else:
        do_c = do.contiguous()
        delta = (do_c * o).float().sum(-1)
    if path == 'two_pass':
        BWD_PATH_CALLS['two_pass'] += 1
        ext.attention_bwd(q, k, v, do_c, lse, delta, attn_mask, dq, dk, dv, scale)
    else:
        BWD_PATH_CALLS['single_pass'] += 1
        ext.attention_bwd_single_pass(
            q, k, v, do_c, None, lse, delta, attn_mask, dq, dk, dv, scale)
    if need_dbias:
        return ext.attention_bwd_dbias(
            q, k, v, do_c, lse, delta, attn_mask, scale, _mask_nsplit(q, k, attn_mask))
    return None


def _gemm_backward(ext, q, k, v, o, lse, do, attn_mask, scale, need_dbias=False):
    """Round-1 exact recompute via hipBLASLt GEMMs (A/B reference path).
    The mask gradient comes from the same dBias kernel as the fused path."""
    if do.dim() == 4 and do.stride(-1) == 1 and do.shape[-1] % 32 == 0 and do.shape[-1] <= 128:
        do, delta = ext.attn_bwd_preprocess(do, o)
    else:
        do = do.contiguous()
        delta = (do * o).float().sum(-1)
    s = (q @ k.transpose(-2, -1)).contiguous()
    p = ext.attn_bwd_softmax(s, lse, attn_mask, scale)
    dv = p.transpose(-2, -1) @ do
    dp = (do @ v.transpose(-2, -1)).contiguous()
    ds = ext.attn_bwd_ds(p, dp, delta, scale)
    dq = ds @ k
    dk = ds.transpose(-2, -1) @ q
    dbias = None
    if need_dbias:
        dbias = ext.attention_bwd_dbias(
            q, k, v, do, lse, delta, attn_mask, scale, _mask_nsplit(q, k, attn_mask))
    return dq, dk, dv, dbias


class _FlashAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, attn_mask, scale):
        ext = _load_extension()
        # kernel reads strided q/k/v (e.g. views into the packed qkv tensor)
        # as long as head_dim is contiguous and 16B-alignment holds
        if not _strides_ok(q):
            q = q.contiguous()
        if not _strides_ok(k):
            k = k.contiguous()
        if not _strides_ok(v):
            v = v.contiguous()
        if attn_mask is not None:
            attn_mask = attn_mask.contiguous().to(torch.float32)
        o, lse = ext.attention_fwd(q, k, v, attn_mask, scale)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.attn_mask = attn_mask
        ctx.scale = scale
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        ext = _load_extension()
        scale = ctx.scale
        need_dbias = ctx.attn_mask is not None and ctx.needs_input_grad[3]
        if _BWD_MODE == 'gemm':
            dq, dk, dv, dbias = _gemm_backward(
                ext, q, k, v, o, lse, do, ctx.attn_mask, scale, need_dbias)
        else:
            dq = torch.empty_like(q, memory_format=torch.contiguous_format)
            dk = torch.empty_like(k, memory_format=torch.contiguous_format)
            dv = torch.empty_like(v, memory_format=torch.contiguous_format)
            dbias = _fused_backward(
                ext, q, k, v, o, lse, do, ctx.attn_mask, scale, dq, dk, dv, need_dbias)
        return dq, dk, dv, dbias, None


class _FlashAttnQkvFn(torch.autograd.Function):
    """Packed-qkv attention: input [B,N,3,H,D], grads written into one packed
    dqkv buffer (kills the unbind/stack grad copies)."""

    @staticmethod
    def forward(ctx, qkv, attn_mask, scale):
        ext = _load_extension()
        B, N, three, H, D = qkv.shape
        q = qkv[:, :, 0].permute(0, 2, 1, 3)  # [B,H,N,D] strided view
        k = qkv[:, :, 1].permute(0, 2, 1, 3)
        v = qkv[:, :, 2].permute(0, 2, 1, 3)
        if attn_mask is not None:
            attn_mask = attn_mask.contiguous().to(torch.float32)
        o, lse = ext.attention_fwd(q, k, v, attn_mask, scale)
        ctx.save_for_backward(qkv, o, lse)
        ctx.attn_mask = attn_mask
        ctx.scale = scale
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse = ctx.saved_tensors
        ext = _load_extension()
        q = qkv[:, :, 0].permute(0, 2, 1, 3)
        k = qkv[:, :, 1].permute(0, 2, 1, 3)
        v = qkv[:, :, 2].permute(0, 2, 1, 3)
        dqkv = torch.empty_like(qkv)
        dq = dqkv[:, :, 0].permute(0, 2, 1, 3)
        dk = dqkv[:, :, 1].permute(0, 2, 1, 3)
        dv = dqkv[:, :, 2].permute(0, 2, 1, 3)
        need_dbias = ctx.attn_mask is not None and ctx.needs_input_grad[1]
        if _BWD_MODE == 'gemm':
            # the A/B reference path reaches the packed entry too (the ViT blocks)
            gq, gk, gv, dbias = _gemm_backward(
                ext, q, k, v, o, lse, do, ctx.attn_mask, ctx.scale, need_dbias)
            dq.copy_(gq)
            dk.copy_(gk)
            dv.copy_(gv)
            return dqkv, dbias, None
        dbias = _fused_backward(
            ext, q, k, v, o, lse, do, ctx.attn_mask, ctx.scale, dq, dk, dv, need_dbias)
        return dqkv, dbias, None


def flash_attention(
        q: torch.Tensor,
        k: torch.Tensor,
        v: torch.Tensor,
        attn_mask: Optional[torch.Tensor] = None,
        dropout_p: float = 0.,
        scale: Optional[float] = None,
) -> torch.Tensor:
    """Fused attention. q,k,v: [B, H, N, D]. attn_mask: additive, broadcastable to [B,H,Nq,Nk]."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if dropout_p > 0.:
        # attention-dropout path falls back to composition (rare in configs we target)
        return _dropout_sdpa(q, k, v, attn_mask, dropout_p, scale)
    if attention_available(q):
        if attn_mask is not None:
            attn_mask = _prep_mask(attn_mask, q, k)
        return _FlashAttnFn.apply(q, k, v, attn_mask, scale)
    if q.is_cuda:
        from . import use_hip
        if use_hip(q):
            # ext present but shape/dtype unsupported (e.g. fp32, D>128): exact composition
            return _math_sdpa(q, k, v, attn_mask, scale)
    return _math_sdpa(q, k, v, attn_mask, scale)


def flash_attention_qkv(
        qkv: torch.Tensor,
        attn_mask: Optional[torch.Tensor] = None,
        dropout_p: float = 0.,
        scale: Optional[float] = None,
) -> torch.Tensor:
    """Packed attention on the qkv projection output.

    qkv: [B, N, 3, H, D] (the reshaped nn.Linear output — no permute/unbind
    copies).  Returns O as a [B,H,N,D] view of BNHD storage, so the usual
    `transpose(1,2).reshape(B,N,C)` is free.
    """
    B, N, three, H, D = qkv.shape
    assert three == 3
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    q = qkv[:, :, 0].permute(0, 2, 1, 3)
    if dropout_p == 0. and attention_available(q) and qkv.stride(-1) == 1:
        if attn_mask is not None:
            k = qkv[:, :, 1].permute(0, 2, 1, 3)
            attn_mask = _prep_mask(attn_mask, q, k)
        return _FlashAttnQkvFn.apply(qkv, attn_mask, scale)
    k = qkv[:, :, 1].permute(0, 2, 1, 3)
    v = qkv[:, :, 2].permute(0, 2, 1, 3)
    return flash_attention(q, k, v, attn_mask=attn_mask, dropout_p=dropout_p, scale=scale)


def _dropout_sdpa(q, k, v, attn_mask, dropout_p, scale):
    attn = (q @ k.transpose(-2, -1)) * scale
    if attn_mask is not None:
        attn = attn + _cyclic_mask(attn_mask, q.shape[0])
    attn = attn.softmax(dim=-1)
    attn = F.dropout(attn, p=dropout_p, training=True)
    return attn @ v
