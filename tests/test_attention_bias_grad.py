"""Additive attention bias is trainable: CPU plumbing + the dBias split rule.

The CPU path of `ops.flash_attention` / `ops.flash_attention_qkv` is the
composition the fused GPU path has to match (tests/test_attention_bias_grad_gpu.py),
so its bias gradient is pinned here against an explicit softmax composition.
"""
import math

import pytest
import torch

import timm_amd  # noqa: F401
from timm_amd import ops
from timm_amd.ops import attention as attn_mod


def _explicit(q, k, v, full_bias, scale):
    attn = (q @ k.transpose(-2, -1)) * scale + full_bias
    return attn.softmax(-1) @ v


def _rel(a, b):
    assert b.norm() > 0
    return ((a - b).norm() / b.norm()).item()


@pytest.mark.parametrize('bias_shape', ['1HNN', 'cyclic', '1H1N'])
@pytest.mark.parametrize('packed', [False, True])
def test_cpu_bias_grad_matches_composition(bias_shape, packed):
    torch.manual_seed(0)
    B, H, N, D = 4, 3, 10, 32
    scale = 1.0 / math.sqrt(D)
    qkv = torch.randn(B, N, 3, H, D)
    shape = {'1HNN': (1, H, N, N), 'cyclic': (2, H, N, N), '1H1N': (1, H, 1, N)}[bias_shape]
    bias = (torch.randn(shape) * 2.0).requires_grad_(True)
    do = torch.randn(B, H, N, D)

    qkv1 = qkv.clone().requires_grad_(True)
    if packed:
        o = ops.flash_attention_qkv(qkv1, attn_mask=bias)
    else:
        q, k, v = qkv1.permute(2, 0, 3, 1, 4).unbind(0)
        o = ops.flash_attention(q, k, v, attn_mask=bias)
    o.backward(do)
    got, got_qkv = bias.grad.clone(), qkv1.grad.clone()

    bias2 = bias.detach().clone().requires_grad_(True)
    qkv2 = qkv.clone().requires_grad_(True)
    q, k, v = qkv2.permute(2, 0, 3, 1, 4).unbind(0)
    # cyclic: batch b reads bias[b % mB], the rule the kernels use
    full = bias2.repeat(B // shape[0], 1, 1, 1) if bias_shape == 'cyclic' else bias2
    _explicit(q, k, v, full, scale).backward(do)

    assert got.shape == bias.shape
    assert torch.isfinite(got).all()
    assert _rel(got, bias2.grad) < 1e-5
    assert _rel(got_qkv, qkv2.grad) < 1e-5


def test_nsplit_one_reduced_batch():
    # nothing to split: a single (batch, head) pair per bias element
    assert attn_mod._dbias_nsplit(1, 1, 4096) == 1
    assert attn_mod._dbias_nsplit(1, 10_000, 1 << 30) == 1
    assert attn_mod._dbias_nsplit(0, 1, 4096) == 1


@pytest.mark.parametrize('n_red', [2, 3, 7, 64, 255, 4096])
@pytest.mark.parametrize('n_tiles', [1, 3, 12, 192, 1023, 1024, 1025, 100_000])
def test_nsplit_bounded_by_reduced_batches(n_red, n_tiles):
    ns = attn_mod._dbias_nsplit(n_red, n_tiles, 49 * 49 * 4)
    assert 1 <= ns <= n_red
    # a split is only worth its slab if it loops over a few pairs
    assert ns == 1 or n_red // ns >= attn_mod._DBIAS_MIN_CHUNK
    # every chunk of ceil(n_red / ns) pairs is non-empty
    chunk = -(-n_red // ns)
    assert (ns - 1) * chunk < n_red
    # grid reaches the target unless capped by n_red; never overshoots by
    # more than one split's worth of tiles
    target = attn_mod._DBIAS_TARGET_BLOCKS
    if n_tiles >= target:
        assert ns == 1
    else:
        assert ns * n_tiles < target + n_tiles * 2


def test_nsplit_workspace_cap():
    cap = attn_mod._DBIAS_MAX_WORKSPACE
    # slab exactly the cap, or larger: no room for more than one slab
    assert attn_mod._dbias_nsplit(4096, 1, cap) == 1
    assert attn_mod._dbias_nsplit(4096, 1, cap * 2) == 1
    # half the cap: two slabs fit, not three
    assert attn_mod._dbias_nsplit(4096, 1, cap // 2) == 2
    for slab in (1 << 10, 1 << 20, 3 << 20, cap // 3, cap // 2 + 1):
        ns = attn_mod._dbias_nsplit(4096, 1, slab)
        assert ns == 1 or ns * slab <= cap


def test_mask_nsplit_swin_and_small():
    """Shape helper feeds the chooser what the kernel reduces over."""
    # Swin stage-1 unshifted: 3 tiles, 4096 windows -> split
    q = torch.empty(4096, 3, 49, 32)
    assert attn_mod._mask_nsplit(q, q, torch.empty(1, 3, 49, 49)) > 1
    # per-sample, per-head bias: one pair per element -> never split
    q = torch.empty(4, 4, 49, 32)
    assert attn_mod._mask_nsplit(q, q, torch.empty(4, 4, 49, 49)) == 1
    # head-broadcast bias reduces over heads: 4 batches x 4 heads -> 16 pairs
    assert attn_mod._mask_nsplit(q, q, torch.empty(1, 1, 49, 49)) == 16 // attn_mod._DBIAS_MIN_CHUNK
    assert attn_mod._mask_nsplit(q, q, torch.empty(1, 4, 49, 49)) == 1


def test_forced_nsplit_and_back():
    q = torch.empty(4096, 3, 49, 32)
    bias = torch.empty(1, 3, 49, 49)
    auto = attn_mod._mask_nsplit(q, q, bias)
    attn_mod.set_dbias_nsplit(7)
    try:
        assert attn_mod._mask_nsplit(q, q, bias) == 7
    finally:
        attn_mod.set_dbias_nsplit(None)
    assert attn_mod._mask_nsplit(q, q, bias) == auto
