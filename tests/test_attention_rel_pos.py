"""rel_pos_hw= of ops.flash_attention on CPU: the reference composition."""
import math

import torch

from timm_amd import ops


def test_rel_pos_cpu_matches_fp32_softmax():
    torch.manual_seed(0)
    B, H, Nq, Kh, Kw, D = 2, 2, 9, 3, 5, 16
    q = torch.randn(B, H, Nq, D)
    k, v = torch.randn(B, H, Kh * Kw, D), torch.randn(B, H, Kh * Kw, D)
    rel_h = torch.randn(B, H, Nq, Kh, requires_grad=True)
    rel_w = torch.randn(B, H, Nq, Kw, requires_grad=True)
    o = ops.flash_attention(q, k, v, rel_pos_hw=(rel_h, rel_w))
    bias = (rel_h[..., :, None] + rel_w[..., None, :]).flatten(-2)
    ref = torch.softmax(q @ k.transpose(-2, -1) / math.sqrt(D) + bias, dim=-1) @ v
    torch.testing.assert_close(o, ref)
    g = torch.autograd.grad(o.sum(), (rel_h, rel_w))
    g_ref = torch.autograd.grad(ref.sum(), (rel_h, rel_w))
    torch.testing.assert_close(g, g_ref)
