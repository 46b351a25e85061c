"""Bool attention masks on the CPU composition: True = the key takes part
(F.scaled_dot_product_attention semantics), a query row with no valid key
gives zeros and zero gradients.  Reference: fp64 masked softmax."""
import math

import pytest
import torch

from timm_amd import ops


def _reference(q, k, v, mask):
    """fp64 softmax over the True entries; rows with none are zero."""
    q, k, v = [t.detach().double().requires_grad_(True) for t in (q, k, v)]
    s = (q @ k.transpose(-2, -1)) / math.sqrt(q.shape[-1])
    e = torch.exp(s - s.amax(-1, keepdim=True)) * mask
    o = (e / e.sum(-1, keepdim=True).clamp(min=1e-300)) @ v
    return o, (q, k, v)


@pytest.mark.parametrize('packed', [False, True])
@pytest.mark.parametrize('key_padding', [True, False])
def test_bool_mask_cpu(packed, key_padding):
    torch.manual_seed(0)
    B, H, N, D = 3, 2, 19, 16
    qkv = torch.randn(B, N, 3, H, D, requires_grad=True)
    q, k, v = [qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3)]
    valid = torch.rand(B, N) > 0.3
    valid[1] = False  # a sample with no valid key
    mask = valid[:, None, None, :]
    if not key_padding:  # full [B,1,Nq,Nk]: also drop some query/key pairs
        mask = mask & (torch.rand(B, 1, N, N) > 0.2)
        mask[2, 0, 5] = False  # a single query row with no valid key

    o = ops.flash_attention_qkv(qkv, attn_mask=mask) if packed \
        else ops.flash_attention(q, k, v, attn_mask=mask)
    do = torch.randn_like(o)
    o.backward(do)
    dq, dk, dv = [qkv.grad[:, :, i].permute(0, 2, 1, 3) for i in range(3)]

    o_ref, ref_in = _reference(q, k, v, mask)
    o_ref.backward(do.double())
    assert torch.isfinite(o).all() and torch.isfinite(qkv.grad).all()
    # fp32 composition against fp64: O(1) values, sums of at most 19 terms at
    # eps 1.2e-7, so errors stay near 1e-6
    assert (o.double() - o_ref).abs().max().item() < 1e-5
    for g, r in zip((dq, dk, dv), ref_in):
        assert (g.double() - r.grad).abs().max().item() < 1e-5
    assert o[1].abs().max().item() == 0.0
    assert qkv.grad[1].abs().max().item() == 0.0
    if not key_padding:
        assert o[2, :, 5].abs().max().item() == 0.0
        assert dq[2, :, 5].abs().max().item() == 0.0
