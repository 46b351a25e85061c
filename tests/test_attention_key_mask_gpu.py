"""Key-padding attention kernels (bool [B,1,1,Nk] mask, bf16, head_dim 64)
against an fp32 masked softmax on the same inputs."""
import math

import pytest
import torch

from timm_amd import ops
from timm_amd.ops import attention as attn_mod

pytestmark = pytest.mark.gpu

B, H, D = 3, 2, 64


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp(min=1e-3)).item()


def _valid(pattern, Nk):
    valid = torch.ones(B, Nk, dtype=torch.bool)
    if pattern == 'tail10':
        valid[1:, -10:] = False
    elif pattern == 'tile1':  # a whole 64-key tile between live ones
        valid[:, 64:128] = False
    elif pattern == 'scattered':
        valid = torch.rand(B, Nk, generator=torch.Generator().manual_seed(3)) >= 0.3
    elif pattern == 'samples':  # none valid / 77-key tail invalid / all valid
        valid[0] = False
        valid[1, -77:] = False
    return valid.cuda()


def _inputs(Nq, Nk, D=D):
    torch.manual_seed(Nq * 1000 + Nk)
    q = torch.randn(B, H, Nq, D, device='cuda', dtype=torch.bfloat16)
    k, v = [torch.randn(B, H, Nk, D, device='cuda', dtype=torch.bfloat16) for _ in range(2)]
    return q, k, v, torch.randn(B, H, Nq, D, device='cuda', dtype=torch.bfloat16)


def _reference(q, k, v, valid, do):
    """fp32 softmax over the valid keys; samples with none give zeros."""
    q, k, v = [t.detach().float().requires_grad_(True) for t in (q, k, v)]
    m = valid[:, None, None, :]
    s = (q @ k.transpose(-2, -1)) / math.sqrt(q.shape[-1])
    e = torch.exp(s - s.amax(-1, keepdim=True)) * m
    o = (e / e.sum(-1, keepdim=True).clamp(min=1e-30)) @ v
    o.backward(do.float())
    return o.detach(), q.grad, k.grad, v.grad


def _run(q, k, v, valid, do):
    q, k, v = [t.clone().requires_grad_(True) for t in (q, k, v)]
    o = ops.flash_attention(q, k, v, attn_mask=valid[:, None, None, :])
    o.backward(do)
    return o.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize('Nq,Nk,pattern', [
    (70, 70, 'tail10'),       # partial tail tile
    (200, 200, 'tile1'),      # skipped tile between live ones
    (33, 130, 'scattered'),   # mixed tiles, Nq != Nk
    (64, 64, 'all'),          # the all-ones branch
    (300, 300, 'samples'),
])
def test_key_mask_numerics(Nq, Nk, pattern):
    q, k, v, do = _inputs(Nq, Nk)
    valid = _valid(pattern, Nk)
    before = dict(attn_mod.KEY_MASK_CALLS)
    got = _run(q, k, v, valid, do)
    assert attn_mod.KEY_MASK_CALLS['fwd'] == before['fwd'] + 1
    assert attn_mod.KEY_MASK_CALLS['bwd'] == before['bwd'] + 1
    ref = _reference(q, k, v, valid, do)
    for g, r, tol in zip(got, ref, (2e-2, 4e-2, 4e-2, 4e-2)):
        assert torch.isfinite(g.float()).all()
        assert rel_err(g, r) < tol, rel_err(g, r)
    dead = (~valid)[:, None, :, None].expand_as(got[2])
    assert got[2][dead].float().abs().sum().item() == 0.0
    assert got[3][dead].float().abs().sum().item() == 0.0
    # bit-reproducible from run to run
    for g, g2 in zip(got, _run(q, k, v, valid, do)):
        assert torch.equal(g, g2)


def test_key_mask_packed():
    Nk, pattern = 200, 'tile1'
    torch.manual_seed(7)
    qkv = torch.randn(B, Nk, 3, H, D, device='cuda', dtype=torch.bfloat16, requires_grad=True)
    q, k, v = [qkv.detach()[:, :, i].permute(0, 2, 1, 3) for i in range(3)]
    valid = _valid(pattern, Nk)
    before = dict(attn_mod.KEY_MASK_CALLS)
    o = ops.flash_attention_qkv(qkv, attn_mask=valid[:, None, None, :])
    do = torch.randn_like(o)
    o.backward(do)
    assert attn_mod.KEY_MASK_CALLS['fwd'] == before['fwd'] + 1
    assert attn_mod.KEY_MASK_CALLS['bwd'] == before['bwd'] + 1
    assert torch.equal(o, _run(q, k, v, valid, do)[0])
    o_ref, *grads = _reference(q, k, v, valid, do)
    assert rel_err(o, o_ref) < 2e-2
    dqkv_ref = torch.stack([g.permute(0, 2, 1, 3) for g in grads], dim=2)
    assert torch.isfinite(qkv.grad.float()).all()
    assert rel_err(qkv.grad, dqkv_ref) < 4e-2


def test_key_mask_other_head_dim_takes_additive_path():
    q, k, v, do = _inputs(70, 70, D=72)
    valid = _valid('tail10', 70)
    before = dict(attn_mod.KEY_MASK_CALLS)
    got = _run(q, k, v, valid, do)
    assert attn_mod.KEY_MASK_CALLS == before
    for g, r, tol in zip(got, _reference(q, k, v, valid, do), (2e-2, 4e-2, 4e-2, 4e-2)):
        assert rel_err(g, r) < tol, rel_err(g, r)


def test_naflexvit_key_mask_matches_float_mask():
    """The blocks get the bool key mask and run the key-mask kernels; logits
    match the same model fed the symmetric float mask (tolerance: the model
    output bound of test_vit_block_gpu_vs_cpu)."""
    from timm_amd.layers import set_fused_attn
    from timm_amd.models.naflexvit import NaFlexVit, NaFlexVitCfg
    torch.manual_seed(0)
    model = NaFlexVit(NaFlexVitCfg(embed_dim=128, depth=2, num_heads=2), num_classes=10)
    model = model.eval().to('cuda', torch.bfloat16)
    gh, gw = 8, 10
    coord = torch.stack(torch.meshgrid(torch.arange(gh), torch.arange(gw), indexing='ij'), -1)
    valid = torch.ones(2, gh * gw, dtype=torch.bool)
    valid[1, 50:] = False
    x = dict(
        patches=torch.randn(2, gh * gw, 16 * 16 * 3, device='cuda', dtype=torch.bfloat16),
        patch_coord=coord.reshape(1, -1, 2).expand(2, -1, -1).cuda(),
        patch_valid=valid.cuda())
    before = dict(attn_mod.KEY_MASK_CALLS)
    with torch.no_grad():
        y_key = model(x)
        assert attn_mod.KEY_MASK_CALLS['fwd'] == before['fwd'] + 2
        set_fused_attn(False)  # the model builds the float mask; the blocks stay fused
        try:
            y_float = model(x)
        finally:
            set_fused_attn(True)
    assert attn_mod.KEY_MASK_CALLS['fwd'] == before['fwd'] + 2
    assert torch.isfinite(y_key.float()).all()
    assert rel_err(y_key, y_float) < 5e-2, rel_err(y_key, y_float)
