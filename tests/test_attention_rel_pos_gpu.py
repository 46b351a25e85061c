"""Decomposed rel-pos attention kernels (rel_pos_hw=, bf16, head_dim 64)
against an fp32 softmax on the same bf16 inputs."""
import math

import pytest
import torch

from timm_amd import ops
from timm_amd.ops import attention as attn_mod

pytestmark = pytest.mark.gpu

B, H = 2, 2
TOLS = (2e-2,) + (4e-2,) * 5  # o, then dq, dk, dv, d rel_h, d rel_w


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp(min=1e-3)).item()


def _inputs(Nq, Kh, Kw, D=64, B=B, H=H, table_dtype=torch.bfloat16):
    torch.manual_seed(Nq * 10000 + Kh * 100 + Kw)
    bf = dict(device='cuda', dtype=torch.bfloat16)
    q = torch.randn(B, H, Nq, D, **bf)
    k, v = [torch.randn(B, H, Kh * Kw, D, **bf) for _ in range(2)]
    rel_h = torch.randn(B, H, Nq, Kh, device='cuda', dtype=table_dtype)
    rel_w = torch.randn(B, H, Nq, Kw, device='cuda', dtype=table_dtype)
    return (q, k, v, rel_h, rel_w), torch.randn(B, H, Nq, D, **bf)


def _reference(inputs, do):
    q, k, v, rel_h, rel_w = [t.detach().float().requires_grad_(True) for t in inputs]
    bias = (rel_h[..., :, None] + rel_w[..., None, :]).flatten(-2)
    o = torch.softmax(q @ k.transpose(-2, -1) / math.sqrt(q.shape[-1]) + bias, dim=-1) @ v
    o.backward(do.float())
    return o.detach(), q.grad, k.grad, v.grad, rel_h.grad, rel_w.grad


def _run(inputs, do):
    q, k, v, rel_h, rel_w = [t.detach().clone().requires_grad_(True) for t in inputs]
    o = ops.flash_attention(q, k, v, rel_pos_hw=(rel_h, rel_w))
    o.backward(do)
    return o.detach(), q.grad, k.grad, v.grad, rel_h.grad, rel_w.grad


def _check(inputs, do, kernels=True):
    before = dict(attn_mod.REL_POS_CALLS)
    got = _run(inputs, do)
    ran = int(kernels)
    assert attn_mod.REL_POS_CALLS == {'fwd': before['fwd'] + ran, 'bwd': before['bwd'] + ran}
    for g, r, tol, t in zip(got, _reference(inputs, do), TOLS, (inputs[0],) + tuple(inputs)):
        assert g.dtype == t.dtype and g.shape == t.shape
        assert torch.isfinite(g.float()).all()
        assert rel_err(g, r) < tol, rel_err(g, r)
    return got


@pytest.mark.parametrize('Nq,Kh,Kw', [
    (196, 14, 14),  # the SAM window: tiles cut grid rows, 4-key tail
    (65, 5, 13),    # one-row query tail, one-key tail
    (64, 8, 8),     # exact tile, Kw divides 64
    (33, 7, 10),    # Nq != Nk
    (128, 64, 2),   # table-width bound, Kh side
    (192, 3, 64),   # table-width bound, Kw side
    (400, 20, 20),  # seven key tiles
])
def test_rel_pos_numerics(Nq, Kh, Kw):
    inputs, do = _inputs(Nq, Kh, Kw)
    got = _check(inputs, do)
    # bit-reproducible from run to run
    for g, g2 in zip(got, _run(inputs, do)):
        assert torch.equal(g, g2)


def test_rel_pos_fp32_tables():
    _check(*_inputs(65, 5, 13, table_dtype=torch.float32))


def test_rel_pos_packed_qkv_views():
    (_, _, _, rel_h, rel_w), do = _inputs(196, 14, 14)
    qkv = torch.randn(B, 196, 3, H, 64, device='cuda', dtype=torch.bfloat16)
    q, k, v = [qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3)]
    assert not q.is_contiguous()
    _check((q, k, v, rel_h, rel_w), do)


def test_rel_pos_never_builds_the_bias():
    """B = 1, H = 2, 64x64 grid: forward + backward stay below the size of one
    bf16 [H,N,N] bias (64 MiB); everything allocated is O(N (d + Kh + Kw))."""
    N, Kh = 4096, 64
    inputs, do = _inputs(N, Kh, Kh, B=1)
    inputs = [t.requires_grad_(True) for t in inputs]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    o = ops.flash_attention(*inputs[:3], rel_pos_hw=tuple(inputs[3:]))
    o.backward(do)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < H * N * N * 2
    assert all(torch.isfinite(t.grad.float()).all() for t in inputs)
    rows = slice(1000, 1064)
    q, k, v, rel_h, rel_w = [t.detach().float() for t in inputs]
    bias = (rel_h[:, :, rows, :, None] + rel_w[:, :, rows, None, :]).flatten(-2)
    ref = torch.softmax(q[:, :, rows] @ k.transpose(-2, -1) / 8. + bias, dim=-1) @ v
    assert rel_err(o[:, :, rows], ref) < 2e-2


def test_rel_pos_other_head_dim_takes_mask_path():
    _check(*_inputs(70, 7, 10, D=80), kernels=False)


def test_samvit_rel_pos_matches_unfused():
    """One windowed and one global block run the rel-pos kernels; logits match
    the materialised bias through torch SDPA (the NaFlex model test's bound)."""
    from timm_amd.layers import set_fused_attn
    from timm_amd.models.vision_transformer_sam import VisionTransformerSAM
    torch.manual_seed(0)
    model = VisionTransformerSAM(
        img_size=96, patch_size=8, embed_dim=128, depth=2, num_heads=2, num_classes=10,
        use_rel_pos=True, window_size=4, global_attn_indexes=(1,), neck_chans=0)
    for name, p in model.named_parameters():
        if 'rel_pos' in name:  # zero-initialised: give the bias something to do
            torch.nn.init.normal_(p, std=0.5)
    model = model.eval().to('cuda', torch.bfloat16)
    x = torch.randn(2, 3, 96, 96, device='cuda', dtype=torch.bfloat16)
    before = dict(attn_mod.REL_POS_CALLS)
    with torch.no_grad():
        y_fused = model(x)
        assert attn_mod.REL_POS_CALLS['fwd'] == before['fwd'] + 2
        set_fused_attn(False)
        try:
            y_ref = model(x)
        finally:
            set_fused_attn(True)
    assert attn_mod.REL_POS_CALLS['fwd'] == before['fwd'] + 2
    assert torch.isfinite(y_fused.float()).all()
    assert rel_err(y_fused, y_ref) < 5e-2, rel_err(y_fused, y_ref)
