"""CPU tests for the fused q/k rotary-embedding op and its model wiring.

On CPU `ops.apply_rope_qk` must be bit-identical to the eager composition the
attention modules used before (prefix cat + apply_rot_embed_cat + cast); the
GPU kernel is covered in test_rope_gpu.py.
"""
import pytest
import torch

import timm_amd
from timm_amd import ops
from timm_amd.layers import apply_rot_embed_cat, set_fused_rope, use_fused_rope

B, H, D, NP = 2, 3, 16, 7


def _eager(q, k, rope, npt, half, out_dtype):
    q = torch.cat([q[:, :, :npt, :], apply_rot_embed_cat(q[:, :, npt:, :], rope, half=half)], 2).to(out_dtype)
    k = torch.cat([k[:, :, :npt, :], apply_rot_embed_cat(k[:, :, npt:, :], rope, half=half)], 2).to(out_dtype)
    return q, k


def _table(form, dtype=torch.float32):
    shape = {'np': (NP, 2 * D), 'hnp': (H, NP, 2 * D), 'b1np': (B, 1, NP, 2 * D)}[form]
    return torch.randn(shape, dtype=dtype)


@pytest.fixture
def fused_rope_switch():
    yield
    set_fused_rope(None)


@pytest.mark.parametrize('npt', [0, 1, 5])
@pytest.mark.parametrize('half', [False, True])
@pytest.mark.parametrize('form', ['np', 'hnp', 'b1np'])
def test_apply_rope_qk_cpu_matches_eager(npt, half, form):
    torch.manual_seed(0)
    q = torch.randn(B, H, npt + NP, D)
    k = torch.randn(B, H, npt + NP, D)
    rope = _table(form)
    q_rot, k_rot = ops.apply_rope_qk(q, k, rope, num_prefix_tokens=npt, half=half)
    q_ref, k_ref = _eager(q, k, rope, npt, half, q.dtype)
    assert q_rot.shape == q.shape and q_rot.dtype == q.dtype
    assert torch.equal(q_rot, q_ref)
    assert torch.equal(k_rot, k_ref)
    assert torch.equal(q_rot[:, :, :npt], q[:, :, :npt])


def test_apply_rope_qk_cpu_out_dtype():
    torch.manual_seed(1)
    q = torch.randn(B, H, 1 + NP, D)
    k = torch.randn(B, H, 1 + NP, D)
    rope = _table('np')
    q_rot, k_rot = ops.apply_rope_qk(q, k, rope, num_prefix_tokens=1, out_dtype=torch.bfloat16)
    q_ref, k_ref = _eager(q, k, rope, 1, False, torch.bfloat16)
    assert q_rot.dtype == torch.bfloat16
    assert torch.equal(q_rot, q_ref) and torch.equal(k_rot, k_ref)


@pytest.mark.parametrize('half', [False, True])
def test_apply_rope_qk_grad_reaches_table(half):
    torch.manual_seed(2)
    q = torch.randn(B, H, 1 + NP, D, requires_grad=True)
    k = torch.randn(B, H, 1 + NP, D, requires_grad=True)
    rope = _table('hnp').requires_grad_(True)
    q_rot, k_rot = ops.apply_rope_qk(q, k, rope, num_prefix_tokens=1, half=half)
    (q_rot.sum() + (k_rot * 2).sum()).backward()
    assert rope.grad is not None and rope.grad.abs().sum() > 0
    assert q.grad is not None and k.grad is not None


def test_rope_available_false_cases():
    q = torch.randn(B, H, NP, D)
    k = torch.randn(B, H, NP, D)
    rope = _table('np')
    # CPU tensors never take the kernel
    assert not ops.rope_available(q, k, rope, False)
    assert not ops.rope_available(q, k, rope, True)
    # learned table
    assert not ops.rope_available(q, k, rope.clone().requires_grad_(True), False)
    # unsupported head dims (12: neither layout; 24: interleaved only)
    q12 = torch.randn(B, H, NP, 12)
    assert not ops.rope_available(q12, q12, torch.randn(NP, 24), False)
    q24 = torch.randn(B, H, NP, 24)
    assert not ops.rope_available(q24, q24, torch.randn(NP, 48), True)


def test_fused_rope_switch(fused_rope_switch, monkeypatch):
    monkeypatch.delenv('TIMM_AMD_FUSED_ROPE', raising=False)
    assert use_fused_rope()
    monkeypatch.setenv('TIMM_AMD_FUSED_ROPE', '0')
    assert not use_fused_rope()  # read at call time
    set_fused_rope(True)
    assert use_fused_rope()
    set_fused_rope(False)
    monkeypatch.setenv('TIMM_AMD_FUSED_ROPE', '1')
    assert not use_fused_rope()
    set_fused_rope(None)
    assert use_fused_rope()


def test_eva02_patch_dropout_train_step():
    """Patch dropout gathers a per-sample rope table; it must reach the blocks
    as [B, 1, N, 2D] so it broadcasts over heads."""
    torch.manual_seed(3)
    model = timm_amd.create_model('eva02_tiny_patch14_224', num_classes=10, patch_drop_rate=0.5)
    model.train()
    x = torch.randn(2, 3, 224, 224)
    y = model(x)
    assert y.shape == (2, 10)
    y.sum().backward()
    grads = [p.grad for p in model.parameters() if p.requires_grad]
    assert any(g is not None for g in grads)
    assert all(torch.isfinite(g).all() for g in grads if g is not None)


def test_eva02_switch_on_off_equal(fused_rope_switch):
    torch.manual_seed(4)
    model = timm_amd.create_model('eva02_tiny_patch14_224', num_classes=10).eval()
    x = torch.randn(1, 3, 224, 224)
    calls = []
    orig = ops.apply_rope_qk

    def counting(*args, **kwargs):
        calls.append(1)
        return orig(*args, **kwargs)

    with torch.no_grad():
        set_fused_rope(False)
        y_off = model(x)
        set_fused_rope(True)
        ops.apply_rope_qk = counting
        try:
            y_on = model(x)
        finally:
            ops.apply_rope_qk = orig
    assert len(calls) == len(model.blocks)
    assert torch.equal(y_on, y_off)
