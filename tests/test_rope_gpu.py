"""GPU tests for the fused q/k rotary-embedding kernel (csrc/rope.hip).

Reference everywhere: the eager composition (prefix cat + apply_rot_embed_cat)
in fp32 on the same inputs upcast, forward and backward through autograd with
a random dy.  Tables are random rather than real sin/cos, so an index mix-up
inside a pair (s[2i] vs s[2i+1]) changes the result.

Run on the MI355X box: pytest tests/test_rope_gpu.py -m gpu -x -q
"""
import itertools

import pytest
import torch

import timm_amd
from timm_amd import ops
from timm_amd.layers import apply_rot_embed_cat, set_fused_rope
from timm_amd.models.eva import EvaAttention

pytestmark = pytest.mark.gpu

# bf16 output = one round-to-nearest of an fp32 result: <= 2^-9 per element, 2x margin
TOL_BF16 = 2 ** -8
# the project's fp32 bound (test_ops_gpu.py)
TOL_FP32 = 2e-5

BF16, FP32 = torch.bfloat16, torch.float32
DTYPE_COMBOS = [(BF16, BF16), (FP32, FP32), (FP32, BF16)]
FORMS = ['np', 'hnp', 'b1np']


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp(min=1e-3)).item()


def _tol(dtype):
    return TOL_BF16 if dtype == BF16 else TOL_FP32


def _eager_fp32(q, k, rope, npt, half):
    rope = rope.float()
    q = torch.cat([q[:, :, :npt, :], apply_rot_embed_cat(q[:, :, npt:, :], rope, half=half)], 2)
    k = torch.cat([k[:, :, :npt, :], apply_rot_embed_cat(k[:, :, npt:, :], rope, half=half)], 2)
    return q, k


def _table(form, B, H, Np, D, dtype):
    shape = {'np': (Np, 2 * D), 'hnp': (H, Np, 2 * D), 'b1np': (B, 1, Np, 2 * D)}[form]
    return torch.randn(shape, device='cuda', dtype=dtype)


def _check_case(B, H, N, npt, D, half, form, tab_dtype, packed, in_dtype, out_dtype):
    tag = f'B{B} H{H} N{N} npt{npt} D{D} half={half} {form} tab={tab_dtype} packed={packed} ' \
          f'{in_dtype}->{out_dtype}'
    rope = _table(form, B, H, N - npt, D, tab_dtype)
    if packed:
        # q/k as permuted views of the packed [B, N, 3, H, D] projection
        src = torch.randn(B, N, 3, H, D, device='cuda', dtype=in_dtype).requires_grad_(True)
        ref = src.detach().float().requires_grad_(True)
        q, k = (src[:, :, i].permute(0, 2, 1, 3) for i in (0, 1))
        q_ref, k_ref = (ref[:, :, i].permute(0, 2, 1, 3) for i in (0, 1))
        leaves, ref_leaves = (src,), (ref,)
    else:
        q = torch.randn(B, H, N, D, device='cuda', dtype=in_dtype).requires_grad_(True)
        k = torch.randn(B, H, N, D, device='cuda', dtype=in_dtype).requires_grad_(True)
        q_ref = q.detach().float().requires_grad_(True)
        k_ref = k.detach().float().requires_grad_(True)
        leaves, ref_leaves = (q, k), (q_ref, k_ref)

    assert ops.rope_available(q, k, rope, half, out_dtype), tag
    q_rot, k_rot = ops.apply_rope_qk(q, k, rope, num_prefix_tokens=npt, half=half, out_dtype=out_dtype)
    y_q, y_k = _eager_fp32(q_ref, k_ref, rope, npt, half)

    assert q_rot.dtype == out_dtype and q_rot.shape == (B, H, N, D), tag
    # [B, N, H, D] storage behind the [B, H, N, D] view
    assert q_rot.transpose(1, 2).is_contiguous() and k_rot.transpose(1, 2).is_contiguous(), tag
    tol = _tol(out_dtype)
    for got, want, name in ((q_rot, y_q, 'q'), (k_rot, y_k, 'k')):
        err = rel_err(got, want)
        assert err < tol, f'{tag}: fwd {name} err {err}'
    assert torch.equal(q_rot[:, :, :npt], q[:, :, :npt].to(out_dtype)), tag
    assert torch.equal(k_rot[:, :, :npt], k[:, :, :npt].to(out_dtype)), tag

    dq = torch.randn(B, H, N, D, device='cuda', dtype=out_dtype)
    dk = torch.randn(B, H, N, D, device='cuda', dtype=out_dtype)
    grads = torch.autograd.grad((q_rot, k_rot), leaves, (dq, dk))
    ref_grads = torch.autograd.grad((y_q, y_k), ref_leaves, (dq.float(), dk.float()))
    tol = _tol(in_dtype)
    for g, g_ref in zip(grads, ref_grads):
        assert g.dtype == in_dtype, tag
        err = rel_err(g, g_ref)
        assert err < tol, f'{tag}: bwd err {err}'
    if packed:
        assert torch.equal(grads[0][:, :, 2], torch.zeros_like(grads[0][:, :, 2])), tag
        assert torch.equal(grads[0][:, :npt, 0], dq[:, :, :npt].transpose(1, 2).to(in_dtype)), tag
    else:
        assert torch.equal(grads[0][:, :, :npt], dq[:, :, :npt].to(in_dtype)), tag
        assert torch.equal(grads[1][:, :, :npt], dk[:, :, :npt].to(in_dtype)), tag


@pytest.mark.parametrize('D,half', [
    (32, False), (32, True), (64, False), (64, True), (128, False), (128, True), (88, False)])
def test_rope_kernel_vs_eager(D, half):
    assert ops.has_ext()
    torch.manual_seed(D + int(half))
    B, H = 2, 3
    for npt, form, tab_dtype, packed, (in_dtype, out_dtype) in itertools.product(
            (0, 1, 5), FORMS, (FP32, BF16), (True, False), DTYPE_COMBOS):
        _check_case(B, H, npt + 9, npt, D, half, form, tab_dtype, packed, in_dtype, out_dtype)


def test_rope_half_unavailable_for_d88():
    q = torch.randn(2, 3, 9, 88, device='cuda', dtype=BF16)
    rope = torch.randn(9, 176, device='cuda')
    assert ops.rope_available(q, q, rope, half=False)
    assert not ops.rope_available(q, q, rope, half=True)


def test_rope_kernel_grid_stride():
    """~534k 16-byte chunks per tensor against the 2048 x 256-thread capped grid."""
    torch.manual_seed(7)
    _check_case(16, 16, 261, 1, 64, False, 'np', FP32, True, BF16, BF16)
    _check_case(32, 16, 261, 1, 64, True, 'b1np', FP32, False, BF16, BF16)  # half: 2 chunks per item


def test_rope_ext_rejects_bad_inputs():
    """Host-side checks fire before any launch."""
    ext = ops.require_ext()
    q = torch.randn(2, 3, 10, 32, device='cuda', dtype=BF16)
    rope = torch.randn(1, 1, 9, 64, device='cuda')
    wide = torch.randn(2, 3, 10, 64, device='cuda', dtype=BF16)
    ext.rope_qk(q, q, rope, 1, False, False, BF16)  # valid baseline
    bad = [
        (q, q, rope[:, :, :8], 1, False),                                  # table rows != N - npt
        (q, q, rope, 11, False),                                           # npt > N
        (q, q, rope, -1, False),                                           # npt < 0
        (q, q, torch.randn(1, 1, 9, 32, device='cuda'), 1, False),         # last dim != 2D
        (q, q, torch.randn(3, 1, 9, 64, device='cuda'), 1, False),         # batch dim not 1|B
        (q, q, torch.randn(1, 2, 9, 64, device='cuda'), 1, False),         # head dim not 1|H
        (q, q[:, :, :, :16], rope, 1, False),                              # q/k shape mismatch
        (q, q, rope[0, 0], 1, False),                                      # rope not 4-D
        (wide[..., ::2], wide[..., ::2], rope, 1, False),                  # strided last dim
        (q[..., 4:28], q[..., 4:28], torch.randn(1, 1, 9, 48, device='cuda'), 1, False),  # misaligned base
        (q[..., :24], q[..., :24], torch.randn(1, 1, 9, 48, device='cuda'), 1, True),     # D % 16 for half
    ]
    for qq, kk, rr, npt, half in bad:
        with pytest.raises(RuntimeError):
            ext.rope_qk(qq, kk, rr, npt, half, False, BF16)
    with pytest.raises(RuntimeError):  # bf16 -> fp32 is a backward-only combination
        ext.rope_qk(q, q, rope, 1, False, False, FP32)
    with pytest.raises(RuntimeError):
        ext.rope_qk(q.half(), q.half(), rope, 1, False, False, torch.float16)


def test_rope_zero_size():
    q = torch.randn(0, 3, 10, 32, device='cuda', dtype=BF16)
    rope = torch.randn(9, 64, device='cuda')
    q_rot, k_rot = ops.apply_rope_qk(q, q, rope, num_prefix_tokens=1)
    assert q_rot.shape == q.shape and k_rot.shape == q.shape


@pytest.fixture
def fused_rope_switch():
    yield
    set_fused_rope(None)


def test_eva_attention_module_fused_vs_eager(fused_rope_switch):
    """EvaAttention bf16 on GPU vs the same module in fp32 on CPU, fused rope on and off."""
    torch.manual_seed(5)
    B, N, dim, heads = 2, 17, 128, 2
    attn = EvaAttention(dim=dim, num_heads=heads, num_prefix_tokens=1).eval()
    with torch.no_grad():
        attn.q_bias.normal_(std=0.1)
        attn.v_bias.normal_(std=0.1)
    x = torch.randn(B, N, dim)
    rope = torch.randn(N - 1, 2 * (dim // heads))
    dy = torch.randn(B, N, dim)

    set_fused_rope(False)
    x_ref = x.clone().requires_grad_(True)
    y_ref = attn(x_ref, rope=rope)
    y_ref.backward(dy)

    attn_gpu = EvaAttention(dim=dim, num_heads=heads, num_prefix_tokens=1).eval()
    attn_gpu.load_state_dict(attn.state_dict())
    attn_gpu = attn_gpu.to('cuda', BF16)
    errs = {}
    for fused in (False, True):
        set_fused_rope(fused)
        xg = x.to('cuda', BF16).requires_grad_(True)
        yg = attn_gpu(xg, rope=rope.cuda())
        yg.backward(dy.to('cuda', BF16))
        errs[fused] = (rel_err(yg.cpu(), y_ref), rel_err(xg.grad.cpu(), x_ref.grad))
    print(f'EvaAttention bf16 vs fp32 CPU (out, dx): eager {errs[False]}, fused {errs[True]}')
    for e_fused, e_eager in zip(errs[True], errs[False]):
        assert e_fused < 2e-2
        assert e_fused <= 1.5 * e_eager + 1e-3


def _record_rope_calls(record):
    orig = ops.apply_rope_qk

    def wrapped(q, k, rope, num_prefix_tokens=0, half=False, out_dtype=None):
        record.append(ops.rope_available(q, k, rope, half, out_dtype))
        return orig(q, k, rope, num_prefix_tokens=num_prefix_tokens, half=half, out_dtype=out_dtype)

    ops.apply_rope_qk = wrapped
    return orig


def test_dispatch_eva02_tiny_uses_kernel():
    torch.manual_seed(6)
    model = timm_amd.create_model('eva02_tiny_patch14_224', num_classes=10).eval().to('cuda', BF16)
    x = torch.randn(1, 3, 224, 224, device='cuda', dtype=BF16)
    record = []
    orig = _record_rope_calls(record)
    try:
        with torch.no_grad():
            y = model(x)
    finally:
        ops.apply_rope_qk = orig
    assert torch.isfinite(y.float()).all()
    assert len(record) == 12 and all(record)


def test_dispatch_mixed_rope_keeps_table_grads():
    torch.manual_seed(8)
    model = timm_amd.create_model('vit_small_patch16_rope_mixed_224', num_classes=10).train().cuda()
    x = torch.randn(1, 3, 224, 224, device='cuda')
    record = []
    orig = _record_rope_calls(record)
    try:
        model(x).float().sum().backward()
    finally:
        ops.apply_rope_qk = orig
    assert len(record) == len(model.blocks) and not any(record)
    assert model.rope.freqs.grad is not None
    assert torch.isfinite(model.rope.freqs.grad.float()).all()
