"""Fused attention for head dims that are no multiple of 32
(csrc/attention_head_dims.hip) through ops.flash_attention_qkv,
ops.flash_attention and the extension's attention_bwd.

Reference: the fp32 composition on the same bf16-rounded inputs, plain
||a-b||/||b||.  Every comparison has two bounds: the project's own (2e-2 on
O, 4e-2 on gradients, tests/test_ops_gpu.py::test_attention_fwd_bwd) and 1.5x
the error of the existing kernels on the same inputs zero-padded to the next
multiple of 32 with scale = D**-0.5 (computed here, not stored; the 1.5x
covers another fp32 summation order at equal precision).  The two-pass
backward is forced so that the padded D = 64 call uses the same algorithm.

D: 8 no full 32-step, half fragment | 48 tail step | 72 two steps + tail +
half fragment | 80 tail, full fragments | 88 rounds to 96, half fragment |
104 the 128 class with a tail | 120 half fragment in the last position.
"""
import pytest
import torch
import torch.nn.functional as F

import timm_amd  # noqa: F401
from timm_amd import ops
from timm_amd.ops import attention as attn_mod

pytestmark = pytest.mark.gpu

DIMS = [8, 48, 72, 80, 88, 104, 120]
O_TOL, GRAD_TOL, VS_PADDED = 2e-2, 4e-2, 1.5
B, H = 2, 3  # H > 1: a store past column D would land in the next head
SENTINEL = 512.0


@pytest.fixture(autouse=True)
def _two_pass():
    assert ops.has_ext(), 'HIP extension must be built (python setup.py build_ext --inplace)'
    attn_mod.set_attn_bwd_path('two_pass')
    yield
    attn_mod.set_attn_bwd_path(None)


def rel_err(a, b):
    a, b = a.detach().float(), b.detach().float()
    return ((a - b).norm() / b.norm()).item()


def _inputs(seed, *shapes):
    g = torch.Generator(device='cuda').manual_seed(seed)
    return [torch.randn(s, device='cuda', dtype=torch.bfloat16, generator=g) for s in shapes]


def _two_bounds(name, got, padded, ref, tol):
    e, ep = rel_err(got, ref), rel_err(padded, ref)
    print(f'{name}: native={e:.3e} padded={ep:.3e}')
    assert torch.isfinite(got.float()).all(), f'{name}: non-finite'
    assert e < tol, f'{name}: err {e}'
    assert e <= VS_PADDED * ep, f'{name}: err {e} > 1.5 x padded kernels {ep}'


@pytest.mark.parametrize('D', DIMS)
def test_packed_qkv(D):
    """flash_attention_qkv on [2, 65, 3, 3, D]: a full and a one-row q tile, a
    partial last kv tile in every kernel, q/k/v and dq/dk/dv interleaved in
    the packed buffers."""
    N, P = 65, -(-D // 32) * 32
    qkv, do = _inputs(D, (B, N, 3, H, D), (B, N, H, D))
    do = do.permute(0, 2, 1, 3)  # the layout of O
    assert ops.attention_available(qkv[:, :, 0].permute(0, 2, 1, 3))

    x = qkv.clone().requires_grad_(True)
    o = ops.flash_attention_qkv(x)
    before = dict(attn_mod.BWD_PATH_CALLS)
    o.backward(do)
    assert attn_mod.BWD_PATH_CALLS['two_pass'] == before['two_pass'] + 1
    assert attn_mod.BWD_PATH_CALLS['single_pass'] == before['single_pass']

    xp = F.pad(qkv, (0, P - D)).requires_grad_(True)
    op = ops.flash_attention_qkv(xp, scale=D ** -0.5)[..., :D]
    op.backward(do)

    xr = qkv.float().requires_grad_(True)
    qr, kr, vr = xr.permute(2, 0, 3, 1, 4).unbind(0)
    o_ref = ((qr @ kr.transpose(-2, -1)) * D ** -0.5).softmax(-1) @ vr
    o_ref.backward(do.float())

    _two_bounds('o', o, op, o_ref, O_TOL)
    _two_bounds('dqkv', x.grad, xp.grad[..., :D], xr.grad, GRAD_TOL)


@pytest.mark.parametrize('mask_kind', ['bias', 'key_padding'])
@pytest.mark.parametrize('D', DIMS)
def test_cross_attention_masks(D, mask_kind):
    """Separate q, k, v with Nq = 33, Nk = 70 and (a) a trainable finite
    [1,H,Nq,Nk] bias, (b) a [B,1,Nq,Nk] mask with the last 5 keys of sample 1
    at -inf: finite gradients, dk and dv of the masked keys exactly 0."""
    Nq, Nk, P = 33, 70, -(-D // 32) * 32
    q, k, v, do = _inputs(D + 1, (B, H, Nq, D), (B, H, Nk, D), (B, H, Nk, D), (B, H, Nq, D))
    if mask_kind == 'bias':
        mask = torch.randn(1, H, Nq, Nk, device='cuda',
                           generator=torch.Generator(device='cuda').manual_seed(D)) * 2.0
    else:
        mask = torch.zeros(B, 1, Nq, Nk, device='cuda')
        mask[1, :, :, Nk - 5:] = float('-inf')
    assert ops.attention_available(q)

    results = {}
    for kind in ('native', 'padded', 'ref'):
        pad = (0, P - D) if kind == 'padded' else (0, 0)
        cast = torch.Tensor.float if kind == 'ref' else torch.Tensor.clone
        leaves = [cast(F.pad(t, pad)).requires_grad_(True) for t in (q, k, v)]
        m = mask.clone().requires_grad_(mask_kind == 'bias')
        if kind == 'ref':
            o = ((leaves[0] @ leaves[1].transpose(-2, -1)) * D ** -0.5 + m).softmax(-1) @ leaves[2]
        else:
            o = ops.flash_attention(*leaves, attn_mask=m, scale=D ** -0.5)[..., :D]
        before = dict(attn_mod.BWD_PATH_CALLS)
        o.backward(do.to(o.dtype))
        if kind == 'native':
            assert attn_mod.BWD_PATH_CALLS['two_pass'] == before['two_pass'] + 1
            assert attn_mod.BWD_PATH_CALLS['single_pass'] == before['single_pass']
        results[kind] = [o] + [t.grad[..., :D] for t in leaves] + [m.grad]

    names = ('o', 'dq', 'dk', 'dv', 'dbias')[:5 if mask_kind == 'bias' else 4]
    for i, name in enumerate(names):
        _two_bounds(name, results['native'][i], results['padded'][i], results['ref'][i],
                    O_TOL if name == 'o' else GRAD_TOL)
    if mask_kind == 'key_padding':
        for i in (2, 3):
            assert results['native'][i][1, :, Nk - 5:].float().abs().max().item() == 0.0


@pytest.mark.parametrize('D', DIMS)
def test_column_guard(D):
    """The extension's attention_bwd called directly with dq, dk, dv as [..., :D]
    views of sentinel-filled [B, H, N, D + 8] buffers: the 8 columns after D
    stay untouched (in a packed dqkv buffer they are the next head)."""
    ext = ops.require_ext()
    N, P, scale = 65, -(-D // 32) * 32, D ** -0.5
    q, k, v, do = _inputs(D + 2, *([(B, H, N, D)] * 4))
    o, lse = ext.attention_fwd(q, k, v, None, scale)
    do_c, delta = ext.attn_bwd_preprocess(do, o)
    bufs = [torch.full((B, H, N, D + 8), SENTINEL, device='cuda', dtype=torch.bfloat16)
            for _ in range(3)]
    ext.attention_bwd(q, k, v, do_c, lse, delta, None, *[b[..., :D] for b in bufs], scale)
    torch.cuda.synchronize()

    padded = [F.pad(t, (0, P - D)).requires_grad_(True) for t in (q, k, v)]
    ops.flash_attention(*padded, scale=scale)[..., :D].backward(do)
    ref = [t.float().requires_grad_(True) for t in (q, k, v)]
    (((ref[0] @ ref[1].transpose(-2, -1)) * scale).softmax(-1) @ ref[2]).backward(do.float())
    for name, buf, p, r in zip(('dq', 'dk', 'dv'), bufs, padded, ref):
        assert (buf[..., D:] == SENTINEL).all(), f'{name}: wrote past column D'
        _two_bounds(name, buf[..., :D], p.grad[..., :D], r.grad, GRAD_TOL)
