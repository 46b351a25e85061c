"""Cross-covariance attention kernels (csrc/xca_attention.hip) against the
plain fp32 composition on the same bf16-rounded qkv, and against the
switched-off path (the bf16 composition of XCA.forward; it holds its
temperature in bf16 as the module's parameter does).

Bounds: the project's absolute ones (2e-2 on O, 4e-2 on dq / dk / dv, 5e-2 on
d temperature, metric |a-b|/|b|) and, except for d temperature (`heads`
strongly cancelling sums, see profiles/window_cos_attention/README.md), 1.5x
the switched-off path's error on the same inputs."""
import math

import pytest
import torch

from timm_amd import ops
from timm_amd.layers import set_fused_xca
from timm_amd.ops.xca_attention import XCA_ATTN_CALLS, _math_xca

pytestmark = pytest.mark.gpu

O_TOL, DQKV_TOL, DTEMP_TOL, REL_MARGIN = 2e-2, 4e-2, 5e-2, 1.5

# (B, N, heads, head_dim)
CASES = [
    (2, 196, 2, 48),   # XCiT's own N, token tail, half MFMA step at d 48
    (1, 17, 1, 32),    # fewer tokens than one tile, one workgroup
    (2, 64, 3, 64),    # exact tiles, 3 heads (head stride in the packed buffer), d 64
    (1, 577, 2, 64),   # many tiles plus a one-token tail
    (1, 784, 1, 32),   # p8 length, d 32
    (3, 40, 2, 32),    # B > 1: the d temperature partials are summed over B
]


def rel_err(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def make_inputs(case, seed=0, dtype=torch.bfloat16):
    B, N, H, d = case
    dim = H * d
    g = torch.Generator(device='cuda').manual_seed(seed)
    torch.manual_seed(seed)  # the Linear's init: same inputs on every run
    lin = torch.nn.Linear(dim, 3 * dim).to('cuda', dtype)

    def randn(*shape):
        return torch.randn(*shape, device='cuda', generator=g)
    x = (randn(B, N, 8) @ randn(8, dim) / math.sqrt(8) + 0.5 * randn(B, N, dim)).to(dtype)
    temperature = 2 + 8 * torch.rand(H, device='cuda', generator=g)
    do = randn(B, N, dim).to(dtype)
    return lin(x).detach(), temperature, do


def arm(fn, qkv0, temp0, do, dtype, temp_dtype=torch.float32):
    qkv = qkv0.clone().to(dtype).requires_grad_(True)
    temp = temp0.clone().to(temp_dtype).requires_grad_(True)
    o = fn(qkv, temp)
    o.backward(do.to(o.dtype))
    return o.detach(), qkv.grad, temp.grad


def reference(qkv0, temp0, do, H):
    return arm(lambda qkv, t: _math_xca(qkv, H, t), qkv0, temp0, do, torch.float32)


def switched_off(qkv0, temp0, do, H, dtype=torch.bfloat16):
    set_fused_xca(False)
    try:
        return arm(lambda qkv, t: ops.cross_covariance_attention(qkv, H, t.view(H, 1, 1)),
                   qkv0, temp0, do, dtype, temp_dtype=dtype)
    finally:
        set_fused_xca(None)


def check(name, new, old, ref, tol, relative=True):
    assert new.shape == ref.shape and torch.isfinite(new).all(), name
    e_new, e_old = rel_err(new, ref), rel_err(old, ref)
    print(f'{name}: new {e_new:.3e} old {e_old:.3e}')
    assert e_new <= tol, (name, e_new)
    if relative:
        assert e_new <= REL_MARGIN * e_old, (name, e_new, e_old)


@pytest.mark.parametrize('case', CASES, ids=[str(i + 1) for i in range(len(CASES))])
def test_fwd_bwd(case):
    H, dim = case[2], case[2] * case[3]
    qkv0, temp0, do = make_inputs(case)
    ref = reference(qkv0, temp0, do, H)
    old = switched_off(qkv0, temp0, do, H)
    calls = dict(XCA_ATTN_CALLS)
    new = arm(lambda qkv, t: ops.cross_covariance_attention(qkv, H, t), qkv0, temp0, do, torch.bfloat16)
    assert XCA_ATTN_CALLS == {'fwd': calls['fwd'] + 1, 'bwd': calls['bwd'] + 1}
    again = arm(lambda qkv, t: ops.cross_covariance_attention(qkv, H, t), qkv0, temp0, do, torch.bfloat16)
    assert torch.equal(new[1], again[1]) and torch.equal(new[2], again[2])

    check('o', new[0], old[0], ref[0], O_TOL)
    # qkv channel order is (3, heads, d): dq, dk, dv separately
    for i, name in enumerate(('dq', 'dk', 'dv')):
        sl = slice(i * dim, (i + 1) * dim)
        check(name, new[1][..., sl], old[1][..., sl], ref[1][..., sl], DQKV_TOL)
    check('dtemp', new[2], old[2], ref[2], DTEMP_TOL, relative=False)


@pytest.mark.parametrize('what', ['fp16', 'head_dim_40', 'non_contiguous', 'switch_off', 'zero_channel'])
def test_dispatch(what):
    case = (2, 40, 2, 40) if what == 'head_dim_40' else (2, 40, 2, 32)
    H, dim = case[2], case[2] * case[3]
    dtype = torch.float16 if what == 'fp16' else torch.bfloat16
    qkv0, temp0, do = make_inputs(case, dtype=dtype)
    if what == 'zero_channel':
        qkv0[0, :, 5] = 0  # channel 5 of q, head 0, batch 0: norm 0, F.normalize gives 0
    ref = reference(qkv0, temp0, do, H)
    calls = dict(XCA_ATTN_CALLS)
    if what == 'switch_off':
        o = switched_off(qkv0, temp0, do, H)[0]
    elif what == 'non_contiguous':
        wide = torch.zeros(case[0], case[1], 3 * dim + 8, device='cuda', dtype=dtype)
        wide[..., :3 * dim] = qkv0
        o = ops.cross_covariance_attention(wide[..., :3 * dim], H, temp0.to(dtype))
    else:
        o = ops.cross_covariance_attention(qkv0, H, temp0 if what == 'zero_channel' else temp0.to(dtype))
    kernel = 1 if what == 'zero_channel' else 0
    assert XCA_ATTN_CALLS == {'fwd': calls['fwd'] + kernel, 'bwd': calls['bwd']}
    assert torch.isfinite(o).all()
    assert rel_err(o, ref[0]) <= O_TOL

