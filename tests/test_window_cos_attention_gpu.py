"""Cosine windowed-attention kernels (csrc/window_cos_attention.hip) against a
plain fp32 composition on the same bf16-rounded qkv, and against the existing
path (bf16 normalize, logit scale folded into q, ops.flash_attention with the
[nW, heads, N, N] bias + mask).

Bounds: the project's absolute ones (2e-2 on O, 4e-2 on dq/dk/dv, 5e-2 on
dbias and d logit_scale, metric |a-b|/|b|) and, except for d logit_scale
(`heads` numbers), 1.5x the existing path's error on the same inputs."""
import pytest
import torch
import torch.nn.functional as F

import timm_amd
from timm_amd import ops
from timm_amd.ops.window_attention import WINDOW_ATTN_CALLS, WINDOW_COS_ATTN_CALLS

pytestmark = pytest.mark.gpu

O_TOL, DQKV_TOL, DBIAS_TOL, DSCALE_TOL, REL_MARGIN = 2e-2, 4e-2, 5e-2, 5e-2, 1.5

# (B, Hf, Wf, heads, window, shift)
CASES = [
    (2, 6, 6, 2, 6, 0),                 # N = 36: partial key tile, fewer row blocks than waves
    (1, 12, 12, 1, 12, 0),              # N = 144: 9 row blocks over 4 waves
    (1, 24, 24, 2, 12, 6),              # four shifted windows, every mask region, wrap-around
    (1, 32, 32, 1, 16, 8),              # N = 256, the maximum, shifted
    (2, 16, 8, 3, 8, 4),                # N = 64, 3 heads, non-square map
    (1, 12, 24, 2, (6, 12), (3, 0)),    # non-square window, N = 72, shift in one dim
    (3, 16, 24, 2, 8, 4),               # 18 windows in 4 dBias chunks of 5, 5, 5, 3
]


def rel_err(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def composed(qkv, bias, ls, heads, ws, ss, attend):
    """roll -> partition -> attend(q, k, v, bias + mask, ls) -> reverse -> roll"""
    B, Hf, Wf, C3 = qkv.shape
    D = C3 // (3 * heads)
    N = ws[0] * ws[1]
    x = torch.roll(qkv, (-ss[0], -ss[1]), (1, 2))
    x = x.view(B, Hf // ws[0], ws[0], Wf // ws[1], ws[1], 3, heads, D)
    q, k, v = x.permute(5, 0, 1, 3, 6, 2, 4, 7).reshape(3, -1, heads, N, D).unbind(0)

    def region(size, win, shift):
        c = torch.arange(size, device=qkv.device)
        return ((c >= size - win).long() + (c >= size - shift).long()) * (shift > 0)
    lab = 3 * region(Hf, ws[0], ss[0])[:, None] + region(Wf, ws[1], ss[1])[None, :]
    lab = lab.view(Hf // ws[0], ws[0], Wf // ws[1], ws[1]).permute(0, 2, 1, 3).reshape(-1, N)
    mask = (lab[:, :, None] != lab[:, None, :]).float() * -100.0   # [nW, N, N]
    o = attend(q, k, v, bias[None] + mask[:, None], ls)             # [B*nW, heads, N, D]
    o = o.view(B, Hf // ws[0], Wf // ws[1], heads, ws[0], ws[1], D)
    o = o.permute(0, 1, 4, 2, 5, 3, 6).reshape(B, Hf, Wf, heads * D)
    return torch.roll(o, ss, (1, 2))


def fp32_attend(q, k, v, bias_mask, ls):
    nW = bias_mask.shape[0]
    s = (F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-2, -1)) * ls.view(1, -1, 1, 1)
    s = (s.view(-1, nW, *s.shape[1:]) + bias_mask).flatten(0, 1)
    return s.softmax(-1) @ v


def flash_attend(q, k, v, bias_mask, ls):
    q = F.normalize(q, dim=-1) * ls.view(1, -1, 1, 1).to(q.dtype)
    return ops.flash_attention(q, F.normalize(k, dim=-1), v, attn_mask=bias_mask, scale=1.0)


def run_case(case, train_bias=True, seed=0, zero_rows=False, backward=True):
    B, Hf, Wf, heads, window, shift = case
    ws = window if isinstance(window, tuple) else (window, window)
    ss = shift if isinstance(shift, tuple) else (shift, shift)
    N, dim = ws[0] * ws[1], heads * 32
    g = torch.Generator(device='cuda').manual_seed(seed)
    torch.manual_seed(seed)  # the Linear's init: same inputs on every run
    lin =torch.nn.Linear(dim, 3 * dim).to('cuda', torch.bfloat16)
    x = torch.randn(B, Hf, Wf, dim, device='cuda', generator=g).bfloat16()
    do = torch.randn(B, Hf, Wf, dim, device='cuda', generator=g).bfloat16()
    bias0 = 16 * torch.sigmoid(torch.randn(heads, N, N, device='cuda', generator=g))
    ls0 = 5 + 15 * torch.rand(heads, device='cuda', generator=g)
    qkv0 = lin(x).detach()
    if zero_rows:  # q and k of a few map positions: norm 0, F.normalize gives 0
        qkv0[0, (0, 5, Hf - 1), (0, 7, Wf - 1), :2 * dim] = 0

    def arm(fn, dtype):
        qkv = qkv0.clone().to(dtype).requires_grad_(True)
        bias = bias0.clone().requires_grad_(train_bias)
        ls = ls0.clone().requires_grad_(True)
        o = fn(qkv, bias, ls)
        if backward:
            o.backward(do.to(o.dtype))
        return o.detach(), qkv.grad, bias.grad, ls.grad

    ref = arm(lambda qkv, b, ls: composed(qkv, b, ls, heads, ws, ss, fp32_attend), torch.float32)
    old = arm(lambda qkv, b, ls: composed(qkv, b, ls, heads, ws, ss, flash_attend), torch.bfloat16)
    calls = dict(WINDOW_COS_ATTN_CALLS)
    new = arm(lambda qkv, b, ls: ops.window_attention(qkv, heads, ws, ss, bias=b, logit_scale=ls),
              torch.bfloat16)
    n_bwd = 1 if backward else 0
    assert WINDOW_COS_ATTN_CALLS == {'fwd': calls['fwd'] + 1, 'bwd': calls['bwd'] + n_bwd}
    return ref, old, new


def check(name, new, old, ref, tol, relative=True):
    assert torch.isfinite(new).all(), name
    e_new, e_old = rel_err(new, ref), rel_err(old, ref)
    print(f'{name}: new {e_new:.3e} old {e_old:.3e}')
    assert e_new <= tol, (name, e_new)
    if relative:
        assert e_new <= REL_MARGIN * e_old, (name, e_new, e_old)


def check_o_dqkv_dscale(case, ref, old, new):
    assert new[0].shape == ref[0].shape and new[1].shape == ref[1].shape
    check('o', new[0], old[0], ref[0], O_TOL)
    heads = case[3]
    # qkv channel order is (3, heads, D): dq, dk, dv separately
    for i, name in enumerate(('dq', 'dk', 'dv')):
        sl = slice(i * heads * 32, (i + 1) * heads * 32)
        check(name, new[1][..., sl], old[1][..., sl], ref[1][..., sl], DQKV_TOL)
    check('dscale', new[3], old[3], ref[3], DSCALE_TOL, relative=False)


@pytest.mark.parametrize('case', CASES, ids=[str(i + 1) for i in range(len(CASES))])
def test_fwd_bwd(case):
    ref, old, new = run_case(case)
    check_o_dqkv_dscale(case, ref, old, new)
    check('dbias', new[2], old[2], ref[2], DBIAS_TOL)


def test_frozen_bias():
    ref, old, new = run_case(CASES[2], train_bias=False)
    assert new[2] is None
    check_o_dqkv_dscale(CASES[2], ref, old, new)


def test_zero_norm_rows():
    ref, old, new = run_case(CASES[2], zero_rows=True, backward=False)
    assert torch.isfinite(new[0]).all()
    assert rel_err(new[0], ref[0]) <= O_TOL


def test_backward_is_bit_reproducible():
    B, Hf, Wf, heads, window, shift = CASES[6]
    torch.manual_seed(1)
    lin = torch.nn.Linear(heads * 32, 3 * heads * 32).to('cuda', torch.bfloat16)
    qkv = lin(torch.randn(B, Hf, Wf, heads * 32, device='cuda').bfloat16())
    bias = torch.randn(heads, window * window, window * window, device='cuda', requires_grad=True)
    ls = (5 + 15 * torch.rand(heads, device='cuda')).requires_grad_(True)
    o = ops.window_attention(qkv, heads, window, shift, bias=bias, logit_scale=ls)
    do = torch.randn_like(o)
    first = torch.autograd.grad(o, (qkv, bias, ls), do, retain_graph=True)
    second = torch.autograd.grad(o, (qkv, bias, ls), do, retain_graph=True)
    assert all(torch.equal(a, b) for a, b in zip(first, second))


@pytest.mark.parametrize('img,window,fused', [(64, 8, True), (192, 24, False)])
def test_swinv2_dispatch(img, window, fused):
    torch.manual_seed(2)
    m = timm_amd.create_model(
        'swinv2_tiny_window8_256', num_classes=10, img_size=img, window_size=window,
        embed_dim=64, depths=(2, 2), num_heads=(2, 4)).to('cuda', torch.bfloat16).train()
    calls, v1_calls = dict(WINDOW_COS_ATTN_CALLS), dict(WINDOW_ATTN_CALLS)
    y = m(torch.randn(2, 3, img, img, device='cuda', dtype=torch.bfloat16))
    y.float().sum().backward()
    assert torch.isfinite(y).all()
    n = 4 if fused else 0
    assert WINDOW_COS_ATTN_CALLS == {'fwd': calls['fwd'] + n, 'bwd': calls['bwd'] + n}
    assert WINDOW_ATTN_CALLS == v1_calls
    attn = m.layers[0].blocks[1].attn
    for p in (attn.cpb_mlp[0].weight, attn.logit_scale):
        assert p.grad is not None and torch.isfinite(p.grad).all()
