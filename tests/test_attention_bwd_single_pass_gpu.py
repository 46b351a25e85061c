"""Single-pass fused attention backward (Nk <= 256, head_dim 64).

Reference: the fp32 composition on the same bf16-rounded inputs, plain
||a-b||/||b||.  Every case has two bounds on dq, dk, dv: the project's 4e-2,
and 1.5x the error of the forced two-pass kernels on the same inputs (computed
here, not stored; it is the bf16 rounding of P and dS, 2.3e-3 .. 2.9e-3 in
profiles/attn_dbias/README.md - the 1.5x covers another fp32 summation order,
not another precision).  Where the reference gradient is analytically zero
(one key: softmax is constant) the RMS must stay under 0.05 instead.
"""
import math

import pytest
import torch

import timm_amd  # noqa: F401
from timm_amd import ops
from timm_amd.ops import attention as attn_mod

pytestmark = pytest.mark.gpu

GRAD_TOL = 4e-2      # tests/test_ops_gpu.py::test_attention_fwd_bwd
VS_TWO_PASS = 1.5
ZERO_RMS = 0.05


@pytest.fixture(autouse=True)
def _restore_path():
    assert ops.has_ext(), 'HIP extension must be built (python setup.py build_ext --inplace)'
    yield
    attn_mod.set_attn_bwd_path(None)


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm()).item()


def _rms(a):
    return a.float().pow(2).mean().sqrt().item()


def _inputs(B, H, Nq, Nk, D=64, seed=0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    q = torch.randn(B, H, Nq, D, device='cuda', dtype=torch.bfloat16, generator=g)
    k = torch.randn(B, H, Nk, D, device='cuda', dtype=torch.bfloat16, generator=g)
    v = torch.randn(B, H, Nk, D, device='cuda', dtype=torch.bfloat16, generator=g)
    do = torch.randn(B, H, Nq, D, device='cuda', dtype=torch.bfloat16, generator=g)
    return q, k, v, do, g


def _expand_cyclic(mask, B):
    if mask is not None and mask.dim() == 4 and 1 < mask.shape[0] < B:
        return mask.repeat(B // mask.shape[0], 1, 1, 1)
    return mask


def _reference(q, k, v, do, mask=None):
    """fp32 composition; returns dq, dk, dv (and dmask when it requires grad)."""
    q2, k2, v2 = [t.detach().float().requires_grad_(True) for t in (q, k, v)]
    attn = (q2 @ k2.transpose(-2, -1)) / math.sqrt(q.shape[-1])
    m2 = None
    if mask is not None:
        m2 = mask.detach().clone().requires_grad_(mask.requires_grad)
        attn = attn + _expand_cyclic(m2, q.shape[0])
    o = attn.softmax(-1) @ v2
    o.backward(do.float())
    return q2.grad, k2.grad, v2.grad, (m2.grad if m2 is not None else None)


def _fused(path, q, k, v, do, mask=None):
    """Grads of ops.flash_attention with the backward forced to `path`;
    asserts through the call counters that this path is the one that ran."""
    attn_mod.set_attn_bwd_path(path)
    before = dict(attn_mod.BWD_PATH_CALLS)
    q1, k1, v1 = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
    m1 = None
    if mask is not None:
        m1 = mask.detach().clone().requires_grad_(mask.requires_grad)
    o = ops.flash_attention(q1, k1, v1, attn_mask=m1)
    o.backward(do)
    other = 'two_pass' if path == 'single_pass' else 'single_pass'
    assert attn_mod.BWD_PATH_CALLS[path] == before[path] + 1, f'{path} did not run'
    assert attn_mod.BWD_PATH_CALLS[other] == before[other], f'{other} ran'
    return q1.grad, k1.grad, v1.grad, (m1.grad if m1 is not None else None)


def _assert_two_bounds(name, got, two_pass, ref, zero_ref=False):
    if zero_ref:
        print(f'{name}: rms single={_rms(got):.3e} two_pass={_rms(two_pass):.3e}')
        assert _rms(got) < ZERO_RMS, f'{name}: rms {_rms(got)}'
        return
    e_sp, e_tp = rel_err(got, ref), rel_err(two_pass, ref)
    print(f'{name}: single={e_sp:.3e} two_pass={e_tp:.3e}')
    assert e_sp < GRAD_TOL, f'{name}: err {e_sp}'
    assert e_sp <= VS_TWO_PASS * e_tp, f'{name}: err {e_sp} > 1.5 x two-pass {e_tp}'


def _check(q, k, v, do, mask=None):
    sp = _fused('single_pass', q, k, v, do, mask)
    tp = _fused('two_pass', q, k, v, do, mask)
    ref = _reference(q, k, v, do, mask)
    one_key = k.shape[2] == 1
    for i, n in enumerate(('dq', 'dk', 'dv')):
        assert torch.isfinite(sp[i].float()).all(), f'{n}: non-finite'
        _assert_two_bounds(n, sp[i], tp[i], ref[i], zero_ref=one_key and n != 'dv')
    return sp, tp, ref


@pytest.mark.parametrize('n', [1, 15, 16, 17, 63, 64, 65, 129, 197, 255, 256])
def test_self_attention_edges(n):
    """One key, 16-key tile edges, wave ownership edges (32 keys per wave,
    2 / 4 / 8-wave workgroups at Nk 64 / 128), last tile skipped or partly
    valid, upper dispatch bound."""
    q, k, v, do, _ = _inputs(2, 3, n, n, seed=n)
    _check(q, k, v, do)


@pytest.mark.parametrize('nq,nk', [(1, 197), (33, 197), (300, 70), (64, 256)])
def test_cross_attention(nq, nk):
    """Nq independent of Nk, several slices with a ragged last one, Nq > 256."""
    q, k, v, do, _ = _inputs(2, 3, nq, nk, seed=nq + nk)
    _check(q, k, v, do)


@pytest.mark.parametrize('mode', ['auto', 'forced'])
def test_dispatch_boundary_257(mode):
    """Nk = 257 is beyond the single-pass kernel: the two-pass kernels run,
    whatever is forced, and the result is still right."""
    q, k, v, do, _ = _inputs(2, 3, 257, 257, seed=257)
    attn_mod.set_attn_bwd_path('single_pass' if mode == 'forced' else None)
    before = dict(attn_mod.BWD_PATH_CALLS)
    q1, k1, v1 = [t.clone().requires_grad_(True) for t in (q, k, v)]
    ops.flash_attention(q1, k1, v1).backward(do)
    assert attn_mod.BWD_PATH_CALLS['two_pass'] == before['two_pass'] + 1
    assert attn_mod.BWD_PATH_CALLS['single_pass'] == before['single_pass']
    ref = _reference(q, k, v, do)
    for got, want in zip((q1.grad, k1.grad, v1.grad), ref):
        assert rel_err(got, want) < GRAD_TOL


def test_default_rule_takes_single_pass_at_vit_shape():
    """Unforced, N = 197 with head_dim 64 goes to the single-pass kernel."""
    q, k, v, do, _ = _inputs(1, 2, 197, 197, seed=5)
    attn_mod.set_attn_bwd_path(None)
    before = dict(attn_mod.BWD_PATH_CALLS)
    q1, k1, v1 = [t.clone().requires_grad_(True) for t in (q, k, v)]
    ops.flash_attention(q1, k1, v1).backward(do)
    assert attn_mod.BWD_PATH_CALLS['single_pass'] == before['single_pass'] + 1
    assert attn_mod.BWD_PATH_CALLS['two_pass'] == before['two_pass']


def _packed(path, qkv, do):
    attn_mod.set_attn_bwd_path(path)
    before = attn_mod.BWD_PATH_CALLS[path]
    qkv1 = qkv.detach().clone().requires_grad_(True)
    ops.flash_attention_qkv(qkv1).backward(do)
    assert attn_mod.BWD_PATH_CALLS[path] == before + 1
    return qkv1.grad


@pytest.mark.parametrize('shape', [(2, 197, 3, 3, 64), (1, 40, 3, 2, 64)])
def test_packed_qkv(shape):
    """flash_attention_qkv: gradients land in one packed dqkv buffer."""
    B, N, _, H, D = shape
    g = torch.Generator(device='cuda').manual_seed(N)
    qkv = torch.randn(shape, device='cuda', dtype=torch.bfloat16, generator=g)
    # O is a [B,H,N,D] view of BNHD storage; give dO the same layout
    do = torch.randn(B, N, H, D, device='cuda', dtype=torch.bfloat16, generator=g).permute(0, 2, 1, 3)
    sp = _packed('single_pass', qkv, do)
    tp = _packed('two_pass', qkv, do)
    qkv2 = qkv.detach().float().requires_grad_(True)
    q2, k2, v2 = qkv2.permute(2, 0, 3, 1, 4).unbind(0)
    o_ref = ((q2 @ k2.transpose(-2, -1)) / math.sqrt(D)).softmax(-1) @ v2
    o_ref.backward(do.float())
    _assert_two_bounds('dqkv', sp, tp, qkv2.grad)


def test_strided_qkv_views():
    """Separate q, k, v that are non-contiguous views with 16-byte-aligned
    strides (row pitch 72 and 80 elements, and a head-major / token-major mix)."""
    B, H, N, D = 2, 3, 70, 64
    g = torch.Generator(device='cuda').manual_seed(3)
    qb = torch.randn(B, H, N, D + 8, device='cuda', dtype=torch.bfloat16, generator=g)
    kb = torch.randn(B, H, N, D + 16, device='cuda', dtype=torch.bfloat16, generator=g)
    vb = torch.randn(B, N, H, D, device='cuda', dtype=torch.bfloat16, generator=g)
    do = torch.randn(B, H, N, D, device='cuda', dtype=torch.bfloat16, generator=g)

    def views(qb, kb, vb):
        return qb[..., :D], kb[..., 16:], vb.permute(0, 2, 1, 3)

    grads = {}
    for path in ('single_pass', 'two_pass'):
        attn_mod.set_attn_bwd_path(path)
        before = attn_mod.BWD_PATH_CALLS[path]
        leaves = [t.clone().requires_grad_(True) for t in (qb, kb, vb)]
        q1, k1, v1 = views(*leaves)
        assert not q1.is_contiguous() and not k1.is_contiguous() and not v1.is_contiguous()
        ops.flash_attention(q1, k1, v1).backward(do)
        assert attn_mod.BWD_PATH_CALLS[path] == before + 1
        grads[path] = views(*[t.grad for t in leaves])
    ref = _reference(*views(qb, kb, vb), do)
    for i, n in enumerate(('dq', 'dk', 'dv')):
        _assert_two_bounds(n, grads['single_pass'][i], grads['two_pass'][i], ref[i])


@pytest.mark.parametrize('layout', ['contiguous', 'bnhd'])
def test_do_layout(layout):
    """dO contiguous [B,H,N,D] and as the transposed view of BNHD storage: the
    kernel reads it through strides and forms delta = rowsum(dO o O) itself;
    delta reaches the result only through dq and dk."""
    B, H, N, D = 2, 3, 197, 64
    q, k, v, do, g = _inputs(B, H, N, N, seed=21)
    if layout == 'bnhd':
        do = do.transpose(1, 2).contiguous().transpose(1, 2)
        assert not do.is_contiguous()
    sp, tp, ref = _check(q, k, v, do)
    # the same values in the other layout give the same bits
    other = do.contiguous() if layout == 'bnhd' else do.transpose(1, 2).contiguous().transpose(1, 2)
    sp2 = _fused('single_pass', q, k, v, other)
    assert torch.equal(sp[0], sp2[0]) and torch.equal(sp[1], sp2[1])


@pytest.mark.parametrize('n', [197, 100])
def test_mask_per_head_bias(n):
    """[1,H,N,N] bias that needs no gradient."""
    q, k, v, do, g = _inputs(2, 3, n, n, seed=n + 1)
    bias = torch.randn(1, 3, n, n, device='cuda', generator=g) * 2.0
    _check(q, k, v, do, bias)


@pytest.mark.parametrize('n', [197, 100])
def test_mask_key_padding_inf(n):
    """[B,1,N,N] with -inf key padding on one batch element: finite
    gradients, and dk, dv of the padded keys exactly zero."""
    B, H = 2, 3
    q, k, v, do, _ = _inputs(B, H, n, n, seed=n + 2)
    pad = 37
    mask = torch.zeros(B, 1, n, n, device='cuda')
    mask[1, :, :, n - pad:] = float('-inf')
    sp, _, _ = _check(q, k, v, do, mask)
    assert sp[1][1, :, n - pad:].float().abs().max().item() == 0.0
    assert sp[2][1, :, n - pad:].float().abs().max().item() == 0.0


@pytest.mark.parametrize('n', [197, 100])
def test_mask_cyclic(n):
    """[2,H,N,N] mask with B = 4 is read as mask[b % 2]."""
    q, k, v, do, g = _inputs(4, 3, n, n, seed=n + 3)
    mask = torch.randn(2, 3, n, n, device='cuda', generator=g) * 2.0
    _check(q, k, v, do, mask)


@pytest.mark.parametrize('n', [197, 100])
def test_mask_bias_requires_grad(n):
    """A bias that wants a gradient: dbias within the same two bounds against
    the two-pass path, and dq, dk, dv still right."""
    q, k, v, do, g = _inputs(2, 3, n, n, seed=n + 4)
    bias = (torch.randn(1, 3, n, n, device='cuda', generator=g) * 2.0).requires_grad_(True)
    sp, tp, ref = _check(q, k, v, do, bias)
    assert sp[3] is not None and sp[3].shape == bias.shape
    assert torch.isfinite(sp[3]).all()
    _assert_two_bounds('dbias', sp[3], tp[3], ref[3])


@pytest.mark.parametrize('n', [49, 64])
@pytest.mark.parametrize('kind', ['bias', 'cyclic', 'bias_grad'])
def test_mask_window_sizes(n, kind):
    """Masked window attention, Nk <= 64: the 2-wave variant with a mask
    ([1,H,N,N] bias, cyclic [2,H,N,N] shift mask with -inf entries, and a bias
    that wants a gradient)."""
    B, H = 4, 3
    q, k, v, do, g = _inputs(B, H, n, n, seed=n + 7)
    if kind == 'cyclic':
        mask = torch.randn(2, H, n, n, device='cuda', generator=g) * 2.0
        mask[1, :, : n // 2, n // 2:] = float('-inf')
        mask[1, :, n // 2:, : n // 2] = float('-inf')
    else:
        mask = torch.randn(1, H, n, n, device='cuda', generator=g) * 2.0
        mask.requires_grad_(kind == 'bias_grad')
    sp, tp, ref = _check(q, k, v, do, mask)
    if kind == 'bias_grad':
        _assert_two_bounds('dbias', sp[3], tp[3], ref[3])


def test_gemm_mode_packed_qkv(monkeypatch):
    """TIMM_AMD_ATTN_BWD=gemm (the GEMM-recompute reference backward) reaches
    the packed-qkv entry."""
    shape = (2, 70, 3, 3, 64)
    g = torch.Generator(device='cuda').manual_seed(70)
    qkv = torch.randn(shape, device='cuda', dtype=torch.bfloat16, generator=g)
    do = torch.randn(2, 70, 3, 64, device='cuda', dtype=torch.bfloat16, generator=g).permute(0, 2, 1, 3)
    monkeypatch.setattr(attn_mod, '_BWD_MODE', 'gemm')
    before = dict(attn_mod.BWD_PATH_CALLS)
    qkv1 = qkv.clone().requires_grad_(True)
    ops.flash_attention_qkv(qkv1).backward(do)
    assert attn_mod.BWD_PATH_CALLS == before, 'a fused backward ran in gemm mode'
    qkv2 = qkv.detach().float().requires_grad_(True)
    q2, k2, v2 = qkv2.permute(2, 0, 3, 1, 4).unbind(0)
    o_ref = ((q2 @ k2.transpose(-2, -1)) / math.sqrt(64)).softmax(-1) @ v2
    o_ref.backward(do.float())
    assert rel_err(qkv1.grad, qkv2.grad) < GRAD_TOL


SENTINEL = 777.0


@pytest.mark.parametrize('nq,nk', [(197, 197), (197, 17), (17, 197), (17, 17)])
def test_bounds_sentinel(nq, nk):
    """The extension entry called directly: dq, dk, dv are views into the
    middle of larger sentinel-filled buffers, and nothing outside them moves."""
    ext = ops.require_ext()
    B, H, D = 2, 3, 64
    q, k, v, do, _ = _inputs(B, H, nq, nk, seed=nq * 3 + nk)
    scale = 1.0 / math.sqrt(D)
    o, lse = ext.attention_fwd(q, k, v, None, scale)

    def padded(n):
        buf = torch.full((B, H, n + 4, D + 16), SENTINEL, device='cuda', dtype=torch.bfloat16)
        return buf, buf[:, :, 2:2 + n, 8:8 + D]

    (bq, dq), (bk, dk), (bv, dv) = padded(nq), padded(nk), padded(nk)
    ext.attention_bwd_single_pass(q, k, v, do, o, lse, None, None, dq, dk, dv, scale)
    torch.cuda.synchronize()
    ref = _reference(q, k, v, do)
    for name, buf, view, want, n in (('dq', bq, dq, ref[0], nq), ('dk', bk, dk, ref[1], nk),
                                     ('dv', bv, dv, ref[2], nk)):
        assert rel_err(view, want) < GRAD_TOL, name
        outside = torch.ones_like(buf, dtype=torch.bool)
        outside[:, :, 2:2 + n, 8:8 + D] = False
        assert (buf[outside] == SENTINEL).all(), f'{name}: wrote outside its view'


@pytest.mark.parametrize('masked', [False, True])
def test_reproducible(masked):
    """No atomics: the same inputs twice give the same bits."""
    q, k, v, do, g = _inputs(2, 3, 197, 197, seed=9)
    mask = torch.randn(1, 3, 197, 197, device='cuda', generator=g) if masked else None
    a = _fused('single_pass', q, k, v, do, mask)
    b = _fused('single_pass', q, k, v, do, mask)
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)
