"""The additive attention bias gets a gradient through the fused flash path.

Op level: bf16 q/k/v, fp32 bias (x2.0, requires_grad) against the fp32
composition on the same bf16-rounded inputs, plain ||a-b||/||b||.
Model level: every parameter of the rel-pos-bias models ends a bf16 GPU
backward with a gradient; the rel-pos gradients are compared with the same
weights in fp32 on the CPU.

Measured on MI355X (see profiles/attn_dbias/README.md): dbias error of the op
cases 1.2e-3 .. 1.7e-3 against the 5e-2 bound; model-level rel-pos gradient
error fused / fused attention kernels off: swin 9.2e-3 / 1.0e-2, swinv2
1.8e-2 / 1.8e-2, beit 3.9e-3 / 3.9e-3, vit_relpos 2.4e-1 / 2.2e-1 (the one
model that passes on the 2x bound only).
"""
import math

import pytest
import torch

import timm_amd
from timm_amd import ops
from timm_amd.layers import set_fused_attn, use_fused_attn
from timm_amd.ops import attention as attn_mod

pytestmark = pytest.mark.gpu

DBIAS_TOL = 5e-2   # the project's bound for masked-attention gradients
GRAD_TOL = 5e-2    # dq/dk/dv bound of test_ops_gpu.py::test_attention_perhead_bias


def rel_err(a, b):
    a, b = a.float(), b.float()
    assert b.norm() > 0, 'reference is all zero'
    return ((a - b).norm() / b.norm()).item()


def _inputs(B, H, Nq, Nk, D, seed=0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    q = torch.randn(B, H, Nq, D, device='cuda', dtype=torch.bfloat16, generator=g)
    k = torch.randn(B, H, Nk, D, device='cuda', dtype=torch.bfloat16, generator=g)
    v = torch.randn(B, H, Nk, D, device='cuda', dtype=torch.bfloat16, generator=g)
    do = torch.randn(B, H, Nq, D, device='cuda', dtype=torch.bfloat16, generator=g)
    return q, k, v, do, g


def _bias(shape, g):
    return (torch.randn(shape, device='cuda', generator=g) * 2.0).requires_grad_(True)


def _expand_cyclic(bias, B):
    """[mB,...] with 1 < mB < B is read as bias[b % mB] by the kernels."""
    if bias.dim() == 4 and 1 < bias.shape[0] < B:
        return bias.repeat(B // bias.shape[0], 1, 1, 1)
    return bias


def _fused(q, k, v, do, bias, extra_mask=None):
    q1, k1, v1 = [t.clone().requires_grad_(True) for t in (q, k, v)]
    mask = bias if extra_mask is None else bias + extra_mask
    o = ops.flash_attention(q1, k1, v1, attn_mask=mask)
    o.backward(do)
    return o, q1.grad, k1.grad, v1.grad


def _reference(q, k, v, do, bias, extra_mask=None):
    """fp32 composition on the bf16-rounded inputs; returns o, dq, dk, dv, dbias."""
    q2, k2, v2 = [t.detach().float().requires_grad_(True) for t in (q, k, v)]
    b2 = bias.detach().clone().requires_grad_(True)
    full = _expand_cyclic(b2, q.shape[0])
    if extra_mask is not None:
        full = full + extra_mask
    attn = (q2 @ k2.transpose(-2, -1)) / math.sqrt(q.shape[-1]) + full
    o = attn.softmax(-1) @ v2
    o.backward(do.float())
    return o, q2.grad, k2.grad, v2.grad, b2.grad


def _check(name, q, k, v, do, bias, extra_mask=None):
    o, dq, dk, dv = _fused(q, k, v, do, bias, extra_mask)
    o_r, dq_r, dk_r, dv_r, db_r = _reference(q, k, v, do, bias, extra_mask)
    assert bias.grad is not None, f'{name}: bias.grad is None'
    assert bias.grad.shape == bias.shape and bias.grad.dtype == bias.dtype
    assert torch.isfinite(bias.grad).all(), f'{name}: non-finite dbias'
    errs = {
        'dbias': rel_err(bias.grad, db_r), 'o': rel_err(o, o_r),
        'dq': rel_err(dq, dq_r), 'dk': rel_err(dk, dk_r), 'dv': rel_err(dv, dv_r)}
    print(f'{name}: ' + ' '.join(f'{n}={e:.3e}' for n, e in errs.items()))
    assert errs['dbias'] < DBIAS_TOL, f'{name}: dbias err {errs["dbias"]}'
    assert errs['o'] < 2e-2, f'{name}: fwd err {errs["o"]}'
    for n in ('dq', 'dk', 'dv'):
        assert errs[n] < GRAD_TOL, f'{name}: {n} err {errs[n]}'
    return bias.grad


@pytest.mark.parametrize('mB', [1, 2, 4])
def test_swin_window_shape(mB):
    """N=49: one partial 64x64 tile, non-swizzled D=32, broadcast/cyclic/per-sample."""
    B, H, N, D = 4, 4, 49, 32
    q, k, v, do, g = _inputs(B, H, N, N, D, seed=1)
    _check(f'swin mB={mB}', q, k, v, do, _bias((mB, H, N, N), g))


@pytest.mark.parametrize('case', [
    ('4 q tiles + 5-row tail, swizzled, odd batch', 3, 2, 197, 197, 64),
    ('cross-attention one past the tile edges', 2, 2, 65, 33, 64),
    ('D=96', 2, 2, 40, 40, 96),
    ('D=128', 2, 1, 70, 70, 128),
], ids=['n197_d64', 'cross_65x33', 'd96', 'd128'])
def test_tile_edges_and_head_dims(case):
    name, B, H, Nq, Nk, D = case
    q, k, v, do, g = _inputs(B, H, Nq, Nk, D, seed=2)
    _check(name, q, k, v, do, _bias((1, H, Nq, Nk), g))


@pytest.mark.parametrize('mB', [4, 1])
def test_head_broadcast(mB):
    """[B,1,N,N] and [1,1,N,N]: the kernel reduces over heads."""
    B, H, N, D = 4, 4, 49, 32
    q, k, v, do, g = _inputs(B, H, N, N, D, seed=3)
    _check(f'head-broadcast mB={mB}', q, k, v, do, _bias((mB, 1, N, N), g))


@pytest.mark.parametrize('kind', ['HNN', '1H1Nk'])
def test_broadcast_inputs(kind):
    """Autograd reduces the kernel's [mB,Hm,Nq,Nk] gradient to the input's shape."""
    B, H, N, D = 4, 4, 49, 32
    q, k, v, do, g = _inputs(B, H, N, N, D, seed=4)
    shape = (H, N, N) if kind == 'HNN' else (1, H, 1, N)
    _check(f'broadcast {kind}', q, k, v, do, _bias(shape, g))


@pytest.mark.parametrize('mB', [1, 4])
def test_key_padding_mask(mB):
    """Learned bias + non-learned -inf key padding [B,1,1,N]: finite gradient,
    exactly zero at the padded columns of a per-sample bias."""
    B, H, N, D = 4, 4, 49, 32
    q, k, v, do, g = _inputs(B, H, N, N, D, seed=5)
    pad = torch.zeros(B, 1, 1, N, device='cuda')
    pad[2, :, :, -10:] = float('-inf')
    bias = _bias((mB, H, N, N), g)
    db = _check(f'key padding mB={mB}', q, k, v, do, bias, extra_mask=pad)
    if mB == B:
        assert (db[2, :, :, -10:] == 0).all()
        assert db[2, :, :, :-10].abs().max() > 0


def test_packed_qkv():
    B, N, H, D = 2, 50, 4, 32
    g = torch.Generator(device='cuda').manual_seed(6)
    qkv = torch.randn(B, N, 3, H, D, device='cuda', dtype=torch.bfloat16, generator=g)
    do = torch.randn(B, N, H, D, device='cuda', dtype=torch.bfloat16, generator=g).permute(0, 2, 1, 3)
    bias = _bias((1, H, N, N), g)
    qkv1 = qkv.clone().requires_grad_(True)
    ops.flash_attention_qkv(qkv1, attn_mask=bias).backward(do)

    qkv2 = qkv.detach().float().requires_grad_(True)
    b2 = bias.detach().clone().requires_grad_(True)
    q, k, v = qkv2.permute(2, 0, 3, 1, 4).unbind(0)
    attn = (q @ k.transpose(-2, -1)) / math.sqrt(D) + b2
    (attn.softmax(-1) @ v).backward(do.float())

    assert bias.grad is not None and torch.isfinite(bias.grad).all()
    e_b, e_qkv = rel_err(bias.grad, b2.grad), rel_err(qkv1.grad, qkv2.grad)
    print(f'packed: dbias={e_b:.3e} dqkv={e_qkv:.3e}')
    assert e_b < DBIAS_TOL
    assert e_qkv < GRAD_TOL


def _split_case(B=256, H=2, mB=2, Hm=None):
    N, D = 49, 32
    q, k, v, do, g = _inputs(B, H, N, N, D, seed=7)
    return q, k, v, do, _bias((mB, Hm or H, N, N), g)


@pytest.mark.parametrize('ragged', [False, True])
def test_split_reduction(ragged):
    """Many reduced batches per bias element: the loop is split over the grid
    and the slabs summed by the second kernel.  The ragged case reduces 18
    (batch, head) pairs in chunks of 5, 5, 5, 3."""
    q, k, v, do, bias = _split_case(9, 2, 1, 1) if ragged else _split_case()
    ns = attn_mod._mask_nsplit(q, k, bias)
    assert ns > 1
    if ragged:
        assert ns == 4
    _check(f'nsplit={ns}', q, k, v, do, bias)


@pytest.mark.parametrize('split', [False, True])
def test_reproducible(split):
    if split:
        q, k, v, do, bias = _split_case()
    else:
        q, k, v, do, g = _inputs(4, 4, 49, 49, 32, seed=8)
        bias = _bias((4, 4, 49, 49), g)
    assert (attn_mod._mask_nsplit(q, k, bias) > 1) == split
    grads = []
    for _ in range(2):
        bias.grad = None
        _fused(q, k, v, do, bias)
        grads.append(bias.grad.clone())
    assert torch.equal(grads[0], grads[1])


def test_no_grad_needed_leaves_dqkv_unchanged():
    q, k, v, do, g = _inputs(4, 4, 49, 49, 32, seed=9)
    bias = _bias((2, 4, 49, 49), g)
    with_grad = _fused(q, k, v, do, bias)
    frozen = bias.detach().clone()
    assert not frozen.requires_grad
    without = _fused(q, k, v, do, frozen)
    assert bias.grad is not None and frozen.grad is None
    for a, b in zip(with_grad, without):
        assert torch.equal(a, b)


def test_gemm_mode(monkeypatch):
    """The TIMM_AMD_ATTN_BWD=gemm A/B path produces the bias gradient too."""
    monkeypatch.setattr(attn_mod, '_BWD_MODE', 'gemm')
    q, k, v, do, g = _inputs(4, 4, 49, 49, 32, seed=10)
    _check('gemm mode', q, k, v, do, _bias((1, 4, 49, 49), g))


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------
MODELS = {
    'swin': ('swin_tiny_patch4_window7_224',
             dict(img_size=56, embed_dim=64, depths=(2, 2), num_heads=(2, 4)), 56),
    'swinv2': ('swinv2_tiny_window8_256',
               dict(img_size=64, embed_dim=64, depths=(2, 2), num_heads=(2, 4), window_size=8), 64),
    'beit': ('beit_base_patch16_224',
             dict(img_size=64, embed_dim=64, depth=2, num_heads=2), 64),
    # init_values=1.0: the default 1e-6 LayerScale scales every gradient behind
    # the blocks by 1e-6 (reference gradient norm 6.8e-9); None would be
    # dropped by create_model
    'vit_relpos': ('vit_relpos_small_patch16_224',
                   dict(img_size=64, embed_dim=64, depth=2, num_heads=2, init_values=1.0), 64),
}
# every place the four models ask whether the fused kernels may run
FUSED_GATES = ('timm_amd.ops.attention', 'timm_amd.models.swin_transformer',
               'timm_amd.models.swin_transformer_v2')
REL_POS_KEYS = ('relative_position_bias_table', 'cpb_mlp', 'rel_pos')


@pytest.fixture
def fused_attn_flag():
    prev = use_fused_attn()
    yield
    set_fused_attn(prev)


def _rel_pos_names(model):
    return [n for n, p in model.named_parameters()
            if p.requires_grad and any(key in n for key in REL_POS_KEYS)]


def _grads(model, x, g):
    model.zero_grad(set_to_none=True)
    (model(x).float() * g).sum().backward()
    return {n: p.grad for n, p in model.named_parameters() if p.requires_grad}


@pytest.mark.parametrize('key', list(MODELS))
def test_model_trains_rel_pos_bias(key, fused_attn_flag, monkeypatch):
    name, kwargs, img = MODELS[key]
    # stochastic depth (0.1 by default in Swin/SwinV2) would drop different
    # blocks in each of the three backward passes compared here
    kwargs = dict(kwargs, drop_path_rate=0.)
    torch.manual_seed(11)
    set_fused_attn(True)
    ref = timm_amd.create_model(name, num_classes=10, **kwargs).train()
    # zero-initialised parameters (classifier heads, post-norm scales) would cut
    # every gradient behind them to exactly 0: fill them with noise
    with torch.no_grad():
        for p in ref.parameters():
            if p.abs().max() == 0:
                p.normal_(std=0.02)
    state = ref.state_dict()
    x = torch.randn(2, 3, img, img)
    g = torch.randn(2, 10)

    names = _rel_pos_names(ref)
    assert names, f'{name}: no relative-position parameters found'
    ref_grads = _grads(ref, x, g)
    assert all(v is not None for v in ref_grads.values())
    ref_cat = torch.cat([ref_grads[n].flatten() for n in names])

    def gpu_cat(fused):
        # the attention modules read the flag when they are constructed; only
        # Swin's consults it, so the eager copy also switches the kernels off
        # where the models ask for them: Swin/SwinV2 then run their bf16
        # composition, BEiT/vit_relpos the op's composition (ops._math_sdpa)
        set_fused_attn(fused)
        if not fused:
            for mod in FUSED_GATES:
                monkeypatch.setattr(mod + '.attention_available', lambda q: False)
        m = timm_amd.create_model(name, num_classes=10, **kwargs)
        m.load_state_dict(state)
        m = m.to('cuda', torch.bfloat16).train()
        grads = _grads(m, x.to('cuda', torch.bfloat16), g.cuda())
        missing = [n for n, v in grads.items() if v is None]
        assert not missing, f'{name} fused={fused}: parameters without grad: {missing}'
        for n in names:
            assert torch.isfinite(grads[n]).all(), f'{name}: non-finite grad in {n}'
        return torch.cat([grads[n].float().cpu().flatten() for n in names])

    err_fused = rel_err(gpu_cat(True), ref_cat)
    err_eager = rel_err(gpu_cat(False), ref_cat)
    print(f'{name}: rel-pos grad err vs fp32 CPU: fused={err_fused:.3e} eager={err_eager:.3e}')
    assert err_fused < DBIAS_TOL or err_fused < 2 * err_eager, (
        f'{name}: fused {err_fused} vs eager {err_eager}')
