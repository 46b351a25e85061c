"""Edge-shape and dispatch-path tests for the norm, elementwise and NHWC
depthwise-conv kernels (csrc/layernorm.hip, elementwise.hip, depthwise_conv.hip).

Reference and tolerance (one rule for the whole module, see `_check`)
---------------------------------------------------------------------
ref64    the plain PyTorch composition of the op in fp64 on the test's inputs
         upcast, gradients through autograd with the test's dy
ideal32  the same composition in fp32
e32      max|ideal32 - ref64| over the tensor: the fp32 noise floor, measured
         from the reference, never from the kernel
u        unit roundoff of the output dtype (bf16 2^-9, fp16 2^-11, fp32 2^-24)

    |got - ref64| <= 2*u*|ref64| + 2*u*s + 4*e32          per element

s is 0 for elementwise outputs (and for conv y/dx, which are rounded once from
an fp32 accumulator), the row's RMS of ref64 for norm outputs and dx, and the
RMS of the summed terms of that column for column reductions (dw, db, dgamma,
dwconv dw/dbias).  2 on u = one rounding to the output type plus margin for an
equally precise rounding point; 4 on e32 = two correct fp32 implementations
that sum in a different order.  Exact answers (dropped samples, relu,
identity, zero gradients) are asserted with equality.

Branch -> case map
------------------
layernorm.hip (one wave per row, 4 rows per block; 16-bit types with
cols % 8 == 0 use 16-byte vectors, lane l owns vectors l, l+64, ...):
  cols    8  one vector, 63 idle lanes (fwd register kernel and fast bwd, kChunks=1)
  cols  100  cols % 8 != 0: scalar fwd, slow (LDS-atomic) bwd for every dtype
  cols  504  kChunks=1, last lane idle                  cols  512  kChunks=1 exact
  cols  520  kChunks=2, one lane in chunk 2             cols 1032  kChunks=4, chunk 4 empty
  cols 2056  LN kChunks=6 partial (RMS: 8)              cols 3072  LN kChunks=6 exact (RMS: 8)
  cols 3080, 4096  LN bwd: slow kernel, RMS bwd: kChunks=8
  cols 4104  slow bwd for both
  forward: register kernel kChunks 1/2/4/8 for cols <= 512/1024/2048/4096 (so 2056, 3072,
             3080, 4096 -> 8), generic re-reading kernel for cols 100, 4104 and all fp32
  fp32       always scalar fwd + slow bwd (test_norm_shapes[*-fp32])
  rows 1/3/5 fewer than / straddling one 4-wave block
  rows 1283  > 320*4: fast bwd grid-strides with a ragged tail (test_norm_many_rows)
  rows 32771 x cols 8: > 8192*4, fwd grid-strides; fp32 also strides the slow bwd (1024 blocks)
  bias=None, transposed x, expanded dy: test_norm_layouts
  cancellation in the variance: test_norm_offset_rows / constant_rows / near_constant / zero_row
  saved mean/rstd: test_layer_norm_saved_stats
elementwise.hip bias_act (bwd fast kernel if cols % 8 == 0 and cols <= 4096):
  cols 8/520/1032/2056,3072/4096 -> kChunks 1/2/4/6/8; cols 100, 4104 -> LDS-atomic slow bwd
  rows 2563 > 640*4: fast bwd grid-strides; 2563 x 108: slow bwd grid-strides (> 1024*256 elements)
  1025 x 4104: > 2048*256*8 elements, fwd grid-strides
  |x+b| up to 30 in every activation: test_bias_act_saturation
elementwise.hip residual_scale_add: {gamma, none} x {keep, none} kernels, 2-D/3-D/4-D,
  cols % 8 != 0 scalar path, n > 1024*256 so the bwd grid-strides
depthwise_conv.hip (weight gradient: stride 1 and K in {3,5,7,9} -> row-sliding
kernel, anything else -> generic kernel with kMaxK = next of 3/5/7/9):
  see DW_CASES; B=1 and 3, bias and none, dy channels-last / NCHW / expanded

Calibration: largest |got - ref64| / tolerance seen on an MI355X
----------------------------------------------------------------
Ratios at the default factors.  bf16 sits just under 1 by construction: the rule's
u = 2^-9 is half of bf16's own rounding error bound (8 significant bits round to
within 2^-8 |x|), so 2*u*|ref64| is exactly one correct rounding; fp16 sits near 0.5.

  op             output   bf16    fp16    fp32     worst case
  layer_norm     y        0.785   0.395   0.276    1283x520
                 dx       0.779   0.381   0.310    1283x520
                 dw       0.923   0.467   1.65 *   1283x520; fp32: 32771x8
                 db       0.898   0.455   1.44 *   offset 8; fp32: 32771x8
                 mean/rstd                0.143 / 0.156
  rms_norm       y        0.796   0.394   0.240    1283x520
                 dx       0.798   0.372   0.241    dy = xhat, 520
                 dw       0.906   0.484   1.79 *   offset 100; fp32: 32771x8
  bias_act       y        0.996   0.500            identity 3x100
                 dx       0.995   0.497            gelu 2563x520
                 db       0.941   0.434            relu 2563x520
  residual       out      0.996   0.500
                 dy       0.988   0.498
                 dgamma   0.927   0.475
  dwconv         y 0.994  dx 0.996  dw 0.939  dbias 0.845   (bf16 only)

  * a correct kernel over the default bound (largest of three runs): see E32_FACTOR,
    which sets 32 in place of 4 for these three (then 0.21 / 0.18 / 0.22).
Before the forward computed the variance in two passes, layer_norm in fp32 reached 15.7 (y)
and 119 (dx) at offset 32, 72 and 434 at offset 64 / std 0.5, 4e3 on near-constant rows, and
returned NaN for constant rows of 300.3 and 1000.7.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import timm_amd  # noqa
from timm_amd import ops
from timm_amd.ops.elementwise import _ResidualScaleAddFn, _act_eager

pytestmark = pytest.mark.gpu

BF16, FP16, FP32, FP64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
UNIT = {BF16: 2.0 ** -9, FP16: 2.0 ** -11, FP32: 2.0 ** -24}
NAME = {BF16: 'bf16', FP16: 'fp16', FP32: 'fp32'}
EPS = 1e-6

# worst got/tolerance ratio per op output, printed when the module finishes
CALIB = {}


@pytest.fixture(scope='module', autouse=True)
def _report_calibration():
    yield
    for key in sorted(CALIB):
        ratio, tag = CALIB[key]
        print(f'\ncalibration {key}: {ratio:.3f}  ({tag})', end='')
    print()


def _ext():
    assert ops.has_ext(), "HIP extension must be built (python setup.py build_ext --inplace)"
    return ops.require_ext()


# Factor on e32 where a correct kernel exceeds the default 4 (measured ratio at 4 alongside;
# atomics arrive in a different order every run, so it moves).
# The fp32 norm backward adds one partial dw/db per block with fp32 atomics: up to 1024
# partials summed as a chain in arrival order, against the pairwise tree behind e32.  A chain
# of n roundings walks ~sqrt(n) ulps where a tree walks ~sqrt(log2 n); for 32771 rows that is
# sqrt(1024 / 15) ~ 8 times the tree's error, so these three get 4 * 8.
E32_FACTOR = {
    'layer_norm.dw[fp32]': 32,   # 1.37 .. 1.65 at 32771 x 8
    'layer_norm.db[fp32]': 32,   # 0.87 .. 1.44 at 32771 x 8
    'rms_norm.dw[fp32]': 32,     # 1.32 .. 1.79 at 32771 x 8
}


def _check(fails, op, tag, got, ref64, ideal32, dtype, s=0.0):
    """The module's one tolerance rule; appends a message to `fails` on a miss."""
    assert got.shape == ref64.shape, f'{op} {tag}: shape {tuple(got.shape)} vs {tuple(ref64.shape)}'
    u = UNIT[dtype]
    got = got.detach().cpu().to(FP64)
    e32 = (ideal32.to(FP64) - ref64).abs().max().item() if ref64.numel() else 0.0
    tol = 2 * u * ref64.abs() + 2 * u * s + E32_FACTOR.get(f'{op}[{NAME[dtype]}]', 4) * e32
    err = (got - ref64).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)
    ratio = torch.nan_to_num(ratio, nan=math.inf, posinf=math.inf)
    if ratio.numel() == 0:
        return
    worst = ratio.argmax().item()
    r = ratio.flatten()[worst].item()
    key = f'{op}[{NAME[dtype]}]'
    print(f'ratio {key} {tag}: {r:.3f}')
    if r > CALIB.get(key, (-1.0, ''))[0]:
        CALIB[key] = (r, tag)
    if not r <= 1.0:
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(worst), ratio.shape))
        fails.append(
            f'{key} {tag}: worst at {idx}: got {got.flatten()[worst].item():.9g} '
            f'ref64 {ref64.flatten()[worst].item():.9g} tol {tol.flatten()[worst].item():.3g} '
            f'(e32 {e32:.3g}) ratio {r:.3g}')


def _reference(fn, inputs, dy, dtype):
    """fn on CPU copies of `inputs` in `dtype`; returns (y, [grad per input])."""
    leaves = [None if t is None else t.detach().cpu().to(dtype).requires_grad_(True) for t in inputs]
    y = fn(*leaves)
    y.backward(dy.detach().cpu().to(dtype))
    return y.detach(), [None if t is None else t.grad for t in leaves]


def _row_rms(t):
    return t.pow(2).mean(-1, keepdim=True).sqrt()


def _col_rms(terms):
    """RMS of the terms summed into each column: [..., cols] -> [cols]."""
    return terms.reshape(-1, terms.shape[-1]).pow(2).mean(0).sqrt()


# ---------------------------------------------------------------------------
# LayerNorm / RMSNorm
# ---------------------------------------------------------------------------

def _norm_compose(rms):
    def fn(x, w, b=None):
        if rms:
            xhat = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS)
        else:
            xc = x - x.mean(-1, keepdim=True)
            xhat = xc * torch.rsqrt(xc.pow(2).mean(-1, keepdim=True) + EPS)
        y = xhat * w
        return y if b is None else y + b
    return fn


def _run_norm(kind, x, w, b, dy, tag, fwd_only=False):
    """x: [..., cols] cuda tensor (any strides); dy None -> back-propagate y.sum()."""
    _ext()
    rms = kind == 'rms_norm'
    dtype = x.dtype
    cols = x.shape[-1]
    if rms:
        b = None
    x1 = x.detach().requires_grad_(True)
    w1 = w.detach().clone().requires_grad_(True)
    b1 = None if b is None else b.detach().clone().requires_grad_(True)
    if rms:
        y = ops.rms_norm(x1, (cols,), w1, EPS)
    else:
        y = ops.layer_norm(x1, (cols,), w1, b1, EPS)
    assert y.dtype == dtype and y.shape == x.shape
    dy_ref = torch.ones_like(y) if dy is None else dy
    inputs = (x, w) if rms or b is None else (x, w, b)
    y64, g64 = _reference(_norm_compose(rms), inputs, dy_ref, FP64)
    y32, g32 = _reference(_norm_compose(rms), inputs, dy_ref, FP32)

    fails = []
    _check(fails, f'{kind}.y', tag, y, y64, y32, dtype, _row_rms(y64))
    if not fwd_only:
        if dy is None:
            y.sum().backward()
        else:
            y.backward(dy)
        x64 = x.detach().cpu().to(FP64)
        xhat64 = _norm_compose(rms)(x64, torch.ones(cols, dtype=FP64))
        dy64 = dy_ref.detach().cpu().to(FP64)
        _check(fails, f'{kind}.dx', tag, x1.grad, g64[0], g32[0], dtype, _row_rms(g64[0]))
        _check(fails, f'{kind}.dw', tag, w1.grad, g64[1], g32[1], dtype, _col_rms(dy64 * xhat64))
        if b1 is not None:
            _check(fails, f'{kind}.db', tag, b1.grad, g64[2], g32[2], dtype, _col_rms(dy64))
    return y, fails


def _norm_params(cols, dtype, gen):
    w = (1.0 + 0.1 * torch.randn(cols, generator=gen)).to(dtype).cuda()
    b = (0.1 * torch.randn(cols, generator=gen)).to(dtype).cuda()
    return w, b


def _gen(seed):
    return torch.Generator().manual_seed(seed)


NORM_COLS = [8, 100, 504, 512, 520, 1032, 2056, 3072, 3080, 4096, 4104]
NORM_ROWS = [1, 3, 5]


@pytest.mark.parametrize('dtype', [BF16, FP16, FP32], ids=lambda d: NAME[d])
@pytest.mark.parametrize('cols', NORM_COLS)
@pytest.mark.parametrize('kind', ['layer_norm', 'rms_norm'])
def test_norm_shapes(kind, cols, dtype):
    """Every (cols class x dtype), rows 1/3/5 rotating over the cols list."""
    rows = NORM_ROWS[(NORM_COLS.index(cols) + [BF16, FP16, FP32].index(dtype)) % 3]
    g = _gen(cols)
    x = torch.randn(rows, cols, generator=g).to(dtype).cuda()
    w, b = _norm_params(cols, dtype, g)
    dy = torch.randn(rows, cols, generator=g).to(dtype).cuda()
    _, fails = _run_norm(kind, x, w, b, dy, f'{rows}x{cols}')
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('kind', ['layer_norm', 'rms_norm'])
@pytest.mark.parametrize('rows,cols,dtype', [
    (1283, 520, BF16),     # fast bwd, kChunks=2, 320 blocks stride over 321 row groups
    (1283, 1032, FP16),    # fast bwd, kChunks=4
    (32771, 8, BF16),      # fwd caps at 8192 blocks; fast bwd strides ~26 times
    (32771, 8, FP32),      # fwd strides; slow bwd caps at 1024 blocks
], ids=lambda v: NAME.get(v, str(v)))
def test_norm_many_rows(kind, rows, cols, dtype):
    g = _gen(rows + cols)
    x = torch.randn(rows, cols, generator=g).to(dtype).cuda()
    w, b = _norm_params(cols, dtype, g)
    dy = torch.randn(rows, cols, generator=g).to(dtype).cuda()
    _, fails = _run_norm(kind, x, w, b, dy, f'{rows}x{cols}')
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('dtype', [BF16, FP32], ids=lambda d: NAME[d])
@pytest.mark.parametrize('kind', ['layer_norm', 'rms_norm'])
def test_norm_layouts(kind, dtype):
    """bias=None (LN), a transposed-view x, a 3-D x, and an expanded dy (y.sum())."""
    g = _gen(7)
    cols = 520
    w, b = _norm_params(cols, dtype, g)
    fails = []
    # transposed view: [cols, rows].t() has stride (1, rows)
    x_t = torch.randn(cols, 6, generator=g).to(dtype).cuda().t()
    assert not x_t.is_contiguous()
    dy = torch.randn(6, cols, generator=g).to(dtype).cuda()
    fails += _run_norm(kind, x_t, w, b, dy, 'transposed-x')[1]
    # 3-D input, no bias, expanded dy
    x3 = torch.randn(2, 3, cols, generator=g).to(dtype).cuda()
    fails += _run_norm(kind, x3, w, None, None, '3d-nobias-sumdy')[1]
    # non-contiguous dy: a column-major buffer
    dy_t = torch.randn(cols, 6, generator=g).to(dtype).cuda().t()
    x = torch.randn(6, cols, generator=g).to(dtype).cuda()
    fails += _run_norm(kind, x, w, None, dy_t, 'nobias-transposed-dy')[1]
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('dtype', [BF16, FP16, FP32], ids=lambda d: NAME[d])
@pytest.mark.parametrize('cols', [520, 768])
@pytest.mark.parametrize('kind', ['layer_norm', 'rms_norm'])
def test_norm_backward_aligned_dy(kind, cols, dtype):
    """dy = xhat: mean(dy*w*xhat) is ~1 instead of ~cols^-1/2 as for a random dy, and dx is
    what is left after gw - xhat*c1 cancels, so a small error in c1 (a wrong divisor, a
    dropped lane) shows in dx at 16-bit precision."""
    g = _gen(cols + 1)
    rows = 9
    x = torch.randn(rows, cols, generator=g).to(dtype).cuda()
    w, b = _norm_params(cols, dtype, g)
    xhat = _norm_compose(kind == 'rms_norm')(x.cpu().to(FP64), torch.ones(cols, dtype=FP64))
    dy = xhat.to(dtype).cuda()
    _, fails = _run_norm(kind, x, w, b, dy, f'aligned-dy-{cols}')
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('dtype', [FP32, BF16], ids=lambda d: NAME[d])
@pytest.mark.parametrize('offset,std', [(0, 1.0), (8, 1.0), (32, 1.0), (100, 1.0), (64, 0.5)])
@pytest.mark.parametrize('kind', ['layer_norm', 'rms_norm'])
def test_norm_offset_rows(kind, offset, std, dtype):
    """|mean| >> std: a one-pass E[x^2] - mean^2 variance cancels here."""
    g = _gen(offset)
    rows, cols = 64, 768
    x = (offset + std * torch.randn(rows, cols, generator=g)).to(dtype).cuda()
    w, b = _norm_params(cols, dtype, g)
    dy = torch.randn(rows, cols, generator=g).to(dtype).cuda()
    _, fails = _run_norm(kind, x, w, b, dy, f'offset{offset}-std{std}')
    assert not fails, '\n'.join(fails)


CONSTANTS = [0.0, 0.1, 3.3, 300.3, 1000.7]


@pytest.mark.parametrize('dtype', [FP32, FP16, BF16], ids=lambda d: NAME[d])
@pytest.mark.parametrize('cols', [768, 100])
@pytest.mark.parametrize('kind', ['layer_norm', 'rms_norm'])
def test_norm_constant_rows(kind, cols, dtype):
    """Exactly constant rows: variance 0, so LN must return the bias and nothing may be NaN."""
    g = _gen(cols)
    x = torch.tensor(CONSTANTS).view(-1, 1).expand(-1, cols).contiguous().to(dtype).cuda()
    w, b = _norm_params(cols, dtype, g)
    dy = torch.randn(len(CONSTANTS), cols, generator=g).to(dtype).cuda()
    y, fails = _run_norm(kind, x, w, b, dy, f'const-{cols}')
    assert torch.isfinite(y.float()).all(), f'non-finite output rows: {(~torch.isfinite(y.float())).any(-1).tolist()}'
    if kind == 'layer_norm':
        b64 = b.cpu().to(FP64).expand_as(y)
        _check(fails, 'layer_norm.y', f'const-{cols}-vs-bias', y, b64, b64, dtype, _row_rms(b64))
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('const', [3.3, 300.3])
@pytest.mark.parametrize('kind', ['layer_norm', 'rms_norm'])
def test_norm_near_constant_rows(kind, const):
    g = _gen(11)
    rows, cols = 16, 768
    x = (const + 1e-3 * torch.randn(rows, cols, generator=g)).cuda()
    w, b = _norm_params(cols, FP32, g)
    dy = torch.randn(rows, cols, generator=g).cuda()
    y, fails = _run_norm(kind, x, w, b, dy, f'near-const-{const}')
    assert torch.isfinite(y).all()
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('dtype', [FP32, BF16], ids=lambda d: NAME[d])
@pytest.mark.parametrize('kind', ['layer_norm', 'rms_norm'])
def test_norm_zero_row_in_batch(kind, dtype):
    g = _gen(13)
    rows, cols = 7, 768
    x = torch.randn(rows, cols, generator=g)
    x[4] = 0.0
    x = x.to(dtype).cuda()
    w, b = _norm_params(cols, dtype, g)
    dy = torch.randn(rows, cols, generator=g).to(dtype).cuda()
    y, fails = _run_norm(kind, x, w, b, dy, 'zero-row')
    assert torch.isfinite(y.float()).all()
    if kind == 'layer_norm':
        assert torch.equal(y[4], b), 'all-zero row must return the bias exactly'
    else:
        assert (y[4] == 0).all()
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('dtype', [FP32, BF16], ids=lambda d: NAME[d])
def test_layer_norm_saved_stats(dtype):
    """mean/rstd as saved for the backward, against fp64 with the fp32 part of the bound."""
    ext = _ext()
    g = _gen(17)
    rows, cols = 64, 768
    x = (32 + torch.randn(rows, cols, generator=g)).to(dtype).cuda()
    w, b = _norm_params(cols, dtype, g)
    y, mean, rstd = ext.layer_norm_fwd(x, w, b, EPS)
    assert mean.dtype == FP32 and rstd.dtype == FP32 and mean.shape == (rows,) and rstd.shape == (rows,)

    def stats(t):
        m = t.mean(-1)
        return m, torch.rsqrt((t - m[:, None]).pow(2).mean(-1) + EPS)
    m64, r64 = stats(x.cpu().to(FP64))
    m32, r32 = stats(x.cpu().to(FP32))
    fails = []
    _check(fails, 'layer_norm.mean', 'offset32', mean, m64, m32, FP32)
    _check(fails, 'layer_norm.rstd', 'offset32', rstd, r64, r32, FP32)
    assert not fails, '\n'.join(fails)


# ---------------------------------------------------------------------------
# bias_act
# ---------------------------------------------------------------------------

ACTS = ['gelu', 'gelu_tanh', 'silu', 'relu', 'identity', 'quick_gelu']
BA_COLS = [8, 100, 520, 1032, 2056, 3072, 4096, 4104]


def _run_bias_act(act, x, b, dy, tag, fails):
    _ext()
    dtype = x.dtype
    x1 = x.detach().clone().requires_grad_(True)
    b1 = b.detach().clone().requires_grad_(True)
    y = ops.bias_act(x1, b1, act)
    assert y.dtype == dtype and y.shape == x.shape

    def fn(xx, bb):
        return _act_eager(xx + bb, act)
    if dy is None:
        with torch.no_grad():
            y64 = fn(x.cpu().to(FP64), b.cpu().to(FP64))
            y32 = fn(x.cpu().to(FP32), b.cpu().to(FP32))
        _check(fails, 'bias_act.y', f'{act}-{tag}', y, y64, y32, dtype)
        return
    y.backward(dy)
    y64, g64 = _reference(fn, (x, b), dy, FP64)
    y32, g32 = _reference(fn, (x, b), dy, FP32)
    _check(fails, 'bias_act.y', f'{act}-{tag}', y, y64, y32, dtype)
    _check(fails, 'bias_act.dx', f'{act}-{tag}', x1.grad, g64[0], g32[0], dtype)
    _check(fails, 'bias_act.db', f'{act}-{tag}', b1.grad, g64[1], g32[1], dtype, _col_rms(g64[0]))
    if act in ('relu', 'identity'):
        # exact in any precision: one rounding of x+b, gradient is dy or 0
        if not torch.equal(y.cpu(), y64.to(dtype)):
            fails.append(f'bias_act.y {act}-{tag}: not bit-exact')
        if not torch.equal(x1.grad.cpu(), g64[0].to(dtype)):
            fails.append(f'bias_act.dx {act}-{tag}: not bit-exact')


@pytest.mark.parametrize('dtype', [BF16, FP16], ids=lambda d: NAME[d])
@pytest.mark.parametrize('cols', BA_COLS)
def test_bias_act_shapes(cols, dtype):
    rows = [1, 3, 5][(BA_COLS.index(cols) + (dtype == FP16)) % 3]
    g = _gen(cols)
    x = (2 * torch.randn(rows, cols, generator=g)).to(dtype).cuda()
    b = torch.randn(cols, generator=g).to(dtype).cuda()
    dy = torch.randn(rows, cols, generator=g).to(dtype).cuda()
    fails = []
    for act in ACTS:
        _run_bias_act(act, x, b, dy, f'{rows}x{cols}', fails)
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('rows,cols,dtype', [
    (2563, 520, BF16),   # fast bwd caps at 640 blocks of 4 rows
    (2563, 108, FP16),   # slow bwd caps at 1024 blocks of 256 elements
], ids=lambda v: NAME.get(v, str(v)))
def test_bias_act_many_rows(rows, cols, dtype):
    g = _gen(rows + cols)
    x = (2 * torch.randn(rows, cols, generator=g)).to(dtype).cuda()
    b = torch.randn(cols, generator=g).to(dtype).cuda()
    dy = torch.randn(rows, cols, generator=g).to(dtype).cuda()
    fails = []
    for act in ('gelu', 'relu'):
        _run_bias_act(act, x, b, dy, f'{rows}x{cols}', fails)
    assert not fails, '\n'.join(fails)


def test_bias_act_forward_grid_stride():
    """1025 x 4104 > 2048 blocks * 256 threads * 8 elements; cols % 8 == 0 so the vector path strides."""
    g = _gen(3)
    x = (2 * torch.randn(1025, 4104, generator=g)).to(BF16).cuda()
    b = torch.randn(4104, generator=g).to(BF16).cuda()
    fails = []
    _run_bias_act('gelu', x, b, None, '1025x4104', fails)
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('dtype', [BF16, FP16], ids=lambda d: NAME[d])
def test_bias_act_saturation(dtype):
    """x + b on the grid k/4, k = -120..120 (|x+b| <= 30), with +0 and -0 sums."""
    grid = torch.arange(-120, 121, dtype=FP32) * 0.25
    cols = 248
    target = torch.zeros(cols)
    target[:241] = grid
    b = torch.tensor([0.0, -0.0, 0.25, -0.5]).repeat(cols // 4)
    x = torch.stack([target - b, -target - b, target - b])
    x[:, 241] = -0.0          # b[241] is -0.0: the sum is -0
    assert (x + b).abs().max() <= 30
    x, b = x.to(dtype).cuda(), b.to(dtype).cuda()
    assert torch.equal((x.float() + b.float())[0, :241].cpu(), grid), 'grid must be exact in the dtype'
    dy = torch.randn(3, cols, generator=_gen(5)).to(dtype).cuda()
    fails = []
    for act in ACTS:
        _run_bias_act(act, x, b, dy, 'sweep30', fails)
    assert not fails, '\n'.join(fails)


# ---------------------------------------------------------------------------
# residual_scale_add
# ---------------------------------------------------------------------------

def _residual_compose(keep):
    def fn(x, y, gamma=None):
        t = y if gamma is None else y * gamma
        if keep is not None:
            t = t * keep.to(t.dtype).view(-1, *([1] * (x.ndim - 1)))
        return x + t
    return fn


def _floor_mag(t, lo=2.0 ** -6):
    """Keep |t| >= lo: dy = dout * gamma * keep is a pure product, and with both factors
    free to be tiny it lands in fp16's subnormal range, where rounding is absolute
    (2^-25) and a bound relative to |ref64| cannot hold for any implementation."""
    return torch.where(t < 0, -1.0, 1.0) * t.abs().clamp(min=lo)


def _run_residual(shape, dtype, has_gamma, keep, tag, fails, seed=0):
    _ext()
    g = _gen(seed + shape[-1])
    x = torch.randn(shape, generator=g).to(dtype).cuda()
    y = torch.randn(shape, generator=g).to(dtype).cuda()
    gamma = _floor_mag(0.5 * torch.randn(shape[-1], generator=g)).to(dtype).cuda() if has_gamma else None
    dout = _floor_mag(torch.randn(shape, generator=g)).to(dtype).cuda()
    keep_dev = None if keep is None else keep.cuda()

    x1 = x.clone().requires_grad_(True)
    y1 = y.clone().requires_grad_(True)
    g1 = None if gamma is None else gamma.clone().requires_grad_(True)
    out = _ResidualScaleAddFn.apply(x1, y1, g1, keep_dev)
    out.backward(dout)

    inputs = (x, y, gamma) if has_gamma else (x, y)
    keep64 = None if keep is None else keep.to(FP64)
    o64, g64 = _reference(_residual_compose(keep64), inputs, dout, FP64)
    o32, g32 = _reference(_residual_compose(keep), inputs, dout, FP32)
    _check(fails, 'residual.out', tag, out, o64, o32, dtype)
    _check(fails, 'residual.dy', tag, y1.grad, g64[1], g32[1], dtype)
    if has_gamma:
        terms = dout.cpu().to(FP64) * y.cpu().to(FP64)
        if keep is not None:
            terms = terms * keep64.view(-1, *([1] * (len(shape) - 1)))
        _check(fails, 'residual.dgamma', tag, g1.grad, g64[2], g32[2], dtype, _col_rms(terms))
    if not torch.equal(x1.grad, dout):
        fails.append(f'residual.dx {tag}: dx must be dout bit-for-bit')
    if keep is not None:
        dropped = (keep == 0).cuda()
        if not torch.equal(out[dropped], x[dropped]):
            fails.append(f'residual.out {tag}: dropped samples must return x bit-for-bit')
        if not (y1.grad[dropped] == 0).all():
            fails.append(f'residual.dy {tag}: dropped samples must get exactly zero gradient')


def _keep(B, flip):
    k = torch.full((B,), 1 / 0.7, dtype=FP32)
    k[(1 - flip)::2] = 0.0    # flip=0: odd samples dropped; flip=1: even samples (incl. sample 0)
    return k


@pytest.mark.parametrize('dtype', [BF16, FP16], ids=lambda d: NAME[d])
@pytest.mark.parametrize('shape', [
    (5, 7, 768),
    (1, 3, 8),
    (6, 100),          # 2-D, cols % 8 != 0: scalar forward
    (3, 4, 5, 96),     # 4-D
    (3, 115, 768),     # 264960 elements > 1024 blocks * 256: backward grid-strides
], ids=lambda s: 'x'.join(map(str, s)))
def test_residual_scale_add_kernels(shape, dtype):
    fails = []
    for has_gamma in (True, False):
        _run_residual(shape, dtype, has_gamma, None, f'gamma={has_gamma}-nokeep', fails)
        for flip in (0, 1):
            _run_residual(shape, dtype, has_gamma, _keep(shape[0], flip),
                          f'gamma={has_gamma}-keep{flip}', fails)
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('has_gamma', [True, False])
def test_residual_scale_add_public_drop_path(has_gamma):
    """The public wrapper draws the mask itself; the same seed reproduces it."""
    _ext()
    shape, dtype, p = (64, 3, 96), BF16, 0.3
    g = _gen(23)
    x = torch.randn(shape, generator=g).to(dtype).cuda()
    y = torch.randn(shape, generator=g).to(dtype).cuda()
    gamma = (0.5 * torch.randn(shape[-1], generator=g)).to(dtype).cuda() if has_gamma else None
    torch.manual_seed(1234)
    out = ops.residual_scale_add(x, y, gamma, drop_prob=p, training=True)
    torch.manual_seed(1234)
    keep = torch.empty(shape[0], device='cuda', dtype=FP32).bernoulli_(1 - p) / (1 - p)
    keep = keep.cpu()
    assert (keep == 0).any() and (keep != 0).any()
    inputs = (x, y, gamma) if has_gamma else (x, y)
    with torch.no_grad():
        o64 = _residual_compose(keep.to(FP64))(*[t.cpu().to(FP64) for t in inputs])
        o32 = _residual_compose(keep)(*[t.cpu().to(FP32) for t in inputs])
    fails = []
    _check(fails, 'residual.out', f'public-gamma={has_gamma}', out, o64, o32, dtype)
    assert torch.equal(out[(keep == 0).cuda()], x[(keep == 0).cuda()])
    # eval mode and drop_prob=0 draw nothing
    out_eval = ops.residual_scale_add(x, y, gamma, drop_prob=p, training=False)
    with torch.no_grad():
        e64 = _residual_compose(None)(*[t.cpu().to(FP64) for t in inputs])
        e32 = _residual_compose(None)(*[t.cpu().to(FP32) for t in inputs])
    _check(fails, 'residual.out', f'public-eval-gamma={has_gamma}', out_eval, e64, e32, dtype)
    assert not fails, '\n'.join(fails)


# ---------------------------------------------------------------------------
# depthwise conv (bf16, channels-last)
# ---------------------------------------------------------------------------

DW_CASES = [
    # C,  H,  W, K, stride, pad
    (8, 5, 9, 3, 1, 1),      # row-sliding weight kernel at K=3, single 8-channel chunk
    (144, 9, 6, 5, 2, 2),    # generic kMaxK=5 at stride 2; 2nd channel super-chunk holds 2 of 16
    (136, 7, 4, 7, 2, 3),    # generic kMaxK=7 at stride 2; 2nd super-chunk holds 1 of 16
    (24, 11, 6, 9, 1, 4),    # row-sliding at K=9
    (16, 6, 10, 4, 1, 1),    # even K: generic kernel, K=4 under kMaxK=5
    (32, 15, 9, 3, 2, 1),    # odd size with stride 2
    (16, 3, 4, 7, 1, 3),     # image smaller than the kernel
    (64, 8, 5, 5, 1, 0),     # no padding; Ho*Wo = 4, so B*Ho*Wo < 16 for B = 1 and 3
    (64, 6, 9, 3, 1, 2),     # over-padded: output larger than input
]


def _dw_compose(stride, pad, dilation=1):
    def fn(x, w, b=None):
        return F.conv2d(x, w, b, stride, pad, dilation, groups=x.shape[1])
    return fn


def _run_dwconv(B, C, H, W, K, stride, pad, has_bias, dy_mode, fails, dilation=1, expect_hip=True):
    _ext()
    tag = f'B{B}-C{C}-{H}x{W}-K{K}-s{stride}-p{pad}-bias={has_bias}-dy={dy_mode}' \
          + (f'-d{dilation}' if dilation != 1 else '')
    g = _gen(C * 1000 + H * 10 + K)
    x = torch.randn(B, C, H, W, generator=g).to(BF16).cuda().contiguous(memory_format=torch.channels_last)
    w = (torch.randn(C, 1, K, K, generator=g) / K).to(BF16).cuda()
    b = torch.randn(C, generator=g).to(BF16).cuda() if has_bias else None
    x1 = x.detach().requires_grad_(True)
    w1 = w.clone().requires_grad_(True)
    b1 = None if b is None else b.clone().requires_grad_(True)
    y = ops.depthwise_conv2d(x1, w1, b1, stride=stride, padding=pad, dilation=dilation)
    Ho = (H + 2 * pad - dilation * (K - 1) - 1) // stride + 1
    Wo = (W + 2 * pad - dilation * (K - 1) - 1) // stride + 1
    assert y.shape == (B, C, Ho, Wo) and y.dtype == BF16, tag
    if expect_hip:
        assert type(y.grad_fn).__name__.startswith('_DepthwiseConvFn'), f'{tag}: HIP path not taken'
    else:
        assert not type(y.grad_fn).__name__.startswith('_DepthwiseConvFn'), f'{tag}: expected F.conv2d'

    if dy_mode == 'sum':
        dy = torch.ones_like(y)
        y.sum().backward()
    else:
        dy = torch.randn(B, C, Ho, Wo, generator=g).to(BF16).cuda()
        if dy_mode == 'nhwc':
            dy = dy.contiguous(memory_format=torch.channels_last)
        y.backward(dy)

    inputs = (x, w, b) if has_bias else (x, w)
    fn = _dw_compose(stride, pad, dilation)
    y64, g64 = _reference(fn, inputs, dy, FP64)
    y32, g32 = _reference(fn, inputs, dy, FP32)
    # RMS of the B*Ho*Wo terms summed into each dw tap: sum dy^2 x^2 is the same
    # weight gradient taken on squared inputs
    x_sq = x.cpu().to(FP64).pow(2)
    w0 = torch.zeros(C, 1, K, K, dtype=FP64, requires_grad=True)
    fn(x_sq, w0).backward(dy.cpu().to(FP64).pow(2))
    s_dw = (w0.grad / (B * Ho * Wo)).sqrt()
    s_db = dy.cpu().to(FP64).pow(2).mean((0, 2, 3)).sqrt()

    _check(fails, 'dwconv.y', tag, y, y64, y32, BF16)
    _check(fails, 'dwconv.dx', tag, x1.grad, g64[0], g32[0], BF16)
    _check(fails, 'dwconv.dw', tag, w1.grad, g64[1], g32[1], BF16, s_dw)
    if has_bias:
        _check(fails, 'dwconv.dbias', tag, b1.grad, g64[2], g32[2], BF16, s_db)


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('case', DW_CASES, ids=lambda c: 'C{}-{}x{}-K{}-s{}-p{}'.format(*c))
def test_depthwise_conv_edges(case, B):
    fails = []
    for has_bias in (True, False):
        for dy_mode in ('nhwc', 'nchw', 'sum'):
            _run_dwconv(B, *case, has_bias, dy_mode, fails)
    assert not fails, '\n'.join(fails)


def test_depthwise_conv_dilation_falls_back():
    """dilation=2 is not implemented in HIP: the op must route to F.conv2d and still match."""
    fails = []
    _run_dwconv(2, 16, 9, 7, 3, 1, 2, True, 'nhwc', fails, dilation=2, expect_hip=False)
    assert not fails, '\n'.join(fails)
