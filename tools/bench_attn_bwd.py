#!/usr/bin/env python3
"""Microbenchmark: fused attention backward, single-pass against two-pass.

`--path` forces which fused backward `ops.flash_attention` /
`ops.flash_attention_qkv` run (`ops.attention.set_attn_bwd_path`):

    two_pass                dQ pass + dK/dV pass behind attn_bwd_preprocess
    single_pass             one workgroup per (batch, head), delta in the kernel
    single_pass_preprocess  the same kernel fed by attn_bwd_preprocess
    auto                    the rule in timm_amd/ops/attention.py

Shapes (`--shape`, or `--shape all` for one JSON line each):

    vitb_packed   256 x 12 x 197 x 64, packed [B,N,3,H,D] qkv (the bench.py block)
    vitl          128 x 16 x 197 x 64, separate q, k, v
    vitb_bias     256 x 12 x 197 x 64 with a [1,H,N,N] bias (no bias gradient)
    win49 / win64 / win144   window attention at head_dim 64: 4096 x 4 x 49,
                  2048 x 4 x 64, 1024 x 4 x 144 (Swin's own head_dim 32 is not
                  a single-pass shape and stays two-pass)
    win49_bias / win64_bias / n100_bias / win144_bias   the same window shapes
                  (and 512 x 12 x 100) with a [1,H,N,N] rel-pos bias
    win49_shift / win144_shift   with a cyclic [64|16,H,N,N] bias + shift mask
    long577       64 x 16 x 577 x 64: Nk > 256, two-pass whatever is forced

One path per process, so each GPU step can run under its own `timeout`:

    timeout -k 10 120 python tools/bench_attn_bwd.py --path two_pass --shape all
    timeout -k 10 120 python tools/bench_attn_bwd.py --path single_pass --shape all

Timing is device events, 10 warmup + 50 timed, around one forward+backward and
around the backward alone (the forward's graph is kept).  For the backward the
line also gives the bytes the algorithm needs (q, k, v, dO, O in; dq, dk, dv
out) over the median against the 6.29 TB/s measured-copy roof, and the useful
FLOPs (10 B H Nq Nk D) over the median against the 2.5 PFLOP/s bf16 MFMA roof.
These are host-launched call times: they include launch gaps and autograd
bookkeeping; kernel times come from the kernel trace.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_ROOF_TBS = 6.29
MFMA_ROOF_TFLOPS = 2500.0

SHAPES = {
    # bias: 0 = none, m = additive fp32 [m, H, N, N] mask (no gradient), read as mask[b % m]
    'vitb_packed': dict(B=256, H=12, N=197, D=64, packed=True, bias=0),
    'vitl': dict(B=128, H=16, N=197, D=64, packed=False, bias=0),
    'vitb_bias': dict(B=256, H=12, N=197, D=64, packed=False, bias=1),
    'win49': dict(B=4096, H=4, N=49, D=64, packed=False, bias=0),
    'win64': dict(B=2048, H=4, N=64, D=64, packed=False, bias=0),
    'win144': dict(B=1024, H=4, N=144, D=64, packed=False, bias=0),
    'win49_bias': dict(B=4096, H=4, N=49, D=64, packed=False, bias=1),
    'win49_shift': dict(B=4096, H=4, N=49, D=64, packed=False, bias=64),
    'win64_bias': dict(B=2048, H=4, N=64, D=64, packed=False, bias=1),
    'n100_bias': dict(B=512, H=12, N=100, D=64, packed=False, bias=1),
    'win144_bias': dict(B=1024, H=4, N=144, D=64, packed=False, bias=1),
    'win144_shift': dict(B=1024, H=4, N=144, D=64, packed=False, bias=16),
    'long577': dict(B=64, H=16, N=577, D=64, packed=False, bias=0),
}
PATHS = ['auto', 'two_pass', 'single_pass', 'single_pass_preprocess']


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument('--path', choices=PATHS, required=True)
    p.add_argument('--shape', default='all', help="a shape name, a comma-separated list, or 'all'")
    p.add_argument('--warmup', type=int, default=10)
    p.add_argument('--iters', type=int, default=50)
    return p.parse_args()


def _timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1) * 1e3)  # us
    times.sort()
    q1, _, q3 = statistics.quantiles(times, n=4)
    return {'median_us': round(statistics.median(times), 1), 'min_us': round(times[0], 1),
            'max_us': round(times[-1], 1), 'q1_us': round(q1, 1), 'q3_us': round(q3, 1)}


def run_shape(name, args, ops, attn_mod):
    s = SHAPES[name]
    B, H, N, D = s['B'], s['H'], s['N'], s['D']
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    bias = torch.randn(s['bias'], H, N, N, device=dev) if s['bias'] else None
    if s['packed']:
        qkv = torch.randn(B, N, 3, H, D, device=dev, dtype=torch.bfloat16).requires_grad_(True)
        inputs = (qkv,)

        def fwd():
            return ops.flash_attention_qkv(qkv, attn_mask=bias)
    else:
        q, k, v = [torch.randn(B, H, N, D, device=dev, dtype=torch.bfloat16).requires_grad_(True)
                   for _ in range(3)]
        inputs = (q, k, v)

        def fwd():
            return ops.flash_attention(q, k, v, attn_mask=bias)

    o = fwd()
    # dO in the layout of O (BNHD storage on the packed path)
    do = torch.randn_like(o)

    before = dict(attn_mod.BWD_PATH_CALLS)
    fb = _timed(lambda: torch.autograd.grad(fwd(), inputs, do), args.warmup, args.iters)
    o = fwd()
    bw = _timed(lambda: torch.autograd.grad(o, inputs, do, retain_graph=True),
                args.warmup, args.iters)
    ran = [p for p in attn_mod.BWD_PATH_CALLS if attn_mod.BWD_PATH_CALLS[p] > before[p]]

    need_bytes = 8 * B * H * N * D * 2
    flops = 10 * B * H * N * N * D
    med = bw['median_us'] * 1e-6
    return {
        'shape': name, 'B': B, 'H': H, 'N': N, 'D': D, 'packed': s['packed'], 'bias': s['bias'],
        'path': args.path, 'kernels_ran': ran, 'dtype': 'bf16',
        'iters': args.iters, 'warmup': args.warmup,
        'fwd_bwd': fb, 'bwd': bw,
        'bwd_needed_bytes': need_bytes, 'bwd_TBps': round(need_bytes / med / 1e12, 3),
        'bwd_share_of_hbm_roof': round(need_bytes / med / 1e12 / HBM_ROOF_TBS, 3),
        'bwd_useful_flops': flops, 'bwd_TFLOPs': round(flops / med / 1e12, 1),
        'bwd_share_of_mfma_roof': round(flops / med / 1e12 / MFMA_ROOF_TFLOPS, 4),
    }


def main():
    args = parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_attn_bwd.py needs a GPU')
    import timm_amd  # noqa: F401
    from timm_amd import ops
    from timm_amd.ops import attention as attn_mod
    assert ops.has_ext(), 'timm_amd._C HIP extension must be built'
    attn_mod.set_attn_bwd_path(None if args.path == 'auto' else args.path)
    names = list(SHAPES) if args.shape == 'all' else args.shape.split(',')
    assert all(n in SHAPES for n in names), names
    for name in names:
        print(json.dumps(run_shape(name, args, ops, attn_mod)), flush=True)


if __name__ == '__main__':
    main()
