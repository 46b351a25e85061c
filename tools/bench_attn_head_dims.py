#!/usr/bin/env python3
"""Microbenchmark: attention at head dims that are no multiple of 32.

`--path` picks what runs for one of the shapes below:

    composition   `_math_sdpa` forward + autograd backward: fp32 [B,H,N,N]
                  scores and softmax in HBM (what these shapes ran before the
                  kernels of csrc/attention_head_dims.hip existed)
    padded        F.pad of q/k/v (or the packed qkv) to the next multiple of 32,
                  the D % 32 == 0 kernels with scale = D**-0.5, and a slice;
                  the pad copies are inside the timing
    native        ops.flash_attention / ops.flash_attention_qkv as they are

Shapes (`--shape`, a comma-separated list, or `all` for one JSON line each):

    so400m_384   64 x 16 x 729 x 72, packed [B,N,3,H,D] qkv
    so400m_224   256 x 16 x 256 x 72, packed
    vith14       64 x 16 x 257 x 80
    vitg14       32 x 16 x 257 x 88
    cait_s       256 x 8 x 197 x 48

One path per process, so each GPU step can run under its own `timeout`:

    timeout -k 10 300 python tools/bench_attn_head_dims.py --path native --shape all

Timing is device events, 10 warmup + 50 timed, around the forward alone and
around one forward+backward; these are host-launched call times.  Each line
also carries torch.cuda.max_memory_allocated over the forward+backward runs
(reset after the inputs exist).
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {
    'so400m_384': dict(B=64, H=16, N=729, D=72, packed=True),
    'so400m_224': dict(B=256, H=16, N=256, D=72, packed=True),
    'vith14': dict(B=64, H=16, N=257, D=80, packed=False),
    'vitg14': dict(B=32, H=16, N=257, D=88, packed=False),
    'cait_s': dict(B=256, H=8, N=197, D=48, packed=False),
}
PATHS = ['composition', 'padded', 'native']


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
    pad = (0, -D % 32)
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    if s['packed']:
        inputs = (torch.randn(B, N, 3, H, D, device=dev, dtype=torch.bfloat16).requires_grad_(True),)
    else:
        inputs = tuple(torch.randn(B, H, N, D, device=dev, dtype=torch.bfloat16).requires_grad_(True)
                       for _ in range(3))

    def fwd():
        if args.path == 'native':
            return ops.flash_attention_qkv(*inputs) if s['packed'] else ops.flash_attention(*inputs)
        if args.path == 'padded':
            padded = [F.pad(t, pad) for t in inputs]
            o = (ops.flash_attention_qkv(*padded, scale=D ** -0.5) if s['packed']
                 else ops.flash_attention(*padded, scale=D ** -0.5))
            return o[..., :D]
        q, k, v = inputs[0].permute(2, 0, 3, 1, 4).unbind(0) if s['packed'] else inputs
        return attn_mod._math_sdpa(q, k, v)

    with torch.no_grad():
        do = torch.randn_like(fwd())  # the layout of O
        fw = _timed(fwd, args.warmup, args.iters)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fb = _timed(lambda: torch.autograd.grad(fwd(), inputs, do), args.warmup, args.iters)
    peak = torch.cuda.max_memory_allocated()
    return {
        'shape': name, 'B': B, 'H': H, 'N': N, 'D': D, 'packed': s['packed'],
        'path': args.path, 'dtype': 'bf16', 'iters': args.iters, 'warmup': args.warmup,
        'fwd': fw, 'fwd_bwd': fb,
        'inputs_and_dO_bytes': base, 'peak_allocated_bytes': peak,
        'peak_above_inputs_MB': round((peak - base) / 2 ** 20, 1),
    }


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--path', choices=PATHS, required=True)
    p.add_argument('--shape', default='all', help="a shape name, a comma-separated list, or 'all'")
    p.add_argument('--warmup', type=int, default=10)
    p.add_argument('--iters', type=int, default=50)
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_attn_head_dims.py needs a GPU')
    import timm_amd  # noqa: F401
    from timm_amd import ops
    from timm_amd.ops import attention as attn_mod
    assert ops.has_ext(), 'timm_amd._C HIP extension must be built'
    names = list(SHAPES) if args.shape == 'all' else args.shape.split(',')
    assert all(n in SHAPES for n in names), names
    for name in names:
        print(json.dumps(run_shape(name, args, ops, attn_mod)), flush=True)


if __name__ == '__main__':
    main()
