#!/usr/bin/env python3
"""Microbenchmark: flash_attention forward+backward with a learned additive bias.

`--impl fused` is `ops.flash_attention` (flash fwd, dQ/dKdV passes and the
dBias pass); `--impl eager` is the bf16 `softmax(q k^T * scale + bias) @ v`
composition that a model runs with fused attention switched off.  Default shape
is the Swin-B stage-1 window attention at batch 64: B_=4096 windows, H=4, N=49,
D=32, bias [mB, H, N, N] with mB=1 (unshifted block) or 64 (shifted block,
bias + shift mask).  BEiT-B is `--batch 64 --heads 12 --tokens 197 --head-dim 64`.

One implementation per process, so each GPU step can run under its own
`timeout`:

    timeout -k 10 120 python tools/bench_attn_bias.py --impl fused
    timeout -k 10 120 python tools/bench_attn_bias.py --impl eager --mask-batch 64

`--nsplit N` overrides the dBias split heuristic (fused only), `--frozen` times
the same call with a bias that needs no gradient (no dBias pass).  Timing is
device events around one forward+backward, after warmup; the result line gives
the median and the min/max/quartile spread over --iters repeats.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument('--impl', choices=['fused', 'eager'], required=True)
    p.add_argument('--batch', type=int, default=4096)
    p.add_argument('--heads', type=int, default=4)
    p.add_argument('--tokens', type=int, default=49)
    p.add_argument('--head-dim', type=int, default=32)
    p.add_argument('--mask-batch', type=int, default=1, help='mB: bias batch dim, divides --batch')
    p.add_argument('--nsplit', type=int, default=0, help='override the dBias split (0: heuristic)')
    p.add_argument('--frozen', action='store_true', help='bias without requires_grad')
    p.add_argument('--warmup', type=int, default=10)
    p.add_argument('--iters', type=int, default=30)
    return p.parse_args()


def main():
    args = parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_attn_bias.py needs a GPU')
    import timm_amd  # noqa: F401
    from timm_amd import ops
    from timm_amd.ops import attention as attn_mod
    assert ops.has_ext(), 'timm_amd._C HIP extension must be built'

    B, H, N, D, mB = args.batch, args.heads, args.tokens, args.head_dim, args.mask_batch
    assert B % mB == 0
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    q, k, v = [torch.randn(B, H, N, D, device=dev, dtype=torch.bfloat16).requires_grad_(True)
               for _ in range(3)]
    bias = (torch.randn(mB, H, N, N, device=dev) * 2.0).requires_grad_(not args.frozen)
    do = torch.randn(B, H, N, D, device=dev, dtype=torch.bfloat16)
    scale = 1.0 / math.sqrt(D)

    if args.impl == 'fused':
        assert ops.attention_available(q)
        nsplit = attn_mod._mask_nsplit(q, k, bias)
        if args.nsplit > 0:
            nsplit = args.nsplit
            attn_mod.set_dbias_nsplit(args.nsplit)

        def fwd():
            return ops.flash_attention(q, k, v, attn_mask=bias, scale=scale)
    else:
        nsplit = None

        def fwd():
            attn = (q @ k.transpose(-2, -1)) * scale
            if mB not in (1, B):
                attn = (attn.view(B // mB, mB, H, N, N) + bias.to(attn.dtype)).view(B, H, N, N)
            else:
                attn = attn + bias.to(attn.dtype)
            return attn.softmax(dim=-1) @ v

    inputs = (q, k, v) if args.frozen else (q, k, v, bias)

    def step():
        return torch.autograd.grad(fwd(), inputs, do)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.iters):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        step()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1) * 1e3)  # us
    times.sort()
    med = statistics.median(times)
    q1, _, q3 = statistics.quantiles(times, n=4)
    print(json.dumps({
        'impl': args.impl, 'bias_requires_grad': not args.frozen, 'nsplit': nsplit,
        'shape': {'B': B, 'H': H, 'N': N, 'D': D, 'mB': mB},
        'dtype': 'bf16', 'bias': 'fp32', 'what': 'forward+backward, device events',
        'iters': args.iters, 'warmup': args.warmup,
        'median_us': round(med, 1), 'min_us': round(times[0], 1), 'max_us': round(times[-1], 1),
        'q1_us': round(q1, 1), 'q3_us': round(q3, 1),
    }))


if __name__ == '__main__':
    main()
