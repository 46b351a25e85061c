#!/usr/bin/env python3
"""Microbenchmark: attention with the decomposed rel-pos bias of SAM / ViTDet.

Times forward and forward+backward (gradients of qkv and of both tables) at
the two attention shapes of `samvit_base_patch16` at 1024^2, bf16, 12 heads,
head_dim 64, q/k/v as views of a packed [B,N,3,H,D] buffer:

    window   B = 25 (windows of one image), N = 196, grid 14x14
    global   B = 1, N = 4096, grid 64x64

for three arms that start from the same tables rel_h [B,H,N,Kh], rel_w [B,H,N,Kw]:

    rel_pos    ops.flash_attention(rel_pos_hw=(rel_h, rel_w)) -> the kernels of
               csrc/attention_rel_pos.hip
    sdpa       bias = rel_h[..., None] + rel_w[..., None, :] as bf16 [B,H,N,N],
               then F.scaled_dot_product_attention(attn_mask=bias): the route
               of the model before these kernels
    mask       the same bias through ops.flash_attention(attn_mask=bias): the
               additive-mask kernels and their dBias pass

The arms alternate inside one process, `--reps` rounds each of `--warmup` +
`--iters` calls timed with device events; a row gives the median over the
rounds of the per-round medians and `spread_us`, the largest minus the
smallest per-round median.  `peak_bytes` is torch's peak allocation above the
inputs over one forward+backward.  Host-launched call times (launch gaps and
autograd bookkeeping included), not kernel times.

    timeout -k 10 600 python tools/bench_attn_rel_pos.py --out rows.jsonl
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, D = 12, 64
SHAPES = {'window': (25, 14), 'global': (1, 64)}  # B, grid side
ARMS = ('rel_pos', 'sdpa', 'mask')


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument('--shapes', default=','.join(SHAPES))
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--iters', type=int, default=30)
    p.add_argument('--reps', type=int, default=3)
    p.add_argument('--out', default=None, help='append the JSON rows to this file')
    return p.parse_args()


def _median_us(fn, warmup, iters):
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
        times.append(t0.elapsed_time(t1) * 1e3)
    return statistics.median(times)


def run_case(name, args, ops, attn_mod):
    B, side = SHAPES[name]
    N = side * side
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    qkv = torch.randn(B, N, 3, H, D, device=dev, dtype=torch.bfloat16).requires_grad_(True)
    rel_h, rel_w = [torch.randn(B, H, N, side, device=dev, dtype=torch.bfloat16).requires_grad_(True)
                    for _ in range(2)]
    leaves = (qkv, rel_h, rel_w)

    def attend(arm):
        q, k, v = [qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3)]
        if arm == 'rel_pos':
            return ops.flash_attention(q, k, v, rel_pos_hw=(rel_h, rel_w))
        bias = (rel_h[..., :, None] + rel_w[..., None, :]).reshape(B, H, N, N)
        if arm == 'sdpa':
            return F.scaled_dot_product_attention(q, k, v, attn_mask=bias)
        return ops.flash_attention(q, k, v, attn_mask=bias)

    do = torch.randn(B, H, N, D, device=dev, dtype=torch.bfloat16)
    with torch.no_grad():  # same result at the timed size
        o_ref = attend('sdpa').float()
        rel_diff = {arm: ((attend(arm).float() - o_ref).norm() / o_ref.norm()).item() for arm in ARMS}

    samples = {arm: {'fwd': [], 'fwd_bwd': []} for arm in ARMS}
    peak, ran = {}, {}
    for _ in range(args.reps):
        for arm in ARMS:
            before = dict(attn_mod.REL_POS_CALLS)

            def fwd():
                with torch.no_grad():
                    return attend(arm)

            def fwd_bwd():
                return torch.autograd.grad(attend(arm), leaves, do)

            samples[arm]['fwd'].append(_median_us(fwd, args.warmup, args.iters))
            samples[arm]['fwd_bwd'].append(_median_us(fwd_bwd, args.warmup, args.iters))
            ran[arm] = attn_mod.REL_POS_CALLS['bwd'] > before['bwd']
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fwd_bwd()
            torch.cuda.synchronize()
            peak[arm] = torch.cuda.max_memory_allocated() - base
    assert ran == {'rel_pos': True, 'sdpa': False, 'mask': False}, ran

    rows = []
    for arm in ARMS:
        row = {'shape': name, 'B': B, 'H': H, 'N': N, 'grid': side, 'D': D, 'arm': arm,
               'dtype': 'bf16', 'iters': args.iters, 'warmup': args.warmup, 'reps': args.reps,
               'peak_bytes': peak[arm], 'bias_bytes': B * H * N * N * 2,
               'fwd_rel_diff_vs_sdpa': float('%.3g' % rel_diff[arm])}
        for what in ('fwd', 'fwd_bwd'):
            s = samples[arm][what]
            row[what + '_us'] = round(statistics.median(s), 1)
            row[what + '_spread_us'] = round(max(s) - min(s), 1)
        rows.append(row)
    return rows


def main():
    args = parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_attn_rel_pos.py needs a GPU')
    import timm_amd  # noqa: F401
    from timm_amd import ops
    from timm_amd.ops import attention as attn_mod
    assert ops.has_ext(), 'timm_amd._C HIP extension must be built'
    for name in args.shapes.split(','):
        for row in run_case(name, args, ops, attn_mod):
            line = json.dumps(row)
            print(line, flush=True)
            if args.out:
                with open(args.out, 'a') as f:
                    f.write(line + '\n')


if __name__ == '__main__':
    main()
