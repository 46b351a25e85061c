#!/usr/bin/env python3
"""Microbenchmark: attention of one Swin W-MSA / SW-MSA block, forward+backward,
map in and map out, rel-pos bias trained, at the Swin-B stage shapes.

`--impl map` is `ops.window_attention` on the qkv Linear's output on the map;
`--impl partition` is the path it replaces for the same work, glue included:
roll -> window partition -> qkv Linear -> permute / unbind ->
`ops.flash_attention` with the [nW, heads, N, N] bias + shift mask -> window
reverse -> roll.  Both run the same qkv Linear.

One configuration per process, so each GPU step can run under its own
`timeout`:

    timeout -k 10 120 python tools/bench_window_attention.py --impl map --stage 1 --shift
    timeout -k 10 120 python tools/bench_window_attention.py --impl partition --stage 1 --shift

Timing is device events around one forward+backward, after warmup; the result
line gives the median and the min/max/quartile spread over --iters repeats.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = {1: (56, 4), 2: (28, 8), 3: (14, 16), 4: (7, 32)}  # Swin-B: map side, heads


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument('--impl', choices=['map', 'partition'], required=True)
    p.add_argument('--stage', type=int, choices=sorted(STAGES), default=1)
    p.add_argument('--batch', type=int, default=128)
    p.add_argument('--window', type=int, default=7)
    p.add_argument('--shift', action='store_true', help='SW-MSA block (shift = window // 2)')
    p.add_argument('--cosine', action='store_true',
                   help='SwinV2 block (cosine attention, log-CPB bias); see cosine_fwd()')
    p.add_argument('--img', type=int, default=256, help='--cosine: image side, map = img / 4 / 2^(stage-1)')
    p.add_argument('--warmup', type=int, default=10)
    p.add_argument('--iters', type=int, default=30)
    return p.parse_args()


def main():
    args = parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_window_attention.py needs a GPU')
    import timm_amd  # noqa: F401
    from timm_amd import ops
    from timm_amd.models.swin_transformer import SwinTransformerBlock, window_partition, window_reverse
    assert ops.has_ext(), 'timm_amd._C HIP extension must be built'

    side, heads = STAGES[args.stage]
    B, win, dim = args.batch, args.window, heads * 32
    if args.cosine:  # SwinV2-B stage shapes, window clamped to the map
        from timm_amd.models.swin_transformer_v2 import SwinTransformerV2Block
        side = args.img // 4 >> (args.stage - 1)
        win = min(win, side)
    shift = win // 2 if args.shift and side > win else 0
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    blk = (SwinTransformerV2Block if args.cosine else SwinTransformerBlock)(
        dim, (side, side), num_heads=heads, window_size=win, shift_size=shift).to(dev, torch.bfloat16)
    attn = blk.attn
    x = torch.randn(B, side, side, dim, device=dev, dtype=torch.bfloat16, requires_grad=True)
    do = torch.randn(B, side, side, dim, device=dev, dtype=torch.bfloat16)

    if args.cosine:
        # Both arms time the block's own `_attn` (qkv Linear + attention +
        # proj, map in and map out): `map` takes the cosine kernels,
        # `partition` is the same block with the gate shut, i.e. roll /
        # partition / normalize / flash_attention / reverse.
        if args.impl == 'partition':
            blk._map_attn_ok = lambda x: False
        inputs = (x, attn.qkv.weight, attn.q_bias, attn.v_bias, attn.logit_scale,
                  attn.cpb_mlp[0].weight, attn.proj.weight)

        def fwd():
            return blk._attn(x)
    elif args.impl == 'map':
        def fwd():
            return ops.window_attention(attn.qkv(x), heads, win, shift,
                                        bias=attn._get_rel_pos_bias()[0], scale=attn.scale)
    else:
        def fwd():
            xs = torch.roll(x, (-shift, -shift), (1, 2)) if shift else x
            xw = window_partition(xs, (win, win)).view(-1, win * win, dim)
            qkv = attn.qkv(xw).reshape(xw.shape[0], win * win, 3, heads, -1).permute(2, 0, 3, 1, 4)
            q, k, v = qkv.unbind(0)
            bias = attn._get_rel_pos_bias()
            if blk.attn_mask is not None:
                bias = bias + blk.attn_mask.unsqueeze(1)
            o = ops.flash_attention(q, k, v, attn_mask=bias, scale=attn.scale)
            o = o.transpose(1, 2).reshape(-1, win, win, dim)
            o = window_reverse(o, (win, win), side, side)
            return torch.roll(o, (shift, shift), (1, 2)) if shift else o

    if not args.cosine:
        inputs = (x, attn.qkv.weight, attn.qkv.bias, attn.relative_position_bias_table)

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
    q1, _, q3 = statistics.quantiles(times, n=4)
    print(json.dumps({
        'impl': args.impl, 'cosine': args.cosine, 'stage': args.stage, 'shift': shift,
        'shape': {'B': B, 'map': side, 'heads': heads, 'window': win, 'D': 32},
        'what': ('SwinV2 block _attn (qkv Linear + cosine window attention + proj)' if args.cosine
                 else 'qkv Linear + window attention') + ', forward+backward, device events',
        'iters': args.iters, 'warmup': args.warmup,
        'median_us': round(statistics.median(times), 1), 'min_us': round(times[0], 1),
        'max_us': round(times[-1], 1), 'q1_us': round(q1, 1), 'q3_us': round(q3, 1),
    }))


if __name__ == '__main__':
    main()
