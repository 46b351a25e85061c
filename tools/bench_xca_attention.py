#!/usr/bin/env python3
"""Microbenchmark: the layers of one XCiT XCA module (qkv Linear +
`ops.cross_covariance_attention` + proj), kernels (`fused`) against the
switched-off bf16 composition (`composed`, the ops of `XCA.forward`), at the
shapes of the XCiT entrypoints.

Both arms are the same layers on the same input; only `set_fused_xca` differs,
and the arms alternate repeat by repeat so that drift of the machine hits both.
One shape per process, so each GPU step can run under its own `timeout`:

    timeout -k 10 120 python tools/bench_xca_attention.py --model xcit_small_12_p16_224
    timeout -k 10 120 python tools/bench_xca_attention.py --model xcit_nano_12_p16_224 --batch 1 --forward-only

Timing is device events around one forward(+backward), after warmup; one JSON
line per arm gives the median and the min / max / quartile spread over --iters
repeats, a last line the ratio of the medians.  `--out` appends the lines to a
jsonl file as well.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# model: (tokens, dim, heads)
SHAPES = {
    'xcit_nano_12_p16_224': (196, 128, 4),     # head_dim 32
    'xcit_small_12_p16_224': (196, 384, 8),    # head_dim 48
    'xcit_medium_24_p16_224': (196, 512, 8),   # head_dim 64
    'xcit_small_12_p8_224': (784, 384, 8),     # head_dim 48, p8 length
}


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument('--model', choices=sorted(SHAPES), default='xcit_small_12_p16_224')
    p.add_argument('--batch', type=int, default=128)
    p.add_argument('--forward-only', action='store_true')
    p.add_argument('--warmup', type=int, default=10)
    p.add_argument('--iters', type=int, default=30)
    p.add_argument('--out', default=None, help='jsonl file to append the result lines to')
    return p.parse_args()


def main():
    args = parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_xca_attention.py needs a GPU')
    import timm_amd  # noqa: F401
    from timm_amd import ops
    from timm_amd.layers import set_fused_xca
    from timm_amd.models.xcit import XCA
    from timm_amd.ops.xca_attention import XCA_ATTN_CALLS
    assert ops.has_ext(), 'timm_amd._C HIP extension must be built'

    N, dim, heads = SHAPES[args.model]
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    mod = XCA(dim, num_heads=heads, qkv_bias=True).to(dev, torch.bfloat16)
    with torch.no_grad():
        mod.temperature.uniform_(1., 4.)
    x = torch.randn(args.batch, N, dim, device=dev, dtype=torch.bfloat16, requires_grad=True)
    do = torch.randn(args.batch, N, dim, device=dev, dtype=torch.bfloat16)
    inputs = (x,) + tuple(mod.parameters())

    def fwd():
        return mod.proj(ops.cross_covariance_attention(mod.qkv(x), heads, mod.temperature))

    def step(fused):
        set_fused_xca(fused)
        if args.forward_only:
            with torch.no_grad():
                return fwd()
        return torch.autograd.grad(fwd(), inputs, do)

    arms = {'fused': True, 'composed': False}
    for _ in range(args.warmup):
        for fused in arms.values():
            step(fused)
    torch.cuda.synchronize()
    calls = dict(XCA_ATTN_CALLS)
    times = {name: [] for name in arms}
    for _ in range(args.iters):
        for name, fused in arms.items():
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            step(fused)
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) * 1e3)  # us
    set_fused_xca(None)
    assert XCA_ATTN_CALLS['fwd'] == calls['fwd'] + args.iters, 'the fused arm must run the kernels'

    lines = []
    for name, ts in times.items():
        ts.sort()
        q1, _, q3 = statistics.quantiles(ts, n=4)
        lines.append({
            'arm': name, 'model': args.model,
            'shape': {'B': args.batch, 'N': N, 'heads': heads, 'D': dim // heads},
            'what': 'XCA layers (qkv Linear + attention + proj), '
                    + ('forward' if args.forward_only else 'forward+backward') + ', device events',
            'iters': args.iters, 'warmup': args.warmup,
            'median_us': round(statistics.median(ts), 1), 'min_us': round(ts[0], 1),
            'max_us': round(ts[-1], 1), 'q1_us': round(q1, 1), 'q3_us': round(q3, 1),
        })
    lines.append({'model': args.model, 'batch': args.batch, 'forward_only': args.forward_only,
                  'composed_over_fused': round(lines[1]['median_us'] / lines[0]['median_us'], 3)})
    for line in lines:
        print(json.dumps(line))
    if args.out:
        with open(args.out, 'a') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
