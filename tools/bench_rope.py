#!/usr/bin/env python3
"""Microbenchmark: fused q/k RoPE op vs the eager composition, forward+backward.

Default shape is the eva02_large_patch14_336 attention block at batch 64:
B=64, H=16, N=577 (1 prefix token), D=64, bf16 q/k as views of the packed
[B, N, 3, H, D] projection, fp32 [N-1, 2D] table.

One implementation per process, so each GPU step can run under its own
`timeout`:

    timeout -k 10 120 python tools/bench_rope.py --impl fused
    timeout -k 10 120 python tools/bench_rope.py --impl eager

Timing is device events around one forward+backward, after warmup; the result
line gives the median and the min/max/quartile spread over --iters repeats.
Achieved bytes/s counts only what the algorithm needs: read and write q and k
once per direction (8 x B*H*N*D*itemsize, plus the table), set against the
measured-copy HBM roof of 6.3 TB/s (8.0 TB/s spec).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_ROOF_TBS = 6.3   # achievable (float4 copy); spec peak is 8.0


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument('--impl', choices=['fused', 'eager'], required=True)
    p.add_argument('--batch', type=int, default=64)
    p.add_argument('--heads', type=int, default=16)
    p.add_argument('--tokens', type=int, default=577)
    p.add_argument('--prefix', type=int, default=1)
    p.add_argument('--head-dim', type=int, default=64)
    p.add_argument('--half', action='store_true', help='half-rotation layout')
    p.add_argument('--warmup', type=int, default=10)
    p.add_argument('--iters', type=int, default=50)
    return p.parse_args()


def main():
    args = parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_rope.py needs a GPU')
    import timm_amd  # noqa: F401
    from timm_amd import ops
    from timm_amd.layers import apply_rot_embed_cat
    assert ops.has_ext(), 'timm_amd._C HIP extension must be built'

    B, H, N, npt, D = args.batch, args.heads, args.tokens, args.prefix, args.head_dim
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    qkv = torch.randn(B, N, 3, H, D, device=dev, dtype=torch.bfloat16).requires_grad_(True)
    rope = torch.randn(N - npt, 2 * D, device=dev, dtype=torch.float32)
    dq = torch.randn(B, H, N, D, device=dev, dtype=torch.bfloat16)
    dk = torch.randn(B, H, N, D, device=dev, dtype=torch.bfloat16)

    def eager(q, k, v):
        # the composition EvaAttention / AttentionRope ran before the fused op
        q = torch.cat([q[:, :, :npt, :], apply_rot_embed_cat(q[:, :, npt:, :], rope, half=args.half)], 2).type_as(v)
        k = torch.cat([k[:, :, :npt, :], apply_rot_embed_cat(k[:, :, npt:, :], rope, half=args.half)], 2).type_as(v)
        return q, k

    def fused(q, k, v):
        assert ops.rope_available(q, k, rope, args.half, v.dtype)
        return ops.apply_rope_qk(q, k, rope, num_prefix_tokens=npt, half=args.half, out_dtype=v.dtype)

    fn = fused if args.impl == 'fused' else eager

    def step():
        q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)
        q_rot, k_rot = fn(q, k, v)
        # grads w.r.t. the q/k views: leaves out the unbind/stack that both paths share
        return torch.autograd.grad((q_rot, k_rot), (q, k), (dq, dk))

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
    need_bytes = 8 * B * H * N * D * qkv.element_size() + 2 * rope.numel() * rope.element_size()
    tbs = need_bytes / (med * 1e-6) / 1e12
    print(json.dumps({
        'impl': args.impl, 'shape': {'B': B, 'H': H, 'N': N, 'npt': npt, 'D': D, 'half': args.half},
        'dtype': 'bf16', 'table': 'fp32', 'what': 'forward+backward, device events',
        'iters': args.iters, 'warmup': args.warmup,
        'median_us': round(med, 1), 'min_us': round(times[0], 1), 'max_us': round(times[-1], 1),
        'q1_us': round(q1, 1), 'q3_us': round(q3, 1),
        'needed_bytes': need_bytes, 'achieved_TBps': round(tbs, 3),
        'share_of_hbm_roof': round(tbs / HBM_ROOF_TBS, 3), 'hbm_roof_TBps': HBM_ROOF_TBS,
    }))


if __name__ == '__main__':
    main()
