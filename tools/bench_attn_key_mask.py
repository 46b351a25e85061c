#!/usr/bin/env python3
"""Microbenchmark: key-padding attention, bool key mask against the additive mask.

Times `ops.flash_attention_qkv` forward and forward+backward on packed
[B,N,3,12,64] bf16 qkv, N in {128, 256, 576, 1024} with B * N held near 32768
(the NaFlex sequence-length buckets; N = 32 and 64, at most one key tile, are
added as the short end of the dispatch rule), for two validity patterns:

    full    every key valid
    mixed   sample i keeps a prefix of 100 / 75 / 50 % of its keys (i % 3)

and three arms:

    key        bool [B,1,1,N] mask -> kernels of csrc/attention_key_mask.hip
               (forced for every N, whatever _KEY_MASK_MIN_NK says, so that the
               numbers can set that threshold)
    additive   fp32 [B,1,N,N] mask from `create_attention_mask` -> the masked
               kernels of attention.hip / attention_bwd*.hip; building the mask
               from the [B,N] validity is timed on its own (`mask_build`)
    none       no mask: the floor

The arms alternate inside one process, `--reps` rounds each of `--warmup` +
`--iters` calls timed with device events; a row gives the median over the
rounds of the per-round medians and `spread_us`, the largest minus the
smallest per-round median: the run-to-run spread to hold a difference against.
These are host-launched call times (launch gaps and autograd bookkeeping
included); kernel times come from a kernel trace.

    timeout -k 10 600 python tools/bench_attn_key_mask.py --out rows.jsonl
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, D, TOKENS = 12, 64, 32768
SEQ_LENS = (32, 64, 128, 256, 576, 1024)
PATTERNS = ('full', 'mixed')
ARMS = ('key', 'additive', 'none')


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument('--seq-lens', default=','.join(map(str, SEQ_LENS)))
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


def _valid(pattern, B, N, dev):
    valid = torch.ones(B, N, dtype=torch.bool, device=dev)
    if pattern == 'mixed':
        for i in range(B):
            valid[i, int(N * (1.0, 0.75, 0.5)[i % 3]):] = False
    return valid


def run_case(N, pattern, args, ops, attn_mod, create_attention_mask):
    B = TOKENS // N
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    qkv = torch.randn(B, N, 3, H, D, device=dev, dtype=torch.bfloat16).requires_grad_(True)
    valid = _valid(pattern, B, N, dev)
    masks = {'key': valid[:, None, None, :], 'additive': create_attention_mask(valid), 'none': None}
    do = torch.randn_like(ops.flash_attention_qkv(qkv))
    # same result at the timed size: O of the two masked arms on the valid
    # query rows (the symmetric additive mask zeroes the padded ones)
    with torch.no_grad():
        rows = valid[:, None, :, None]
        o_key = ops.flash_attention_qkv(qkv, attn_mask=masks['key']).float() * rows
        o_add = ops.flash_attention_qkv(qkv, attn_mask=masks['additive']).float() * rows
        rel_diff = ((o_key - o_add).norm() / o_add.norm()).item()

    samples = {arm: {'fwd': [], 'fwd_bwd': []} for arm in ARMS}
    build = []
    ran = {}
    for _ in range(args.reps):
        for arm in ARMS:
            mask = masks[arm]
            before = dict(attn_mod.KEY_MASK_CALLS)

            def fwd():
                with torch.no_grad():
                    return ops.flash_attention_qkv(qkv, attn_mask=mask)

            def fwd_bwd():
                return torch.autograd.grad(ops.flash_attention_qkv(qkv, attn_mask=mask), qkv, do)

            samples[arm]['fwd'].append(_median_us(fwd, args.warmup, args.iters))
            samples[arm]['fwd_bwd'].append(_median_us(fwd_bwd, args.warmup, args.iters))
            ran[arm] = attn_mod.KEY_MASK_CALLS['bwd'] > before['bwd']
        build.append(_median_us(lambda: create_attention_mask(valid), args.warmup, args.iters))
    assert ran == {'key': True, 'additive': False, 'none': False}, ran

    rows = []
    for arm in ARMS:
        row = {'N': N, 'B': B, 'H': H, 'D': D, 'pattern': pattern, 'arm': arm,
               'valid_fraction': round(valid.float().mean().item(), 3),
               'key_mask_kernels': ran[arm], 'dtype': 'bf16',
               'iters': args.iters, 'warmup': args.warmup, 'reps': args.reps}
        for what in ('fwd', 'fwd_bwd'):
            s = samples[arm][what]
            row[what + '_us'] = round(statistics.median(s), 1)
            row[what + '_spread_us'] = round(max(s) - min(s), 1)
        if arm == 'key':
            row['fwd_rel_diff_vs_additive'] = float('%.3g' % rel_diff)
        if arm == 'additive':
            row['mask_build_us'] = round(statistics.median(build), 1)
            row['mask_bytes'] = B * N * N * 4
        rows.append(row)
    return rows


def main():
    args = parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_attn_key_mask.py needs a GPU')
    import timm_amd  # noqa: F401
    from timm_amd import ops
    from timm_amd.models.naflexvit import create_attention_mask
    from timm_amd.ops import attention as attn_mod
    assert ops.has_ext(), 'timm_amd._C HIP extension must be built'
    attn_mod._KEY_MASK_MIN_NK = 1  # arm 'key' always runs the new kernels
    for N in map(int, args.seq_lens.split(',')):
        for pattern in PATTERNS:
            for row in run_case(N, pattern, args, ops, attn_mod, create_attention_mask):
                line = json.dumps(row)
                print(line, flush=True)
                if args.out:
                    with open(args.out, 'a') as f:
                        f.write(line + '\n')


if __name__ == '__main__':
    main()
