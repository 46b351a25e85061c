#!/usr/bin/env python3
"""Driver benchmark contract: flagship training step throughput.

Measures BASELINE.json's headline metric — train samples/sec for
vit_base_patch16_224 at 224x224 bf16 — on N GPUs of one node (weak scaling,
one rank per GPU over RCCL).  Protocol mirrors the reference's benchmark.py
(synthetic randn inputs, random-init weights, warmup + timed steps with
device sync around the timed region — /root/reference/benchmark.py:305-420).

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]
A plain run sets up, warms up, times K train steps and prints the result line.
--full adds the inference row (infer_* keys) measured before the train phase.
--dump-outputs DIR writes what the last timed step computed as DIR/<name>.npy;
that step then starts from the state after the run's first step, so that its
outputs are the same from run to run.
For N>1 the driver launches via torch.distributed.run with one rank per GPU;
rank/world info is read from the env.
"""
import argparse
import json
import os
import time

# hipBLASLt GEMM algorithm autotuning (TunableOp): +7% train step on ViT-B.
# Tuned results are cached in-repo (tunableop/) so driver runs on fresh boxes
# load them instead of re-tuning; missing shapes tune during warmup.
_REPO = os.path.dirname(os.path.abspath(__file__))
os.makedirs(os.path.join(_REPO, 'tunableop'), exist_ok=True)
os.environ.setdefault('PYTORCH_TUNABLEOP_ENABLED', '1')
os.environ.setdefault('PYTORCH_TUNABLEOP_TUNING', '1')
os.environ.setdefault('PYTORCH_TUNABLEOP_FILENAME', os.path.join(_REPO, 'tunableop', 'bench_gemm.csv'))

import torch


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument('--gpus', type=int, default=1)
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--model', type=str, default='vit_base_patch16_224')
    p.add_argument('--batch-size', type=int, default=256, help='per-GPU train batch size')
    p.add_argument('--infer-batch-size', type=int, default=1024,
                   help='per-GPU infer batch size (reference benchmark uses b1024)')
    p.add_argument('--img-size', type=int, default=224)
    p.add_argument('--mode', type=str, default=None, choices=['both', 'train', 'infer'],
                   help="'both' measures infer then train and emits one JSON line "
                        "with train as the headline metric + infer_* keys "
                        "(default: 'train', or 'both' with --full)")
    p.add_argument('--full', action='store_true',
                   help='also measure everything beyond the headline figure (the inference row)')
    p.add_argument('--dump-outputs', type=str, default=None, metavar='DIR',
                   help='after the timed steps, write the outputs of the last timed step '
                        'to DIR/<name>.npy (float32); that step starts from the state '
                        'after the first step of the run')
    p.add_argument('--amp-dtype', type=str, default='bfloat16')
    p.add_argument('--opt', type=str, default='adamw', choices=['adamw', 'muon'],
                   help='optimizer for the train phase (muon = NS-kernel path, BASELINE config #4)')
    p.add_argument('--channels-last', action='store_true', default=None,
                   help='NHWC memory format (default: auto-on for conv nets)')
    args = p.parse_args()
    if args.mode is None:
        args.mode = 'both' if args.full else 'train'
    return args


# --dump-outputs: parameters are sampled, not dumped whole (ViT-B is 330 MB in fp32)
_PARAM_SAMPLE = 1024


def _sample_params(model):
    """Fixed seeded sample of every parameter after the last optimizer step."""
    g = torch.Generator().manual_seed(0)
    chunks = []
    for _, p in sorted(model.named_parameters()):
        flat = p.detach().reshape(-1)
        idx = torch.randint(0, flat.numel(), (min(_PARAM_SAMPLE, flat.numel()),), generator=g)
        chunks.append(flat[idx.to(flat.device)].float().cpu())
    return torch.cat(chunks)


class _TrainState:
    """Copy of the model's and optimizer's tensors, to put back in place later."""

    def __init__(self, model, optimizer):
        self.model = {k: v.detach().clone() for k, v in model.state_dict().items()}
        self.optim = {p: {k: v.clone() if torch.is_tensor(v) else v for k, v in st.items()}
                      for p, st in optimizer.state.items()}

    @torch.no_grad()
    def restore(self, model, optimizer):
        for k, v in model.state_dict().items():
            v.copy_(self.model[k])
        for p, st in self.optim.items():
            for k, v in st.items():
                if torch.is_tensor(v):
                    optimizer.state[p][k].copy_(v)
                else:
                    optimizer.state[p][k] = v


def _dump_outputs(out_dir, arrays):
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    for name, t in arrays.items():
        np.save(os.path.join(out_dir, name + '.npy'), t.detach().float().cpu().numpy())


def main():
    args = parse_args()

    world_size = int(os.environ.get('WORLD_SIZE', 1))
    rank = int(os.environ.get('RANK', 0))
    local_rank = int(os.environ.get('LOCAL_RANK', 0))
    distributed = world_size > 1

    assert torch.cuda.is_available(), 'bench.py requires a GPU (MI355X)'
    device = torch.device(f'cuda:{local_rank}')
    torch.cuda.set_device(device)

    if distributed:
        torch.distributed.init_process_group(backend='nccl')

    import timm_amd
    from timm_amd import ops
    assert ops.has_ext(), 'timm_amd._C HIP extension must be built for bench'

    dtype = torch.bfloat16 if args.amp_dtype == 'bfloat16' else torch.float16
    torch.manual_seed(42 + rank)
    # inputs come from generators of their own so they are identical from run
    # to run whichever phases are measured
    gen_infer = torch.Generator(device=device).manual_seed(1000 + rank)
    gen_train = torch.Generator(device=device).manual_seed(2000 + rank)
    dumped = {}

    model = timm_amd.create_model(args.model, num_classes=1000)
    model = model.to(device=device, dtype=dtype)

    # NHWC routes depthwise/dense convs to our gfx950 kernels / MIOpen's fast
    # paths; transformer models stay NCHW (patchify GEMM is layout-free)
    channels_last = args.channels_last
    if channels_last is None:
        conv_families = ('convnext', 'resnet', 'efficientnet', 'mobilenet', 'regnet', 'nfnet', 'densenet')
        channels_last = any(f in args.model for f in conv_families)
    if channels_last:
        model = model.to(memory_format=torch.channels_last)

    n_gpus = world_size

    def timed_run(step_fn, per_gpu_batch):
        """Warmup + exactly K timed steps, sync'd on both sides, MAX over ranks.
        Returns (aggregate samples/sec, ms/step, what the last timed step returned)."""
        for _ in range(args.warmup):
            step_fn()
        if distributed:
            torch.distributed.barrier()
        torch.cuda.synchronize()
        last = None
        t0 = time.perf_counter()
        for _ in range(args.steps):
            last = step_fn()
        torch.cuda.synchronize()
        if distributed:
            torch.distributed.barrier()
        t1 = time.perf_counter()
        elapsed = t1 - t0
        if distributed:
            t = torch.tensor([elapsed], device=device)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            elapsed = t.item()
        return per_gpu_batch * n_gpus * args.steps / elapsed, elapsed / args.steps * 1000., last

    # reference benchmark CSVs: RTX3090 train b192 / RTX4090 infer b1024
    TRAIN_BASE, INFER_BASE = 390.86, 2992.79
    infer_sps = infer_ms = None

    if args.mode in ('both', 'infer'):
        model.eval()
        Bi = args.infer_batch_size
        xi = torch.randn(Bi, 3, args.img_size, args.img_size, device=device, dtype=dtype,
                         generator=gen_infer)
        if channels_last:
            xi = xi.contiguous(memory_format=torch.channels_last)

        @torch.no_grad()
        def infer_step():
            return model(xi)

        infer_sps, infer_ms, infer_out = timed_run(infer_step, Bi)
        if args.dump_outputs and infer_out is not None:
            dumped['infer_logits'] = infer_out.float().cpu()
        del xi, infer_out
        torch.cuda.empty_cache()

    if args.mode in ('both', 'train'):
        model.train()
        if distributed:
            from timm_amd.parallel import BucketedDataParallel
            model = BucketedDataParallel(model, bucket_cap_mb=50.)
        if args.opt == 'muon':
            from timm_amd.optim.muon import Muon
            optimizer = Muon(model.parameters(), lr=1e-3, weight_decay=0.05)
        else:
            from timm_amd.optim import AdamW
            optimizer = AdamW(model.parameters(), lr=1e-4, weight_decay=0.05)

        B = args.batch_size
        x = torch.randn(B, 3, args.img_size, args.img_size, device=device, dtype=dtype,
                        generator=gen_train)
        if channels_last:
            x = x.contiguous(memory_format=torch.channels_last)
        target = torch.randint(0, 1000, (B,), device=device, generator=gen_train)

        def train_step():
            for bucket in getattr(model, '_buckets', []):
                bucket.flat.zero_()
            if not distributed:
                optimizer.zero_grad(set_to_none=True)
            out = model(x)
            loss = torch.nn.functional.cross_entropy(out.float(), target)
            loss.backward()
            if distributed:
                model.finish_gradient_sync()
            optimizer.step()
            return out, loss

        timed_step = train_step
        if args.dump_outputs and args.warmup + args.steps > 1:
            # bf16 weights turn the rounding noise of the fp32-atomic gradient
            # reductions into whole-ulp differences that grow step by step, so
            # the state after many steps differs from run to run.  For a dump
            # that two runs (or two builds) can be compared by, the last timed
            # step starts from the state the run had after its first step.
            total, done, first = args.warmup + args.steps, 0, None

            def timed_step():
                nonlocal done, first
                if done == total - 1:
                    first.restore(model, optimizer)
                res = train_step()
                done += 1
                if done == 1:
                    first = _TrainState(model, optimizer)
                return res

        train_sps, train_ms, train_out = timed_run(timed_step, B)
        if args.dump_outputs and train_out is not None:
            dumped['train_logits'] = train_out[0].float().cpu()
            dumped['train_loss'] = train_out[1].float().reshape(1).cpu()
            dumped['train_params_sample'] = _sample_params(model)

    if args.dump_outputs and rank == 0:
        _dump_outputs(args.dump_outputs, dumped)

    if rank == 0:
        if args.mode == 'infer':
            head_metric, head_sps, head_ms, head_base, gb = (
                'infer_samples_per_sec', infer_sps, infer_ms, INFER_BASE,
                args.infer_batch_size * n_gpus)
        else:
            head_metric, head_sps, head_ms, head_base, gb = (
                'train_samples_per_sec', train_sps, train_ms, TRAIN_BASE,
                args.batch_size * n_gpus)
        result = {
            'metric': head_metric,
            'value': round(head_sps, 2),
            'unit': 'samples/sec',
            'n_gpus': n_gpus,
            'steps': args.steps,
            'warmup': args.warmup,
            'ms_per_step': round(head_ms, 3),
            'higher_is_better': True,
            'scaling': 'weak',
            'vs_baseline': round(head_sps / head_base, 3),
            'dtype': 'bf16' if dtype == torch.bfloat16 else 'fp16',
            'data': 'synthetic',
            'config': {
                'model': args.model,
                'global_batch': gb,
                'img_size': args.img_size,
                'parallelism': f'dp{n_gpus}',
            },
        }
        if args.mode == 'both' and infer_sps is not None:
            # the BASELINE metric is "infer + train samples/sec": attach the
            # infer row to the same JSON line so the driver certifies both
            result['infer_samples_per_sec'] = round(infer_sps, 2)
            result['infer_ms_per_step'] = round(infer_ms, 3)
            result['infer_batch'] = args.infer_batch_size * n_gpus
            result['infer_vs_baseline'] = round(infer_sps / INFER_BASE, 3)
        print(json.dumps(result))

    if distributed:
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
