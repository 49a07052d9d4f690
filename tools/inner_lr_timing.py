#!/usr/bin/env python3
"""Time the fused MAML call with a scalar inner step (mi_meta_batch_maml_tv), with per-parameter steps (mi_meta_batch_maml_lr) and with
per-parameter steps + their gradient, at the headline size (Mini-ImageNet 5-way 5-shot, 5 second-order steps, 32 tasks) and at 5-way
1-shot, 1 step, 32 tasks.

A sample is the wall clock of --calls back-to-back calls ending in torch.cuda.synchronize(), divided by the calls; the three variants
alternate inside every repeat of one process, after a warm-up of each; the figure is the median of --repeats samples (min and max beside
it).  The vector is uniform at the scalar's value, so the three variants do the same adaptation.  Prints one JSON line per size.

    python tools/inner_lr_timing.py [--repeats 9] [--calls 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from exploring_meta_amd.engine import MetaEngine, ModelSpec  # noqa: E402
from exploring_meta_amd.utils import synthetic  # noqa: E402

SIZES = [dict(name='headline', shots=5, K=5, tasks=32), dict(name='5w1s', shots=1, K=1, tasks=32)]
WAYS, LR = 5, 0.5


def sample_ms(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--calls', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('inner_lr_timing needs the GPU: there is nothing to time without it')
    eng = MetaEngine(ModelSpec.mini_imagenet(WAYS))
    shapes = ModelSpec.mini_imagenet(WAYS).param_shapes()
    theta = torch.cat([torch.from_numpy(v).reshape(-1) for v in synthetic.ref_init_weights(dict(shapes), 11).values()]).float().cuda()
    vec = torch.full((1, eng.param_count), LR, dtype=torch.float32, device='cuda')
    for size in SIZES:
        data, labels = synthetic.make_uniform_meta_batch('min', list(range(size['tasks'])), WAYS, size['shots'])
        data, labels = torch.from_numpy(data).cuda(), torch.from_numpy(labels).cuda()
        S, K = size['shots'], size['K']
        variants = dict(scalar=lambda: eng.meta_batch(theta, data, labels, S, K, LR),
                        vector=lambda: eng.meta_batch_lr(theta, data, labels, S, K, vec),
                        vector_lr_grad=lambda: eng.meta_batch_lr(theta, data, labels, S, K, vec, want_lr_grad=True))
        for fn in variants.values():
            sample_ms(fn, 2)
        samples = {k: [] for k in variants}
        for _ in range(args.repeats):
            for k, fn in variants.items():
                samples[k].append(sample_ms(fn, args.calls))
        row = dict(size=size, calls=args.calls, repeats=args.repeats)
        for k, xs in samples.items():
            row[k + '_ms'] = dict(median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3))
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
