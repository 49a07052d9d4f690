#!/usr/bin/env python3
"""Time the fused MAML call with per-step query passes (mi_meta_batch_maml_steps) against the plain calls it stands in for, at the
headline size (Mini-ImageNet 5-way 5-shot, K = 5 steps, 32 tasks):

  trajectory  the evaluation call that scores the query set after 0..K steps (grad_tasks = 0) against the K + 1 plain evaluation calls
              with adapt_steps = 0..K it replaces (K against K (K + 1) / 2 support passes);
  training    the second-order training call with the multi-step loss against the plain second-order training call (K more query
              forward + backward passes).

A sample is the wall clock of --calls back-to-back repetitions ending in torch.cuda.synchronize(), divided by the repetitions; the two
sides of a comparison alternate inside every repeat of one process, after a warm-up of each; the figure is the median of --repeats
samples (min and max beside it).  Prints one JSON line per comparison.

    python tools/msl_timing.py [--repeats 9] [--calls 5]
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
from exploring_meta_amd.core_functions import msl_weights  # noqa: E402
from exploring_meta_amd.engine import MetaEngine, ModelSpec  # noqa: E402
from exploring_meta_amd.utils import synthetic  # noqa: E402

WAYS, SHOTS, K, TASKS, LR = 5, 5, 5, 32, 0.5


def sample_ms(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def compare(name, variants, repeats, calls):
    for fn in variants.values():
        sample_ms(fn, 2)
    samples = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            samples[k].append(sample_ms(fn, calls))
    row = dict(comparison=name, ways=WAYS, shots=SHOTS, K=K, tasks=TASKS, calls=calls, repeats=repeats)
    for k, xs in samples.items():
        row[k + '_ms'] = dict(median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3))
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--calls', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('msl_timing needs the GPU: there is nothing to time without it')
    eng = MetaEngine(ModelSpec.mini_imagenet(WAYS))
    shapes = ModelSpec.mini_imagenet(WAYS).param_shapes()
    theta = torch.cat([torch.from_numpy(v).reshape(-1) for v in synthetic.ref_init_weights(dict(shapes), 11).values()]).float().cuda()
    data, labels = synthetic.make_uniform_meta_batch('min', list(range(TASKS)), WAYS, SHOTS)
    data, labels = torch.from_numpy(data).cuda(), torch.from_numpy(labels).cuda()
    w = torch.tensor(msl_weights(K, 0, 10), dtype=torch.float32, device='cuda')

    def plain_trajectory():
        for j in range(K + 1):
            eng.meta_batch(theta, data, labels, SHOTS, j, LR, with_grad=False)
    compare('trajectory', dict(steps_call=lambda: eng.meta_batch_steps(theta, data, labels, SHOTS, K, w, inner_lr=LR, grad_tasks=0),
                               plain_calls_0_to_K=plain_trajectory), args.repeats, args.calls)
    compare('training', dict(steps_call=lambda: eng.meta_batch_steps(theta, data, labels, SHOTS, K, w, inner_lr=LR),
                             plain_call=lambda: eng.meta_batch(theta, data, labels, SHOTS, K, LR)), args.repeats, args.calls)


if __name__ == '__main__':
    main()
