#!/usr/bin/env python3
"""Time the vector-step and multi-step-loss ANIL calls (mi_meta_batch_anil_lr, mi_meta_batch_anil_steps) against the plain ANIL call at
the cfg3 size (Mini-ImageNet ANIL trunk, 5-way 5-shot, 32 tasks, K = 5 head steps, second order):

  trajectory  the evaluation call that scores the query set after 0..K steps (with_grad = 0) against the K + 1 plain evaluation calls
              with adapt_steps = 0..K it replaces (one trunk pass against K + 1);
  training    the second-order training call with the multi-step loss against the plain second-order training call (K more head
              passes over the query features, K accumulations of the query cotangent);
  vector      the vector call, and the vector call with lr_grad, against the scalar call.

A sample is the wall clock of --calls back-to-back repetitions ending in torch.cuda.synchronize(), divided by the repetitions; the
sides of a comparison alternate inside every repeat of one process, after a warm-up of each; the figure is the median of --repeats
samples (min and max beside it).  Prints one JSON line per comparison.

    python tools/anil_steps_timing.py [--repeats 9] [--calls 5]
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
        raise SystemExit('anil_steps_timing needs the GPU: there is nothing to time without it')
    spec = ModelSpec.anil(WAYS)
    eng = MetaEngine(spec)
    theta = torch.cat([torch.from_numpy(v).reshape(-1) for v in synthetic.ref_init_weights(dict(spec.param_shapes()), 11).values()]).float().cuda()
    data, labels = synthetic.make_uniform_meta_batch('min', list(range(TASKS)), WAYS, SHOTS)
    data, labels = torch.from_numpy(data).cuda(), torch.from_numpy(labels).cuda()
    w = torch.tensor(msl_weights(K, 0, 10), dtype=torch.float32, device='cuda')
    vec = torch.full((K, eng.head_param_count()), LR, dtype=torch.float32, device='cuda')

    def plain_trajectory():
        for j in range(K + 1):
            eng.meta_batch_anil(theta, data, labels, SHOTS, j, LR, with_grad=False)
    compare('trajectory', dict(steps_call=lambda: eng.meta_batch_anil_steps(theta, data, labels, SHOTS, K, w, inner_lr=LR, with_grad=False),
                               plain_calls_0_to_K=plain_trajectory), args.repeats, args.calls)
    compare('training', dict(steps_call=lambda: eng.meta_batch_anil_steps(theta, data, labels, SHOTS, K, w, inner_lr=LR),
                             plain_call=lambda: eng.meta_batch_anil(theta, data, labels, SHOTS, K, LR)), args.repeats, args.calls)
    compare('vector', dict(scalar_call=lambda: eng.meta_batch_anil(theta, data, labels, SHOTS, K, LR),
                           vector_call=lambda: eng.meta_batch_anil_lr(theta, data, labels, SHOTS, K, vec),
                           vector_call_lr_grad=lambda: eng.meta_batch_anil_lr(theta, data, labels, SHOTS, K, vec, want_lr_grad=True)),
            args.repeats, args.calls)


if __name__ == '__main__':
    main()
