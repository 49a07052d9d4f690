#!/usr/bin/env python3
"""Time the fused MAML call with per-step parameter offsets (mi_meta_batch_maml_offsets) against the same call without them, second
order, Mini-ImageNet net, 32 tasks, at the headline size (5-way 5-shot, K = 5) and at 5-way 1-shot, K = 1:

  plain     the same call without offsets (the scalar step: meta_batch);
  offsets   with offsets N(0, 0.05^2) on the BatchNorm tensors (the per-step BatchNorm preset);
  offsets+g ... and the offset gradient (one fold per inner step).

A sample is the wall clock of --calls back-to-back repetitions ending in torch.cuda.synchronize(), divided by the repetitions; the
variants alternate inside every repeat of one process, after a warm-up of each; the figure is the median of --repeats samples (min and
max beside it).  Prints one JSON line per size.

    python tools/step_offsets_timing.py [--repeats 9] [--calls 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from exploring_meta_amd.engine import MetaEngine, ModelSpec  # noqa: E402
from exploring_meta_amd.utils import synthetic  # noqa: E402

WAYS, TASKS, LR = 5, 32, 0.5
SIZES = (('headline', 5, 5), ('one_shot_one_step', 1, 1))      # name, shots, K


def sample_ms(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def compare(name, shots, K, variants, repeats, calls):
    for fn in variants.values():
        sample_ms(fn, 2)
    samples = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            samples[k].append(sample_ms(fn, calls))
    row = dict(size=name, ways=WAYS, shots=shots, K=K, tasks=TASKS, calls=calls, repeats=repeats)
    for k, xs in samples.items():
        row[k + '_ms'] = dict(median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3))
    print(json.dumps(row), flush=True)


def bn_offsets(shapes, K, std=0.05, seed=31):
    """[K, P] fp32: N(0, std^2) on the BatchNorm tensors, zero elsewhere."""
    P = sum(int(np.prod(s)) for s in shapes.values())
    v = (std * np.random.RandomState(seed).standard_normal((K, P))).astype(np.float32)
    off = 0
    for name, shp in shapes.items():
        n = int(np.prod(shp))
        if '.normalize.' not in name:
            v[:, off:off + n] = 0.0
        off += n
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--calls', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('step_offsets_timing needs the GPU: there is nothing to time without it')
    eng = MetaEngine(ModelSpec.mini_imagenet(WAYS))
    shapes = dict(ModelSpec.mini_imagenet(WAYS).param_shapes())
    theta = torch.cat([torch.from_numpy(v).reshape(-1) for v in synthetic.ref_init_weights(shapes, 11).values()]).float().cuda()
    for name, shots, K in SIZES:
        data, labels = synthetic.make_uniform_meta_batch('min', list(range(TASKS)), WAYS, shots)
        data, labels = torch.from_numpy(data).cuda(), torch.from_numpy(labels).cuda()
        ofs = torch.from_numpy(bn_offsets(shapes, K)).cuda()
        compare(name, shots, K, {
            'plain': lambda: eng.meta_batch(theta, data, labels, shots, K, LR),
            'offsets': lambda: eng.meta_batch_offsets(theta, data, labels, shots, K, ofs, inner_lr=LR),
            'offsets_grad': lambda: eng.meta_batch_offsets(theta, data, labels, shots, K, ofs, inner_lr=LR, want_offsets_grad=True),
        }, args.repeats, args.calls)


if __name__ == '__main__':
    main()
