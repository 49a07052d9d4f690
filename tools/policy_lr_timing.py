#!/usr/bin/env python3
"""Time the policy's fused MAML call with a scalar inner step (mi_policy_meta_batch), with per-parameter steps
(mi_policy_meta_batch_lr) and with per-parameter steps + their gradient, at the maml_ppo driver's default sizes (2-100-100-2 tanh policy,
20 tasks x 20 episodes x 100 steps per replay, PPO with ppo_epochs 3, second order), for adapt_steps 1 and 3.

A sample is the wall clock of --calls back-to-back calls ending in torch.cuda.synchronize(), divided by the calls; the three variants
alternate inside every repeat of one process, after a warm-up of each; the figure is the median of --repeats samples (min and max beside
it).  The vector is uniform at the scalar's value with one row per adapt step, so the three variants do the same adaptation.  The replays
are seeded normal states / actions / advantages of full length (the cost does not depend on their values).  Prints one JSON line per size.

    python tools/policy_lr_timing.py [--repeats 9] [--calls 5] [--adapt_steps 1 3]
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
from exploring_meta_amd.core_functions import DiagNormalPolicy  # noqa: E402

TASKS, EPISODES, PATH, EPOCHS, LR, CLIP = 20, 20, 100, 3, 0.01, 0.1


def sample_ms(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def replays(n, gen):
    B = EPISODES * PATH
    r = lambda *s: torch.randn(*s, generator=gen).cuda()
    d = dict(states=r(n, TASKS, B, 2), actions=r(n, TASKS, B, 2), adv=r(n, TASKS, B),
             count=torch.full((n, TASKS), B, dtype=torch.int32, device='cuda'))
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--adapt_steps', type=int, nargs='+', default=[1, 3])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('policy_lr_timing needs the GPU: there is nothing to time without it')
    torch.manual_seed(1)
    pol = DiagNormalPolicy(2, 2, activation='tanh').cuda()
    eng, theta = pol.engine(), pol.flat()
    gen = torch.Generator().manual_seed(2)
    for K in args.adapt_steps:
        sup = replays(K, gen)
        qry = {k: v[0] for k, v in replays(1, gen).items()}
        step_batch = [b for b in range(K) for _ in range(EPOCHS)]
        vec = torch.full((K, eng.param_count), LR, dtype=torch.float32, device='cuda')
        kw = dict(loss='ppo', clip=CLIP)
        variants = dict(scalar=lambda: eng.meta_batch(theta, sup, qry, step_batch, LR, **kw),
                        vector=lambda: eng.meta_batch_lr(theta, sup, qry, step_batch, vec, step_batch, want_lr_grad=False, **kw),
                        vector_lr_grad=lambda: eng.meta_batch_lr(theta, sup, qry, step_batch, vec, step_batch, want_lr_grad=True, **kw))
        for fn in variants.values():
            sample_ms(fn, 2)
        samples = {k: [] for k in variants}
        for _ in range(args.repeats):
            for k, fn in variants.items():
                samples[k].append(sample_ms(fn, args.calls))
        row = dict(adapt_steps=K, tasks=TASKS, episodes=EPISODES, max_path_length=PATH, ppo_epochs=EPOCHS, calls=args.calls,
                   repeats=args.repeats)
        for k, xs in samples.items():
            row[k + '_ms'] = dict(median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3))
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
