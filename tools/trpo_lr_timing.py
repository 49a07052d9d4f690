#!/usr/bin/env python3
"""Time the TRPO calls with one inner-loop step (mi_trpo_*_steps) against the same calls with a per-parameter step-size table
(mi_trpo_*_steps_lr) at the size of BASELINE config 5: 20 tasks x 20 episodes x 100 steps per replay, the 2-100-100-2 policy.

Three settings, each timing "surrogate + gradient" and "one curvature product":
    fused      ReLU, K = 1: the fused sweeps (the cfg5 hot path), Fisher product
    per_layer  ReLU, K = 3: the per-layer path, Fisher product
    general    tanh, K = 3: the exact KL Hessian product (ANIL-TRPO), after surrogate + kl_prepare (whose time is reported too)

A sample is the device time between two events around --calls back-to-back calls, divided by the calls; scalar and vector alternate inside
every repeat of one process, after a warm-up of each; the figure is the median of --repeats samples (min and max beside it).  The table is
uniform at the scalar's value with one row per update, so both variants do the same adaptation.  The replays are seeded normal states /
actions / advantages of full length (the cost does not depend on their values).  Prints one JSON line per setting.

    python tools/trpo_lr_timing.py [--repeats 9] [--calls 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from exploring_meta_amd.core_functions import DiagNormalPolicy  # noqa: E402

TASKS, EPISODES, PATH, LR, DAMPING = 20, 20, 100, 0.1, 1e-5


def sample_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def replays(n, gen):
    B = EPISODES * PATH
    r = lambda *s: torch.randn(*s, generator=gen).cuda()
    return dict(states=r(n, TASKS, B, 2), actions=r(n, TASKS, B, 2), adv=r(n, TASKS, B),
                count=torch.full((n, TASKS), B, dtype=torch.int32, device='cuda'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--calls', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('trpo_lr_timing needs the GPU: there is nothing to time without it')
    gen = torch.Generator().manual_seed(2)
    for setting, act, K, general in (('fused', 'relu', 1, False), ('per_layer', 'relu', 3, False), ('general', 'tanh', 3, True)):
        torch.manual_seed(1)
        pol = DiagNormalPolicy(2, 2, activation=act).cuda()
        eng, theta = pol.engine(), pol.flat()
        sup = replays(K, gen)
        qry = {k: v[0] for k, v in replays(1, gen).items()}
        B = EPISODES * PATH
        old_loc = torch.randn(TASKS, B, 2, generator=gen).cuda()
        old_scale = torch.ones(TASKS, 2, device='cuda')
        v = torch.randn(eng.param_count, generator=gen).cuda()
        steps = dict(scalar=(LR, None), vector=(torch.full((K, eng.param_count), LR, dtype=torch.float32, device='cuda'), list(range(K))))

        def surrogate(lr, rows):
            return lambda: eng.surrogate(theta, sup, qry, old_loc, old_scale, lr, True, step_lr_row=rows)

        def prepare(lr, rows):
            return lambda: eng.kl_prepare(sup, qry, old_loc, old_scale, lr, step_lr_row=rows)

        def product(lr, rows):
            if general:
                return lambda: eng.fvp_general(sup, qry, old_scale, lr, DAMPING, v, step_lr_row=rows)
            return lambda: eng.fvp(sup, qry, lr, DAMPING, v, step_lr_row=rows)
        phases = ['surrogate_grad'] + (['kl_prepare'] if general else []) + ['product']
        make = dict(surrogate_grad=surrogate, kl_prepare=prepare, product=product)
        samples = {(ph, k): [] for ph in phases for k in steps}
        for rep in range(args.repeats + 1):                      # repeat 0 is the warm-up
            for k, (lr, rows) in steps.items():                  # a variant's product works on the context its own surrogate left
                for ph in phases:
                    ms = sample_ms(make[ph](lr, rows), args.calls if rep else 2)
                    if rep:
                        samples[(ph, k)].append(ms)
        row = dict(setting=setting, activation=act, adapt_steps=K, tasks=TASKS, episodes=EPISODES, max_path_length=PATH, calls=args.calls,
                   repeats=args.repeats)
        for (ph, k), xs in samples.items():
            row[f'{ph}_{k}_ms'] = dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4))
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
