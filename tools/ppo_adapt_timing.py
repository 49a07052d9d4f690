#!/usr/bin/env python3
"""Time one maml_ppo meta-iteration on device rollouts with the task loop and with --batch_tasks (fast_adapt_ppo_tasks: one rollout,
one advantage launch and one mi_policy_update call per adapt step for ALL tasks, then one mi_policy_meta_batch call), at the driver's
default sizes (20 tasks x 20 episodes x 100 steps, ppo_epochs 3), for adapt_steps 1 and 3.

Wall clock of the second iteration of a two-iteration driver run (the first warms up code objects, workspaces and the allocator),
fenced with torch.cuda.synchronize(); --repeats runs per mode, the two modes alternating; the median is reported.  The launches of
one iteration (kernels, and memcpy / memset nodes separately) are counted in a further run of each mode under torch.profiler; where the
profiler records no device activity the counts are null.

    python tools/ppo_adapt_timing.py [--repeats 10] [--adapt_steps 1 3]
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
from exploring_meta_amd.rl import maml_ppo  # noqa: E402

TASKS, EPISODES, PATH = 20, 20, 100


def second_iteration_ms(p, batch_tasks, on_second=None):
    """Run the driver for two iterations; wall time from the end of the first (fenced) to the end of the second (fenced)."""
    stamps = []

    def log(_line):
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
        if len(stamps) == 1 and on_second is not None:
            on_second[0].__enter__()

    maml_ppo.run(dict(p, num_iterations=2), log=log, rollout='device', batch_tasks=batch_tasks)
    if on_second is not None:
        torch.cuda.synchronize()
        on_second[0].__exit__(None, None, None)
    return (stamps[1] - stamps[0]) * 1e3


def count_launches(p, batch_tasks):
    from torch.profiler import ProfilerActivity, profile
    prof = profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA])
    try:
        second_iteration_ms(p, batch_tasks, on_second=[prof])
    except RuntimeError as e:                                      # (a profiler build without device tracing)
        print(f'launch count unavailable: {e}')
        return None, None
    kernels = copies = 0
    for e in prof.events():
        if str(getattr(e, 'device_type', '')).endswith('CUDA'):
            if e.name.startswith(('Memcpy', 'Memset')):
                copies += 1
            else:
                kernels += 1
    return (kernels, copies) if kernels else (None, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--adapt_steps', type=int, nargs='+', default=[1, 3])
    ap.add_argument('--no-count', action='store_true', help='skip the launch counts')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    results = []
    for K in args.adapt_steps:
        p = dict(maml_ppo.params, meta_batch_size=TASKS, adapt_batch_size=EPISODES, max_path_length=PATH, adapt_steps=K)
        times = {False: [], True: []}
        for mode in (False, True):                                # one untimed run of each: code objects, workspaces
            second_iteration_ms(p, mode)
        for _ in range(args.repeats):
            for mode in (False, True):                            # alternating
                times[mode].append(second_iteration_ms(p, mode))
        med = {m: statistics.median(v) for m, v in times.items()}
        counts = {m: (None, None) if args.no_count else count_launches(p, m) for m in (False, True)}
        row = dict(adapt_steps=K, tasks=TASKS, episodes=EPISODES, max_path_length=PATH, ppo_epochs=p['ppo_epochs'], repeats=args.repeats,
                   task_loop_ms=dict(median=round(med[False], 2), min=round(min(times[False]), 2), max=round(max(times[False]), 2)),
                   batch_tasks_ms=dict(median=round(med[True], 2), min=round(min(times[True]), 2), max=round(max(times[True]), 2)),
                   ratio=round(med[False] / med[True], 2), batched_is_faster=bool(med[True] < med[False]),
                   task_loop_launches=dict(kernels=counts[False][0], copies=counts[False][1]),
                   batch_tasks_launches=dict(kernels=counts[True][0], copies=counts[True][1]))
        results.append(row)
        print(f"adapt_steps {K}: task loop {med[False]:9.2f} ms (min {min(times[False]):.2f}, max {max(times[False]):.2f}) | --batch_tasks "
              f"{med[True]:9.2f} ms (min {min(times[True]):.2f}, max {max(times[True]):.2f}) | ratio {med[False] / med[True]:.2f} | launches "
              f"{counts[False]} vs {counts[True]} (kernels, copies)")
    print(json.dumps(results))


if __name__ == '__main__':
    main()
