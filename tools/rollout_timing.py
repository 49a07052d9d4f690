#!/usr/bin/env python3
"""Time the Particles2D rollouts of the MAML-TRPO path at cfg5 sizes (20 tasks x 20 episodes x 100 steps, the default 2-100-100-2
policy), with torch.cuda.synchronize() fences after a warm-up:
  (a) the host-loop runner (Particles2DRunner, rollout='host') for ONE task -- the yardstick;
  (b) the device rollout (mi_particles_rollout through rollout_tasks) of ALL 20 tasks;
  (c) one full maml_trpo iteration with rollout='host' and with rollout='device' (a driver run of --iterations iterations, divided).
Expectation: (b) for 20 tasks takes less time than (a) for one.

    python tools/rollout_timing.py [--repeats 5]
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
from exploring_meta_amd import core_functions as cf  # noqa: E402
from exploring_meta_amd.rl import maml_trpo  # noqa: E402

TASKS, EPISODES, PATH = 20, 20, 100


def wall_ms(fn, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--iterations', type=int, default=2, help='maml_trpo iterations per timed driver run')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    cf.set_device(dev)
    torch.manual_seed(0)
    policy = cf.DiagNormalPolicy(2, 2).to(dev)
    goals = np.random.RandomState(0).uniform(-0.5, 0.5, size=(TASKS, 2))
    gen = torch.Generator(device=dev).manual_seed(0)
    host = cf.Particles2DRunner(goals[0], PATH, gen, dev)
    ids = [0]

    def device_all():
        cf.rollout_tasks(policy, goals, list(range(ids[0], ids[0] + TASKS)), 0, EPISODES, PATH, dev)
        ids[0] += TASKS

    host.run(policy, EPISODES)                                            # warm-up: code objects, allocator
    device_all()
    a = wall_ms(lambda: host.run(policy, EPISODES), args.repeats)
    b = wall_ms(device_all, args.repeats)

    p = dict(maml_trpo.params, num_iterations=args.iterations, meta_batch_size=TASKS, adapt_batch_size=EPISODES, max_path_length=PATH)
    quiet = lambda *_: None
    maml_trpo.run(dict(p, num_iterations=1), log=quiet, rollout='device')  # warm-up of the meta-step's kernels
    c_dev = [t / args.iterations for t in wall_ms(lambda: maml_trpo.run(p, log=quiet, rollout='device'), max(1, args.repeats // 2))]
    c_host = [t / args.iterations for t in wall_ms(lambda: maml_trpo.run(p, log=quiet, rollout='host'), 1)]

    med = statistics.median
    res = dict(tasks=TASKS, episodes=EPISODES, max_path_length=PATH, repeats=args.repeats,
               host_runner_one_task_ms=dict(median=round(med(a), 3), min=round(min(a), 3), max=round(max(a), 3)),
               device_rollout_all_tasks_ms=dict(median=round(med(b), 3), min=round(min(b), 3), max=round(max(b), 3)),
               maml_trpo_iteration_ms=dict(host=round(med(c_host), 1), device=round(med(c_dev), 1)),
               device_all_tasks_faster_than_host_one_task=bool(med(b) < med(a)))
    print(f'(a) host-loop runner, ONE task         {med(a):10.3f} ms  (min {min(a):.3f}, max {max(a):.3f}; {args.repeats} runs)')
    print(f'(b) device rollout, ALL {TASKS} tasks        {med(b):10.3f} ms  (min {min(b):.3f}, max {max(b):.3f})')
    print(f'(c) maml_trpo iteration, rollout=host   {med(c_host):10.1f} ms;  rollout=device {med(c_dev):10.1f} ms')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
