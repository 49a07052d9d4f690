#!/usr/bin/env python3
"""Time the two draws of TaskSampler (utils/task_sampler.py) on a synthetic resident dataset: uint8, 64 classes x 600 images of
3 x 84 x 84, 5-way 5-shot, T = 32 tasks per call (the Mini-ImageNet training configuration's sampler load).  Reports
  - host milliseconds of `sample_indices` alone (the numpy draw of draw='host');
  - wall milliseconds per `sample_batch` over `--calls` calls with one device synchronisation at the end, for draw='host' and
    draw='device', alternated `--rounds` times in the same run (median and range over the rounds);
  - the device-event time of the mi_draw_tasks launch alone (`draw_device`), and of draw + gather (`sample_batch`, draw='device').

    python tools/sampler_timing.py [--calls 200] [--rounds 5]
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
from exploring_meta_amd.utils.task_sampler import ResidentDataset, TaskSampler  # noqa: E402

CLASSES, PER_CLASS, SHAPE, WAYS, SHOTS, TASKS = 64, 600, (3, 84, 84), 5, 5, 32


def wall_ms(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def event_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator(device='cuda').manual_seed(0)
    imgs = torch.randint(0, 256, (CLASSES * PER_CLASS,) + SHAPE, dtype=torch.uint8, device='cuda', generator=g)
    labels = np.repeat(np.arange(CLASSES), PER_CLASS)
    ds = ResidentDataset(imgs, labels)
    host = TaskSampler(ds, WAYS, SHOTS, seed=1234, draw='host')
    dev = TaskSampler(ds, WAYS, SHOTS, seed=1234, draw='device')
    for _ in range(10):                                                   # warm-up: code objects, allocator
        host.sample_batch(TASKS)
        dev.sample_batch(TASKS)
    t0 = time.perf_counter()
    for _ in range(args.calls):
        host.sample_indices(TASKS)
    indices_ms = (time.perf_counter() - t0) * 1e3 / args.calls
    rounds = {'host': [], 'device': []}
    for _ in range(args.rounds):                                          # alternated, so that drift of the machine hits both alike
        rounds['host'].append(wall_ms(lambda: host.sample_batch(TASKS), args.calls))
        rounds['device'].append(wall_ms(lambda: dev.sample_batch(TASKS), args.calls))
    draw_ms = event_ms(lambda: dev.draw_device(TASKS), args.calls)
    both_ms = event_ms(lambda: dev.sample_batch(TASKS), args.calls)
    res = dict(dataset=f'{CLASSES} classes x {PER_CLASS} uint8 images {SHAPE}', ways=WAYS, shots=SHOTS, tasks=TASKS, calls=args.calls,
               rounds=args.rounds, host_sample_indices_ms=round(indices_ms, 4),
               sample_batch_wall_ms={k: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
                                     for k, v in rounds.items()},
               draw_device_event_ms_per_call=round(draw_ms, 4), sample_batch_device_event_ms_per_call=round(both_ms, 4))
    print(f'host sample_indices alone            {indices_ms:8.4f} ms per call (T = {TASKS})')
    for k, v in rounds.items():
        print(f'sample_batch draw={k!r:9s} wall      {statistics.median(v):8.4f} ms per call (median of {args.rounds} rounds of {args.calls} calls, '
              f'range {min(v):.4f} .. {max(v):.4f})')
    print(f'draw_device, device events           {draw_ms:8.4f} ms per call (back-to-back launches: bounded below by the launch rate)')
    print(f'sample_batch draw=\'device\', events   {both_ms:8.4f} ms per call')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
