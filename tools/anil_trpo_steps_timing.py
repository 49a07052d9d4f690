#!/usr/bin/env python3
"""Time the exact KL Hessian path of ANIL-TRPO for adapt_steps K = 1, 2, 3, 5 at the driver's default sizes (20 tasks x 20 episodes x
100 steps, device rollouts): milliseconds per kl_prepare, per Hessian-vector product and per whole meta_optimize_trpo(anil=True), the
launches of one product and the workspace bytes.

Every K runs mi_trpo_kl_prepare_steps / mi_trpo_fvp_general_steps; K = 1 is the yardstick (a K-step product does about K times its
sweeps).

Every figure is the median of --repeats wall-clock samples fenced with torch.cuda.synchronize(), after one untimed call.  The
launches of one product (kernels, and memcpy / memset nodes separately) are counted under torch.profiler; where the profiler records no
device activity the counts are null.

    python tools/anil_trpo_steps_timing.py [--repeats 20] [--adapt_steps 1 2 3 5]
"""
import argparse
import ctypes as C
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
from exploring_meta_amd.core_functions.rl import _SurrogateContext  # noqa: E402
from exploring_meta_amd.rl import anil_trpo  # noqa: E402

TASKS, EPISODES, PATH = 20, 20, 100


def median_ms(fn, repeats):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def count_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
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


def one_case(K, repeats, dev, count=True):
    p = dict(anil_trpo.params, meta_batch_size=TASKS, adapt_batch_size=EPISODES, max_path_length=PATH, adapt_steps=K)
    torch.manual_seed(p['seed'])
    policy = cf.DiagNormalPolicyANIL(2, 2, p['fc_neurons']).to(dev)
    baseline = cf.LinearValue(2, 2)
    goals = np.random.RandomState(p['seed']).uniform(-0.5, 0.5, size=(TASKS, 2))
    results = cf.fast_adapt_trpo_tasks(goals, policy, baseline, p, p['seed'], 0, anil=True, first_order=True)
    olds, replays = [r[0] for r in results], [r[2] for r in results]
    ctx = _SurrogateContext(replays, olds, policy, baseline, p)
    theta, eng = policy.flat(), ctx.engine
    v = torch.randn(theta.shape, generator=torch.Generator().manual_seed(5)).to(dev)
    T, B = ctx.qry['states'].shape[0], ctx.qry['states'].shape[1]
    ws = C.c_size_t()
    eng._check(eng.lib.mi_trpo_general_steps_workspace_bytes(eng._h, T, B, K, C.byref(ws)))
    ctx.evaluate(theta, want_grad=True)
    prep = median_ms(lambda: ctx.prepare_general_kl(theta), repeats)
    product = lambda: ctx.fvp(theta, v)
    prod = median_ms(product, repeats)
    kernels, copies = count_launches(product) if count else (None, None)
    row = dict(adapt_steps=K, tasks=T, batch=B, repeats=repeats,
               kl_prepare_ms=dict(median=round(prep[0], 3), min=round(prep[1], 3), max=round(prep[2], 3)),
               product_ms=dict(median=round(prod[0], 3), min=round(prod[1], 3), max=round(prod[2], 3)),
               product_launches=dict(kernels=kernels, copies=copies), workspace_bytes=int(ws.value))
    flat0 = policy.flat().clone()

    def whole():
        policy.load_flat(flat0)                                # every sample starts from the same parameters
        cf.meta_optimize_trpo(p, policy, baseline, replays, olds, anil=True)
    m = median_ms(whole, max(3, repeats // 4))
    row['meta_optimize_ms'] = dict(median=round(m[0], 2), min=round(m[1], 2), max=round(m[2], 2))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--adapt_steps', type=int, nargs='+', default=[1, 2, 3, 5])
    ap.add_argument('--no-count', action='store_true', help='skip the launch counts')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    cf.set_device(dev)
    rows = []
    for K in args.adapt_steps:
        rows.append(one_case(K, args.repeats, dev, count=not args.no_count))
    base = next((r['product_ms']['median'] for r in rows if r['adapt_steps'] == 1), None)
    for r in rows:
        r['product_vs_K_one_step'] = None if base is None else round(r['product_ms']['median'] / (r['adapt_steps'] * base), 2)
        print(f"K {r['adapt_steps']}: kl_prepare {r['kl_prepare_ms']['median']:.3f} ms | product {r['product_ms']['median']:.3f} ms "
              f"(x{r['product_vs_K_one_step']} of K products at K = 1) | meta_optimize {r.get('meta_optimize_ms', {}).get('median')} ms | "
              f"launches {r['product_launches']} | workspace {r['workspace_bytes'] / 2 ** 20:.1f} MiB")
    print(json.dumps(rows))


if __name__ == '__main__':
    main()
