#!/usr/bin/env python3
"""Time the ridge-regression head (mi_ridge_head, mi_meta_batch_ridge) with HIP events:

  kernel   mi_ridge_head alone at (T = 32, n = 25, feat 1600, ways 5) and (T = 32, n = 5, feat 128, ways 5), forward only and forward +
           backward, with mi_metric_head (proto) on the same features beside it.  A sample is one event pair around --launches
           back-to-back launches (the features stay in L2 / the Infinity Cache, as they do behind the trunk), divided by the launches;
           host_enqueue_us beside it is the host's cost of enqueueing one launch (an event figure close to it is the host's rate, not
           the kernel's).
  fused    mi_meta_batch_ridge with a gradient at cfg3's shape (Mini-ImageNet ANIL trunk, 5-way 5-shot, 32 tasks) beside
           mi_meta_batch_metric (proto) on the same inputs; a sample is one event pair around --calls calls, the sides alternating
           inside every repeat after a warm-up of each.  With --census the per-launch profile of one call of each side follows.

Prints one JSON line per row: mean, standard deviation, min and max of --repeats samples, in microseconds (kernel) / milliseconds (fused).

    python tools/ridge_head_timing.py [--repeats 15] [--launches 50] [--calls 5] [--census]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))
from exploring_meta_amd.engine import MetaEngine, ModelSpec  # noqa: E402
from exploring_meta_amd.utils import synthetic  # noqa: E402
from metric_head_timing import KERNEL_SHAPES, SHOTS, TASKS, WAYS, compare  # noqa: E402

LAM, ALPHA = 1.0, 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=15)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--census', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ridge_head_timing needs the GPU: there is nothing to time without it')
    spec = ModelSpec.anil(WAYS)
    eng = MetaEngine(spec)
    for T, n, feat, ways in KERNEL_SHAPES:
        fs = torch.from_numpy((3.0 * synthetic.hash_uniform(3, (T, n, feat))).astype('float32')).cuda()
        fq = torch.from_numpy((3.0 * synthetic.hash_uniform(4, (T, n, feat))).astype('float32')).cuda()
        y = (torch.arange(n, dtype=torch.int32) * ways // n).repeat(T, 1).cuda().contiguous()
        loss, acc, dh = torch.empty(T, device='cuda'), torch.empty(T, device='cuda'), torch.empty(T, 2, device='cuda')
        logits, dfs, dfq = torch.empty(T, n, ways, device='cuda'), torch.empty_like(fs), torch.empty_like(fq)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

        def ridge(grad):                 # the C entries on preallocated outputs: nothing but the launch between the events
            rc = eng.lib.mi_ridge_head(st, p(fs), p(fq), p(y), p(y), T, n, n, feat, ways, LAM, ALPHA, p(loss), p(acc), p(logits),
                                       p(dfs if grad else None), p(dfq if grad else None), p(dh if grad else None), None, 0)
            assert rc == 0, eng.lib.mi_last_error(None)

        def proto(grad):
            rc = eng.lib.mi_metric_head(st, p(fs), p(fq), p(y), p(y), T, n, n, feat, ways, 0, 1.0 / feat, p(loss), p(acc), p(logits),
                                        p(dfs if grad else None), p(dfq if grad else None), None, 0)
            assert rc == 0, eng.lib.mi_last_error(None)
        row = dict(kind='kernel', tasks=T, n=n, feat=feat, ways=ways, lam=LAM, alpha=ALPHA, launches=args.launches, repeats=args.repeats)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.launches):
            ridge(True)
        row['host_enqueue_us'] = round((time.perf_counter() - t0) * 1e6 / args.launches, 3)
        torch.cuda.synchronize()
        compare(row, dict(ridge_forward=lambda: ridge(False), ridge_forward_backward=lambda: ridge(True),
                          proto_forward=lambda: proto(False), proto_forward_backward=lambda: proto(True)), args.repeats, args.launches, 'us')
    theta = torch.cat([torch.from_numpy(v).reshape(-1) for v in synthetic.ref_init_weights(dict(spec.param_shapes()), 11).values()]).float().cuda()
    data, labels = synthetic.make_uniform_meta_batch('min', list(range(TASKS)), WAYS, SHOTS)
    data, labels = torch.from_numpy(data).cuda(), torch.from_numpy(labels).cuda()
    sides = dict(metric_proto=lambda: eng.meta_batch_metric(theta, data, labels, SHOTS, metric='proto', scale=2.0 ** -8),
                 ridge=lambda: eng.meta_batch_ridge(theta, data, labels, SHOTS, lam=LAM, scale=1.0))
    compare(dict(kind='fused', ways=WAYS, shots=SHOTS, tasks=TASKS, calls=args.calls, repeats=args.repeats), sides, args.repeats, args.calls, 'ms')
    if args.census:
        for name, fn in sides.items():
            fn()
            eng.profile(True)
            fn()
            torch.cuda.synchronize()
            prof = {f'{op}/{layer}': dict(ms=round(ms, 4), launches=int(cnt)) for (op, layer), (ms, cnt) in eng.profile_collect().items()}
            eng.profile(False)
            print(json.dumps(dict(kind='census', side=name, total_ms=round(sum(v['ms'] for v in prof.values()), 4), launches=prof)), flush=True)


if __name__ == '__main__':
    main()
