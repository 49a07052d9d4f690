#!/usr/bin/env python3
"""Time the logistic-regression head (mi_logreg_head, mi_meta_batch_logreg) with HIP events:

  kernel   mi_logreg_head alone at (T = 32, n = 25, feat 1600, ways 5), (T = 32, n = 5, feat 128, ways 5) and one wide task (T = 1, n = 36,
           feat 515, ways 36), forward only and forward + backward, with mi_ridge_head and mi_metric_head (proto) on the same features beside it.  A sample is one event pair around
           --launches back-to-back launches (the features stay in L2 / the Infinity Cache, as they do behind the trunk), divided by the
           launches, the sides alternating inside every repeat; host_enqueue_us beside it is the host's cost of enqueueing one launch.
           The row carries the solver's counts on these inputs from the host model (tests/logreg_head_oracle.closed_form): the most
           Newton steps of a task and the most CG steps of a task over all its solves, the backward's included -- a launch lasts as long
           as its slowest workgroup, so (forward + backward time) / cg_total bounds the time of one CG step from above.
  fused    mi_meta_batch_logreg with a gradient at cfg3's shape (Mini-ImageNet ANIL trunk, 5-way 5-shot, 32 tasks) beside
           mi_meta_batch_ridge on the same inputs; a sample is one event pair around --calls calls, the sides alternating inside every
           repeat after a warm-up of each.  With --census the per-launch profile of one call of each side follows.

Prints one JSON line per row: mean, standard deviation, min and max of --repeats samples, in microseconds (kernel) / milliseconds (fused).

    python tools/logreg_head_timing.py [--repeats 15] [--launches 50] [--calls 5] [--census]
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
sys.path.insert(0, os.path.join(REPO, 'tests'))
from exploring_meta_amd.engine import MetaEngine, ModelSpec  # noqa: E402
from exploring_meta_amd.utils import synthetic  # noqa: E402
from metric_head_timing import KERNEL_SHAPES, SHOTS, TASKS, WAYS, compare  # noqa: E402

LAM, ALPHA = 1.0, 1.0
WIDE_SHAPE = ((1, 36, 515, 36),)          # one task of 36 x 36 tables (136480 bytes of LDS): the per-CG-step time the worst case is derived from


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=15)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--census', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('logreg_head_timing needs the GPU: there is nothing to time without it')
    import logreg_head_oracle as LH
    spec = ModelSpec.anil(WAYS)
    eng = MetaEngine(spec)
    for T, n, feat, ways in KERNEL_SHAPES + WIDE_SHAPE:
        fs_h = (3.0 * synthetic.hash_uniform(3, (T, n, feat))).astype('float32')
        fq_h = (3.0 * synthetic.hash_uniform(4, (T, n, feat))).astype('float32')
        fs, fq = torch.from_numpy(fs_h).cuda(), torch.from_numpy(fq_h).cuda()
        y = (torch.arange(n, dtype=torch.int32) * ways // n).repeat(T, 1).contiguous()
        info = LH.closed_form(fs_h, fq_h, y.numpy(), y.numpy(), ways, LAM, ALPHA)[-1]
        y = y.cuda()
        loss, acc, dh = torch.empty(T, device='cuda'), torch.empty(T, device='cuda'), torch.empty(T, 2, device='cuda')
        logits, dfs, dfq = torch.empty(T, n, ways, device='cuda'), torch.empty_like(fs), torch.empty_like(fq)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

        def two_hyper(entry, alpha):     # the C entries on preallocated outputs: nothing but the launch between the events
            def run(grad):
                rc = entry(st, p(fs), p(fq), p(y), p(y), T, n, n, feat, ways, LAM, alpha, p(loss), p(acc), p(logits),
                           p(dfs if grad else None), p(dfq if grad else None), p(dh if grad else None), None, 0)
                assert rc == 0, eng.lib.mi_last_error(None)
            return run
        logreg, ridge = two_hyper(eng.lib.mi_logreg_head, ALPHA), two_hyper(eng.lib.mi_ridge_head, 8.0)

        def proto(grad):
            rc = eng.lib.mi_metric_head(st, p(fs), p(fq), p(y), p(y), T, n, n, feat, ways, 0, 1.0 / feat, p(loss), p(acc), p(logits),
                                        p(dfs if grad else None), p(dfq if grad else None), None, 0)
            assert rc == 0, eng.lib.mi_last_error(None)
        row = dict(kind='kernel', tasks=T, n=n, feat=feat, ways=ways, lam=LAM, alpha=ALPHA, launches=args.launches, repeats=args.repeats,
                   newton=info['newton'], cg_most_of_one_solve=info['cg'], cg_total=info['cg_total'], halvings=info['halve'])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.launches):
            logreg(True)
        row['host_enqueue_us'] = round((time.perf_counter() - t0) * 1e6 / args.launches, 3)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dfs).all())
        compare(row, dict(logreg_forward=lambda: logreg(False), logreg_forward_backward=lambda: logreg(True),
                          ridge_forward=lambda: ridge(False), ridge_forward_backward=lambda: ridge(True),
                          proto_forward=lambda: proto(False), proto_forward_backward=lambda: proto(True)), args.repeats, args.launches, 'us')
    theta = torch.cat([torch.from_numpy(v).reshape(-1) for v in synthetic.ref_init_weights(dict(spec.param_shapes()), 11).values()]).float().cuda()
    data, labels = synthetic.make_uniform_meta_batch('min', list(range(TASKS)), WAYS, SHOTS)
    data, labels = torch.from_numpy(data).cuda(), torch.from_numpy(labels).cuda()
    sides = dict(ridge=lambda: eng.meta_batch_ridge(theta, data, labels, SHOTS, lam=LAM, scale=1.0),
                 logreg=lambda: eng.meta_batch_logreg(theta, data, labels, SHOTS, lam=LAM, scale=ALPHA))
    out = sides['logreg']()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[0]).all()), 'a task of the fused call was flagged'
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
