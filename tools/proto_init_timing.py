#!/usr/bin/env python3
"""Time the Proto-MAML head initialisation (mi_proto_init, mi_proto_init_bwd, mi_meta_batch_anil_proto) with HIP
events:

  kernel   mi_proto_init and mi_proto_init_bwd alone at (T = 32, n = 25, feat 1600, ways 5) and (T = 32, n = 5, feat 128, ways 5).  A
           sample is one event pair around --launches back-to-back launches (the features stay in L2 / the Infinity Cache, as they do
           behind the trunk), divided by the launches; host_enqueue_us beside it is the host's cost of enqueueing one launch (an event
           figure close to it is the host's rate, not the kernel's).
  fused    mi_meta_batch_anil_proto with a gradient at cfg3's shape (Mini-ImageNet ANIL trunk, 5-way 5-shot, 32 tasks) beside
           mi_meta_batch_anil (K = 1) and, with the multi-step loss, beside mi_meta_batch_anil_steps (K = 5), second order, in the same
           run on the same inputs; a sample is one event pair around --calls calls, the sides alternating inside every repeat after a
           warm-up of each.  With --census the per-launch profile of one call of each side follows.

Prints one JSON line per row: mean, standard deviation, min and max of --repeats samples, in microseconds (kernel) / milliseconds (fused).

    python tools/proto_init_timing.py [--repeats 15] [--launches 50] [--calls 5] [--census]
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

SCALE, STEP = 2.0 ** -8, 2.0 ** -7          # tests/proto_init_oracle.py's `min` case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=15)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--census', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('proto_init_timing needs the GPU: there is nothing to time without it')
    spec = ModelSpec.anil(WAYS)
    eng = MetaEngine(spec)
    for T, n, feat, ways in KERNEL_SHAPES:
        ph = ways * feat + ways
        fs = torch.from_numpy((3.0 * synthetic.hash_uniform(3, (T, n, feat))).astype('float32')).cuda()
        lam = torch.from_numpy((2.0 * synthetic.hash_uniform(5, (T, ph)) - 1.0).astype('float32')).cuda()
        y = (torch.arange(n, dtype=torch.int32) * ways // n).repeat(T, 1).cuda().contiguous()
        head, dfs, dscale = torch.empty(T, ph, device='cuda'), torch.zeros_like(fs), torch.empty(T, device='cuda')
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr())

        def forward():                   # the C entries on preallocated outputs: nothing but the launch between the events
            rc = eng.lib.mi_proto_init(st, p(fs), p(y), T, n, feat, ways, 1.0 / feat, p(head), ph)
            assert rc == 0, eng.lib.mi_last_error(None)

        def backward():
            rc = eng.lib.mi_proto_init_bwd(st, p(fs), p(y), p(lam), ph, T, n, feat, ways, 1.0 / feat, p(dfs), p(dscale))
            assert rc == 0, eng.lib.mi_last_error(None)
        row = dict(kind='kernel', tasks=T, n=n, feat=feat, ways=ways, launches=args.launches, repeats=args.repeats)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.launches):
            forward()
        row['host_enqueue_us'] = round((time.perf_counter() - t0) * 1e6 / args.launches, 3)
        torch.cuda.synchronize()
        compare(row, dict(proto_init=forward, proto_init_bwd=backward), args.repeats, args.launches, 'us')
    theta = torch.cat([torch.from_numpy(v).reshape(-1) for v in synthetic.ref_init_weights(dict(spec.param_shapes()), 11).values()]).float().cuda()
    data, labels = synthetic.make_uniform_meta_batch('min', list(range(TASKS)), WAYS, SHOTS)
    data, labels = torch.from_numpy(data).cuda(), torch.from_numpy(labels).cuda()
    w5 = torch.full((5,), 0.2, device='cuda')
    sides = dict(anil_K1=lambda: eng.meta_batch_anil(theta, data, labels, SHOTS, 1, STEP),
                 proto_K1=lambda: eng.meta_batch_anil_proto(theta, data, labels, SHOTS, 1, SCALE, inner_lr=STEP),
                 anil_steps_K5=lambda: eng.meta_batch_anil_steps(theta, data, labels, SHOTS, 5, w5, inner_lr=STEP),
                 proto_steps_K5=lambda: eng.meta_batch_anil_proto(theta, data, labels, SHOTS, 5, SCALE, inner_lr=STEP, step_w=w5))
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
