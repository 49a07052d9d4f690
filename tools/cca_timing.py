#!/usr/bin/env python3
"""Time mi_cca (csrc/cca.hip) at the representation sizes of the representation-change study: MiniImagenetCNN 5-way 5-shot
(p = 25 images) layers 0-4 and -1, for 1 and 32 pairs per call (rc_vision.run_rep_cca makes one call per layer over all tasks).
Prints the time of one `cca` call from device events after a warm-up of every shape and, beside it, the host time of the fp64
numpy restatement (tests/cca_oracle.py) on the same arrays copied back, one pair after the other.

    python tools/cca_timing.py [--reps 20] [--epsilon 1e-10]
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from exploring_meta_amd.utils.cca import cca  # noqa: E402
import cca_oracle  # noqa: E402

SHAPES = [  # (label, n, p)
    ('min5w5s layer 0', 21168, 25), ('min5w5s layer 1', 56448, 25), ('min5w5s layer 2', 14112, 25),
    ('min5w5s layer 3', 3200, 25), ('min5w5s layer 4', 800, 25), ('min5w5s layer -1', 25, 5),
]
PAIRS = (1, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--epsilon', type=float, default=1e-10)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    g = torch.Generator(device='cuda').manual_seed(0)
    rows = []
    for label, n, p in SHAPES:
        for pairs in PAIRS:
            xs = torch.relu(torch.randn(pairs, n, p, device='cuda', generator=g))
            ys = torch.relu(xs + 0.5 * torch.randn(pairs, n, p, device='cuda', generator=g))
            cca(xs, ys, args.epsilon)                              # warm-up of this shape
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                r, det = cca(xs, ys, args.epsilon, detail=True)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / args.reps
            hx, hy = xs.cpu().numpy(), ys.cpu().numpy()
            t0 = time.perf_counter()
            host = [cca_oracle.cca(hx[k], hy[k], args.epsilon) for k in range(pairs)]
            host_ms = (time.perf_counter() - t0) * 1e3
            err = max(abs(float(r.mean[k]) - host[k]['mean']) for k in range(pairs))
            sweeps = det.sweeps[:, :3].max(0).values.tolist()
            row = dict(shape=label, n=n, p=p, pairs=pairs, gpu_ms_per_call=round(ms, 4), host_oracle_ms=round(host_ms, 3),
                       input_bytes=2 * pairs * n * p * 4, max_sweeps=sweeps, mean_err_vs_host=err)
            rows.append(row)
            print(f'{label:18s} n={n:6d} p={p:3d} pairs={pairs:2d}: GPU {ms:8.3f} ms/call   host oracle {host_ms:9.2f} ms   '
                  f'sweeps (x, y, svd) {sweeps}   |mean - host| {err:.1e}', flush=True)
    print(json.dumps(rows))


if __name__ == '__main__':
    main()
