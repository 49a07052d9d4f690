#!/usr/bin/env python3
"""Time mi_cka (csrc/cka.hip) at the representation sizes of the representation-change study: MiniImagenetCNN 5-way 5-shot
(p = 25 images) layers 0-4 and -1 over 10 tasks (one batched call per layer, as rc_vision.run_rep_cka makes it), and the
64-filter trunk's layer 1 (n = 112896) once.  Prints ms per pair from device events after a warm-up of every shape, and the work
the passes need (from the shapes), so that a separate `rocprofv3 --kernel-trace --stats` run can be turned into shares of peak.

    python tools/cka_timing.py [--reps 3]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from exploring_meta_amd.utils.cka import cka  # noqa: E402

TR = 64                      # distance tile (cka.hip)
VALU_PEAK = 256 * 4 * 32 * 2.4e9    # fp32 lane-operations per second of one MI355X (an FMA is one operation)

SHAPES = [  # (label, n, p, pairs)
    ('min5w5s layer 0', 21168, 25, 10), ('min5w5s layer 1', 56448, 25, 10), ('min5w5s layer 2', 14112, 25, 10),
    ('min5w5s layer 3', 3200, 25, 10), ('min5w5s layer 4', 800, 25, 10), ('min5w5s layer -1', 25, 5, 10),
    ('64-filter layer 1', 112896, 25, 1),
]


def work(n, p):
    """Per pair: distance entries each pass evaluates (median rounds and centred products over the tiles j >= i, row sums over
    all), the vector operations they cost (2p per distance: a subtraction and an FMA per feature) and the compulsory bytes."""
    T = (n + TR - 1) // TR
    upper, full = T * (T + 1) // 2 * TR * TR, T * T * TR * TR
    entries = {'histogram x3': 3 * 2 * upper, 'row sums': 2 * full, 'centred products': 2 * upper}
    ops = {k: v * 2 * p for k, v in entries.items()}
    return entries, ops, 2 * n * p * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator(device='cuda').manual_seed(0)
    rows = []
    for label, n, p, pairs in SHAPES:
        xs = torch.relu(torch.randn(pairs, n, p, device='cuda', generator=g))
        ys = torch.relu(xs + 0.5 * torch.randn(pairs, n, p, device='cuda', generator=g))
        cka(xs, ys)                                            # warm-up of this shape
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            r = cka(xs, ys)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.reps / pairs
        entries, ops, nbytes = work(n, p)
        total_ops = sum(ops.values())
        row = dict(shape=label, n=n, p=p, pairs=pairs, ms_per_pair=round(ms, 4), distance_entries=sum(entries.values()),
                   valu_lane_ops=total_ops, valu_share_of_peak=round(total_ops / (ms * 1e-3) / VALU_PEAK, 3),
                   compulsory_bytes=nbytes, linear=float(r.linear[0]), kernel=float(r.kernel[0]))
        rows.append(row)
        print(f'{label:20s} n={n:6d} p={p:3d} pairs={pairs:2d}: {ms:9.3f} ms/pair  '
              f'distance entries {sum(entries.values()):.3e}  VALU lane-ops {total_ops:.3e} '
              f'({row["valu_share_of_peak"]:.0%} of peak)  linear {row["linear"]:.4f} kernel {row["kernel"]:.4f}', flush=True)
    print(json.dumps(rows))


if __name__ == '__main__':
    main()
