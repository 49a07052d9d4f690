#!/usr/bin/env python3
"""Time the step-wise policy learner's two device calls at the DiagNormalPolicy defaults (2-100-100-2, ReLU), 2000 rows per task, for
1 task and for 20: mi_policy_vjp and mi_policy_hvp on the fused sweep and on the per-layer path, and torch's own autograd on an
nn.Sequential MLP of the same shape on the same card -- what a user would otherwise run: per task a forward and
``grad(loc, params, grad_outputs=dloc)`` (VJP), or ``g = grad(..., create_graph=True); grad(g . v, params + [dloc])`` (HVP).

A sample is the wall clock of --calls back-to-back calls ending in torch.cuda.synchronize(), divided by the calls; the three variants
alternate inside every repeat, after a warm-up of each; the figure is the median of --repeats samples (min and max beside it).  Before
timing, the fused and per-layer results are compared, and torch's against them.  Prints one JSON line per (tasks, product).

    python tools/policy_learner_timing.py [--repeats 15] [--calls 50] [--activation relu]
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
from exploring_meta_amd.engine import PolicyEngine  # noqa: E402

S, A, H, ROWS = 2, 2, (100, 100), 2000


def sample_ms(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=15)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--activation', default='relu', choices=['relu', 'tanh'])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('policy_learner_timing needs the GPU: there is nothing to time without it')
    dev = torch.device('cuda')
    eng = PolicyEngine(S, A, H, dev, activation=args.activation)
    act = torch.nn.ReLU if args.activation == 'relu' else torch.nn.Tanh
    mlp = torch.nn.Sequential(torch.nn.Linear(S, H[0]), act(), torch.nn.Linear(H[0], H[1]), act(), torch.nn.Linear(H[1], A)).to(dev)
    params = list(mlp.parameters())
    g = torch.Generator().manual_seed(0)
    theta = torch.cat([torch.zeros(A)] + [p.detach().reshape(-1).cpu() for p in params]).to(dev)       # engine order: sigma first
    for T in (1, 20):
        states = torch.randn(T, ROWS, S, generator=g).to(dev)
        dloc = torch.randn(T, ROWS, A, generator=g).to(dev)
        v = torch.randn(T, theta.numel(), generator=g).to(dev)
        vparts = [[x.reshape(p.shape) for x, p in zip(torch.split(v[t, A:], [p.numel() for p in params]), params)] for t in range(T)]

        def torch_vjp():
            return [torch.autograd.grad(mlp(states[t]), params, grad_outputs=dloc[t]) for t in range(T)]

        def torch_hvp():
            out = []
            for t in range(T):
                d = dloc[t].clone().requires_grad_(True)
                gs = torch.autograd.grad(mlp(states[t]), params, grad_outputs=d, create_graph=True)
                out.append(torch.autograd.grad(sum((a * b).sum() for a, b in zip(gs, vparts[t])), params + [d], allow_unused=True))
            return out

        def hip(product, fused):
            def run():
                eng.set_fused_learner(fused)
                return eng.vjp(theta, states, dloc) if product == 'vjp' else eng.hvp(theta, states, dloc, v)
            return run

        flat = lambda gs: torch.cat([torch.zeros(A, device=dev)] + [(torch.zeros_like(p) if x is None else x).reshape(-1) for x, p in zip(gs, params)])
        rel = lambda a, b: float((a - b).norm() / b.norm())
        for product in ('vjp', 'hvp'):
            variants = dict(fused=hip(product, True), per_layer=hip(product, False), torch_autograd=torch_vjp if product == 'vjp' else torch_hvp)
            a, b, c = variants['fused'](), variants['per_layer'](), variants['torch_autograd']()
            if product == 'vjp':
                agree = dict(fused_vs_per_layer=rel(a, b), fused_vs_torch=rel(a, torch.stack([flat(x) for x in c])))
            else:
                agree = dict(fused_vs_per_layer=rel(a[0], b[0]), loc_dot_fused_vs_per_layer=rel(a[1], b[1]),
                             fused_vs_torch=rel(a[0], torch.stack([flat(x[:-1]) for x in c])),
                             loc_dot_fused_vs_torch=rel(a[1], torch.stack([x[-1] for x in c])))
            for fn in variants.values():                       # warm-up of every variant at this shape
                sample_ms(fn, 3)
            samples = {k: [] for k in variants}
            for _ in range(args.repeats):
                for k, fn in variants.items():
                    samples[k].append(sample_ms(fn, args.calls))
            row = dict(tasks=T, rows=ROWS, product=product, activation=args.activation, agreement=agree, calls=args.calls, repeats=args.repeats)
            for k, xs in samples.items():
                row[k + '_ms'] = dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4))
            print(json.dumps(row), flush=True)
    eng.set_fused_learner(True)


if __name__ == '__main__':
    main()
