#!/usr/bin/env python3
"""R2-D2's differentiable ridge-regression head on the 4-conv trunk of ``vision/anil_vision.py``, on the batched HIP engine: the head's
inner problem solved exactly on the support set, no inner loop; the regulariser and the logit scale are meta-learned with the trunk.

``features = Sequential(ConvBase(...), Lambda(view(-1, fc_neurons)))`` as in the ANIL driver, Adam over the trunk and the head's two
scalars (``RidgeHead``: log_lam, log_scale), per-iteration train + validation meta-batches, gradient / meta_batch_size -- each half ONE
``meta_batch_adapt_ridge`` call (mi_meta_batch_ridge: the trunk once on all rows, one ridge-head launch for the whole meta-batch, the
trunk backward), task-sharded over ranks under ``torchrun`` with one RCCL all-reduce.  Meta-test by ``evaluate_ridge``.  The trunk's
checkpoints carry the ANIL driver's names (``model_checkpoints/model_features_<it+1>.pt``, ``features.pt``), with the head's two scalars
beside them (``model_ridge_head_<it+1>.pt``, ``ridge_head.pt``), so a ridge trunk loads wherever an ANIL trunk does.  Tasks come from
the seeded synthetic generator (datasets are not available offline).

    python -m exploring_meta_amd.vision.ridge_vision --dataset min --shots 5 --lam 50 --scale 8 --num_iterations 10
"""
import argparse
import os
import random

import numpy as np
import torch

from ..core_functions.anil import anil_engine
from ..core_functions.ridge import RidgeHead, evaluate_ridge, meta_batch_adapt_ridge
from ..core_functions.vision_models import RunningStatsFold
from ..sharding import init_process_group, reduce_meta_batch, shard_range
from . import anil_vision
from .maml_vision import SyntheticTasks

params = {
    "ways": 5, "shots": 5, "outer_lr": 0.003, "meta_batch_size": 32, "num_iterations": 10000, "save_every": 1000, "seed": 42,
    "lam": 1.0, "scale": 1.0,
}


def build(dataset, ways, device, lam=1.0, scale=1.0, fix_head=False):
    """The ANIL driver's ``features`` (its linear head is built and dropped) and the ridge head's two scalars."""
    features, _ = anil_vision.build(dataset, ways, 0.0, device)
    return features, RidgeHead(lam, scale, learnable=not fix_head).to(device)


def run(dataset, p, log=print):
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    torch.cuda.set_device(local)
    if world > 1:
        init_process_group(local)
    random.seed(p['seed']); np.random.seed(p['seed']); torch.manual_seed(p['seed']); torch.cuda.manual_seed(p['seed'])
    device = torch.device('cuda', local)
    features, head = build(dataset, p['ways'], device, p['lam'], p['scale'], p.get('fix_head', False))
    all_parameters = list(features.parameters()) + list(head.parameters())
    opt = torch.optim.Adam(all_parameters, lr=p['outer_lr'])
    T = p['meta_batch_size']
    lo, hi = shard_range(T, rank, world)
    train, valid = SyntheticTasks(dataset, p['ways'], p['shots'], 0), SyntheticTasks(dataset, p['ways'], p['shots'], 10 ** 6)
    metrics = {}
    zero = torch.zeros((), device=device)
    save_dir = p.get('save_dir') or ''
    if save_dir and rank == 0:
        os.makedirs(os.path.join(save_dir, 'model_checkpoints'), exist_ok=True)

    for it in range(p['num_iterations']):
        opt.zero_grad()
        ids = list(range(it * T + lo, it * T + hi))
        # BatchNorm buffers of `features` (saved with every checkpoint): one trunk pass per task and phase, as in the ANIL driver
        fold = None
        if save_dir:
            eng = anil_engine(features, p['ways'], 28 if dataset == 'omni' else 84, device)
            fold = RunningStatsFold(eng, features[0], eng.spec, T, lo, hi, 1, 2 * p['ways'] * p['shots'])
        if ids:
            d, l = train.sample_batch(ids)
            total, losses, accs = meta_batch_adapt_ridge(features, head, d.to(device), l.to(device), p['shots'], p['ways'])
            total.backward()
            if fold:
                fold.collect(0)
            with torch.no_grad():
                d, l = valid.sample_batch([10 ** 6 + i for i in ids])
                _, vlosses, vaccs = meta_batch_adapt_ridge(features, head, d.to(device), l.to(device), p['shots'], p['ways'])
            if fold:
                fold.collect(1)
            sums = [losses.sum(), accs.sum(), vlosses.sum(), vaccs.sum()]
        else:                                    # meta_batch_size < world size: this rank owns no task, contributes zeros
            sums = [zero, zero, zero, zero]
        flat = torch.cat([(q.grad if q.grad is not None else torch.zeros_like(q)).reshape(-1) for q in all_parameters])
        flat, lsum, asum, ex = reduce_meta_batch(flat, sums[0], sums[1], extra=sums[2:] + ([fold.contribution] if fold else []))
        vlsum, vasum = ex[0], ex[1]
        if fold:
            fold.apply(ex[2])
        off = 0
        for q in all_parameters:
            g = flat[off:off + q.numel()].view_as(q) * (1.0 / T)
            q.grad = g.clone() if q.grad is None else q.grad.copy_(g)
            off += q.numel()
        opt.step()
        metrics = {'train_loss': (lsum / T).item(), 'train_acc': (asum / T).item(),
                   'valid_loss': (vlsum / T).item(), 'valid_acc': (vasum / T).item(), 'lam': head.lam, 'scale': head.scale}
        if rank == 0:
            log(f'iter {it}: {metrics}')
            if save_dir and it % p['save_every'] == 0:
                torch.save(features.state_dict(), os.path.join(save_dir, 'model_checkpoints', f'model_features_{it + 1}.pt'))
                torch.save(head.state_dict(), os.path.join(save_dir, 'model_checkpoints', f'model_ridge_head_{it + 1}.pt'))
    test = SyntheticTasks(dataset, p['ways'], p['shots'], 2 * 10 ** 6)
    metrics['test_acc'] = evaluate_ridge(p, test, features, head, device)
    if rank == 0 and save_dir:
        torch.save(features.state_dict(), os.path.join(save_dir, 'features.pt'))
        torch.save(head.state_dict(), os.path.join(save_dir, 'ridge_head.pt'))
    if world > 1:
        torch.distributed.destroy_process_group()
    return (features, head), metrics


def build_parser():
    parser = argparse.ArgumentParser(description='R2-D2 ridge-regression head on Vision (MI355X engine)')
    parser.add_argument('--dataset', type=str, default='min', help='omni or min')
    for k, v in params.items():
        parser.add_argument(f'--{k}', type=type(v), default=v)
    parser.add_argument('--fix_head', action='store_true', help='lam and scale stay at their initial values (not meta-learned)')
    parser.add_argument('--save_dir', type=str, default='',
                        help="write model_checkpoints/model_{features,ridge_head}_<it+1>.pt every save_every iterations and features.pt / "
                             "ridge_head.pt at the end (the trunk under the ANIL driver's names)")
    return parser


def main(argv=None, log=print):
    """Parse the flags and run; returns ((features, head), metrics of the last iteration with test_acc)."""
    args = build_parser().parse_args(argv)
    p = dict(params)
    p.update({k: getattr(args, k) for k in params})
    p['save_dir'] = args.save_dir
    p['fix_head'] = args.fix_head
    return run(args.dataset, p, log=log)


if __name__ == '__main__':
    main()
