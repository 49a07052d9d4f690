"""The training loop of the drivers whose iteration is one fused call per half on the ANIL trunk (``vision.anil_vision``,
``vision.protonet_vision``, ``vision.ridge_vision``, ``vision.logreg_vision``): rank setup, seeding, per-iteration train + validation meta-batches task-sharded over
ranks, the BatchNorm buffers of the trunk folded when checkpoints are written, ONE all-reduce, gradient / meta_batch_size, Adam, the
checkpoint cadence.  What differs between the drivers comes from ``setup``."""
import os
import random

import numpy as np
import torch

from ..core_functions.anil import anil_engine
from ..core_functions.vision_models import RunningStatsFold
from ..sharding import init_process_group, reduce_meta_batch, shard_range
from .maml_vision import SyntheticTasks


def train_trunk(dataset, p, log, setup):
    """``setup(device)`` runs after the seeding (it builds the modules, so it draws the initial weights) and returns a dict:

    features        the ANIL ``features`` Sequential (its ConvBase first): its BatchNorm buffers are tracked when --save_dir is given
    parameters      what Adam steps and the ranks all-reduce, in this order
    train           (it, data, labels) -> (total, losses [T], accs [T]); ``total.backward()`` follows
    valid           (data, labels) -> (_, losses [T], accs [T]), called under ``torch.no_grad()``
    checkpoints     {file stem: module}: model_checkpoints/model_<stem>_<it+1>.pt every save_every iterations, <stem>.pt by ``save_final``
    extra_metrics   (optional) () -> dict, added to every iteration's logged metrics
    after           (metrics, test_tasks, rank, save_final): what follows training -- the driver's tests and ``save_final()``, in its own
                    order; test_tasks() makes the test ``SyntheticTasks``
    result          what the driver returns beside the metrics

    Returns (result, metrics of the last iteration as ``after`` left them)."""
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    torch.cuda.set_device(local)
    if world > 1:
        init_process_group(local)
    random.seed(p['seed']); np.random.seed(p['seed']); torch.manual_seed(p['seed']); torch.cuda.manual_seed(p['seed'])
    device = torch.device('cuda', local)
    s = setup(device)
    features, all_parameters, checkpoints = s['features'], s['parameters'], s['checkpoints']
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
        # BatchNorm buffers of `features` (saved with every checkpoint): one features(data) pass per task and phase (anil.py fast_adapt)
        fold = None
        if save_dir:
            eng = anil_engine(features, p['ways'], 28 if dataset == 'omni' else 84, device)
            fold = RunningStatsFold(eng, features[0], eng.spec, T, lo, hi, 1, 2 * p['ways'] * p['shots'])
        if ids:
            d, l = train.sample_batch(ids)
            total, losses, accs = s['train'](it, d.to(device), l.to(device))
            total.backward()
            if fold:
                fold.collect(0)
            with torch.no_grad():
                d, l = valid.sample_batch([10 ** 6 + i for i in ids])
                _, vlosses, vaccs = s['valid'](d.to(device), l.to(device))
            if fold:
                fold.collect(1)
            sums = [losses.sum(), accs.sum(), vlosses.sum(), vaccs.sum()]
        else:                                    # meta_batch_size < world size: this rank owns no task, contributes zeros
            sums = [zero, zero, zero, zero]
        flat = torch.cat([(q.grad if q.grad is not None else torch.zeros_like(q)).reshape(-1) for q in all_parameters])
        flat, lsum, asum, ex = reduce_meta_batch(flat, sums[0], sums[1], extra=sums[2:] + ([fold.contribution] if fold else []))
        vlsum, vasum = ex[0], ex[1]                                           # one all-reduce, valid sums (and buffers) included
        if fold:
            fold.apply(ex[2])
        off = 0
        for q in all_parameters:                                                     # anil_vision.py:139-140
            g = flat[off:off + q.numel()].view_as(q) * (1.0 / T)
            q.grad = g.clone() if q.grad is None else q.grad.copy_(g)
            off += q.numel()
        opt.step()
        metrics = {'train_loss': (lsum / T).item(), 'train_acc': (asum / T).item(),
                   'valid_loss': (vlsum / T).item(), 'valid_acc': (vasum / T).item(), **s.get('extra_metrics', dict)()}
        if rank == 0:
            log(f'iter {it}: {metrics}')
            if save_dir and it % p['save_every'] == 0:                                # anil_vision.py:143-145
                # save_model_checkpoint(m, 'features_<it+1>') -> model_checkpoints/model_features_<it+1>.pt (utils/experiment.py:89-90)
                for stem, module in checkpoints.items():
                    torch.save(module.state_dict(), os.path.join(save_dir, 'model_checkpoints', f'model_{stem}_{it + 1}.pt'))

    def save_final():                                                                 # anil_vision.py:163-164
        if rank == 0 and save_dir:
            for stem, module in checkpoints.items():
                torch.save(module.state_dict(), os.path.join(save_dir, f'{stem}.pt'))

    s['after'](metrics, lambda: SyntheticTasks(dataset, p['ways'], p['shots'], 2 * 10 ** 6), rank, save_final)
    if world > 1:
        torch.distributed.destroy_process_group()
    return s['result'], metrics
