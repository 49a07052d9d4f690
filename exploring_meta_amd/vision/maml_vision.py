#!/usr/bin/env python3
"""Counterpart of the reference's ``vision/maml_vision.py`` on the batched HIP engine.

Same experiment (seeds, model, ``MAML(model, lr, first_order)``, Adam(outer_lr), CrossEntropy, per-iteration train +
validation meta-batches, gradient / meta_batch_size, meta-test with ``evaluate``), same flags plus ``--first_order`` (the
reference hard-codes second order, maml_vision.py:84) -- but the ``for task in range(meta_batch_size)`` loop
(maml_vision.py:102-124) is ONE ``meta_batch_adapt`` call for both halves (train tasks with, validation tasks without the backward
half: ``grad_tasks``), and with ``torchrun`` the meta-batch is sharded over
ranks with one RCCL all-reduce.  Datasets are not available offline: tasks come from the seeded synthetic generator
(``utils/synthetic.py``) with the reference's batch layout.

    python -m exploring_meta_amd.vision.maml_vision --dataset min --shots 5 --adapt_steps 5 --num_iterations 10
"""
import argparse
import os
import random

import numpy as np
import torch

from ..core_functions import MAML, InnerLR, StepOffsets, MiniImagenetCNN, OmniglotCNN, evaluate, meta_batch_adapt, meta_batch_adapt_steps, msl_weights
from ..core_functions.vision_models import RunningStatsFold
from ..sharding import init_process_group, reduce_meta_batch, shard_range
from ..utils import synthetic

params = {
    "ways": 5, "shots": 1, "outer_lr": 0.003, "inner_lr": 0.5, "adapt_steps": 1, "meta_batch_size": 32,
    "num_iterations": 10000, "save_every": 1000, "seed": 42,
}


class SyntheticTasks:
    """Stand-in for an l2l TaskDataset: ``sample()`` returns (data [2*S*W,C,H,W], labels [2*S*W])."""

    def __init__(self, dataset, ways, shots, first_id):
        self.dataset, self.ways, self.shots, self.next = dataset, ways, shots, first_id

    def sample(self):
        d, l = synthetic.make_task(self.dataset, self.next, self.ways, self.shots)
        self.next += 1
        return torch.from_numpy(d), torch.from_numpy(l)

    def sample_batch(self, ids):
        d, l = synthetic.make_meta_batch(self.dataset, ids, self.ways, self.shots)
        return torch.from_numpy(d), torch.from_numpy(l)


def inner_lr_of(model, p):
    """The ``lr`` argument of ``MAML`` for these parameters: the plain number (the reference's run) unless one of
    --inner_lr_per / --learn_inner_lr / --per_step_lr / --freeze asks for step sizes per parameter."""
    per, learn, per_step, freeze = p.get('inner_lr_per', 'scalar'), p.get('learn_inner_lr', False), p.get('per_step_lr', False), \
        tuple(p.get('freeze') or ())
    if p.get('per_step_bn') and not p.get('per_step_bn_adapt_bn'):
        # MAML++'s default: the BatchNorm tensors carry per-step offsets and leave the inner loop (step size 0)
        freeze += tuple(n for n in StepOffsets(model, 1, 'bn', learnable=False).bn_prefixes() if not any(n.startswith(f) for f in freeze))
    if per == 'scalar' and not learn and not per_step and not freeze:
        return p['inner_lr']
    return InnerLR(model, p['inner_lr'], per=per, steps=max(p['adapt_steps'], 1) if per_step else 1, learnable=learn, frozen=freeze)


def step_offsets_of(model, p):
    """The ``offsets`` argument of ``MAML``: None (today's run) unless --per_step_bn asks for per-step BatchNorm weights and biases."""
    if not p.get('per_step_bn'):
        return None
    if p['adapt_steps'] < 1:
        raise ValueError('--per_step_bn needs --adapt_steps >= 1')
    return StepOffsets(model, p['adapt_steps'], 'bn')


def add_trunk_test_flags(parser, when, note=''):
    """--nil_test / --ridge_test (--ridge_lam, --ridge_scale) / --logreg_test (--logreg_lam, --logreg_scale): the trunk alone under a
    closed-form or exactly solved head, scored ``when``."""
    parser.add_argument('--nil_test', action='store_true',
                        help=f'{when} also log nil_test_acc: the trunk scored on meta_batch_size test tasks by the NIL cosine head, no inner loop{note}')
    parser.add_argument('--ridge_test', action='store_true',
                        help=f'{when} also log ridge_test_acc: the trunk under the exactly solved ridge-regression head (R2-D2) with the fixed '
                             f'--ridge_lam / --ridge_scale, no inner loop{note}')
    parser.add_argument('--ridge_lam', type=float, default=1.0, metavar='LAM', help="--ridge_test: the ridge head's regulariser")
    parser.add_argument('--ridge_scale', type=float, default=1.0, metavar='S', help="--ridge_test: the ridge head's logit scale")
    parser.add_argument('--logreg_test', action='store_true',
                        help=f'{when} also log logreg_test_acc: the trunk under the logistic-regression head solved to convergence (the limit of '
                             f"ANIL's inner loop under its own loss) with the fixed --logreg_lam / --logreg_scale{note}")
    parser.add_argument('--logreg_lam', type=float, default=1.0, metavar='LAM', help="--logreg_test: the head's regulariser")
    parser.add_argument('--logreg_scale', type=float, default=1.0, metavar='S', help="--logreg_test: the head's logit scale")


def trunk_test_params(args):
    return dict(nil_test=args.nil_test, ridge_test=args.ridge_test, ridge_lam=args.ridge_lam, ridge_scale=args.ridge_scale,
                logreg_test=args.logreg_test, logreg_lam=args.logreg_lam, logreg_scale=args.logreg_scale)


def trunk_tests(p, test_tasks, trunk, device, rank, metrics, log):
    """--nil_test: how good are the features alone?  The head is thrown away (NIL, no inner loop).  --ridge_test: how good is the exactly
    solved head on these features (R2-D2's ridge regression, fixed lam / scale)?  --logreg_test: the same question under the loss ANIL's
    inner loop runs (logistic regression solved to convergence).  Each on meta_batch_size tasks of its own ``test_tasks()``."""
    if p.get('nil_test'):
        from ..core_functions.metric import evaluate_nil
        metrics['nil_test_acc'] = evaluate_nil(p, test_tasks(), trunk, device)
        if rank == 0:
            log(f"nil_test_acc: {metrics['nil_test_acc']}")
    if p.get('ridge_test'):
        from ..core_functions.ridge import RidgeHead, evaluate_ridge
        metrics['ridge_test_acc'] = evaluate_ridge(p, test_tasks(), trunk, RidgeHead(p['ridge_lam'], p['ridge_scale'], learnable=False), device)
        if rank == 0:
            log(f"ridge_test_acc: {metrics['ridge_test_acc']}")
    if p.get('logreg_test'):
        from ..core_functions.logreg import LogRegHead, evaluate_logreg
        metrics['logreg_test_acc'] = evaluate_logreg(p, test_tasks(), trunk, LogRegHead(p['logreg_lam'], p['logreg_scale'], learnable=False), device)
        if rank == 0:
            log(f"logreg_test_acc: {metrics['logreg_test_acc']}")


def run(dataset, p, first_order=False, log=print):
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    torch.cuda.set_device(local)
    if world > 1:
        init_process_group(local)
    random.seed(p['seed']); np.random.seed(p['seed']); torch.manual_seed(p['seed']); torch.cuda.manual_seed(p['seed'])
    device = torch.device('cuda', local)
    model = (OmniglotCNN(p['ways']) if dataset == 'omni' else MiniImagenetCNN(p['ways'])).to(device)
    if p.get('ridge_test') and isinstance(model, OmniglotCNN):
        raise NotImplementedError('--ridge_test scores flattened features; OmniglotCNN feeds its head their spatial mean (use --dataset min)')
    if p.get('logreg_test') and isinstance(model, OmniglotCNN):
        raise NotImplementedError('--logreg_test scores flattened features; OmniglotCNN feeds its head their spatial mean (use --dataset min)')
    if p.get('nil_test') and isinstance(model, OmniglotCNN):      # (before the training, not after it)
        raise NotImplementedError('--nil_test scores flattened features; OmniglotCNN feeds its head their spatial mean (use --dataset min)')
    maml = MAML(model, lr=inner_lr_of(model, p), first_order=first_order, offsets=step_offsets_of(model, p))
    opt = torch.optim.Adam(maml.parameters(), p['outer_lr'])
    # MAML++'s cosine outer schedule over the run (--cosine_outer_lr); None: the constant outer_lr, today's run
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=max(p['num_iterations'], 1), eta_min=p.get('min_outer_lr', 0.0)) \
        if p.get('cosine_outer_lr') else None
    fo_its = int(p.get('first_order_iterations', 0))      # MAML++'s derivative-order annealing: iterations < N make the first-order call
    loss = torch.nn.CrossEntropyLoss(reduction='mean')
    T = p['meta_batch_size']
    lo, hi = shard_range(T, rank, world)
    train, valid = SyntheticTasks(dataset, p['ways'], p['shots'], 0), SyntheticTasks(dataset, p['ways'], p['shots'], 10 ** 6)
    metrics = {}
    zero = torch.zeros((), device=device)
    save_dir = p.get('save_dir') or ''
    if save_dir and rank == 0:
        os.makedirs(os.path.join(save_dir, 'model_checkpoints'), exist_ok=True)
    msl_its = int(p.get('msl_iterations', 0)) if p.get('multi_step_loss') and p['adapt_steps'] >= 1 else 0
    step_w = torch.zeros(max(p['adapt_steps'], 1), device=device)      # annealed in place: the engine reads the weights on the device

    def adapt(it, data, labels, grad_tasks=None):
        """One fused call for these tasks: the multi-step loss of MAML++ while it < --msl_iterations (--multi_step_loss), else the plain call.
        (objective, losses [T], accs [T]) -- the logged loss and accuracy are those of the last step either way."""
        learner = maml.clone(first_order=True) if it < fo_its else maml.clone()
        if it >= msl_its or not torch.is_grad_enabled():
            return meta_batch_adapt(learner, data, labels, p['adapt_steps'], p['shots'], p['ways'], grad_tasks=grad_tasks)
        step_w.copy_(torch.tensor(msl_weights(p['adapt_steps'], it, msl_its)))
        total, losses, accs = meta_batch_adapt_steps(learner, data, labels, p['adapt_steps'], p['shots'], p['ways'], step_weights=step_w,
                                                     grad_tasks=grad_tasks)
        return total, losses[-1], accs[-1]

    for it in range(p['num_iterations']):
        opt.zero_grad()
        ids = list(range(it * T + lo, it * T + hi))
        # BatchNorm buffers (saved with every checkpoint, utils/experiment.py:85-90): tracked when checkpoints are written
        fold = RunningStatsFold(model.engine(), model.base, model.spec(), T, lo, hi, p['adapt_steps'] + 1,
                                p['ways'] * p['shots']) if save_dir else None
        if ids and not fold:
            # train and validation halves of the iteration (maml_vision.py:102-124) in ONE fused call: the first len(ids) tasks carry
            # the backward half, the validation tasks ride through the same launches
            d, l = train.sample_batch(ids)
            dv, lv = valid.sample_batch([10 ** 6 + i for i in ids])
            n = len(ids)
            total, losses, accs = adapt(it, torch.cat([d, dv]).to(device), torch.cat([l, lv]).to(device), grad_tasks=n)
            total.backward()                                                 # accumulates the SUM over this rank's train tasks
            sums = [losses[:n].sum(), accs[:n].sum(), losses[n:].sum(), accs[n:].sum()]
        elif ids:                                # with checkpoints: two calls, so that the BatchNorm buffers fold in the reference's call order
            d, l = train.sample_batch(ids)
            total, losses, accs = adapt(it, d.to(device), l.to(device))
            total.backward()                                                 # accumulates the SUM over this rank's tasks
            fold.collect(0)
            with torch.no_grad():
                d, l = valid.sample_batch([10 ** 6 + i for i in ids])
                _, vlosses, vaccs = meta_batch_adapt(maml.clone(), d.to(device), l.to(device), p['adapt_steps'], p['shots'], p['ways'])
            fold.collect(1)
            sums = [losses.sum(), accs.sum(), vlosses.sum(), vaccs.sum()]
        else:                                    # meta_batch_size < world size: this rank owns no task, contributes zeros
            sums = [zero, zero, zero, zero]
        flat = torch.cat([(q.grad if q.grad is not None else torch.zeros_like(q)).reshape(-1) for q in maml.parameters()])
        flat, lsum, asum, ex = reduce_meta_batch(flat, sums[0], sums[1], extra=sums[2:] + ([fold.contribution] if fold else []))
        vlsum, vasum = ex[0], ex[1]                                           # one all-reduce, valid sums (and buffers) included
        if fold:
            fold.apply(ex[2])
        off = 0
        for q in maml.parameters():                                          # maml_vision.py:139-140
            g = flat[off:off + q.numel()].view_as(q) * (1.0 / T)
            q.grad = g.clone() if q.grad is None else q.grad.copy_(g)
            off += q.numel()
        opt.step()
        if sched is not None:
            sched.step()
        metrics = {'train_loss': (lsum / T).item(), 'train_acc': (asum / T).item(),
                   'valid_loss': (vlsum / T).item(), 'valid_acc': (vasum / T).item()}
        if rank == 0:
            log(f'iter {it}: {metrics}')
            if save_dir and it % p['save_every'] == 0:                        # maml_vision.py:143-144, utils/experiment.py:85-90
                torch.save(model.state_dict(), os.path.join(save_dir, 'model_checkpoints', f'model_{it}.pt'))
    test = SyntheticTasks(dataset, p['ways'], p['shots'], 2 * 10 ** 6)
    metrics['test_acc'] = evaluate(p, test, maml, loss, device)
    trunk_tests(p, lambda: SyntheticTasks(dataset, p['ways'], p['shots'], 2 * 10 ** 6), model, device, rank, metrics, log)
    if world > 1:
        torch.distributed.destroy_process_group()
    if save_dir and rank == 0:
        torch.save(model.state_dict(), os.path.join(save_dir, 'model.pt'))       # utils/experiment.py:85-87
        if isinstance(maml.lr, InnerLR):
            torch.save(maml.lr.state_dict(), os.path.join(save_dir, 'inner_lr.pt'))
        if maml.offsets is not None:
            torch.save(maml.offsets.state_dict(), os.path.join(save_dir, 'step_offsets.pt'))
    return model, metrics


def build_parser():
    parser = argparse.ArgumentParser(description='MAML on Vision (MI355X engine)')
    parser.add_argument('--dataset', type=str, default='min', help='omni or min')
    for k, v in params.items():
        parser.add_argument(f'--{k}', type=type(v), default=v)
    parser.add_argument('--first_order', action='store_true')
    parser.add_argument('--save_dir', type=str, default='', help='write model_checkpoints/model_<it>.pt every save_every iterations and model.pt at the end (reference state_dict keys)')
    parser.add_argument('--inner_lr_per', choices=('scalar', 'tensor', 'parameter'), default='scalar',
                        help='one inner step size per model, per parameter tensor or per entry')
    parser.add_argument('--learn_inner_lr', action='store_true', help='the inner step sizes are meta-learned with the model (MetaSGD)')
    parser.add_argument('--per_step_lr', action='store_true', help='one set of step sizes per inner step')
    parser.add_argument('--freeze', nargs='+', default=[], metavar='PREFIX', help="parameter-name prefixes that are not adapted (e.g. 'base.0.')")
    parser.add_argument('--multi_step_loss', action='store_true',
                        help='MAML++ multi-step loss: the outer objective weights the query loss after every inner step (msl_weights)')
    parser.add_argument('--msl_iterations', type=int, default=0, metavar='N',
                        help='iterations over which the multi-step weights anneal to the final step; from iteration N on the plain call runs')
    parser.add_argument('--per_step_bn', action='store_true',
                        help='MAML++ per-step BatchNorm weights and biases: learnable per-step offsets on the BatchNorm tensors, which leave the inner loop')
    parser.add_argument('--per_step_bn_adapt_bn', action='store_true', help='with --per_step_bn: the BatchNorm tensors stay in the inner loop')
    parser.add_argument('--first_order_iterations', type=int, default=0, metavar='N',
                        help='MAML++ derivative-order annealing: iterations < N make the first-order call')
    parser.add_argument('--cosine_outer_lr', action='store_true', help='cosine-anneal the outer learning rate over num_iterations')
    parser.add_argument('--min_outer_lr', type=float, default=0.0, metavar='X', help='the floor of --cosine_outer_lr')
    add_trunk_test_flags(parser, 'after the test accuracy', ' (flattened features: --dataset min)')
    return parser


def params_of(args):
    """The run's parameter dict from parsed flags (the defaults are the reference's run)."""
    p = {k: getattr(args, k) for k in params}
    p.update(save_dir=args.save_dir, inner_lr_per=args.inner_lr_per, learn_inner_lr=args.learn_inner_lr, per_step_lr=args.per_step_lr,
             freeze=list(args.freeze), multi_step_loss=args.multi_step_loss, msl_iterations=args.msl_iterations,
             per_step_bn=args.per_step_bn, per_step_bn_adapt_bn=args.per_step_bn_adapt_bn, first_order_iterations=args.first_order_iterations,
             cosine_outer_lr=args.cosine_outer_lr, min_outer_lr=args.min_outer_lr, **trunk_test_params(args))
    return p


def main(argv=None, log=print):
    """Parse the flags and run; returns (model, metrics of the last iteration)."""
    args = build_parser().parse_args(argv)
    p = dict(params)
    p.update(params_of(args))
    return run(args.dataset, p, first_order=args.first_order, log=log)


if __name__ == '__main__':
    main()
