#!/usr/bin/env python3
"""Counterpart of the reference's ``vision/anil_vision.py`` on the batched HIP engine.

Same experiment: ``features = Sequential(ConvBase(...), Lambda(view(-1, fc_neurons)))``, ``head = MAML(Linear(fc_neurons,
ways), lr)``, Adam over trunk + head, CrossEntropy, per-iteration train + validation meta-batches, gradient /
meta_batch_size (anil_vision.py:86-99,110-141) -- with the ``for task in range(meta_batch_size)`` loop (:114-132) as ONE
``meta_batch_adapt_anil`` call per half (mi_meta_batch_anil: trunk once on all rows, head-only inner loop, outer gradient into
trunk and head), task-sharded over ranks under ``torchrun`` with one RCCL all-reduce.  Tasks come from the seeded synthetic
generator (datasets are not available offline).

    python -m exploring_meta_amd.vision.anil_vision --dataset min --shots 5 --adapt_steps 1 --num_iterations 10

``--proto_init`` (Proto-MAML, ``core_functions/proto_anil.py``): the head's inner loop starts, per task, from the support prototypes instead
of from the learned ``head``; ``log_scale`` is optimised beside trunk and step sizes (``--fix_proto_scale``: it stays at
``--proto_scale``), ``proto_init.pt`` is saved beside ``head.pt``, and the driver returns ``(features, head, init)``.
"""
import argparse
import os

import torch

from ..core_functions import MAML, ConvBase, InnerLR, msl_weights
from ..core_functions.anil import meta_batch_adapt_anil, meta_batch_adapt_anil_steps
from ..core_functions.proto_anil import ProtoInit, meta_batch_adapt_proto_anil
from .maml_vision import add_trunk_test_flags, inner_lr_of, trunk_test_params, trunk_tests
from .trunk_loop import train_trunk

params = {
    "ways": 5, "shots": 5, "outer_lr": 0.003, "inner_lr": 0.5, "adapt_steps": 1, "meta_batch_size": 32,
    "num_iterations": 10000, "save_every": 1000, "seed": 42,
}


class Lambda(torch.nn.Module):
    """reference anil_vision.py:46-53"""

    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, x):
        return self.fn(x)


def build(dataset, ways, inner_lr, device, p=None):
    """features / head exactly as the reference constructs them (anil_vision.py:40-43,86-94).  p: the run's parameters when the flags
    --inner_lr_per / --learn_inner_lr / --per_step_lr / --freeze ask for step sizes per head parameter (an ``InnerLR`` over the head's
    ``weight`` / ``bias``, as in vision.maml_vision); else the plain number."""
    if dataset == 'omni':
        fc_neurons = 128
        features = ConvBase(output_size=64, hidden=32, channels=1, max_pool=False)
    else:
        fc_neurons = 1600
        features = ConvBase(output_size=64, channels=3, max_pool=True)
    features = torch.nn.Sequential(features, Lambda(lambda x: x.view(-1, fc_neurons))).to(device)
    linear = torch.nn.Linear(fc_neurons, ways).to(device)
    head = MAML(linear, lr=inner_lr if p is None else inner_lr_of(linear, p)).to(device)
    return features, head


def run(dataset, p, log=print):
    def setup(device):
        features, head = build(dataset, p['ways'], p['inner_lr'], device, p)
        msl_its = int(p.get('msl_iterations', 0)) if p.get('multi_step_loss') and p['adapt_steps'] >= 1 else 0
        step_w = torch.zeros(max(p['adapt_steps'], 1), device=device)      # annealed in place: the engine reads the weights on the device
        init = ProtoInit(p.get('proto_scale', 1.0), learnable=not p.get('fix_proto_scale')).to(device) if p.get('proto_init') else None

        def plain(data, labels):
            if init is None:
                return meta_batch_adapt_anil(head.clone(), features, data, labels, p['adapt_steps'], p['shots'], p['ways'])
            return meta_batch_adapt_proto_anil(head.clone(), features, init, data, labels, p['adapt_steps'], p['shots'], p['ways'])

        def adapt(it, data, labels):
            """One fused call: the multi-step loss while it < --msl_iterations (--multi_step_loss), else the plain call.  The logged loss and
            accuracy are those of the last step either way."""
            if it >= msl_its or not torch.is_grad_enabled():
                return plain(data, labels)
            step_w.copy_(torch.tensor(msl_weights(p['adapt_steps'], it, msl_its)))
            if init is None:
                total, losses, accs = meta_batch_adapt_anil_steps(head.clone(), features, data, labels, p['adapt_steps'], p['shots'], p['ways'],
                                                                  step_weights=step_w)
            else:
                total, losses, accs = meta_batch_adapt_proto_anil(head.clone(), features, init, data, labels, p['adapt_steps'], p['shots'],
                                                                  p['ways'], step_weights=step_w)
            return total, losses[-1], accs[-1]

        def after(metrics, test_tasks, rank, save_final):
            save_final()
            if rank == 0 and p.get('save_dir') and isinstance(head.lr, InnerLR):
                torch.save(head.lr.state_dict(), os.path.join(p['save_dir'], 'inner_lr.pt'))
            trunk_tests(p, test_tasks, features, device, rank, metrics, log)

        # anil_vision.py:97; head.parameters() includes a learnable InnerLR's values (a submodule of MAML), so they are stepped by the
        # optimiser and all-reduced with the rest
        s = dict(features=features, parameters=list(features.parameters()) + list(head.parameters()), train=adapt, valid=plain,
                 checkpoints={'features': features, 'head': head}, after=after, result=(features, head))
        if init is not None:             # log_scale beside trunk and step sizes; the head's weight and bias receive zeros and stay
            s['parameters'] += list(init.parameters())
            s['checkpoints']['proto_init'] = init
            s.update(extra_metrics=lambda: {'proto_scale': init.scale}, result=(features, head, init))
        return s

    return train_trunk(dataset, p, log, setup)


def build_parser():
    parser = argparse.ArgumentParser(description='ANIL on Vision (MI355X engine)')
    parser.add_argument('--dataset', type=str, default='min', help='omni or min')
    for k, v in params.items():
        parser.add_argument(f'--{k}', type=type(v), default=v)
    parser.add_argument('--save_dir', type=str, default='', help='write model_checkpoints/model_{features,head}_<it+1>.pt every save_every iterations and features.pt / head.pt (/ inner_lr.pt) at the end')
    parser.add_argument('--inner_lr_per', choices=('scalar', 'tensor', 'parameter'), default='scalar',
                        help="one inner step size for the head, per tensor of it ('weight', 'bias') or per entry")
    parser.add_argument('--learn_inner_lr', action='store_true', help='the inner step sizes are meta-learned with the model (MetaSGD)')
    parser.add_argument('--per_step_lr', action='store_true', help='one set of step sizes per inner step')
    parser.add_argument('--freeze', nargs='+', default=[], metavar='PREFIX', help="prefixes of the head's parameter names that are not adapted ('weight', 'bias')")
    parser.add_argument('--multi_step_loss', action='store_true',
                        help='MAML++ multi-step loss: the outer objective weights the query loss after every head step (msl_weights)')
    parser.add_argument('--msl_iterations', type=int, default=0, metavar='N',
                        help='iterations over which the multi-step weights anneal to the final step; from iteration N on the plain call runs')
    parser.add_argument('--proto_init', action='store_true',
                        help="Proto-MAML: the head's inner loop starts from the task's support prototypes (W_0 = 2 s c, b_0 = -s |c|^2), not from the learned head")
    parser.add_argument('--proto_scale', type=float, default=1.0, metavar='S', help='the initial scale s of --proto_init')
    parser.add_argument('--fix_proto_scale', action='store_true', help='s stays at --proto_scale (not meta-learned)')
    add_trunk_test_flags(parser, 'after training')
    return parser


def parse_args(argv=None):
    return build_parser().parse_args(argv)


def params_of(args):
    """The run's parameter dict from parsed flags (the defaults are the reference's run)."""
    p = {k: getattr(args, k) for k in params}
    p.update(save_dir=args.save_dir, inner_lr_per=args.inner_lr_per, learn_inner_lr=args.learn_inner_lr, per_step_lr=args.per_step_lr,
             freeze=list(args.freeze), multi_step_loss=args.multi_step_loss, msl_iterations=args.msl_iterations, proto_init=args.proto_init,
             proto_scale=args.proto_scale, fix_proto_scale=args.fix_proto_scale, **trunk_test_params(args))
    return p


def main(argv=None, log=print):
    """Parse the flags and run; returns ((features, head), metrics of the last iteration); with --proto_init (features, head, init)."""
    args = parse_args(argv)
    p = dict(params)
    p.update(params_of(args))
    return run(args.dataset, p, log=log)


if __name__ == '__main__':
    main()
