#!/usr/bin/env python3
"""Prototypical Networks (and the NIL cosine head as a training objective) on the 4-conv trunk of ``vision/anil_vision.py``, on the
batched HIP engine: no inner loop, no head.

``features = Sequential(ConvBase(...), Lambda(view(-1, fc_neurons)))`` as in the ANIL driver, Adam over the trunk, per-iteration train +
validation meta-batches, gradient / meta_batch_size -- each half ONE ``meta_batch_adapt_metric`` call (mi_meta_batch_metric: the trunk
once on all rows, one metric-head launch for the whole meta-batch, the trunk backward), task-sharded over ranks under ``torchrun`` with
one RCCL all-reduce.  Meta-test by ``evaluate_nil`` with the training metric.  The trunk's checkpoints carry the ANIL driver's names
(``model_checkpoints/model_features_<it+1>.pt``, ``features.pt``), so a ProtoNet trunk loads wherever an ANIL trunk does.  Tasks come
from the seeded synthetic generator (datasets are not available offline).

    python -m exploring_meta_amd.vision.protonet_vision --dataset min --shots 5 --metric proto --scale 0.00390625 --num_iterations 10
"""
import argparse

from ..core_functions.metric import evaluate_nil, meta_batch_adapt_metric
from . import anil_vision
from .trunk_loop import train_trunk

params = {
    "ways": 5, "shots": 5, "outer_lr": 0.003, "meta_batch_size": 32, "num_iterations": 10000, "save_every": 1000, "seed": 42,
    "metric": "proto", "scale": 1.0,
}


def build(dataset, ways, device):
    """The ANIL driver's ``features`` (its head is built and dropped: a metric head has no parameters)."""
    features, _ = anil_vision.build(dataset, ways, 0.0, device)
    return features


def run(dataset, p, log=print):
    head = dict(metric=p['metric'], scale=p['scale'])

    def setup(device):
        features = build(dataset, p['ways'], device)

        def after(metrics, test_tasks, rank, save_final):
            metrics['test_acc'] = evaluate_nil(p, test_tasks(), features, device, **head)
            save_final()

        return dict(features=features, parameters=list(features.parameters()),
                    train=lambda it, d, l: meta_batch_adapt_metric(features, d, l, p['shots'], p['ways'], **head),
                    valid=lambda d, l: meta_batch_adapt_metric(features, d, l, p['shots'], p['ways'], **head),
                    checkpoints={'features': features}, after=after, result=features)

    return train_trunk(dataset, p, log, setup)


def build_parser():
    parser = argparse.ArgumentParser(description='Prototypical Networks / NIL head on Vision (MI355X engine)')
    parser.add_argument('--dataset', type=str, default='min', help='omni or min')
    for k, v in params.items():
        if k == 'metric':
            parser.add_argument('--metric', choices=('proto', 'cosine'), default=v,
                                help='proto: class means and squared distances; cosine: the NIL head, summed cosine similarities')
        else:
            parser.add_argument(f'--{k}', type=type(v), default=v)
    parser.add_argument('--save_dir', type=str, default='',
                        help='write model_checkpoints/model_features_<it+1>.pt every save_every iterations and features.pt at the end (the ANIL driver\'s names)')
    return parser


def main(argv=None, log=print):
    """Parse the flags and run; returns (features, metrics of the last iteration with test_acc)."""
    args = build_parser().parse_args(argv)
    p = dict(params)
    p.update({k: getattr(args, k) for k in params})
    p['save_dir'] = args.save_dir
    return run(args.dataset, p, log=log)


if __name__ == '__main__':
    main()
