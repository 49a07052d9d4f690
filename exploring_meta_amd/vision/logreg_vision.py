#!/usr/bin/env python3
"""The logistic-regression head on the 4-conv trunk of ``vision/anil_vision.py``, on the batched HIP engine: the head's inner problem
under softmax cross-entropy solved to convergence on the support set (the limit of ANIL's inner loop under its own loss), differentiated
through the optimum; the regulariser and the logit scale are meta-learned with the trunk.

``features = Sequential(ConvBase(...), Lambda(view(-1, fc_neurons)))`` as in the ANIL driver, Adam over the trunk and the head's two
scalars (``LogRegHead``: log_lam, log_scale), per-iteration train + validation meta-batches, gradient / meta_batch_size -- each half ONE
``meta_batch_adapt_logreg`` call (mi_meta_batch_logreg: the trunk once on all rows, one head launch for the whole meta-batch, the trunk
backward), task-sharded over ranks under ``torchrun`` with one RCCL all-reduce.  Meta-test by ``evaluate_logreg``.  The trunk's
checkpoints carry the ANIL driver's names (``model_checkpoints/model_features_<it+1>.pt``, ``features.pt``), with the head's two scalars
beside them (``model_logreg_head_<it+1>.pt``, ``logreg_head.pt``), so a trunk trained here loads wherever an ANIL trunk does.  Tasks come
from the seeded synthetic generator (datasets are not available offline).

    python -m exploring_meta_amd.vision.logreg_vision --dataset min --shots 5 --lam 50 --scale 1 --num_iterations 10
"""
import argparse

from ..core_functions.logreg import LogRegHead, evaluate_logreg, meta_batch_adapt_logreg
from . import anil_vision
from .trunk_loop import train_trunk

params = {
    "ways": 5, "shots": 5, "outer_lr": 0.003, "meta_batch_size": 32, "num_iterations": 10000, "save_every": 1000, "seed": 42,
    "lam": 1.0, "scale": 1.0,
}


def build(dataset, ways, device, lam=1.0, scale=1.0, fix_head=False):
    """The ANIL driver's ``features`` (its linear head is built and dropped) and the head's two scalars."""
    features, _ = anil_vision.build(dataset, ways, 0.0, device)
    return features, LogRegHead(lam, scale, learnable=not fix_head).to(device)


def run(dataset, p, log=print):
    def setup(device):
        features, head = build(dataset, p['ways'], device, p['lam'], p['scale'], p.get('fix_head', False))

        def after(metrics, test_tasks, rank, save_final):
            metrics['test_acc'] = evaluate_logreg(p, test_tasks(), features, head, device)
            save_final()

        return dict(features=features, parameters=list(features.parameters()) + list(head.parameters()),
                    train=lambda it, d, l: meta_batch_adapt_logreg(features, head, d, l, p['shots'], p['ways']),
                    valid=lambda d, l: meta_batch_adapt_logreg(features, head, d, l, p['shots'], p['ways']),
                    checkpoints={'features': features, 'logreg_head': head}, extra_metrics=lambda: {'lam': head.lam, 'scale': head.scale},
                    after=after, result=(features, head))

    return train_trunk(dataset, p, log, setup)


def build_parser():
    parser = argparse.ArgumentParser(description='Logistic-regression head solved to convergence on Vision (MI355X engine)')
    parser.add_argument('--dataset', type=str, default='min', help='omni or min')
    for k, v in params.items():
        parser.add_argument(f'--{k}', type=type(v), default=v)
    parser.add_argument('--fix_head', action='store_true', help='lam and scale stay at their initial values (not meta-learned)')
    parser.add_argument('--save_dir', type=str, default='',
                        help="write model_checkpoints/model_{features,logreg_head}_<it+1>.pt every save_every iterations and features.pt / "
                             "logreg_head.pt at the end (the trunk under the ANIL driver's names)")
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
