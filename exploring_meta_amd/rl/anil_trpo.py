#!/usr/bin/env python3
"""Counterpart of the reference's ``rl/anil_trpo.py`` (:104-129) on Particles2D: ``DiagNormalPolicyANIL`` (tanh body, linear head),
``fast_adapt_trpo(..., anil=True, first_order=True)`` with the body under no_grad during the inner updates, and
``meta_optimize_trpo(..., anil=True)`` -- whose KL Hessian-vector product is exact for new != old
(``PolicyEngine.fvp_general``, for any ``--adapt_steps``).

    python -m exploring_meta_amd.rl.anil_trpo --meta_batch_size 20 --num_iterations 5 [--adapt_steps 2] [--rollout device]
                                              [--inner_lr_per tensor [--per_step_lr] [--freeze mean.0.]]      (fixed steps: see maml_trpo)
"""
import argparse

from .maml_trpo import add_lr_flags, params as _maml_params, run as _run

# rl/anil_trpo.py:20-41 (inner_lr 0.01, outer_lr 0.1, fc_neurons 100); path length / batch sizes as the Particles2D defaults
params = dict(_maml_params, inner_lr=0.01, outer_lr=0.1, fc_neurons=100)


def run(p, log=print, rollout=None):
    return _run(p, log=log, anil=True, rollout=rollout)


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description='ANIL-TRPO on Particles2D (MI355X engine)')
    for k, v in params.items():
        parser.add_argument(f'--{k}', type=type(v), default=v)
    parser.add_argument('--rollout', choices=('host', 'device'), default='host', help='see maml_trpo')
    add_lr_flags(parser)
    args = parser.parse_args()
    for k in params:
        params[k] = getattr(args, k)
    params.update(inner_lr_per=args.inner_lr_per, per_step_lr=args.per_step_lr, freeze=list(args.freeze))
    run(params, rollout=args.rollout)
