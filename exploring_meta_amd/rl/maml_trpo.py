#!/usr/bin/env python3
"""Counterpart of the reference's ``rl/maml_trpo.py`` for Particles2D on the batched HIP policy engine.

Same structure (rl/maml_trpo.py:82-134): per iteration sample ``meta_batch_size`` tasks, for each task
``learner = deepcopy(policy)`` -> ``fast_adapt_trpo(task, learner, baseline, params, first_order=True)``, then
``meta_optimize_trpo(params, policy, baseline, iter_replays, iter_policies)``.  The environment (learn2learn Particles2D) and
the cherry Runner are replaced by ``Particles2DRunner``.  With torchrun the task list is sharded over ranks and the meta
optimisation's means are completed by small all-reduces (core_functions/rl.py::_SurrogateContext._allmean).

    python -m exploring_meta_amd.rl.maml_trpo --meta_batch_size 20 --num_iterations 5 [--rollout device]

``--rollout device`` rolls the episodes out on the device (mi_particles_rollout) for all tasks of the rank at
once through ``fast_adapt_trpo_tasks``.  Iteration ``it``, task ``g`` of the meta-batch, run ``k`` (support steps, then the query) draws
its noise from ``(seed, (it * meta_batch_size + g) * (adapt_steps + 1) + k)``: every rank takes its slice of one global id range, so a
run is reproducible from (seed, iteration, task) at any world size.  The default, ``host``, is the host-loop runner with the torch
generator.

``--inner_lr_per tensor|parameter``, ``--per_step_lr`` and ``--freeze PREFIX ...`` (the PPO driver's flags, without ``--learn_inner_lr``:
TRPO's outer step is a trust region over theta alone) wrap the policy as ``MAML(policy, lr=InnerLR(...))`` with FIXED step sizes per
tensor / per entry (/ per adapt step); a frozen prefix (``mean.0.``: the first Linear) gets the step 0 and moves by the outer step only.
The calls are then mi_policy_adapt_lr / mi_trpo_*_steps_lr.  The defaults build the bare policy, as before.
"""
import argparse
import os
import random
from copy import deepcopy

import numpy as np
import torch

from ..core_functions import (DiagNormalPolicy, DiagNormalPolicyANIL, InnerLR, LinearValue, MAML, Particles2DRunner, fast_adapt_trpo,
                              meta_optimize_trpo, fast_adapt_trpo_tasks, set_device)
from ..sharding import init_process_group, shard_range

params = {
    'inner_lr': 0.1, 'max_path_length': 100, 'adapt_steps': 1, 'adapt_batch_size': 20, 'meta_batch_size': 20,
    'outer_lr': 0.3, 'backtrack_factor': 0.5, 'ls_max_steps': 15, 'max_kl': 0.01, 'tau': 1.0, 'gamma': 0.99,
    'num_iterations': 10, 'seed': 42,
}


def wrap_policy(net, p):
    """The policy the loop works with: ``net`` itself (the reference's run) unless one of --inner_lr_per / --per_step_lr / --freeze asks
    for step sizes per parameter -- then ``MAML(net, lr=InnerLR(..., learnable=False))`` (prefixes name the policy's own parameters,
    ``mean.0.`` = the first Linear)."""
    per, per_step, freeze = p.get('inner_lr_per', 'scalar'), p.get('per_step_lr', False), tuple(p.get('freeze') or ())
    if per == 'scalar' and not per_step and not freeze:
        return net
    lr = InnerLR(net, p['inner_lr'], per=per, steps=max(p['adapt_steps'], 1) if per_step else 1, learnable=False, frozen=freeze)
    return MAML(net, lr=lr.to(net.sigma.device))


def add_lr_flags(parser):
    parser.add_argument('--inner_lr_per', choices=('scalar', 'tensor', 'parameter'), default='scalar',
                        help='fixed inner-loop step sizes: one number (default), one per parameter tensor, or one per entry')
    parser.add_argument('--per_step_lr', action='store_true', help='a row of step sizes per adapt step')
    parser.add_argument('--freeze', nargs='*', default=[], metavar='PREFIX',
                        help="parameter-name prefixes with inner-loop step 0 (e.g. mean.0.): they move by the outer step only")


def run(p, log=print, anil=False, rollout=None):
    rollout = rollout or p.get('rollout', 'host')
    if rollout not in ('host', 'device'):
        raise ValueError("rollout must be 'host' or 'device'")
    world, rank, local = (int(os.environ.get(k, d)) for k, d in (('WORLD_SIZE', '1'), ('RANK', '0'), ('LOCAL_RANK', '0')))
    torch.cuda.set_device(local)
    if world > 1:
        init_process_group(local)
    dev = torch.device('cuda', local)
    set_device(dev)
    random.seed(p['seed']); np.random.seed(p['seed']); torch.manual_seed(p['seed'])
    rng = np.random.RandomState(p['seed'])
    gen = torch.Generator(device=dev).manual_seed(p['seed'] + rank)
    baseline = LinearValue(2, 2)                      # reference passes env.action_size as the ridge coefficient (:85)
    # anil: rl/anil_trpo.py:85 -- tanh body + linear head, inner updates with the body under no_grad (rl.py:381-382)
    policy = wrap_policy((DiagNormalPolicyANIL(2, 2, p.get('fc_neurons', 100)) if anil else DiagNormalPolicy(2, 2)).to(dev), p)
    lo, hi = shard_range(p['meta_batch_size'], rank, world)
    for it in range(p['num_iterations']):
        goals = rng.uniform(-0.5, 0.5, size=(p['meta_batch_size'], 2))        # env.sample_tasks: identical on every rank
        iter_replays, iter_policies, iter_reward, iter_loss = [], [], 0.0, 0.0
        if rollout == 'device':
            runs = p['adapt_steps'] + 1
            results = fast_adapt_trpo_tasks(goals[lo:hi], policy, baseline, p, p['seed'], (it * p['meta_batch_size'] + lo) * runs,
                                            anil=anil, first_order=True)
            iter_policies, iter_replays = [r[0] for r in results], [r[2] for r in results]
            iter_reward = sum(r[3] for r in results)
            iter_loss = sum(torch.stack([r[1].reshape(()) for r in results]).tolist())        # (one read-back for all tasks)
        for goal in (goals[lo:hi] if rollout == 'host' else ()):
            learner = deepcopy(policy)
            task = Particles2DRunner(goal, p['max_path_length'], gen, dev)
            learner, eval_loss, task_replay, task_rew, _ = fast_adapt_trpo(task, learner, baseline, p, anil=anil, first_order=True)
            iter_reward += task_rew
            iter_loss += eval_loss.item()
            iter_replays.append(task_replay)
            iter_policies.append(learner)
        out = meta_optimize_trpo(p, policy, baseline, iter_replays, iter_policies, anil=anil)
        if rank == 0:
            log(f'iter {it}: average_return {iter_reward / (hi - lo):.3f} loss {iter_loss / (hi - lo):.4f} '
                f'line-search step {out["accepted"]}')
    if world > 1:
        torch.distributed.destroy_process_group()
    return policy


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description='MAML-TRPO on Particles2D (MI355X engine)')
    for k, v in params.items():
        parser.add_argument(f'--{k}', type=type(v), default=v)
    parser.add_argument('--anil', action='store_true', help='ANIL-TRPO (reference rl/anil_trpo.py): DiagNormalPolicyANIL, head-only inner loop')
    parser.add_argument('--rollout', choices=('host', 'device'), default='host',
                        help='host: Python loop over the steps, torch-generator noise; device: one mi_particles_rollout call per adapt step')
    add_lr_flags(parser)
    args = parser.parse_args()
    for k in params:
        params[k] = getattr(args, k)
    params.update(inner_lr_per=args.inner_lr_per, per_step_lr=args.per_step_lr, freeze=list(args.freeze))
    run(params, anil=args.anil, rollout=args.rollout)
