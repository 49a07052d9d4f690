#!/usr/bin/env python3
"""Counterpart of the reference's ``rl/maml_ppo.py`` (and ``rl/anil_ppo.py`` with ``--anil``) for Particles2D on the HIP
policy engine.

Same structure (rl/maml_ppo.py:84-131): ``policy = MAML(DiagNormalPolicy(...), lr=inner_lr)``, Adam(outer_lr) on its
parameters; per iteration and task ``learner = policy.clone()`` -> ``fast_adapt_ppo(task, learner, baseline, params)`` ->
``(eval_loss, reward, success)``; ``av_loss = sum / meta_batch_size``; ``av_loss.backward(); meta_optimizer.step()``.  The
second-order gradient through the ``ppo_epochs`` clipped-surrogate updates comes out of one fused call per task
(mi_policy_meta_batch).  Under torchrun the task list is sharded over ranks and the gradients are all-reduced (RCCL).

With ``--rollout device --batch_tasks`` a rank adapts its whole slice of the tasks in one batched call
(``fast_adapt_ppo_tasks``: per adapt step one rollout, one advantage launch and one mi_policy_update call over all tasks, then one
mi_policy_meta_batch call for the losses and the summed gradient), with the rollout ids the task loop uses.

``--inner_lr_per tensor|parameter``, ``--learn_inner_lr``, ``--per_step_lr`` and ``--freeze PREFIX ...`` (the vision driver's flags) build
``MAML(net, lr=InnerLR(...))``: one inner step size per tensor / entry / adapt step, meta-learned with the policy, tensors frozen by name
prefix; the fused calls are then mi_policy_update_lr / mi_policy_meta_batch_lr.  The defaults build ``MAML(net, lr=inner_lr)``.

    python -m exploring_meta_amd.rl.maml_ppo --meta_batch_size 20 --num_iterations 5 [--anil] [--rollout device [--batch_tasks]]
                                             [--inner_lr_per tensor --learn_inner_lr [--per_step_lr] [--freeze mean.0.]]
"""
import argparse
import os
import random

import numpy as np
import torch

from ..core_functions import (MAML, DiagNormalPolicy, DiagNormalPolicyANIL, InnerLR, LinearValue, Particles2DRunner, fast_adapt_ppo,
                              fast_adapt_ppo_tasks, set_device)
from ..sharding import init_process_group, shard_range

params = {
    'ppo_epochs': 3, 'ppo_clip_ratio': 0.1, 'inner_lr': 0.01, 'max_path_length': 100, 'adapt_steps': 1, 'adapt_batch_size': 20,
    'meta_batch_size': 20, 'outer_lr': 0.01, 'activation': 'tanh', 'tau': 1.0, 'gamma': 0.99, 'num_iterations': 10, 'seed': 42,
}


def inner_lr_of(net, p):
    """The ``lr`` argument of ``MAML`` for these parameters: the plain number (the reference's run) unless one of --inner_lr_per /
    --learn_inner_lr / --per_step_lr / --freeze asks for step sizes per parameter (the vision driver's flags; prefixes name the
    policy's parameters: 'mean.0.', 'body.0.', 'head.', 'sigma')."""
    per, learn, per_step, freeze = p.get('inner_lr_per', 'scalar'), p.get('learn_inner_lr', False), p.get('per_step_lr', False), \
        tuple(p.get('freeze') or ())
    if per == 'scalar' and not learn and not per_step and not freeze:
        return p['inner_lr']
    return InnerLR(net, p['inner_lr'], per=per, steps=max(p['adapt_steps'], 1) if per_step else 1, learnable=learn, frozen=freeze)


def run(p, anil=False, log=print, rollout=None, batch_tasks=False):
    rollout = rollout or p.get('rollout', 'host')
    if rollout not in ('host', 'device'):
        raise ValueError("rollout must be 'host' or 'device'")
    if batch_tasks and rollout != 'device':
        raise ValueError("batch_tasks adapts all tasks on device rollouts: it needs rollout='device'")
    world, rank, local = (int(os.environ.get(k, d)) for k, d in (('WORLD_SIZE', '1'), ('RANK', '0'), ('LOCAL_RANK', '0')))
    torch.cuda.set_device(local)
    if world > 1:
        init_process_group(local)
    dev = torch.device('cuda', local)
    set_device(dev)
    random.seed(p['seed']); np.random.seed(p['seed']); torch.manual_seed(p['seed'])
    rng = np.random.RandomState(p['seed'])
    gen = torch.Generator(device=dev).manual_seed(p['seed'] + rank)
    baseline = LinearValue(2, 2)
    net = DiagNormalPolicyANIL(2, 2, 100) if anil else DiagNormalPolicy(2, 2, activation=p['activation'])
    net = net.to(dev)
    # a learnable InnerLR is a submodule of the wrapper: Adam and the all-reduce below carry its values with policy.parameters()
    policy = MAML(net, lr=inner_lr_of(net, p))
    meta_optimizer = torch.optim.Adam(policy.parameters(), lr=p['outer_lr'])
    T = p['meta_batch_size']
    lo, hi = shard_range(T, rank, world)
    for it in range(p['num_iterations']):
        meta_optimizer.zero_grad()
        goals = rng.uniform(-0.5, 0.5, size=(T, 2))                           # env.sample_tasks: identical on every rank
        iter_reward, iter_loss = 0.0, 0.0
        runs = p['adapt_steps'] + 1
        if batch_tasks:
            # the slice lo:hi in one call; task g keeps the ids (it * T + g) * runs .. + runs - 1 of the loop below
            res = fast_adapt_ppo_tasks(goals[lo:hi], policy, baseline, p, p['seed'], (it * T + lo) * runs, anil=anil, want_replays=False)
            iter_loss = res.total_loss
            iter_reward = sum(res.reward.tolist())                             # (the iteration's one read-back)
        walk = () if batch_tasks else goals[lo:hi]                             # without the flag: task by task, as before
        for g, goal in enumerate(walk, start=lo):
            learner = policy.clone()
            # rollout='device': task g of iteration `it` owns the ids (it * T + g) * runs .. + runs - 1 at any world size
            task = Particles2DRunner(goal, p['max_path_length'], gen, dev, rollout=rollout, seed=p['seed'], first_id=(it * T + g) * runs)
            eval_loss, task_rew, _ = fast_adapt_ppo(task, learner, baseline, p, anil=anil)
            iter_reward += task_rew
            iter_loss = iter_loss + eval_loss
        av_loss = iter_loss / T                                                # this rank's share of the meta-batch mean
        av_loss.backward()
        if world > 1:
            flat = torch.cat([q.grad.reshape(-1) for q in policy.parameters()] + [av_loss.detach().reshape(1), torch.tensor([iter_reward], device=dev)])
            torch.distributed.all_reduce(flat)
            off = 0
            for q in policy.parameters():
                q.grad.copy_(flat[off:off + q.numel()].view_as(q))
                off += q.numel()
            av_loss, iter_reward = flat[off], flat[off + 1].item()
        meta_optimizer.step()
        if rank == 0:
            log(f'iter {it}: average_return {iter_reward / T:.3f} loss {float(av_loss.detach()):.5f}')
    if world > 1:
        torch.distributed.destroy_process_group()
    return policy


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description='MAML-PPO / ANIL-PPO on Particles2D (MI355X engine)')
    for k, v in params.items():
        parser.add_argument(f'--{k}', type=type(v), default=v)
    parser.add_argument('--anil', action='store_true')
    parser.add_argument('--rollout', choices=('host', 'device'), default='host',
                        help='host: Python loop over the steps, torch-generator noise; device: one mi_particles_rollout call per run of a task')
    parser.add_argument('--batch_tasks', action='store_true',
                        help='adapt all tasks of a rank in one batched call per adapt step (needs --rollout device)')
    parser.add_argument('--inner_lr_per', choices=('scalar', 'tensor', 'parameter'), default='scalar',
                        help='one inner step size per model, per parameter tensor or per entry')
    parser.add_argument('--learn_inner_lr', action='store_true', help='the inner step sizes are meta-learned with the policy (MetaSGD)')
    parser.add_argument('--per_step_lr', action='store_true', help='one set of step sizes per adapt step')
    parser.add_argument('--freeze', nargs='+', default=[], metavar='PREFIX', help="parameter-name prefixes that are not adapted (e.g. 'mean.0.')")
    args = parser.parse_args()
    if args.batch_tasks and args.rollout != 'device':
        parser.error('--batch_tasks needs --rollout device')
    for k in params:
        params[k] = getattr(args, k)
    params.update(inner_lr_per=args.inner_lr_per, learn_inner_lr=args.learn_inner_lr, per_step_lr=args.per_step_lr, freeze=list(args.freeze))
    run(params, anil=args.anil, rollout=args.rollout, batch_tasks=args.batch_tasks)
