#!/usr/bin/env python3
"""Continual-learning reward / success matrices of a policy (reference misc_scripts/cl_rl.py:53-112) on Particles2D goals, driven step
by step: for every goal i a copy of the learner is adapted for ``adapt_steps`` x {rollout, update}, then evaluated on every goal j.

The update is the reference's: ``vpg`` -- ``learner.adapt(vpg_a2c_loss(episodes, learner, ...))``, autograd through the HIP policy
(mi_policy_vjp); ``ppo`` -- ``single_ppo_update``; ``trpo`` -- ``trpo_update``.  Result files and plots stay with the caller."""
from copy import deepcopy

import numpy as np
import torch

from ..core_functions.rl import Particles2DRunner, get_ep_successes, single_ppo_update, trpo_update, vpg_a2c_loss, _as_replay, _unwrap
from ..utils.cl_metrics import calc_cl_metrics

default_params = {"algo": "vpg", "anil": False, "adapt_steps": 1, "adapt_batch_size": 10, "eval_batch_size": 10, "inner_lr": 0.1,
                  "gamma": 0.99, "tau": 1.0, "max_path_length": 100, "seed": 42}


def acting_policy(learner):
    """The bare policy a runner acts with: the learner's fast weights in a detached copy once it has any, the wrapped policy otherwise."""
    if getattr(learner, '__dict__', {}).get('_fast') is not None:
        return learner.adapted_policy()
    return _unwrap(learner)


def adapt_on_goal(policy, baseline, runner, cl_params):
    """``adapt_steps`` x {rollout, update} of a COPY of ``policy`` (a ``MAML`` wrapper) on the runner's goal -> the adapted learner."""
    algo, anil = cl_params['algo'], bool(cl_params.get('anil', False))
    if algo not in ('vpg', 'ppo', 'trpo'):
        raise ValueError(f"algo must be 'vpg', 'ppo' or 'trpo', got {algo!r}")
    learner = deepcopy(policy)
    if anil:
        _unwrap(learner).turn_off_body_grads()
    for _ in range(cl_params['adapt_steps']):
        episodes = runner.run(acting_policy(learner), episodes=cl_params['adapt_batch_size'])
        if algo == 'vpg':
            learner.adapt(vpg_a2c_loss(episodes, learner, baseline, cl_params['gamma'], cl_params['tau']), allow_unused=anil)
        elif algo == 'ppo':
            single_ppo_update(episodes, learner, baseline, cl_params, anil=anil)
        else:
            learner = trpo_update(episodes, learner, baseline, cl_params['inner_lr'], cl_params['gamma'], cl_params['tau'], anil=anil,
                                  first_order=True)
    return learner


def evaluate_on_goal(learner, runner, cl_params):
    """-> (mean episode reward, success rate) of ``eval_batch_size`` episodes of the learner on the runner's goal."""
    E = cl_params['eval_batch_size']
    with torch.no_grad():
        ep = _as_replay(runner.run(acting_policy(learner), episodes=E))
    return ep['rewards'].sum().item() / E, get_ep_successes(ep, cl_params['max_path_length']) / E


def goal_runner(goal, cl_params, dev, generator, rollout, first_id):
    return Particles2DRunner(goal, cl_params['max_path_length'], generator, dev, rollout=rollout, seed=cl_params.get('seed', 42),
                             first_id=first_id)


def run_cl_rl_exp(policy, baseline, goals, cl_params=default_params, generator=None, rollout='host', dev=None):
    """``policy``: a ``MAML`` wrapper around a DiagNormalPolicy (its ``lr`` is the vpg / ppo step size); ``goals`` [N, 2].
    ``rollout='device'`` draws the noise of every run from ``(cl_params['seed'], id)``: with K = adapt_steps, the adaptation on goal i
    owns the ids i (K + N) + k, its evaluation on goal j the id i (K + N) + K + j.
    Returns (rew_matrix, suc_matrix, metrics of the rewards, metrics of the success rates); rows: adapted on, columns: evaluated on."""
    goals = np.asarray(goals, dtype=np.float32).reshape(-1, 2)
    n, K = len(goals), cl_params['adapt_steps']
    dev = dev or _unwrap(policy).sigma.device
    rew_matrix, suc_matrix = np.zeros((n, n)), np.zeros((n, n))
    for i in range(n):
        learner = adapt_on_goal(policy, baseline, goal_runner(goals[i], cl_params, dev, generator, rollout, i * (K + n)), cl_params)
        for j in range(n):
            runner = goal_runner(goals[j], cl_params, dev, generator, rollout, i * (K + n) + K + j)
            rew_matrix[i, j], suc_matrix[i, j] = evaluate_on_goal(learner, runner, cl_params)
    return rew_matrix, suc_matrix, calc_cl_metrics(rew_matrix), calc_cl_metrics(suc_matrix)
