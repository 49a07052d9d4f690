"""Inputs shared by tests/test_gpu_adapt_tasks.py (GPU) and tests/test_adapt_tasks_host.py (CPU): the goals, sizes and policies of the
batched VPG / DiCE / PPO fast-adapt tests, and the fp64 oracle walk (oracle/rl_ref.py) on replays a call returned."""
from collections import OrderedDict

import numpy as np
import torch

from exploring_meta_amd import core_functions as cf
from oracle import rl_ref as RL

FIELDS = ('states', 'actions', 'next_states', 'rewards', 'dones')
GOALS = [[0.02, -0.03], [0.3, -0.2], [-0.4, 0.1]]          # the first is reached early: ragged row counts
EPISODES, PATH, SEED, FIRST_ID = 4, 12, 31, 1018
PARAMS = dict(max_path_length=PATH, adapt_batch_size=EPISODES, gamma=0.99, tau=1.0, ppo_epochs=3, ppo_clip_ratio=0.1)

# Two policies (sigma, inner_lr, last bias set to the first goal):
#  'ragged': a scale of 0.02 and a first step that lands on the first goal -- the only way an episode of a random policy ends inside the
#            0.01 box within 12 steps -- so that task's runs have fewer rows than the others (run 0 under FIRST_ID: 37 of 48 for all three
#            policies, 2e-3 clear of the box's edge on the fp64 restatement of the rollout, tests/test_adapt_tasks_host.py).  The curvature of the inner losses grows like 1 / sigma^2 (inner_lr / sigma^2 = 5 here), which
#            is fine for comparing two fp32 paths that run the same kernels;
#  'smooth': a scale of 0.3 with inner_lr = 0.05 (inner_lr / sigma^2 = 0.55, steps of norm ~0.05 like tests/test_gpu_rl.py), where the
#            fp64 oracle's own fp32 run stays 10x inside the bars of test_policy_meta_batch_vpg_ppo on every case; used against the oracle.
#  The clipped PPO case (inner_lr = 2.0) has unit scale in both: exp(logp - logp_old) stays finite after a step of 2 x gradient.
REGIMES = dict(ragged=(0.02, 2e-3, True), smooth=(0.3, 0.05, True))

# (algo, activation, anil, first_order, dice, adapt_steps, clipped)
CASES = OrderedDict([
    ('vpg-relu-1', ('vpg', 'relu', False, False, False, 1, False)),
    ('vpg-tanh-2', ('vpg', 'tanh', False, False, False, 2, False)),
    ('vpg-anil-2', ('vpg', 'tanh', True, False, False, 2, False)),
    ('vpg-relu-fo-2', ('vpg', 'relu', False, True, False, 2, False)),
    ('dice-relu-2', ('vpg', 'relu', False, False, True, 2, False)),
    ('dice-anil-1', ('vpg', 'tanh', True, False, True, 1, False)),
    ('ppo-relu-1', ('ppo', 'relu', False, False, False, 1, False)),
    ('ppo-tanh-2', ('ppo', 'tanh', False, False, False, 2, False)),
    ('ppo-anil-2', ('ppo', 'tanh', True, False, False, 2, False)),
    ('ppo-relu-clip-1', ('ppo', 'relu', False, False, False, 1, True)),     # inner_lr = 2.0: the clip is active
])


def _regime(name, regime):
    return (1.0, 2.0, False) if CASES[name][6] else REGIMES[regime]


def case_params(name, regime):
    # the clipped case narrows the band as tests/test_gpu_rl.py does, so that most ratios leave it after the first epoch
    return dict(PARAMS, inner_lr=_regime(name, regime)[1], adapt_steps=CASES[name][5], ppo_clip_ratio=0.02 if CASES[name][6] else 0.1)


def make_policy(act, anil, sigma, drift, seed=1):
    """The reference's initialisers under a fixed seed (CPU; the caller moves it); ``drift``: the last bias is the first goal.  ANIL
    policies are the tanh DiagNormalPolicyANIL."""
    torch.manual_seed(seed)
    pol = cf.DiagNormalPolicyANIL(2, 2, 100) if anil else cf.DiagNormalPolicy(2, 2, activation=act)
    with torch.no_grad():
        pol.sigma.fill_(float(np.log(sigma)))
        if drift:
            pol._engine_params()[-1].copy_(torch.tensor(GOALS[0]))
    return pol


def case_policy(name, regime):
    sigma, _, drift = _regime(name, regime)
    return make_policy(CASES[name][1], CASES[name][2], sigma, drift)


def oracle_leaves(pol):
    """The policy's parameters as the oracle's fp64 leaves ('sigma', 'mean.0.weight', ...: the engine's order)."""
    names = list(RL.policy_param_shapes().keys())
    return OrderedDict((k, q.detach().cpu().double().clone().requires_grad_(True)) for k, q in zip(names, pol._engine_params()))


def replay64(r):
    n = int(r['states'].shape[0])
    return {k: r[k].detach().cpu().double().reshape(n, -1) for k in FIELDS}


def oracle_walk(name, regime, leaves, task_replays):
    """fast_adapt_vpg / fast_adapt_ppo restated in fp64 autograd (RL.replay_vpg / RL.replay_ppo) on every task's replays ->
    (losses [T], adapted flat parameters [T][P], gradient summed over tasks [P])."""
    algo, act, anil, first_order, dice, steps, _ = CASES[name]
    P = case_params(name, regime)
    activation = torch.relu if act == 'relu' else torch.tanh
    losses, thetas, gsum = [], [], 0.0
    for reps in task_replays:
        reps = [replay64(r) for r in reps]
        if algo == 'vpg':
            loss, pk = RL.replay_vpg(leaves, reps[:-1], reps[-1], P, RL.LinearValue(2, 2), first_order=first_order, activation=activation,
                                     anil=anil, dice=dice)
        else:
            loss, pk = RL.replay_ppo(leaves, reps[:-1], reps[-1], P, RL.LinearValue(2, 2), activation=activation, anil=anil)
        g = torch.autograd.grad(loss, list(leaves.values()))
        gsum = gsum + torch.cat([x.reshape(-1) for x in g])
        losses.append(float(loss))
        thetas.append(torch.cat([v.detach().reshape(-1) for v in pk.values()]).numpy())
    return losses, thetas, gsum.numpy()
