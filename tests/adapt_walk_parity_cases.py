"""The calls behind tests/golden/adapt_walk_parent.npz, shared by tools/record_adapt_walk_parity.py (which runs them on the commit
BEFORE the task-by-task walk became the one-task case of the batched adapt loop) and tests/test_gpu_adapt_walk_parity.py (which runs
them on the code under test): the task-by-task walk of fast_adapt_vpg / fast_adapt_ppo over the ten cases of adapt_tasks_cases in the
'ragged' regime, fast_adapt_trpo at one and two steps, three of those with the host advantages forced, and single_ppo_update and
trpo_update -> trpo_a2c_loss on one replay each.  The replays themselves are not recorded: their row counts are, and a rollout
is a pure function of (parameters, goal, seed, id), so equal adapted parameters and equal counts mean equal replays.  The adapted
parameters are expected bit for bit and recorded as SHA-256 digests of their fp32 bytes: the 47 vectors of 10,604 values do not
compress, and with the 12 gradients (which are held to a bar and so recorded in full) they would take a committed file past 1 MiB."""
import hashlib
import os
from collections import OrderedDict
from copy import deepcopy

import numpy as np
import torch

import adapt_tasks_cases as AC

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'adapt_walk_parent.npz')
TRPO_PARAMS = dict(inner_lr=0.1, max_path_length=12, adapt_steps=1, adapt_batch_size=4, gamma=0.99, tau=1.0)   # tests/test_gpu_rollout.py
TRPO_SEED, TRPO_FIRST_ID = 31, 1000


class _Counter:
    """A runner that notes the row count of every replay it hands out."""

    def __init__(self, runner):
        self.runner, self.counts = runner, []

    def run(self, policy, episodes):
        out = self.runner.run(policy, episodes)
        self.counts.append(int(out['states'].shape[0]))
        return out


def _np(t):
    return t.detach().cpu().numpy()


def _digest(theta):
    return hashlib.sha256(np.ascontiguousarray(_np(theta), dtype=np.float32).tobytes()).hexdigest()


def walk(cf, name):
    """test_batched_equals_the_task_by_task_walk's walk of one case."""
    algo, act, anil, first_order, dice, steps, _ = AC.CASES[name]
    P = AC.case_params(name, 'ragged')
    pol = AC.case_policy(name, 'ragged').cuda()
    base = cf.LinearValue(2, 2)
    total, out = 0.0, dict(valid_loss=[], reward=[], success=[], theta_sha256=[], counts=[])
    for i, goal in enumerate(AC.GOALS):
        runner = _Counter(cf.Particles2DRunner(goal, AC.PATH, rollout='device', seed=AC.SEED, first_id=AC.FIRST_ID + i * (steps + 1)))
        learner = cf.MAML(pol, lr=P['inner_lr'])
        if algo == 'vpg':
            loss, rew, suc = cf.fast_adapt_vpg(runner, learner, base, P, anil=anil, first_order=first_order, dice=dice)
        else:
            loss, rew, suc = cf.fast_adapt_ppo(runner, learner, base, P, anil=anil)
        total = total + loss
        for k, v in zip(out, (_np(loss), rew, suc, _digest(learner._adapted_policy.flat()), runner.counts)):
            out[k].append(v)
    total.backward()
    out['grad'] = _np(torch.cat([q.grad.reshape(-1) for q in pol._engine_params()]))
    out['baseline'] = np.array(base.weight).reshape(-1)
    return out


def trpo_walk(cf, steps):
    """test_fast_adapt_trpo_tasks_equals_the_task_by_task_walk's walk."""
    P = dict(TRPO_PARAMS, adapt_steps=steps)
    torch.manual_seed(1)
    pol, base = cf.DiagNormalPolicy(2, 2).cuda(), cf.LinearValue(2, 2)
    with torch.no_grad():
        pol.sigma.fill_(float(np.log(0.1)))
    out = dict(valid_loss=[], reward=[], success=[], theta_sha256=[], counts=[])
    for i, goal in enumerate(AC.GOALS):
        runner = _Counter(cf.Particles2DRunner(goal, P['max_path_length'], rollout='device', seed=TRPO_SEED,
                                               first_id=TRPO_FIRST_ID + i * (steps + 1)))
        learner, loss, _, rew, suc = cf.fast_adapt_trpo(runner, deepcopy(pol), base, P, first_order=True)
        for k, v in zip(out, (_np(loss), rew, suc, _digest(learner.flat()), runner.counts)):
            out[k].append(v)
    out['baseline'] = np.array(base.weight).reshape(-1)
    return out


def single_updates(cf, _=None):
    """single_ppo_update, and trpo_update -> trpo_a2c_loss (update_vf=False) with the updated policy, on one replay each."""
    P = dict(AC.PARAMS, inner_lr=0.05)
    pol = AC.make_policy('relu', False, 0.3, True).cuda()
    runner = cf.Particles2DRunner(AC.GOALS[1], AC.PATH, rollout='device', seed=AC.SEED, first_id=5)
    sup, qry = runner.run(pol, AC.EPISODES), runner.run(pol, AC.EPISODES)
    base = cf.LinearValue(2, 2)
    new = cf.trpo_update(sup, pol, base, P['inner_lr'], P['gamma'], P['tau'])
    out = dict(trpo_theta_sha256=_digest(new.flat()), trpo_valid_loss=_np(cf.trpo_a2c_loss(qry, new, base, P['gamma'], P['tau'], update_vf=False)),
               trpo_baseline=np.array(base.weight).reshape(-1))
    base = cf.LinearValue(2, 2)
    loss = cf.single_ppo_update(sup, cf.MAML(pol, lr=P['inner_lr']), base, P)
    out.update(ppo_theta_sha256=_digest(pol.flat()), ppo_valid_loss=_np(loss), ppo_baseline=np.array(base.weight).reshape(-1))
    return out


# call -> (function, its argument, whether the host advantages are forced: core_functions.rl._gae_on_device answers False)
CALLS = OrderedDict([(f'walk/{name}', (walk, name, False)) for name in AC.CASES])
CALLS.update([('trpo/1', (trpo_walk, 1, False)), ('trpo/2', (trpo_walk, 2, False)), ('single', (single_updates, None, False)),
              ('walk_host/vpg-tanh-2', (walk, 'vpg-tanh-2', True)), ('walk_host/ppo-relu-1', (walk, 'ppo-relu-1', True)),
              ('trpo_host/2', (trpo_walk, 2, True))])


def compute(cf, rlm):
    """Every recorded quantity as {'<call>/<quantity>': array} (what the recorder stores)."""
    arrays, on_device = {}, rlm._gae_on_device
    for call, (fn, arg, host) in CALLS.items():
        rlm._gae_on_device = (lambda *a: False) if host else on_device
        try:
            arrays.update({f'{call}/{k}': np.asarray(v) for k, v in fn(cf, arg).items()})
        finally:
            rlm._gae_on_device = on_device
    return arrays
